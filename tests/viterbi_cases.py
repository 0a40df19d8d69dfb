"""Hand-built graphs and traces on which the Viterbi stage (K5, k_viterbi) meets exact cost
ties (the lowest index among equal minima, for a predecessor and for the winner
at the end of a sub-path).  A helper module (no tests, no fixtures):
tests/test_viterbi_cases_cpu.py pins what every trace reaches, with the oracle and the
restatement of tests/viterbi_ref.py; tests/test_gpu_viterbi_ties.py runs the batches through
the three k_viterbi instances.

The building block is a one-way road along a line y = const whose pieces are bundles of
duplicate edges: n edges between the same two nodes with the same two-point shape.  The
duplicates of a bundle get bit-equal projections (cand_sqd, cand_p), the candidate search
orders them by edge id, and write_graph numbers them in input order: a duplicate's candidate
index is its rank in the bundle.  Stored lengths (length=) are free per duplicate and longer
than the geometry, so the cost order inside a bundle is the order of the stored lengths and
duplicates of equal stored length tie exactly.

Two graphs: SUITES['k32'] (radius 50 m, at most 22 candidates: the two K <= 32 instances) and
SUITES['wide'] (ragged.CONFIGS['wide']: radius 200 m, 64 candidates, bundles of 40 and 50:
k_viterbi<1> and its global backtrack).  Every edge is its own OSMLR segment, so the segments and
reports after the Viterbi stage say which duplicate won."""
import os

import numpy as np

from reporter_amd.graphfile import write_graph
from tests import kat_graphs as K

SHUFFLE_SEED = 11       # the fixed shuffle of the all-cases batch (numpy default_rng)
LANE = 400.0            # metres between two roads of the k32 graph (radius 50 m, islands at +150 m)
WIDE_LANE = 800.0       # ... of the wide graph (radius 200 m)
LAND = 3200.0           # a road's landing piece starts here: more than breakage_distance (2 km) away
MODE_CYCLE = (0, 1, 1, 0, 0, 2, 2, 0)  # trace i of the all-cases batch: auto, bicycle, pedestrian


def lens(n, tied, base=200.0):
    """Stored lengths of a bundle of n duplicates: `base` metres for the tied indices, 1 to 5 m
    more for the others (whole metres: exact in the file's float32)."""
    return [base if i in tied else base + 1.0 + (i % 5) for i in range(n)]


class Net:
    """Nodes and edges of one graph; key -> input index of every edge."""

    def __init__(self):
        self.nodes, self.edges, self.key = [], [], {}

    def node(self, x, y):
        self.nodes.append(K.ll(x, y))
        return len(self.nodes) - 1

    def bundle(self, key, a, b, lengths):
        """len(lengths) duplicate edges a -> b; keys (key, 0), (key, 1), .. in edge-id order."""
        for r, L in enumerate(lengths):
            self.key[(key, r)] = len(self.edges)
            self.edges.append(dict(src=a, dst=b, way=100 + len(self.edges), level=1, speed=50, length=float(L)))

    def road(self, key, y, pieces, x0=0.0):
        """A one-way road eastwards from (x0, y): pieces = [(metres, stored lengths)], piece q gets
        the keys ((key, q), r).  Returns the node ids."""
        ids = [self.node(x0, y)]
        x = x0
        for q, (geom, lengths) in enumerate(pieces):
            x += geom
            ids.append(self.node(x, y))
            self.bundle((key, q), ids[-2], ids[-1], lengths)
        return ids

    def write(self, path):
        segs = [dict(id=K.osmlr(1, 440, i + 1), edges=[i]) for i in range(len(self.edges))]
        new = write_graph(path, self.nodes, self.edges, segs)
        return {k: int(new[v]) for k, v in self.key.items()}


class Suite:
    """One graph, its named traces and the batches made of them."""

    def __init__(self, name, cfgs):
        self.name, self.cfgs = name, cfgs
        self.net = Net()
        self.cases = {}     # case -> [trace names], in the order of the all-cases batch
        self.points, self.dt, self.mode = {}, {}, {}
        self.path, self.ids = None, None

    def add(self, case, name, points, dt):
        assert name not in self.points, name
        self.cases.setdefault(case, []).append(name)
        self.points[name], self.dt[name] = points, dt

    def finish(self, path):
        self.path = path
        self.ids = self.net.write(path)
        for i, name in enumerate(self.all_names()):
            self.mode[name] = MODE_CYCLE[i % len(MODE_CYCLE)]

    def all_names(self):
        return [n for names in self.cases.values() for n in names]

    def batches(self):
        """batch name -> trace names: every case alone, all cases, that batch reversed and
        under one fixed shuffle."""
        out = {case: list(names) for case, names in self.cases.items()}
        names = self.all_names()
        out['all'] = names
        out['reversed'] = names[::-1]
        out['shuffled'] = [names[int(i)] for i in np.random.default_rng(SHUFFLE_SEED).permutation(len(names))]
        return out

    def batch(self, names):
        return K.batch([K.trace(self.points[n], dt=self.dt[n]) for n in names], [self.mode[n] for n in names])


def _mid(q, piece=120.0, y=2.0):
    """The probe beside the middle of piece q of a road of equal pieces (60 m from both ends:
    outside the 50 m radius of the neighbouring pieces)."""
    return (piece * q + piece / 2, y)


# the tied index sets of pred_pairs: the two halves of the split scan, the lower index in the odd
# half, the same half, the U = 8 chunk boundary, a chunk boundary inside one half, across both
# halves at the U = 16 boundary; a three-way tie and all 18
PRED_PAIRS = [(0, 1), (1, 2), (0, 2), (1, 3), (7, 8), (14, 16), (15, 17), (15, 16), (3, 8, 12), tuple(range(18))]
END_PAIRS = [(0, 1), (1, 3), (0, 16), (3, 19)]       # butterfly distances 1, 2 and 16
WIDE_PRED = [(15, 16), (31, 32), (32, 33), (47, 48)]
WIDE_END = [(0, 32), (31, 32)]                       # butterfly distance 32 (and 1 across it)
LONG_LENS = [104, 105, 128, 129]
LONG_TIES = {3: (2, 11), 103: (5, 14), 127: (9, 16)}  # state -> tied duplicates of its bundle of 18
DT = 120   # seconds between probes 120 m apart: twice that bounds a pedestrian's 162 s for 230 m
WIDE_DT = 400
LONG_DT = 15


def tname(kind, tied):
    return kind + '_' + ('all' if len(tied) > 4 else '_'.join(str(i) for i in tied))


def build_k32(path):
    s = Suite('k32', ('gtt', 'deployed', 'mixed'))
    net, lane = s.net, [0]

    def y():
        lane[0] += 1
        return LANE * (lane[0] - 1)
    one = [200.0]
    # ---- pred_pairs: a source bundle of 18, then a single edge (two pieces of it)
    for tied in PRED_PAIRS:
        y0 = y()
        net.road(tname('pred', tied), y0, [(120.0, lens(18, tied)), (120.0, one), (120.0, one)])
        s.add('pred_pairs', tname('pred', tied), [(x, y0 + dy) for x, dy in (_mid(0), _mid(1), _mid(2))], DT)
    # ---- end_ties: a single edge, a bundle of 20, and a landing piece 3.2 km on
    for tied in END_PAIRS:
        y0 = y()
        net.road(tname('end', tied), y0, [(120.0, one), (120.0, lens(20, tied))])
        net.road(tname('land', tied), y0, [(120.0, one)], x0=LAND)
        a, b = (60.0, y0 + 2), (180.0, y0 + 2)
        s.add('end_ties', tname('end', tied), [a, b], DT)                                      # the trace end
        s.add('end_ties', tname('brk', tied), [a, b, (LAND + 30, y0 + 2), (LAND + 90, y0 + 2)], DT)  # a forced step
    y0 = LANE * (lane[0] - 1)  # (the last end_ties road) a state alone between two forced steps, and alone in its trace
    s.add('end_ties', 'one_state_sub', [(LAND + 30, y0 + 2), (180.0, y0 + 2), (LAND + 90, y0 + 2)], DT)
    s.add('end_ties', 'one_state_trace', [(180.0, y0 + 2)], DT)
    # ---- both: two bundles in a row, the predecessor tie behind the end tie
    for k, (pt, et) in enumerate([((5, 9), (2, 7)), ((1, 16), (16, 18))]):
        y0 = y()
        net.road('both%d' % k, y0, [(120.0, lens(18, pt)), (120.0, lens(20, et))])
        s.add('both', 'both%d' % k, [(60.0, y0 + 2), (180.0, y0 + 2)], DT)
    # ---- ragged_K: 18 -> 2 -> 18 candidates beside 2 -> 18 -> 2 in one wave
    y0 = y()
    net.road('rag0', y0, [(120.0, lens(18, (9, 17))), (120.0, [200.0, 203.0]), (120.0, lens(18, (4, 6)))])
    s.add('ragged_K', 'rag0', [(x, y0 + dy) for x, dy in (_mid(0), _mid(1), _mid(2))], DT)
    y0 = y()
    net.road('rag1', y0, [(120.0, [200.0, 200.0]), (120.0, lens(18, (2, 10))), (120.0, [200.0, 203.0])])
    s.add('ragged_K', 'rag1', [(x, y0 + dy) for x, dy in (_mid(0), _mid(1), _mid(2))], DT)
    # ---- unreachable: N0 .. N4 at x = 0, 120, .. 480; two stubs that start nowhere and end at N2
    # (stored 125 / 130 m: the shorter way on), a spur N1 -> D that ends nowhere, an island of
    # three duplicates 150 m north
    y0 = y()
    n = net.road('unr', y0, [(120.0, one), (120.0, one), (120.0, [200.0, 205.0]), (120.0, one)])
    net.bundle('stub0', net.node(124.0, y0 - 6.0), n[2], [125.0])
    net.bundle('stub1', net.node(124.0, y0 - 9.0), n[2], [130.0])
    net.bundle('spur', n[1], net.node(236.0, y0 + 6.0), [200.0])
    net.road('island', y0 + 150.0, [(240.0, [300.0, 305.0, 310.0])], x0=360.0)
    s.add('unreachable', 'unreachable', [(60.0, y0 + 2), (180.0, y0 - 2.5), (300.0, y0 + 2), (420.0, y0 + 152),
                                         (540.0, y0 + 152)], DT)
    # ---- route_tie: two equal duplicates in the middle of the route, no state on them
    y0 = y()
    net.road('rt', y0, [(120.0, one), (120.0, [200.0, 200.0]), (120.0, one)])
    s.add('route_tie', 'route_tie', [(60.0, y0 + 2), (300.0, y0 + 2)], DT)
    # ---- long: 129 pieces of 20 m, a state on each; the pieces of LONG_TIES are bundles of 18
    y0 = y()
    net.road('long', y0, [(20.0, lens(18, LONG_TIES[q], 21.0) if q in LONG_TIES else [21.0]) for q in range(129)])
    for n_states in LONG_LENS:
        s.add('long', 'long%d' % n_states, [(20.0 * q + 10.0, y0 + 2) for q in range(n_states)], LONG_DT)
    s.finish(path)
    return s


def build_wide(path):
    s = Suite('wide', ('wide',))
    net, lane = s.net, [0]

    def y():
        lane[0] += 1
        return WIDE_LANE * (lane[0] - 1)
    one = [600.0]
    for tied in WIDE_PRED:
        y0 = y()
        net.road(tname('pred', tied), y0, [(500.0, lens(50, tied, 600.0)), (500.0, one)])
        s.add('pred_wide', tname('pred', tied), [(250.0, y0 + 2), (750.0, y0 + 2)], WIDE_DT)
    for tied in WIDE_END:
        y0 = y()
        net.road(tname('end', tied), y0, [(500.0, one), (500.0, lens(40, tied, 600.0))])
        net.road(tname('land', tied), y0, [(500.0, one)], x0=4000.0)
        a, b = (250.0, y0 + 2), (750.0, y0 + 2)
        s.add('end_wide', tname('end', tied), [a, b], WIDE_DT)
        s.add('end_wide', tname('brk', tied), [a, b, (4220.0, y0 + 2), (4280.0, y0 + 2)], WIDE_DT)
    s.finish(path)
    return s


SUITES = {'k32': build_k32, 'wide': build_wide}
_BUILT = {}


def suite(name, graph_dir):
    """The suite `name`, its graph written once per process."""
    key = (name, graph_dir)
    if key not in _BUILT:
        _BUILT[key] = SUITES[name](os.path.join(graph_dir, 'viterbi_ties_%s.otrg' % name))
    return _BUILT[key]


_ORACLE = {}


def oracle_result(name, cfg, batch, graph_dir):
    """(suite, traces, the oracle's result) of a batch under a configuration, computed once per
    process; callers leave the result unchanged."""
    from oracle import pyoracle as po
    from tests import ragged
    key = (name, cfg, batch, graph_dir)
    if key not in _ORACLE:
        s = suite(name, graph_dir)
        tr = s.batch(s.batches()[batch])
        _ORACLE[key] = (s, tr, po.match_batch(po.Graph(s.path), tr, ragged.oracle_params(cfg)))
    return _ORACLE[key]
