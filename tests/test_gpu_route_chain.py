"""The node search's bookkeeping between two rounds (the key count and the
probe-chain overflow are carried in registers, the target's words and the first pending chunk
are read ahead of the round), on hand-built one-way out-trees, field by field against the
oracle and against work counters recorded before the change (tests/golden/
route_chain_counts.json):

  (1) `tree`: a ternary out-tree of depth 6 (1,093 nodes), every stored length 10 m, so a whole
      level is final in one round.  A trace goes from the edge into the root to an edge at
      depth 6.  The table holds 4, 13, 40, 121 keys after the first rounds; the round that
      settles depth 4 offers 243 more, so the 160-slot table (and the 256- and 448-slot ones)
      runs out of slots inside a round, by probe exhaustion and not at the load limit; depth 5
      does the same to the 1,024-slot table (364 keys + 729).  The 2,048-slot table holds the
      1,093 keys, but the 729 pending leaves outgrow its 512-entry pending list (the capacity
      test the rounds already hold in a register), so the search ends in the 4,096-slot tier.
      Rounds of 9, 27 and 81 final nodes: 2, 4 and more relax chunks of a 32-lane group and
      the per-round settle cap.
  (2) `hubs`: a node with 12 out-edges whose heads have 12 each (keys 1, 13, 157): two thirds
      of the keys arrive through the CSR-tail pass, and the table is past its load limit of
      140 keys after the second round.  A key count without the tail's keys runs another round.
  (3) the traces run as batches of 1, 2 and 3 (the searches of a wave finish in different
      rounds, a lane group idles beside a running one); the second trace runs against the
      one-way edges: its searches end on an empty pending list.
  (4) once more with libotr_tiercheck.so and OTR_FORCE_EDGE=128: the retry tiers stop after
      2 (3) rounds, dump and resume, so the resumed tables start from a dump's key count.

Each batch runs with route_work on and off.  A case that does not reach its path fails: the
tiers named above each ran a search (route_tier_work), the hubs' searches relaxed more than
four edges per node with out-edges (only the tail pass does), and the tree settled more than
eight nodes per round on average (a round of more than 8 nodes has at least two relax chunks).
The graphs' extent is chosen so that the size estimate of the long step (keys = half the node
density x reach^2) lies between the small tier's limit and the first tier's: the search starts
in the first tier.  Runs in child processes (one library per process)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'route_chain_counts.json')
# settled, relaxed, transitions, searches, settled and relaxed in the retry tiers, rounds, keys
COUNTERS = (3, 4, 5, 6, 9, 10, 13, 14)
SMALL_KEYS, FIRST_KEYS = 24.0, 140.0  # estimates above / up to these start in the first tier


def build_fan(path, fanout, depth, corner):
    """W (-100, 0) -> R (0, 0), then the full out-tree of `fanout` below R to `depth` (a last
    level of one node when depth is written (d, 1)); every tree edge is one-way with a stored
    length of 10 m.  The path of first children ends in P (200, 0) -> T (400, 0), the target
    edge; every other tree node sits in a 2 m lattice north of the road (x 170.., y 600..),
    out of every probe's reach.  An unconnected road 20 m south of P-T gives the last probes
    a candidate that is never reached.  Two short island edges at (-corner, -corner) and
    (corner + 400, corner + 400) set the extent of the graph (the size estimate's density)."""
    from reporter_amd.graphfile import write_graph
    from tests import kat_graphs as K
    depth, last = depth if isinstance(depth, tuple) else (depth, None)
    nodes, edges = [K.ll(-100, 0), K.ll(0, 0)], []
    edges.append(dict(src=0, dst=1, way=100, level=1, speed=50))
    level, first, lattice = [1], 1, 0
    for d in range(1, depth + 1):
        nxt = []
        for u in level:
            for c in range(fanout if last is None or d < depth else (last if u == first else 0)):
                v = len(nodes)
                on_path = u == first and c == 0
                if on_path and d == depth - 1:
                    nodes.append(K.ll(200, 0))
                elif on_path and d == depth:
                    nodes.append(K.ll(400, 0))
                else:
                    nodes.append(K.ll(170 + 2 * (lattice % 34), 600 + 2 * (lattice // 34)))
                    lattice += 1
                edges.append(dict(src=u, dst=v, way=101 + d, level=1, speed=50, length=10.0))
                nxt.append(v)
        if nxt:
            first = nxt[0]
        level = nxt
    target = len(edges) - 1 if last is not None else None
    if target is None:  # the full tree: the first edge of the last level's first group
        target = next(i for i, e in enumerate(edges) if e['dst'] == first)
    # an unconnected one-way road beside the target edge: a candidate of the last probes that no
    # search reaches, so the searches run until nothing is pending (the whole tree)
    # (its first edge gives the candidate's tail node an in-edge: a node without one has an
    # unbounded IN gap and counts as unreachable at once)
    for x in (100, 200, 400):
        nodes.append(K.ll(x, -20))
    for k in (3, 2):
        edges.append(dict(src=len(nodes) - k, dst=len(nodes) - k + 1, way=98, level=1, speed=50))
    for x in (-corner, corner + 400):
        nodes.append(K.ll(x, x))
        nodes.append(K.ll(x + 10, x))
        edges.append(dict(src=len(nodes) - 2, dst=len(nodes) - 1, way=99, level=1, speed=50))
    write_graph(path, nodes, edges, [dict(id=K.osmlr(1, 420, 1), edges=[target])])
    traces = [[(-60, 2), (-5, 2), (270, 2), (330, 2)],     # W-R, then on P-T
              [(270, 2), (330, 2), (-60, 2), (-5, 2)],     # against the one-way edges: unreachable
              [(-60, -2), (-5, -2), (270, -2), (330, -2)]]
    return [K.trace(p, dt=20) for p in traces]


def build_tree(path):
    return build_fan(path, 3, 6, 500)


def build_hubs(path):
    return build_fan(path, 12, (3, 1), 0)


def first_tier_estimate(path, gc_m=275.0, dt=20, factor=5.0, time_factor=2.0):
    """The engine's size estimate of the long step (k_tasks): half the node density of the
    graph's cell grid times reach^2, reach = min(length bound, time bound x 50 km/h)."""
    import math
    from reporter_amd.graphfile import GraphFile
    h = GraphFile(path).h
    m = 20037581.187 / 180.0
    mlat = h['grid_min_lat'] + 0.5 * h['grid_rows'] * h['grid_cell_deg']
    area = (h['grid_rows'] * h['grid_cell_deg'] * m) * (h['grid_cols'] * h['grid_cell_deg'] * m *
                                                        math.cos(math.radians(mlat)))
    reach = min(factor * gc_m, time_factor * dt * 50 / 3.6)
    return 0.5 * h['n_nodes'] / area * reach * reach


CHILD = r'''
import json
import os
import sys
sys.path.insert(0, %r)
from oracle import pyoracle as po
from oracle.compare import compare
from reporter_amd import _lib
from reporter_amd import matcher as M
from tests import kat_graphs as K
from tests import test_gpu_route_chain as T
gdir, retry = %r, %r
out = {}
for name, build in (('chain_tree', T.build_tree), ('chain_hubs', T.build_hubs)):
    path = os.path.join(gdir, name + '.otrg')
    trs = build(path)
    est = T.first_tier_estimate(path)
    assert T.SMALL_KEYS < est <= T.FIRST_KEYS, (name, est)  # the long step starts in the first tier
    opts = {'turn_penalty_factor': 0}
    M.configure(M.default_config(path, **opts))
    g = po.Graph(path)
    for n in range(1, len(trs) + 1):
        b = K.batch(trs[:n])
        want = po.match_batch(g, b, po.params(**{k: float(v) for k, v in opts.items()}))
        r = M.Matcher().match_batch(b, copy_out=True, route_work=True)
        assert r.status == 0, r.status
        c = [int(r.counters[k]) for k in range(24)]
        got = _lib.result_to_numpy(r)
        errors, stats = compare(got, want)
        assert not errors, (name, n, errors)
        r2 = M.Matcher().match_batch(b, copy_out=True, route_work=False)
        assert r2.status == 0, r2.status
        errors, stats = compare(_lib.result_to_numpy(r2), got)
        exact = [v for k, v in stats.items() if k.endswith('_bitexact')]  # (floats bit-exact too)
        assert not errors and exact and all(exact), (name, n, errors, stats)
        w = [[int(r.route_tier_work[t][k]) for k in range(4)] for t in range(16)]
        code = [int(r.route_tier_code[t]) for t in range(16)]
        print(name, n, 'est %%.1f' %% est, 'searches', c[6], 'settled', c[3], 'relaxed', c[4], 'rounds', c[13],
              'keys', c[14], 'resumed', c[11], 'dumped', c[12], 'tiers', [x[0] for x in w])
        out['%%s/%%d' %% (name, n)] = {'counters': {str(k): c[k] for k in T.COUNTERS},
                                       'tier_work': [x[:3] for x in w],  # (searches, settled, relaxed)
                                       'tier_code': code}
        if retry:
            # forced stops after 2 (3) rounds: searches were dumped in one tier and resumed in
            # the next (as tests/test_gpu_route_rounds.py), and the retry tiers settled nodes
            assert c[12] > 0 and c[11] > 0 and c[12] >= c[11] and c[9] > 0, (name, n, c)
            continue
        if name == 'chain_tree':
            # the first tier and the 256-, 448 x 2-, 1024- and 2048-slot tiers each ran a search
            # (the tables to 1,024 slots ran out of slots inside a round, the 2,048-slot one out
            # of pending list), the 4,096-slot tier ended it and none went beyond
            assert code[:6] == [1602, 2561, 4482, 10241, 20481, 40961], code
            assert all(w[t][0] > 0 for t in range(6)) and not any(w[t][0] for t in (6, 7, 8)), w
            # more than 8 settled nodes per round on average: rounds of two and more relax chunks
            assert c[3] > 8 * c[13], (c[3], c[13])
            assert w[5][1] >= 1093, w[5]  # the last table settled the whole tree
        else:
            # the search from R outgrew the first table (156 relaxations: 12 + 144) and went on
            # in the 256-slot tier, which held it.  14 nodes of the graph have out-edges, and the
            # adjacency slots give at most 4 relaxations per settled node: more than 56 per
            # search means the tail pass ran
            assert w[0][2] >= 156, w[0]
            assert w[1][0] > 0 and not any(w[t][0] for t in (2, 3, 4, 5, 6, 7, 8)), w
            assert w[1][2] > 4 * 14 * w[1][0], w[1]
print('work ' + json.dumps(out, sort_keys=True))
print('chain ok')
'''


def run_child(graph_dir, retry):
    env = dict(os.environ)
    for k in ('OTR_LIB', 'OTR_TIERS', 'OTR_EST_K', 'OTR_FORCE_EDGE', 'OTR_NDUMP_GB', 'OTR_OPT_RESERVE_GB',
              'OTR_SMALL_KEYS', 'OTR_TINY_KEYS', 'OTR_ROUTE_G'):
        env.pop(k, None)
    if retry:
        lib = os.path.join(ROOT, 'reporter_amd', 'libotr_tiercheck.so')
        assert os.path.exists(lib), 'build first: python -m reporter_amd.build'
        env.update(OTR_LIB=lib, OTR_FORCE_EDGE='128')
    p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, retry)], env=env, capture_output=True,
                       text=True, timeout=240)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and 'chain ok' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('work ')][-1]
    return json.loads(line[len('work '):])


def test_route_chain_equals_oracle_and_recorded_work(graph_dir):
    got = run_child(graph_dir, False)
    with open(GOLDEN) as f:
        want = json.load(f)['cases']
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k] == want[k], (k, got[k], want[k])


def test_route_chain_retry_tiers_resume(graph_dir):
    run_child(graph_dir, True)
