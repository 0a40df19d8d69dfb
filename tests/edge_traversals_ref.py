"""Edge traversals and per-edge speed entries restated in plain
Python floats: binary64, one operation at a time (no FMA), integer millimetres.  A helper
module (no tests, no fixtures): tests/test_edge_traversals_cpu.py pins what it computes,
tests/test_gpu_edge_traversals.py holds k_edge_traversals and the observation kernels equal
to it bit for bit.

traversals(res, traces, graph) takes a match result dict (the oracle's or the engine's), the
gen.Traces that were matched and the GraphFile, and returns the eleven arrays of
otr_traversal_result plus, under 'subpaths', what each sub-path looked like (for the tests).
observations(trav, graph, q) turns the complete traversals into otr_hist_entry records."""
import math

import numpy as np

from tests.matched_points_ref import KMAX, NO_EDGE, Geometry, part_mm

NO_ID = 0xFFFFFFFFFFFFFFFF
NO_SEGMENT = 0xFFFFFFFF
INVALID_SEGMENT_ID = 0x3fffffffffff
HIST_ENTRY = np.dtype([('file', '<u8'), ('id', '<u8'), ('next_id', '<u8'), ('speed_bin', '<u4'), ('count', '<u4')])
FIELDS = ('trace_off', 'edge', 'way', 'seg_id', 'first_state', 'f0', 'f1', 's0_mm', 's1_mm', 't_enter', 't_exit')
TYPES = {'trace_off': np.int64, 'edge': np.uint32, 'way': np.uint32, 'seg_id': np.uint64, 'first_state': np.int64,
         'f0': np.float64, 'f1': np.float64, 's0_mm': np.int64, 's1_mm': np.int64, 't_enter': np.float64,
         't_exit': np.float64}
T0 = 1483228800   # the hand-built batches start here


def time_at(pos, tm, x):
    """K7's time_at over one sub-path: pos / tm of its states (at least two), x a route position."""
    b = len(pos) - 1
    m = b
    for i in range(1, b + 1):
        if pos[i] >= x:
            m = i
            break
    k = m - 1
    if pos[k + 1] > pos[k]:
        return tm[k] + (tm[k + 1] - tm[k]) * (float(x - pos[k]) / float(pos[k + 1] - pos[k]))
    return tm[k]


def traversals(res, traces, graph):
    geo = Geometry(graph)
    soff = [int(x) for x in res['trace_state_off']]
    roff = [int(x) for x in res['trace_route_off']]
    cand_edge = np.asarray(res['cand_edge']).reshape(-1, KMAX)
    cand_p = np.asarray(res['cand_p']).reshape(-1, KMAX)
    rows = []       # (edge, first_state, f0, f1, s0, s1, t_enter, t_exit)
    trace_off = [0]
    subpaths = []
    for t in range(traces.n_traces):
        act = [s for s in range(soff[t], soff[t + 1]) if int(res['cand_count'][s]) > 0]
        win = {}
        for s in act:
            w = int(res['winner'][s])
            assert w >= 0, (t, s)
            win[s] = (int(cand_edge[s, w]), float(cand_p[s, w]))
        # the sub-paths' edge lists of this trace, in order (single-state sub-paths have none)
        route = [int(x) for x in res['route_edge'][roff[t]:roff[t + 1]]]
        lists, cur = [], []
        for x in route:
            if x == NO_EDGE:
                lists.append(cur)
                cur = []
            else:
                cur.append(x)
        if route:
            lists.append(cur)
        sub = [int(res['subpath'][s]) for s in act]
        k, li = 0, 0
        while k < len(act):
            k1 = k + 1
            while k1 < len(act) and sub[k1] == sub[k]:
                k1 += 1
            states = act[k:k1]
            rec = {'trace': t, 'states': states, 'pos': [0], 'first': len(rows), 'n': 0, 'returns': 0}
            if k1 - k > 1:
                lst = lists[li]
                li += 1
                assert lst and lst[0] == win[states[0]][0], (t, k)
                at = 1
                pos = [0]
                tm = [float(int(traces.time[int(res['state_probe'][s])])) for s in states]
                opened = (win[states[0]][0], win[states[0]][1], 0)   # (edge, f0, s0)
                spans = []                                           # (edge, f0, f1, s0, s1)
                for q in range(1, len(states)):
                    (ea, pa), (eb, pb) = win[states[q - 1]], win[states[q]]
                    if eb == ea and pb >= pa:
                        pos.append(pos[-1] + part_mm(pb - pa, geo.len_mm(ea)))
                        continue
                    if eb == ea:
                        rec['returns'] += 1
                    end = lst.index(eb, at)    # up to and including the next occurrence of eb
                    path = lst[at:end]
                    at = end + 1
                    s1 = pos[-1] + part_mm(1.0 - pa, geo.len_mm(ea))
                    spans.append((opened[0], opened[1], 1.0, opened[2], s1))
                    x = s1
                    for e in path:
                        spans.append((e, 0.0, 1.0, x, x + geo.len_mm(e)))
                        x += geo.len_mm(e)
                    pos_b = x + part_mm(pb, geo.len_mm(eb))
                    pos.append(pos_b)
                    opened = (eb, 0.0, pos_b - part_mm(pb, geo.len_mm(eb)))
                    assert opened[2] == x
                spans.append((opened[0], opened[1], win[states[-1]][1], opened[2], pos[-1]))
                assert at == len(lst), (t, k, at, len(lst))   # the sub-path's list is consumed exactly
                for e, f0, f1, s0, s1 in spans:
                    rows.append((e, states[0], f0, f1, s0, s1, time_at(pos, tm, s0), time_at(pos, tm, s1)))
                rec['pos'] = pos
                rec['n'] = len(spans)
            subpaths.append(rec)
            k = k1
        assert li == len(lists), (t, li, len(lists))
        trace_off.append(len(rows))
    edge = np.array([r[0] for r in rows], np.uint32)
    seg = np.asarray(graph.edge_seg)[edge] if len(rows) else np.zeros(0, np.uint32)
    out = {
        'trace_off': np.array(trace_off, np.int64),
        'edge': edge,
        'way': (np.asarray(graph.edge_way)[edge] if len(rows) else np.zeros(0)).astype(np.uint32),
        'seg_id': np.array([int(graph.seg_id[int(s)]) if int(s) != NO_SEGMENT else NO_ID for s in seg], np.uint64),
        'first_state': np.array([r[1] for r in rows], np.int64),
        'f0': np.array([r[2] for r in rows], np.float64),
        'f1': np.array([r[3] for r in rows], np.float64),
        's0_mm': np.array([r[4] for r in rows], np.int64),
        's1_mm': np.array([r[5] for r in rows], np.int64),
        't_enter': np.array([r[6] for r in rows], np.float64),
        't_exit': np.array([r[7] for r in rows], np.float64),
        'subpaths': subpaths,
    }
    return out


def observations(trav, graph, q=3600):
    """The otr_hist_entry records (HIST_ENTRY) of the complete traversals, in traversal order."""
    q = int(q) if int(q) > 0 else 3600
    n = len(trav['edge'])
    out = []
    for j in range(n):
        f0, f1 = float(trav['f0'][j]), float(trav['f1'][j])
        te, tx = float(trav['t_enter'][j]), float(trav['t_exit'][j])
        dt = tx - te
        if not (f0 == 0.0 and f1 == 1.0 and dt > 0.5):
            continue
        e = int(trav['edge'][j])
        level = (int(graph.edge_attr[e]) >> 11) & 7
        file = ((int(math.floor(te)) // q) << 25) | (level << 22)
        nxt = INVALID_SEGMENT_ID
        if j + 1 < n and int(trav['first_state'][j + 1]) == int(trav['first_state'][j]):
            nxt = int(trav['edge'][j + 1])
        v = float(int(trav['s1_mm'][j]) - int(trav['s0_mm'][j])) / 1000.0
        v = v / dt
        v = v * 3.6
        v = v / 20.0
        out.append((file, e, nxt, min(int(v), 7), 1))
    return np.array(out, dtype=HIST_ENTRY) if out else np.zeros(0, HIST_ENTRY)


def same_bits(got, want):
    """The names of the arrays that differ (bit for bit) between two traversal results."""
    bad = []
    for k in FIELDS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
            bad.append(k)
    return bad


def group_continues(graph, ep, e):
    """K7's rule: does edge e continue the segment group whose last edge is ep?"""
    from reporter_amd.graphfile import ATTR_INTERNAL, ATTR_SEG_BEGIN, ATTR_SEG_END
    key = int(graph.edge_seg[ep])
    ap, a = int(graph.edge_attr[ep]), int(graph.edge_attr[e])
    if key != NO_SEGMENT:
        return int(graph.edge_seg[e]) == key and not (ap & ATTR_SEG_END) and not (a & ATTR_SEG_BEGIN)
    return int(graph.edge_seg[e]) == NO_SEGMENT and bool(a & ATTR_INTERNAL) == bool(ap & ATTR_INTERNAL)


# ---- the batch of the speed entries' known answers ----------------------------------------
def kat3(graph_dir):
    """Three collinear one-way edges E0, E1, E2 on the equator (nodes at lon 0, 0.001, 0.002,
    0.003; ways 1, 2, 3) and three traces 2.2 m north of them (interpolation_distance 50):
    A probes at lon .0005, .0025, both at +0 s: E1 is traversed in no time;
    B the same places at +0, +20 s: E1 from +5 to +15 s;
    C .0005, .0015, .0025 at +0, +10, +10 s: E1 from +5 to +10 s."""
    import os
    from reporter_amd.graphfile import write_graph
    from reporter_amd.tools.gen import Traces
    path = os.path.join(graph_dir, 'edge_traversals_kat3.otrg')
    new = write_graph(path, [(0.0, 0.0), (0.0, 0.001), (0.0, 0.002), (0.0, 0.003)],
                      [dict(src=0, dst=1, way=1), dict(src=1, dst=2, way=2), dict(src=2, dst=3, way=3)])
    y = 0.00002
    rows = [([0.0005, 0.0025], [0, 0]), ([0.0005, 0.0025], [0, 20]), ([0.0005, 0.0015, 0.0025], [0, 10, 10])]
    lat = np.array([y for r in rows for _ in r[0]], np.float64)
    lon = np.array([x for r in rows for x in r[0]], np.float64)
    tm = np.array([T0 + s for r in rows for s in r[1]], np.int64)
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r[0]) for r in rows])
    return path, Traces(lat, lon, tm, off, np.zeros(len(rows), np.uint8)), [int(x) for x in new]

