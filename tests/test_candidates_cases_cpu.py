"""The candidate cases of tests/candidates_ref.py on the CPU: the oracle's candidates equal the
grid-free brute force bit for bit (which pins oracle.c's grid walk and ownership rule, and
write_graph's registration of edges in cells, to a statement that has no grid), and the cases
still sit where k_candidates can go wrong.  The pins are requirements on the inputs of
tests/test_gpu_candidates.py, not measurements: when a builder changes, this file says which
edge the GPU test lost."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import candidates_ref as cr
from tests import matched_points_ref as mref


def _full(run, i):
    """Everything probe i of the run finds, uncut: (edges, fractions, squared distances, found)."""
    m = run.modes[i] if run.modes[i] < cr.N_MODES else 0
    return cr.brute_candidates(run.graph, run.probes[i][0], run.probes[i][1], run.radii()[i], m, run.graph.n_edges)


def _kmax(run, i):
    m = run.modes[i] if run.modes[i] < cr.N_MODES else 0
    return min(int(run.oracle_params()[m].max_candidates), mref.KMAX)


def _paths(run):
    return [cr.path_of(*cr.window(run.graph, p[0], p[1], r)) for p, r in zip(run.probes, run.radii())]


@pytest.mark.parametrize('case', cr.CASES)
def test_oracle_equals_brute_force(case, graph_dir):
    n = 0
    for run in cr.runs_of(case, graph_dir):
        G = po.Graph(run.path)
        for name, order in cr.batches(run):
            res = po.match_batch(G, run.traces(order), run.oracle_params())
            bad = cr.differences(run, order, res)
            assert not bad, (name, bad[:3])
            n += len(order)
    print('%s: %d states' % (case, n))
    assert n > 0


def test_orders():
    for n in (1, 2, 9, 14):
        o = cr.orders(n)
        assert o['written'] == list(range(n)) and o['reversed'] == o['written'][::-1]
        assert set(o['rotated']) == set(range(n)) and len(o['rotated']) % 2 == 1
        if n > 2:
            # every probe's wave partner under k_candidates<2> differs between as written and rotated
            def partner(order, s):
                return order[s ^ 1] if (s ^ 1) < len(order) else None
            for s, i in enumerate(o['rotated'][:n]):
                assert partner(o['rotated'], s) != partner(o['written'], i), (n, i)


def test_instance_rule(graph_dir):
    """Batch::candidates (otr_engine.hip) runs k_candidates<2> iff every mode keeps at most 32
    candidates and no search radius can exceed 100 m: with per-probe accuracies a mode's largest
    radius is its max_search_radius, without them min(max_search_radius, max(search_radius,
    gps_accuracy)).  Which instance ran cannot be seen through the C-ABI: the runs meant for <2>
    satisfy the rule and the ones meant for <1> only break it."""
    seen = set()
    for case in cr.CASES:
        for run in cr.runs_of(case, graph_dir):
            prm = run.oracle_params()
            two = True
            for m in range(cr.N_MODES):
                q = prm[m]
                kmax = max(1, min(int(q.max_candidates), mref.KMAX))
                rmax = q.max_search_radius if run.accuracy is not None else \
                    min(q.max_search_radius, max(q.search_radius, q.gps_accuracy))
                two = two and kmax <= 32 and rmax <= 100.0
            assert two == (run.instance == 2), run.name
            seen.add((case, run.instance))
    assert seen == {('star', 1), ('star', 2), ('dense', 1), ('dense', 2), ('poly', 2), ('border', 2), ('corner', 2),
                    ('exact_radius', 2), ('modes', 2)}


def test_star_cuts_inside_ties(graph_dir):
    runs = {r.name: r for r in cr.runs_of('star', graph_dir)}
    for cd in ('0.0005', '5e-05'):
        for kmax in (5, 16):
            run = runs['star_%s_k%d' % (cd, kmax)]
            _, _, d2, found = _full(run, 0)   # the hub
            assert found == 40 and _kmax(run, 0) == kmax
            assert d2[kmax - 2] == d2[kmax - 1] == d2[kmax] == d2[kmax + 1], (kmax, d2[:kmax + 2])
        # n == kmax and n == kmax + 1: nothing to cut, one to cut
        assert _full(runs['star_%s_k16' % cd], 3)[3] == 16 and _full(runs['star_%s_k5' % cd], 4)[3] == 6
        found = [_full(runs['star_%s_k64' % cd], i)[3] for i in range(len(run.probes))]
        assert found[:3] == [40, 40, 40] and found[-3:] == [0, 0, 0] and 0 < found[5] < 5, found
    # the hub lies on a cell boundary of both grids (its edges are registered on both sides)
    for cd in (0.0005, 0.00005):
        assert abs(cr.HUB[0] / cd - round(cr.HUB[0] / cd)) < 1e-6 and abs(cr.HUB[1] / cd - round(cr.HUB[1] / cd)) < 1e-6


def test_dense_compacts_many_times(graph_dir):
    for run in cr.runs_of('dense', graph_dir):
        found = [_full(run, i)[3] for i in range(len(run.probes))]
        kmax = _kmax(run, 0)
        if kmax == 64:
            assert max(found) > 2 * 64 and run.instance == 1
        # k_candidates keeps kmax and takes one pass of its lanes (64, or 32 two states per wave)
        # on top: more than this many found means several compactions in one state
        assert max(found) > 3 * (kmax + (32 if run.instance == 2 else 64)), (run.name, max(found))
        assert min(found) == 0
        modes = sorted(set(run.modes))
        assert modes == [0, 1, 2, 7]
        # edges closed to the mode: a pedestrian finds more than a car, a mode byte of 7 what a car finds
        by = {m: [f for f, mm in zip(found, run.modes) if mm == m] for m in modes}
        assert by[7] == by[0] and sum(by[2]) > sum(by[0]) > 0
    attr = cr.runs_of('dense', graph_dir)[0].graph.edge_attr
    assert 0.3 < float(np.mean((attr & 7) == 4)) < 0.36 and set((attr & 7).tolist()) == {4, 7}


def test_grids_choose_the_path(graph_dir):
    """Per graph file over its option sets: the coarse grids stay on the window path, every fine
    grid has probes cell by cell (a window dimension > 16) and on the window path (a window of
    1 to 16 cells both ways)."""
    per = {}
    for case in ('star', 'dense'):
        for run in cr.runs_of(case, graph_dir):
            per.setdefault(run.path, set()).update(_paths(run))
    assert len(per) == 2 + 2 * len(cr.DENSE_CENTRES)
    for path, kinds in per.items():
        fine = cr._GRAPHS[path].h['grid_cell_deg'] < 0.0001
        assert kinds == ({'win', 'slow', 'none'} if fine else {'win', 'none'}), (path, kinds)
    # a high latitude: the fine window is several times wider than tall
    north = [r for r in cr.runs_of('dense', graph_dir) if r.name == 'dense_north_2e-05_k32_r50'][0]
    rows, cols = cr.window(north.graph, north.probes[0][0], north.probes[0][1], 50.0)
    assert cols > 2.5 * rows > 40
    # negative coordinates, and a grid that straddles zero both ways
    sw = [r for r in cr.runs_of('dense', graph_dir) if 'southwest' in r.name][0].graph.h
    assert sw['grid_min_lat'] < -33 and sw['grid_min_lon'] < -70
    og = [r for r in cr.runs_of('dense', graph_dir) if 'origin' in r.name][0].graph
    assert og.h['grid_min_lat'] < 0 < float(og.node_ll[0::2].max())
    assert og.h['grid_min_lon'] < 0 < float(og.node_ll[1::2].max())


def test_border_windows(graph_dir):
    run, = cr.runs_of('border', graph_dir)
    wins = [cr.window(run.graph, p[0], p[1], r) for p, r in zip(run.probes, run.radii())]
    assert set(run.radii()) == {cr.BORDER_RADIUS}
    assert {(16, 16), (16, 17), (17, 16), (17, 17), (1, 16), (16, 1)} <= set(wins), wins
    kinds = [cr.path_of(*w) for w in wins]
    # one group of a k_candidates<2> wave on the window path, the other cell by cell, both ways round
    pairs = {(kinds[o[s]], kinds[o[s + 1]]) for o in cr.orders(len(wins)).values() for s in range(0, len(o) - 1, 2)}
    assert ('win', 'slow') in pairs and ('slow', 'win') in pairs, pairs
    found = [c[3] for c in run.expected()]
    # (16, 16) and the wider windows around the hub see every edge; outside the four sides some, off the corners none
    assert [f for f, w in zip(found, wins) if min(w) >= 16] == [40, 40, 40, 40]
    assert sorted(found)[:6] == [0] * 6 and sorted(found)[6:10] == [6] * 4, found


def test_corner_cells_own_candidates(graph_dir):
    """The first and the last cell of a cell-by-cell window (and its other two corners) each
    report a candidate: a loop over the cells that starts late or stops early loses one.  (On a
    grid of square cells the corner cells of a window of more than 16 cells lie outside the
    radius, and the rim of the grid is empty: only a short and wide window has such cells.)"""
    run, = cr.runs_of('corner', graph_dir)
    geo = mref.Geometry(run.graph)
    la, lo = run.probes[0]
    rows, cols = cr.window(run.graph, la, lo, cr.CORNER_RADIUS)
    assert rows == 2 and cols > cr.KWIN and cr.path_of(rows, cols) == 'slow'
    r0, c0 = cr.window_origin(run.graph, la, lo, cr.CORNER_RADIUS)
    h = run.graph.h
    assert r0 > 0 and c0 > 0 and r0 + rows < h['grid_rows'] and c0 + cols < h['grid_cols']   # not clamped
    edges = run.expected()[0][0]
    assert sorted(edges) == [0, 1, 2, 3, 4]
    own = {e: cr.owner_cell(run.graph, geo, e, la, lo) for e in edges}
    cells = {e: (own[e][0] - r0) * cols + own[e][1] - c0 for e in edges}
    assert [cells[e] for e in range(4)] == [0, cols, cols - 1, rows * cols - 1], (cells, rows, cols)
    # the second probe's box ends a column further east (its last cell is empty), the third sits in the southern row
    assert cr.window(run.graph, *run.probes[1], cr.CORNER_RADIUS) == (2, cols + 1)
    assert [len(c[0]) for c in run.expected()] == [5, 5, 5]
    assert cr.owner_cell(run.graph, geo, 4, *run.probes[2])[0] == r0 + 1 > \
        cr.window_origin(run.graph, *run.probes[2], cr.CORNER_RADIUS)[0] == r0


def test_poly_hands_over_to_shape_ll(graph_dir):
    runs = cr.runs_of('poly', graph_dir)
    g = runs[0].graph
    geo = mref.Geometry(g)
    assert np.diff(g.edge_shape).tolist() == list(cr.POLY_POINTS)
    nf = len(cr.POLY_FRACS)
    for e, n in enumerate(cr.POLY_POINTS):
        seg = [cr.nearest_segment(geo, e, *runs[0].probes[e * nf + i]) for i in range(nf)]
        if n >= 5:   # segment 3 ends at the first point read from shape_ll
            assert min(seg) < 3 and 3 in seg, (n, seg)
        if n >= 6:   # (an edge of five points has no segment after it)
            assert max(seg) > 3, (n, seg)
        assert seg == sorted(seg) and seg[0] <= 1 and seg[-1] >= n - 3, (n, seg)
    found = [c[3] for c in runs[0].expected()]
    assert max(found) == 8 and min(found) >= 5   # the middle lines' probes reach all eight edges
    assert [r.over['max_candidates'] for r in runs] == [32, 3]
    # the 70-point edge is a candidate of probes beside every other line
    assert all(any(7 in runs[0].expected()[e * nf + i][0] for i in range(nf)) for e in range(3, 8))


def test_exact_radius(graph_dir):
    at, below = cr.runs_of('exact_radius', graph_dir)
    for (r, b), sec_at, sec_below, i in zip(cr.exact_radii(at.graph), ('auto', 'bicycle'), ('auto', 'bicycle'), (0, 1)):
        best = mref.project(mref.Geometry(at.graph), 0, *at.probes[i])[0]
        assert b < r and b * b < best <= r * r
        assert r * r == best   # the distance is exactly the radius: `best <= r2` is taken with equality
        assert at.sections[sec_at]['search_radius'] == r and below.sections[sec_below]['search_radius'] == b
        assert at.radii()[i] == r and below.radii()[i] == b
    assert [c[3] for c in at.expected()] == [1, 1] and [c[3] for c in below.expected()] == [0, 0]
    assert 29 < at.radii()[0] < 31 and 59 < at.radii()[1] < 61


def test_modes_mix_in_every_pair(graph_dir):
    acc, plain = cr.runs_of('modes', graph_dir)
    assert acc.accuracy is not None and plain.accuracy is None
    for run in (acc, plain):
        for name, o in cr.orders(len(run.probes)).items():
            m = [run.modes[i] for i in o]
            assert all(m[s] != m[s + 1] for s in range(0, len(m) - 1, 2)), (name, m)
        assert sorted({_kmax(run, i) for i in range(len(run.probes))}) == [5, 17, 32]
    assert len(set(acc.radii())) >= 4 and sorted(set(acc.radii())) == [20.0, 28.5, 35.0, 50.0, 60.0, 100.0]
    assert sorted(set(plain.radii())) == [20.0, 35.0, 50.0]
    assert {a for a in acc.accuracy} == set(cr.MODES_ACCURACY) and min(cr.MODES_ACCURACY) < 0
    # per-mode kmax: a state of every mode is cut at its own
    for m, k in ((0, 32), (1, 5), (2, 17)):
        assert any(c[3] > k and len(c[0]) == k for c, mm in zip(acc.expected(), acc.modes) if mm == m), m
