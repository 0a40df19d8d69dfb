"""Edge traversals and per-edge speed entries without a GPU: the
interface (exports, flag, struct layout, the no-batch error), invariants of the restatement
tests/edge_traversals_ref.py on the oracle's results, its anchors to what the oracle itself
computes (segment start and end times, route_edge), its link to the matched points (K12),
what the GPU test's batches cover, and known answers on hand-built roads at latitude 0."""
import ctypes
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from reporter_amd import _lib
from reporter_amd.graphfile import GraphFile
from tests import edge_traversals_ref as ref
from tests import matched_points_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}
# (batch, configuration) of the invariants, the anchor and the K12 link
BATCHES = [('ragged', 'gtt'), ('ragged', 'deployed'), ('city', 'gtt'), ('city', 'deployed250')]


def oracle_traversals(batch, cfg, graph_dir):
    """(graph, traces, the oracle's result, the restatement's traversals, the builder's extras),
    computed once; callers leave them unchanged."""
    key = (batch, cfg)
    if key not in _CACHE:
        extras = ()
        if batch == 'ragged':
            from tests import ragged
            path, tr, want, _ = ragged.oracle_result('ragged_city', cfg, graph_dir)
        else:
            built = (ref.kat3 if batch == 'kat3' else getattr(mref, batch))(graph_dir)
            path, tr, extras = built[0], built[1], built[2:]
            prm = po.params(**{k: float(v) for k, v in mref.OPTIONS[cfg].items()})
            want = po.match_batch(po.Graph(path), tr, prm, threads=8)
        G = GraphFile(path)
        _CACHE[key] = (G, tr, want, ref.traversals(want, tr, G), extras)
    return _CACHE[key]


# ---- interface ----------------------------------------------------------------------------
def test_exports_and_flag():
    L = _lib.lib()
    for name in ('otr_edge_traversals', 'otr_edge_observations'):
        assert name in _lib.EXPORTS and hasattr(L, name)
    hdr = open(os.path.join(ROOT, 'include', 'otr.h')).read()
    assert '#define OTR_BATCH_EDGE_TRAVERSALS 64' in hdr
    assert _lib.OTR_BATCH_EDGE_TRAVERSALS == 64
    for name in ('otr_edge_traversals', 'otr_edge_observations', 'otr_traversal_result'):
        assert name in hdr


def test_traversal_result_layout_against_c_header(tmp_path):
    """The ctypes mirror of otr_traversal_result has the C compiler's size and offsets."""
    import shutil
    import subprocess
    if not shutil.which('gcc'):
        pytest.skip('no C compiler')
    cname, cls = 'otr_traversal_result', _lib.TraversalResult
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "otr.h"', 'int main(void) {',
            'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for f in cls._fields_:
        prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    prog.append('return 0; }')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(prog))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls) == 24 + 22 * 8
    assert [f[0] for f in cls._fields_[4:15]] == list(ref.FIELDS)
    assert [f[0] for f in cls._fields_[15:]] == ['d_' + k for k in ref.FIELDS]
    for f in cls._fields_:
        assert int(got['%s.%s' % (cname, f[0])]) == getattr(cls, f[0]).offset, f[0]


def test_no_batch_is_a_bad_request():
    from reporter_amd import matcher as M
    m = M.Matcher()
    r = _lib.TraversalResult()
    rc = _lib.lib().otr_edge_traversals(m._h, ctypes.byref(r))
    assert rc == _lib.OTR_BAD_REQUEST == 400
    assert 'OTR_BATCH_EDGE_TRAVERSALS' in _lib.last_error()
    ptr, n = ctypes.c_void_p(), ctypes.c_int64()
    rc = _lib.lib().otr_edge_observations(m._h, 3600, ctypes.byref(ptr), ctypes.byref(n))
    assert rc == 400 and 'OTR_BATCH_EDGE_TRAVERSALS' in _lib.last_error()
    with pytest.raises(RuntimeError, match='OTR_BATCH_EDGE_TRAVERSALS'):
        m.edge_traversals()
    with pytest.raises(RuntimeError, match='OTR_BATCH_EDGE_TRAVERSALS'):
        m.edge_observations()


# ---- invariants of the restatement --------------------------------------------------------
def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize('batch,cfg', BATCHES)
def test_reference_invariants(batch, cfg, graph_dir):
    _, tr, want, tv, _ = oracle_traversals(batch, cfg, graph_dir)
    assert len(tv['trace_off']) == tr.n_traces + 1 and tv['trace_off'][0] == 0
    n = int(tv['trace_off'][-1])
    assert n > 0 and all(len(tv[k]) == n for k in ref.FIELDS[1:])
    roff = np.asarray(want['trace_route_off'], np.int64)
    for t in range(tr.n_traces):   # the traversal edges are route_edge without its separators
        r = np.asarray(want['route_edge'][roff[t]:roff[t + 1]], np.uint32)
        a, b = int(tv['trace_off'][t]), int(tv['trace_off'][t + 1])
        assert tv['edge'][a:b].tolist() == r[r != mref.NO_EDGE].tolist(), t
    assert (tv['t_enter'] <= tv['t_exit']).all() and (tv['s0_mm'] <= tv['s1_mm']).all()
    assert ((tv['f0'] >= 0.0) & (tv['f0'] <= 1.0) & (tv['f1'] >= 0.0) & (tv['f1'] <= 1.0)).all()
    covered = 0
    for sp in tv['subpaths']:
        a, k = sp['first'], sp['n']
        if len(sp['states']) < 2:
            assert k == 0
            continue
        assert k >= 1 and (tv['first_state'][a:a + k] == sp['states'][0]).all()
        assert tv['s0_mm'][a] == 0 and tv['s1_mm'][a + k - 1] == sp['pos'][-1]
        assert (tv['s1_mm'][a:a + k - 1] == tv['s0_mm'][a + 1:a + k]).all()
        assert (_bits(tv['t_exit'][a:a + k - 1]) == _bits(tv['t_enter'][a + 1:a + k])).all()
        assert (tv['f0'][a + 1:a + k] == 0.0).all() and (tv['f1'][a:a + k - 1] == 1.0).all()
        covered += k
    assert covered == n


# ---- the anchor to the oracle: K7's segments are groups of traversals ----------------------
@pytest.mark.parametrize('batch,cfg', BATCHES)
def test_segment_times_are_traversal_times(batch, cfg, graph_dir):
    G, tr, want, tv, _ = oracle_traversals(batch, cfg, graph_dir)
    soff = np.asarray(want['trace_seg_off'], np.int64)
    n_seg = checked_start = checked_end = 0
    for t in range(tr.n_traces):
        a, b = int(tv['trace_off'][t]), int(tv['trace_off'][t + 1])
        groups = []   # (first, last) traversal of each group
        for j in range(a, b):
            if j == a or tv['first_state'][j] != tv['first_state'][j - 1] or \
                    not ref.group_continues(G, int(tv['edge'][j - 1]), int(tv['edge'][j])):
                groups.append([j, j])
            else:
                groups[-1][1] = j
        assert len(groups) == soff[t + 1] - soff[t], t
        for (first, last), s in zip(groups, range(int(soff[t]), int(soff[t + 1]))):
            n_seg += 1
            st, en = float(want['seg_start'][s]), float(want['seg_end'][s])
            if st != -1.0:
                checked_start += 1
                assert _bits(st) == _bits(tv['t_enter'][first]), (t, s)
            if en != -1.0:
                checked_end += 1
                assert _bits(en) == _bits(tv['t_exit'][last]), (t, s)
    print('%s/%s: %d segments, %d starts and %d ends equal' % (batch, cfg, n_seg, checked_start, checked_end))
    assert 2 * checked_start >= n_seg and 2 * checked_end >= n_seg
    if (batch, cfg) == ('ragged', 'gtt'):
        assert (n_seg, checked_start, checked_end) == (3312, 2134, 2239)


# ---- the link to K12 ------------------------------------------------------------------------
@pytest.mark.parametrize('batch,cfg', [('ragged', 'gtt'), ('city', 'gtt'), ('city', 'deployed250')])
def test_matched_points_lie_in_their_traversals(batch, cfg, graph_dir):
    G, tr, want, tv, _ = oracle_traversals(batch, cfg, graph_dir)
    pts = mref.matched_points(want, tr, G)
    by_state = {}   # state -> its sub-path
    for sp in tv['subpaths']:
        for s in sp['states']:
            by_state[s] = sp
    checked = alone = 0
    for i in np.flatnonzero(pts['kind'] > 0):
        sp = by_state[int(pts['state'][i])]
        if len(sp['states']) < 2:
            alone += 1
            assert sp['n'] == 0 and pts['kind'][i] == 1
            continue
        a, k = sp['first'], sp['n']
        e, x = int(pts['edge'][i]), int(pts['pos_mm'][i])
        assert any(int(tv['edge'][j]) == e and tv['s0_mm'][j] <= x <= tv['s1_mm'][j] for j in range(a, a + k)), i
        checked += 1
    print('%s/%s: %d matched probes in a traversal, %d alone in their sub-path' % (batch, cfg, checked, alone))
    assert checked > 1000


# ---- what the ragged batch covers -----------------------------------------------------------
def test_ragged_covers_the_traversal_shapes(graph_dir):
    _, tr, _, tv, _ = oracle_traversals('ragged', 'gtt', graph_dir)
    per = np.diff(tv['trace_off'])
    zero = int((tv['s0_mm'] == tv['s1_mm']).sum())
    returns = sum(sp['returns'] for sp in tv['subpaths'])
    single = sum(1 for sp in tv['subpaths'] if sp['n'] == 1)
    print('per trace max %d, above 128: %d, none: %d; zero-length %d, returns %d, single %d'
          % (per.max(), (per > 128).sum(), (per == 0).sum(), zero, returns, single))
    assert per.max() > 128          # a trace beyond two 64-lane rounds
    assert (per == 0).any()
    assert zero > 0 and returns > 0 and single > 0
    assert (int(per.max()), int((per > 128).sum()), int((per == 0).sum()), zero, returns, single) == \
        (526, 16, 5, 93, 5, 57)


# ---- known answers at latitude 0 ------------------------------------------------------------
FTOL, TTOL = 1e-9, 1e-6


def _rows(tv, t):
    a, b = int(tv['trace_off'][t]), int(tv['trace_off'][t + 1])
    return [(int(tv['edge'][j]), float(tv['f0'][j]), float(tv['f1'][j]), int(tv['s0_mm'][j]), int(tv['s1_mm'][j]),
             float(tv['t_enter'][j]) - ref.T0, float(tv['t_exit'][j]) - ref.T0) for j in range(a, b)]


def _check(rows, want):
    assert len(rows) == len(want), rows
    for got, w in zip(rows, want):
        assert got[0] == w[0] and got[3] == w[3] and got[4] == w[4], (got, w)
        assert abs(got[1] - w[1]) < FTOL and abs(got[2] - w[2]) < FTOL, (got, w)
        assert abs(got[5] - w[5]) < TTOL and abs(got[6] - w[6]) < TTOL, (got, w)


def test_kat_traversals(graph_dir):
    _, tr, _, tv, (ids,) = oracle_traversals('kat', 'gtt50', graph_dir)
    e0, e1 = ids
    _check(_rows(tv, 0), [(e0, 0.1, 1.0, 0, 100188, 0.0, 9.0), (e1, 0.0, 0.9, 100188, 200376, 9.0, 18.0)])
    _check(_rows(tv, 1), [(e0, 0.1, 0.7, 0, 66792, 0.0, 6.0)])
    _check(_rows(tv, 2), [(e0, 0.7, 1.0, 0, 33396, 0.0, 3.0), (e1, 0.0, 0.3, 33396, 66792, 3.0, 6.0)])
    # trace 3: its 66 m step in 2 s breaks the route-time bound: two one-state sub-paths
    _check(_rows(tv, 3), [])
    assert tv['way'].tolist() == [1] * len(tv['way']) and (tv['seg_id'] == ref.NO_ID).all()
    assert tv['first_state'][0] == 0


def test_kat3_traversals_and_entries(graph_dir):
    G, tr, _, tv, (ids,) = oracle_traversals('kat3', 'gtt50', graph_dir)
    e0, e1, e2 = ids
    times = {0: (0.0, 0.0, 0.0, 0.0), 1: (0.0, 5.0, 15.0, 20.0), 2: (0.0, 5.0, 10.0, 10.0)}
    for t, (a, b, c, d) in times.items():
        _check(_rows(tv, t), [(e0, 0.5, 1.0, 0, 55660, a, b), (e1, 0.0, 1.0, 55660, 166980, b, c),
                              (e2, 0.0, 0.5, 166980, 222640, c, d)])
    assert tv['way'].tolist() == [1, 2, 3] * 3
    obs = ref.observations(tv, G, 3600)
    assert obs.tolist() == [(13824702808064, e1, e2, 2, 1), (13824702808064, e1, e2, 4, 1)]
    assert ref.observations(tv, G, 0).tolist() == obs.tolist()   # quantisation <= 0: 3600


def test_observations_on_a_hand_made_list():
    class Graph:
        edge_attr = np.array([0 << 11, 1 << 11, 2 << 11, 2 << 11, 0], np.uint32)
    t0 = float(ref.T0 + 7200)
    #            complete   partial    dt == 0.5   fast (capped)  last of its sub-path  another sub-path
    tv = {'edge': np.array([0, 1, 2, 3, 4, 1], np.uint32),
          'first_state': np.array([10, 10, 10, 10, 10, 20], np.int64),
          'f0': np.array([0.0, 0.25, 0.0, 0.0, 0.0, 0.0]), 'f1': np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0]),
          's0_mm': np.array([0, 100000, 200000, 300000, 1300000, 0], np.int64),
          's1_mm': np.array([100000, 200000, 300000, 1300000, 1400000, 50000], np.int64),
          't_enter': np.array([t0, t0 + 10, t0 + 20, t0 + 20.5, t0 + 30.5, t0 + 3599.5]),
          't_exit': np.array([t0 + 10, t0 + 20, t0 + 20.5, t0 + 30.5, t0 + 40.5, t0 + 3609.5])}
    hour = (ref.T0 + 7200) // 3600
    obs = ref.observations(tv, Graph, 3600)
    assert obs.tolist() == [
        ((hour << 25) | (0 << 22), 0, 1, 1, 1),                          # 100 m in 10 s: 36 km/h
        ((hour << 25) | (2 << 22), 3, 4, 7, 1),                          # 1 km in 10 s: 360 km/h, bin 7
        ((hour << 25) | (0 << 22), 4, ref.INVALID_SEGMENT_ID, 1, 1),     # the sub-path ends here
        ((hour << 25) | (1 << 22), 1, ref.INVALID_SEGMENT_ID, 0, 1)]     # 50 m in 10 s, entered in this hour
    assert ref.observations(tv, Graph, 1800)['file'][0] == ((ref.T0 + 7200) // 1800) << 25


def test_edge_speeds_figures():
    """tools/edge_speeds.figures on a hand-made result: counts, and the true edges found per trace."""
    from reporter_amd.tools.edge_speeds import figures
    tv = {'trace_off': np.array([0, 3, 3, 4], np.int64), 'edge': np.array([7, 8, 9, 5], np.uint32),
          'f0': np.array([0.5, 0.0, 0.0, 0.2]), 'f1': np.array([1.0, 1.0, 0.5, 0.4]),
          's0_mm': np.array([0, 10, 20, 0], np.int64), 's1_mm': np.array([10, 20, 20, 7], np.int64)}
    truth = np.array([7, 7, 8, 6, 9, 4, 4, 5, 5], np.uint32)     # traces of 5, 2 and 2 probes
    f = figures(tv, truth, np.array([0, 5, 7, 9], np.int64))
    assert (f['traversals'], f['complete'], f['complete_share'], f['zero_length']) == (4, 1, 0.25, 1)
    assert f['true_edges'] == 6 and f['true_edge_share'] == round(4 / 6, 6)   # 7, 8, 9 of 7, 8, 6, 9; none of 4; 5
    assert f['true_edge_share_trace_mean'] == round((0.75 + 0.0 + 1.0) / 3, 6)
