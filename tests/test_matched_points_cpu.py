"""Matched points without a GPU: what the batches of
tests/test_gpu_matched_points.py cover (pinned on the oracle's results), invariants of the
reference tests/matched_points_ref.py on them, known answers on hand-built graphs at
latitude 0, and the interface (export, struct layout, the no-batch error)."""
import ctypes
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from reporter_amd import _lib
from reporter_amd.graphfile import GraphFile
from tests import matched_points_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CITY_CONFIGS = ('gtt', 'deployed', 'gtt250', 'deployed250')
_CACHE = {}


def oracle_points(builder, cfg, graph_dir):
    """(traces, the oracle's result, the reference's points) of a batch under OPTIONS[cfg],
    computed once; callers leave them unchanged."""
    key = (builder.__name__, cfg)
    if key not in _CACHE:
        built = builder(graph_dir)
        path, tr = built[0], built[1]
        prm = po.params(**{k: float(v) for k, v in ref.OPTIONS[cfg].items()})
        want = po.match_batch(po.Graph(path), tr, prm, threads=8)
        _CACHE[key] = (tr, want, ref.matched_points(want, tr, GraphFile(path)), built[2:])
    return _CACHE[key]


# ---- coverage of the GPU test's batches ---------------------------------------------------
def test_city_default_covers_all_kinds(graph_dir):
    tr, _, pts, _ = oracle_points(ref.city, 'gtt', graph_dir)
    kind = pts['kind']
    assert len(kind) == tr.n_probes == 1920
    assert (kind == 0).any() and (kind == 1).any() and (kind == 2).any()
    assert sum(g['clamped'] for g in pts['gaps']) > 0
    assert sum(g['moved'] for g in pts['gaps']) > 0


@pytest.mark.parametrize('cfg', ['gtt250', 'deployed250'])
def test_city_250_covers_long_gaps_and_many_pieces(cfg, graph_dir):
    _, _, pts, _ = oracle_points(ref.city, cfg, graph_dir)
    gaps = pts['gaps']
    assert max(len(g['probes']) for g in gaps) > 64        # a gap beyond a 64-probe chunk
    assert max(len(g['pieces']) for g in gaps) >= 4
    assert sum(g['clamped'] for g in gaps) > 0 and sum(g['moved'] for g in gaps) > 0
    kind = pts['kind']
    assert (kind == 0).any() and (kind == 1).any() and (kind == 2).any()


def test_ragged_covers_the_trace_shapes(graph_dir):
    from tests import ragged
    path, tr, want, _ = ragged.oracle_result('ragged_city', 'gtt', graph_dir)
    pts = ref.matched_points(want, tr, GraphFile(path))
    n = np.diff(tr.offsets)
    assert (n == 0).any() and (n == 1).any()
    cov = ragged.coverage(want, tr)
    assert any(s > 0 and a == 0 for s, a in zip(cov['states'], cov['active']))   # a trace with no active state
    assert max(len(b) for b in cov['breaks']) > 60
    kind = pts['kind']
    assert (kind == 0).any() and (kind == 1).any()
    for t in range(tr.n_traces):   # a trace without an active state has no matched probe
        if cov['active'][t] == 0:
            assert (kind[tr.offsets[t]:tr.offsets[t + 1]] == 0).all()


def test_arc_walks_past_64_shape_segments(graph_dir):
    path = ref.arc(graph_dir)[0]
    G = GraphFile(path)
    assert int(np.diff(G.edge_shape).max()) - 1 > 100
    tr, _, pts, _ = oracle_points(ref.arc, 'gtt50', graph_dir)
    long_edge = int(np.argmax(np.diff(G.edge_shape)))
    on = pts['edge'] == long_edge
    assert (pts['kind'][on] == 2).sum() > 20 and (pts['kind'][on] == 1).sum() > 5
    assert (pts['kind'] > 0).all()
    # 3.005 m beside the arc; the shape points are stored in micro-degrees (up to 7.9 cm off,
    # diagonally), the probes rounded to 1e-7 degrees (0.8 cm) and a chord's sagitta is 0.8 cm
    assert np.abs(pts['dist'][on] - 3.005).max() < 0.15


# ---- invariants ---------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', CITY_CONFIGS)
def test_reference_invariants(cfg, graph_dir):
    _, _, pts, _ = oracle_points(ref.city, cfg, graph_dir)
    assert ((pts['frac'] >= 0.0) & (pts['frac'] <= 1.0)).all()
    un = pts['kind'] == 0
    assert (pts['edge'][un] == ref.NO_EDGE).all() and (pts['state'][un] == -1).all() and (pts['pos_mm'][un] == -1).all()
    for k in ('frac', 'lat', 'lon', 'dist'):
        assert (pts[k][un] == 0.0).all()
    assert (pts['dist'][~un] >= 0.0).all()
    for g in pts['gaps']:
        p = [g['pos_a']] + [int(pts['pos_mm'][i]) for i in g['probes']] + [g['pos_b']]
        assert all(x <= y for x, y in zip(p, p[1:])), g
        edges = {e for e, _, _ in g['pieces']}
        for i in g['probes']:
            assert pts['kind'][i] == 2 and int(pts['edge'][i]) in edges and pts['state'][i] == g['a']


# ---- known answers at latitude 0 ----------------------------------------------------------
TOL = 1e-9   # degrees / fraction units: 0.1 mm, far above rounding, far below a wrong segment or piece


@pytest.fixture(scope='module')
def kat(graph_dir):
    tr, _, pts, (ids,) = oracle_points(ref.kat, 'gtt50', graph_dir)
    return tr, pts, ids


def _trace(tr, pts, t):
    a, b = int(tr.offsets[t]), int(tr.offsets[t + 1])
    return {k: pts[k][a:b] for k in ref.FIELDS}, tr.lon[a:b]


def test_kat_two_collinear_edges(kat):
    tr, pts, (e0, e1) = kat
    p, lon = _trace(tr, pts, 0)
    assert p['kind'].tolist() == [1, 2, 2, 1, 2, 2, 1, 2, 2, 1]
    assert p['edge'].tolist() == [e0] * 5 + [e1] * 5
    want_frac = np.where(lon < 0.001, lon / 0.001, (lon - 0.001) / 0.001)
    assert np.abs(p['frac'] - want_frac).max() < TOL
    assert np.abs(p['lat']).max() < TOL and np.abs(p['lon'] - lon).max() < TOL
    assert np.abs(p['dist'] - ref.KAT_NORTH * ref.KM).max() < 1e-6
    assert (np.diff(p['pos_mm']) > 0).all() and p['pos_mm'][0] == 0
    assert p['state'].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3]


def test_kat_step_backwards_is_clamped_to_the_cursor(kat):
    tr, pts, (e0, _) = kat
    p, lon = _trace(tr, pts, 1)
    assert p['kind'].tolist() == [1, 2, 2, 1] and p['edge'].tolist() == [e0] * 4
    assert abs(p['frac'][1] - 0.4) < TOL
    assert p['frac'][2] == p['frac'][1] and p['lon'][2] == p['lon'][1] and p['pos_mm'][2] == p['pos_mm'][1]
    assert abs(p['lon'][2] - 0.0004) < TOL   # not its own projection at 0.0003


def test_kat_later_piece_keeps_the_cursor(kat):
    tr, pts, (e0, e1) = kat
    p, _ = _trace(tr, pts, 2)
    assert p['kind'].tolist() == [1, 2, 2, 1]
    assert p['edge'].tolist() == [e0, e1, e1, e1]
    assert abs(p['frac'][1] - 0.05) < TOL and abs(p['lon'][1] - 0.00105) < TOL
    assert p['frac'][2] == p['frac'][1] and p['lon'][2] == p['lon'][1]   # nearest to e0, but never backwards


def test_kat_probe_after_the_last_active_state(kat):
    tr, pts, _ = kat
    p, _ = _trace(tr, pts, 3)
    assert p['kind'].tolist() == [1, 1, 0, 0]
    assert p['edge'][2] == ref.NO_EDGE and p['state'][2] == -1 and p['pos_mm'][2] == -1 and p['dist'][2] == 0.0


def test_match_quality_figures():
    """tools/match_quality.quality on a hand-made result: shares over the matched kinds only."""
    from reporter_amd.tools.match_quality import quality
    pts = {'kind': np.array([1, 1, 2, 2, 2, 0], np.uint8), 'edge': np.array([7, 8, 9, 9, 5, ref.NO_EDGE], np.uint32),
           'dist': np.array([1.0, 3.0, 2.0, 2.0, 2.0, 0.0])}
    q = quality(pts, np.array([7, 7, 9, 9, 9, 4], np.uint32))
    assert (q['state_probes'], q['interpolated_probes'], q['unmatched_probes']) == (2, 3, 1)
    assert q['state_true_edge_share'] == 0.5 and q['interpolated_true_edge_share'] == round(2 / 3, 6)
    assert q['matched_true_edge_share'] == 0.6 and q['dist_mean_m'] == 2.0


# ---- interface ----------------------------------------------------------------------------
def test_export_and_flag():
    assert 'otr_matched_points' in _lib.EXPORTS and hasattr(_lib.lib(), 'otr_matched_points')
    hdr = open(os.path.join(ROOT, 'include', 'otr.h')).read()
    assert '#define OTR_BATCH_MATCHED_POINTS %d' % _lib.OTR_BATCH_MATCHED_POINTS in hdr
    assert _lib.OTR_BATCH_MATCHED_POINTS == 32


def test_point_result_layout_against_c_header(tmp_path):
    """The ctypes mirror of otr_point_result has the C compiler's size and offsets."""
    import shutil
    import subprocess
    if not shutil.which('gcc'):
        pytest.skip('no C compiler')
    cname, cls = 'otr_point_result', _lib.PointResult
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
    assert int(got[cname]) == ctypes.sizeof(cls) == 16 + 16 * 8
    for f in cls._fields_:
        assert int(got['%s.%s' % (cname, f[0])]) == getattr(cls, f[0]).offset, f[0]


def test_no_batch_is_a_bad_request():
    from reporter_amd import matcher as M
    m = M.Matcher()
    r = _lib.PointResult()
    rc = _lib.lib().otr_matched_points(m._h, ctypes.byref(r))
    assert rc == _lib.OTR_BAD_REQUEST == 400
    assert 'OTR_BATCH_MATCHED_POINTS' in _lib.last_error()
    with pytest.raises(RuntimeError, match='OTR_BATCH_MATCHED_POINTS'):
        m.matched_points()
