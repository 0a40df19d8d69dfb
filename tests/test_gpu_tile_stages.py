"""The output stages on the GPU at their chunk and window edges: K8 k_histogram, K9 k_tile_rows
and K10 sort + cull on ragged_city and many_reports of tests/ragged.py, against the CPU
restatements oracle/tiles.py and oracle/hist.py from the oracle's reports (integers, compared
exactly).  many_reports has traces of 0, 1, 63, 64, 65, 127, 128, 129, 192 and more than 192
reports: K9's second and later chunks of 64 with the carried row base, K8's strides.  At 60 s
buckets a report gives up to three rows (a lane places more than one row, the simple and the
stream rules differ, most files have one to three rows); the histogram's window starts at an
aligned base, inside the batch's time range, and at bases that are no multiple of the
quantisation (include/otr.h: the histogram covers [base, base + hist_hours * quantisation)).
What the batches cover is pinned by tests/test_tile_stage_cases_cpu.py."""
import numpy as np
import pytest

from oracle import hist as oh
from oracle import tiles as ot
from oracle.compare import compare
from reporter_amd import _lib
from reporter_amd import matcher as M
from reporter_amd import simple_reporter as sr
from reporter_amd.tools import gen
from tests import ragged

pytestmark = pytest.mark.gpu

JOBS = [('ragged_city', 'gtt'), ('many_reports', 'gtt'), ('many_reports', 'deployed')]
GTT = [j for j in JOBS if j[1] == 'gtt']
QS = (3600, 60)
RULES = {'simple': _lib.OTR_TILE_RULES_SIMPLE, 'stream': _lib.OTR_TILE_RULES_STREAM}
PRIVACY = (1, 2, 3)
WINDOWS = [(b, q, w) for (b, q), ws in ragged.HIST_WINDOWS.items() for w in ws]


class _DevArr:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {'shape': (n,), 'typestr': typestr, 'data': (int(ptr), False), 'version': 2}


def _from_device(ptr, n, typestr):
    import torch
    if n == 0:
        return np.zeros(0, np.uint8 if typestr == '|u1' else np.int32)
    torch.cuda.synchronize()
    return torch.as_tensor(_DevArr(ptr, n, typestr), device='cuda').clone().cpu().numpy()


def _match(batch, cfg, graph_dir):
    """Everything the tests below compare, of one batch under one configuration: the device runs
    happen here, in order (the engine's configuration is the process's), the tests only compare."""
    path, tr = (ragged.CASES[batch][0] if batch in ragged.CASES else ragged.OTHER_BATCHES[batch])(graph_dir)
    M.configure(ragged.engine_config(path, cfg))
    m = M.Matcher()
    out = {'rows': {}, 'kept': {}, 'n_rows': {}, 'hist': {}}
    r = m.match_batch(tr, copy_out=True)
    out['res'] = {k: np.asarray(v).copy() for k, v in _lib.result_to_numpy(r).items()}
    out['status'] = int(r.status)
    out['n_rows'][3600] = int(out['res']['n_rows'])
    out['n_rows'][60] = int(m.match_batch(tr, copy_out=False, quantisation=60).n_rows)  # K8 counts the rows
    w = _lib.TILE_ROW.itemsize
    for q in QS:
        for name, rules in RULES.items():
            r = m.match_batch(tr, copy_out=False, tile_rows=True, tile_rules=rules, quantisation=q)
            n = int(r.n_rows)
            out['rows'][(q, name)] = (n, _from_device(r.d_rows, n * w, '|u1').view(_lib.TILE_ROW))
            if q == 60 and cfg == 'gtt':  # K10 from the rows in HBM
                for p in PRIVACY:
                    out['kept'][(name, p)] = sr.cull_rows(m, None, p, device_ptr=r.d_rows, n=n, rules=rules)
    if cfg == 'gtt':
        for q in QS:
            for name, rel, hours in ragged.HIST_WINDOWS[(batch, q)]:
                r = m.match_batch(tr, copy_out=False, quantisation=q, hist_base_time=gen.T_BEGIN + rel,
                                  hist_hours=hours)
                out['hist'][(q, name)] = (int(r.n_rows), int(r.hist_len),
                                          _from_device(r.d_hist, int(r.hist_len), '<i4'))
    m.close()
    return out


@pytest.fixture(scope='module')
def runs(graph_dir):
    return {(batch, cfg): _match(batch, cfg, graph_dir) for batch, cfg in JOBS}


def _want(batch, cfg, graph_dir):
    path, tr, want, _ = ragged.oracle_result(batch, cfg, graph_dir)
    first, last = ragged.trace_times(tr)
    return path, tr, want, first, last


_ROWS = {}


def _want_rows(batch, cfg, q, rules, graph_dir):
    """The restatement's rows, computed once per process (callers leave them unchanged)."""
    key = (batch, cfg, q, rules)
    if key not in _ROWS:
        _, _, want, first, last = _want(batch, cfg, graph_dir)
        _ROWS[key] = ot.rows_from_reports(want, first, last, q) if rules == 'simple' else \
            ot.stream_rows_from_reports(want, q)
    return _ROWS[key]


@pytest.mark.parametrize('batch,cfg', JOBS)
def test_result_equals_oracle(batch, cfg, runs, graph_dir):
    got = runs[(batch, cfg)]
    want = _want(batch, cfg, graph_dir)[2]
    errors, stats = compare(got['res'], want)
    assert not errors, errors
    assert got['status'] == 0 and stats['n_rep'] > 0


@pytest.mark.parametrize('rules', list(RULES))
@pytest.mark.parametrize('q', QS)
@pytest.mark.parametrize('batch,cfg', JOBS)
def test_device_rows_equal_restatement(batch, cfg, q, rules, runs, graph_dir):
    """K9: the rows in HBM, order included, and their number."""
    n, got = runs[(batch, cfg)]['rows'][(q, rules)]
    want = _want_rows(batch, cfg, q, rules, graph_dir)
    assert n == len(got) == len(want) > 100
    assert np.array_equal(got, want)


@pytest.mark.parametrize('q', QS)
@pytest.mark.parametrize('batch,cfg', JOBS)
def test_histogram_stage_counts_the_simple_rows(batch, cfg, q, runs, graph_dir):
    """K8 without tile rows: n_rows is the number of rows of the simple rules."""
    assert runs[(batch, cfg)]['n_rows'][q] == len(_want_rows(batch, cfg, q, 'simple', graph_dir))


@pytest.mark.parametrize('privacy', PRIVACY)
@pytest.mark.parametrize('rules', list(RULES))
@pytest.mark.parametrize('batch,cfg', GTT)
def test_device_cull_equals_restatement(batch, cfg, rules, privacy, runs, graph_dir):
    """K10 at 60 s buckets (many files of one to three rows) from the rows K9 left in HBM."""
    kept = runs[(batch, cfg)]['kept'][(rules, privacy)]
    rows = _want_rows(batch, cfg, 60, rules, graph_dir)
    if rules == 'simple':
        got, want = sr.rows_to_tiles(kept, 60), ot.tiles(rows, privacy, q=60)
    else:
        got = sr.rows_to_tiles(kept, 60, source='reporter', rules=_lib.OTR_TILE_RULES_STREAM)
        want = ot.stream_tiles(rows, privacy, q=60, source='reporter')
    assert got == want and (len(want) > 0 or privacy > 1)
    if privacy == 1:
        assert sum(len(v) for v in got.values()) == len(rows)


@pytest.mark.parametrize('batch,q,window', WINDOWS, ids=['%s-%d-%s' % (b, q, w[0]) for b, q, w in WINDOWS])
def test_device_histogram_window(batch, q, window, runs, graph_dir):
    """K8's dense histogram of a window [base, base + buckets * q): a row whose bucket starts
    before the base is left out, also when it starts less than one bucket before it."""
    from reporter_amd.graphfile import GraphFile
    name, rel, hours = window
    path, tr, res, first, last = _want(batch, 'gtt', graph_dir)
    G = GraphFile(path)
    idx = {int(s): i for i, s in enumerate(G.seg_id)}
    want, rows = oh.histogram(res, first, last, idx, len(G.seg_id), gen.T_BEGIN + rel, hours, q)
    n_rows, hist_len, got = runs[(batch, 'gtt')]['hist'][(q, name)]
    assert hist_len == hours * len(G.seg_id) * _lib.HIST_BINS
    got = got.reshape(hours, len(G.seg_id), _lib.HIST_BINS)
    print('%s q %d %s: device counts %d, restatement %d of %d rows' % (batch, q, name, int(got.sum()),
                                                                      int(want.sum()), rows))
    assert n_rows == rows == len(_want_rows(batch, 'gtt', q, 'simple', graph_dir))
    assert np.array_equal(got, want)
