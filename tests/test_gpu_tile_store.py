"""The tile store in HBM (K15, include/otr.h otr_tile_store_*) against its restatement
tests/tile_store_ref.py, by the bytes of the row arrays and the file table: the hand-built script
from host and from device arrays with flushes in between; rows that survive every other call on
the matcher; capacity and refusals; the city stream through the session store with add_session
after every push, in two chunkings; and finished rows through add_rows.  What the script covers
is pinned by tests/test_tile_store_cpu.py.  One child process per job."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import sessions_ref as R
from tests import tile_store_ref as TS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = TS.SCRIPT_Q
CHILD = r'''
import sys, pickle, time
sys.path.insert(0, %r)
graph_dir, dst, job = %r, %r, %r
import numpy as np
import torch
from reporter_amd import matcher as M
from reporter_amd import _lib
from reporter_amd import simple_reporter as sr
from reporter_amd.tools import gen
from tests import matched_points_ref as mref
from tests import sessions_ref as R
from tests import tile_store_ref as TS

Q = TS.SCRIPT_Q
NAMES = ['rep_off'] + [k for k, _ in TS.REPORT_TYPES]


def refused(f, *a, **kw):
    try:
        f(*a, **kw)
    except ValueError as e:
        return str(e)
    return None


def on_device(rep):
    """The reports dict as device pointers (the tensors are kept alive by the caller)."""
    keep = [torch.from_numpy(np.ascontiguousarray(rep[k]).view(np.int64 if rep[k].dtype == np.uint64 else rep[k].dtype)
                             .copy()).cuda() for k in NAMES]
    torch.cuda.synchronize()
    d = {k: (t.data_ptr() if t.numel() else 0) for k, t in zip(NAMES, keep)}
    d['n_windows'] = len(rep['rep_off']) - 1
    return d, keep


def tiny():
    path = gen.graph_path('tiny', graph_dir)
    M.configure(M.default_config(path, device=0))
    return path


out = {}
adds = TS.script_adds()
if job == 'scripted':
    tiny()
    m = M.Matcher()
    for privacy in (1, 2):
        for memory in ('host', 'device'):
            m.tile_store_open(1 << 16, Q, privacy)
            got = {'adds': [], 'flushes': []}
            for i, a in enumerate(adds):
                if memory == 'device':
                    d, keep = on_device(a)
                    got['adds'].append(m.tile_store_add_reports(d, device=True))
                else:
                    got['adds'].append(m.tile_store_add_reports(a))
                if i in TS.SCRIPT_FLUSH_AFTER:
                    got['flushes'].append(m.tile_store_flush())
            m.tile_store_close()
            out[(privacy, memory)] = got
elif job == 'persistence':
    path = tiny()
    m = M.Matcher()
    traces = gen.make_traces(path, 8, 40, 5, 8.0, 7)

    def batch():
        r = m.match_batch(traces, copy_out=True, tile_rows=True, tile_rules=_lib.OTR_TILE_RULES_STREAM, quantisation=Q)
        res = {k: np.asarray(v) for k, v in _lib.result_to_numpy(r).items()}
        return r, res

    r, out['before'] = batch()
    out['before_rows'] = sr.cull_rows(m, None, 1, device_ptr=r.d_rows, n=r.n_rows, rules=_lib.OTR_TILE_RULES_STREAM)
    m.tile_store_open(1 << 12, Q, 2)
    out['add0'] = m.tile_store_add_reports(adds[0])
    r, out['after'] = batch()
    out['after_rows'] = sr.cull_rows(m, None, 1, device_ptr=r.d_rows, n=r.n_rows, rules=_lib.OTR_TILE_RULES_STREAM)
    out['culled2'] = len(sr.cull_rows(m, None, 2, device_ptr=r.d_rows, n=r.n_rows))
    out['hist'] = len(sr.hist_reduce(m, r.d_rows, r.n_rows, privacy=1, rows_in=True))
    m.sessions_open(4, 4, report_dist=500.0, report_count=3, report_time=0, session_gap=60000)
    out['pushed'] = m.sessions_push(R.refusal_points([3, 3, 3, 3]))['n_windows']
    d, keep = on_device(adds[1])
    out['add1'] = m.tile_store_add_reports(d, device=True)
    out['add2'] = m.tile_store_add_reports(adds[2])
    out['flush'] = m.tile_store_flush()
elif job == 'capacity':
    tiny()
    m = M.Matcher()
    n0 = len(TS.rows_of(adds[0], Q))
    m.tile_store_open(n0, Q, 1)
    out['twice'] = refused(m.tile_store_open, 8, Q, 1)
    out['no_session'] = refused(m.tile_store_add_session)
    out['add0'] = m.tile_store_add_reports(adds[0])
    out['too_many'] = refused(m.tile_store_add_reports, adds[1])
    out['too_many_rows'] = refused(m.tile_store_add_rows, np.zeros(1, _lib.TILE_ROW))
    out['zero_windows'] = m.tile_store_add_reports(TS.reports_of([]))
    out['flush0'] = m.tile_store_flush()
    out['add1'] = m.tile_store_add_reports(adds[1])
    out['flush1'] = m.tile_store_flush()
    out['flush_empty'] = m.tile_store_flush()
    # a session result without windows: added once, refused twice; none after the store is gone
    m.sessions_open(4, 4)
    out['no_result'] = refused(m.tile_store_add_session)
    m.sessions_push({k: np.zeros(0, dt) for k, dt in R.POINT_TYPES})
    out['session_empty'] = m.tile_store_add_session()
    out['session_twice'] = refused(m.tile_store_add_session)
    m.sessions_close()
    out['session_closed'] = refused(m.tile_store_add_session)
    # a report with more buckets than any store holds is refused like any other add
    huge = TS.reports_of([[(TS.sid(1, 5, 1), TS.NO_ID, 1.0, 1e17, 10, 0)]])
    out['huge'] = refused(m.tile_store_add_reports, huge)
    out['bad_off'] = refused(m.tile_store_add_reports, dict(adds[1], rep_off=np.array([0, 2, 1], np.int64)))
    out['after_refusals'] = m.tile_store_flush()
    m.tile_store_close()
    out['closed'] = refused(m.tile_store_flush)
elif job == 'city':
    path, pts = R.city_stream(graph_dir)
    M.configure(M.default_config(path, **mref.OPTIONS['gtt']))
    m = M.Matcher()
    n = len(pts['key'])
    cuts = {'one': [0, n], 'seven': list(range(0, n, 7)) + [n]}
    end_ts = int(pts['timestamp'].max()) + R.CITY['session_gap'] + 1
    for case, privacy, shift in ((1, 1, 0), (2, 2, 0), ('shifted', 2, TS.CITY_SHIFT)):
        moved = dict(pts, time=pts['time'] + shift, timestamp=pts['timestamp'] + 1000 * shift)
        for name, c in cuts.items():
            t0 = time.perf_counter()
            m.sessions_open(**R.CITY)
            m.tile_store_open(1 << 16, Q, privacy)
            got = {'results': [], 'adds': []}
            for i in range(len(c) - 1):
                got['results'].append(m.sessions_push(R.take(moved, c[i], c[i + 1])))
                got['adds'].append(m.tile_store_add_session())
            got['punctuate'] = m.sessions_punctuate(end_ts + 1000 * shift)
            got['adds'].append(m.tile_store_add_session())
            got['flush'] = m.tile_store_flush()
            m.tile_store_close()
            m.sessions_close()
            got['seconds'] = time.perf_counter() - t0
            out[(case, name)] = got
else:
    tiny()
    m = M.Matcher()
    m.tile_store_open(1 << 12, Q, 1)
    for a in adds[:3]:
        m.tile_store_add_reports(a)
    fl = out['flush'] = m.tile_store_flush()
    out['add_device'] = m.tile_store_add_rows(device_ptr=fl['d_rows'], n=fl['n_rows'])
    out['again_device'] = m.tile_store_flush()
    out['add_host'] = m.tile_store_add_rows(fl['rows'])
    out['again_host'] = m.tile_store_flush()
    out['payloads'] = sr.stream_tile_payloads(fl, 'auto', 'reporter')
pickle.dump(out, open(dst, 'wb'))
print('tile store ok')
'''

_RUNS = {}


@pytest.fixture(scope='module')
def run_job(graph_dir, tmp_path_factory):
    def get(job):
        if job not in _RUNS:
            env = dict(os.environ)
            for k in ('OTR_VIT_SPLIT', 'OTR_TIERS', 'OTR_EST_K', 'OTR_LIB', 'OTR_SMALL_KEYS', 'OTR_SMALL_PATH_KEYS',
                      'OTR_TINY_KEYS'):
                env.pop(k, None)
            dst = str(tmp_path_factory.mktemp('tile_store') / (job + '.pkl'))
            t0 = time.perf_counter()
            p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, dst, job)], env=env,
                               capture_output=True, text=True, timeout=240)
            assert p.returncode == 0 and 'tile store ok' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
            print('child %s: %.1f s' % (job, time.perf_counter() - t0))
            with open(dst, 'rb') as f:
                _RUNS[job] = pickle.load(f)
        return _RUNS[job]
    return get


def _same(got, want):
    bad = TS.differing(got, want)
    assert not bad, bad


def _same_counts(got, want):
    for k in ('n_reports', 'n_valid', 'n_rows_added', 'n_rows'):
        assert got[k] == want[k], (k, got, want)


@pytest.mark.parametrize('memory', ['host', 'device'])
@pytest.mark.parametrize('privacy', [1, 2])
def test_scripted(privacy, memory, run_job):
    """The script's five adds and three flushes: every add's counts and every flush equal the
    restatement, from host arrays and from arrays in HBM."""
    got = run_job('scripted')[(privacy, memory)]
    want_adds, want_flushes = TS.script_flushes(privacy)
    assert len(got['adds']) == len(want_adds) and len(got['flushes']) == len(want_flushes) == 3
    for g, w in zip(got['adds'], want_adds):
        _same_counts(g, w)
    for g, w in zip(got['flushes'], want_flushes):
        _same(g, w)
    print('scripted privacy %d %s: rows in %s kept %s, files %s empty %s, add ms %s flush ms %s' % (
        privacy, memory, [f['n_rows_in'] for f in got['flushes']], [f['n_rows'] for f in got['flushes']],
        [f['n_files'] for f in got['flushes']], [f['n_files_empty'] for f in got['flushes']],
        [round(a['device_ms'], 3) for a in got['adds']], [round(f['device_ms'], 3) for f in got['flushes']]))


def _defined(res):
    out = dict(res)
    live = np.arange(res['cand_edge'].shape[1])[None, :] < res['cand_count'][:, None]
    for k in ('cand_edge', 'cand_p', 'cand_sqd'):
        out[k] = np.where(live, res[k], 0)
    return out


def test_rows_persist_across_other_calls(run_job):
    """Between two adds the matcher runs a batch with tile rows, two culls of them, a histogram
    reduce and a session push with a real match: the flush still holds every row added, and the
    batch computes what it computed before the store existed."""
    r = run_job('persistence')
    ref = TS.Store(1 << 12, Q, 2)
    adds = TS.script_adds()
    for name, a in zip(('add0', 'add1', 'add2'), adds):
        _same_counts(r[name], ref.add_reports(a))
    _same(r['flush'], ref.flush())
    assert r['pushed'] == 1 and r['hist'] > 0 and len(r['before_rows']) > 0 and r['culled2'] >= 0
    before, after = _defined(r['before']), _defined(r['after'])
    for k, a in before.items():
        b = after[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert r['before_rows'].tobytes() == r['after_rows'].tobytes()


def test_capacity_and_refusals(run_job):
    r = run_job('capacity')
    adds = TS.script_adds()
    n0 = len(TS.rows_of(adds[0], Q))
    ref = TS.Store(n0, Q, 1)
    _same_counts(r['add0'], ref.add_reports(adds[0]))           # fits exactly
    assert r['add0']['n_rows'] == n0
    assert r['too_many'] and 'max_rows' in r['too_many']
    assert r['too_many_rows'] and 'max_rows' in r['too_many_rows']
    assert r['zero_windows'] == dict(r['zero_windows'], n_reports=0, n_valid=0, n_rows_added=0, n_rows=n0)
    _same(r['flush0'], ref.flush())                             # exactly the first add
    _same_counts(r['add1'], ref.add_reports(adds[1]))           # after the flush the refused add fits
    _same(r['flush1'], ref.flush())
    empty = ref.flush()
    _same(r['flush_empty'], empty)
    assert r['flush_empty']['n_files'] == 0 and r['flush_empty']['row_off'].tolist() == [0]
    assert r['twice'] and 'already' in r['twice']
    for k in ('no_session', 'no_result', 'session_closed'):
        assert r[k] and 'otr_sessions_push' in r[k], k
    assert (r['session_empty']['n_reports'], r['session_empty']['n_rows']) == (0, 0)
    assert r['session_twice'] and 'already added' in r['session_twice']
    assert r['huge'] and 'max_rows' in r['huge']
    assert r['bad_off'] and 'rep_off' in r['bad_off']
    _same(r['after_refusals'], empty)
    assert r['closed'] and 'otr_tile_store_open' in r['closed']


@pytest.mark.parametrize('case', [1, 2, 'shifted'])
def test_city_stream_any_chunking(case, run_job):
    """Formatter -> sessions -> tiles on the city stream (R.city_stream, R.CITY, config gtt, q = 60)
    with real matching: add_session after every push and after the final punctuate, at privacy 1
    and 2 (cases 1 and 2).  Both chunkings flush to the same bytes, equal to the restatement fed
    with the same results in forward order.

    The stream yields three valid reports, at seconds 35.2-52.9, 28.4-40.0 and 8.5-14.7 of three
    different minutes (the oracle's and the device's figures agree), so its rows lie in three
    buckets but no report of it crosses a bucket boundary.  Case 'shifted' is the same stream
    with every time TS.CITY_SHIFT = 10 s later, at privacy 2: the first report then spans seconds
    45.2-62.9 and fans out into two rows in two files, which is asserted there."""
    r = run_job('city')
    privacy = 2 if case == 'shifted' else case
    flushes = {}
    for name in ('one', 'seven'):
        got = r[(case, name)]
        ref = TS.Store(1 << 16, Q, privacy)
        assert len(got['adds']) == len(got['results']) + 1 > 1
        for res, add in zip(got['results'], got['adds']):
            _same_counts(add, ref.add_reports(R.by_trigger(res)))
        _same_counts(got['adds'][-1], ref.add_reports(got['punctuate']))   # an eviction: rank order as it is
        arrival = ref.arrival_rows()
        want = ref.flush()
        _same(got['flush'], want)
        flushes[name] = got['flush']
        # the job proves something: more than one add (above), rows in more than one bucket
        n_valid = sum(a['n_valid'] for a in got['adds'])
        assert len(set((arrival['file'] >> np.uint64(25)).tolist())) > 1
        assert len(arrival) >= n_valid > 0
        if case == 'shifted':                                # a report with two or more rows
            assert len(arrival) > n_valid
        print('city %s %s: %d adds, %d reports, %d valid, %d rows in, %d kept, %d files (%d empty), add ms %.2f, '
              'flush ms %.2f, %.1f s' % (case, name, len(got['adds']), sum(a['n_reports'] for a in got['adds']),
                                         n_valid, want['n_rows_in'], want['n_rows'], want['n_files'],
                                         want['n_files_empty'], sum(a['device_ms'] for a in got['adds']),
                                         got['flush']['device_ms'], got['seconds']))
    _same(flushes['one'], flushes['seven'])


def test_finished_rows(run_job):
    """The kept rows of a flush put back through add_rows, from HBM and from the host, at privacy
    1: the flush is the rows given."""
    r = run_job('rows')
    fl = r['flush']
    _, want = TS.script_flushes(1)
    _same(fl, want[0])
    kept = np.diff(fl['row_off'])
    for add, again in (('add_device', 'again_device'), ('add_host', 'again_host')):
        assert r[add] == dict(r[add], n_reports=0, n_valid=0, n_rows_added=fl['n_rows'], n_rows=fl['n_rows'])
        _same(r[again], dict(fl, n_unclean=kept, n_rows_in=fl['n_rows'], n_files_empty=0))
    from oracle import tiles as T
    lines = T.stream_tiles(np.concatenate([TS.rows_of(a, Q) for a in TS.script_adds()[:3]]), 1, Q)
    header = ('segment_id,next_segment_id,duration,count,length,queue_length,minimum_timestamp,maximum_timestamp,'
              'source,vehicle_type')
    assert r['payloads'] == {k: header + ''.join(v) for k, v in lines.items()}
