"""The tile store's snapshot, restore and Segment.ListSerder records in HBM (K20, include/otr.h
otr_tile_store_open_ex .. otr_tile_store_restore_records) against the restatement
tests/tile_records_ref.py, byte for byte: exports of the hand-built script at several slice sizes,
restores from host and from unaligned device memory, every refusal, the map rules, snapshots, and
a streaming run stopped and resumed in another matcher.  One child process per job."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import tile_records_ref as X
from tests import tile_store_ref as TS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = TS.SCRIPT_Q
SIZES = (1, 3, 64, 65, 256)
SHIFTS = (0, 1, 4, 7)
CHILD = r'''
import sys, pickle
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
from tests import tile_records_ref as X
from tests import tile_store_ref as TS

Q = TS.SCRIPT_Q
SIZES = (1, 3, 64, 65, 256)
SHIFTS = (0, 1, 4, 7)
DEV = (('start', np.int64), ('tile_id', np.int64), ('slice', np.int32), ('rec_off', np.int64), ('name_off', np.int64))


def refused(f, *a, **kw):
    try:
        f(*a, **kw)
    except ValueError as e:
        return (str(e), getattr(e, 'result', None))
    return None


def tiny():
    path = gen.graph_path('tiny', graph_dir)
    M.configure(M.default_config(path, device=0))
    return path


def device_copies(rec):
    """The export's device arrays, copied back."""
    ns, nt = rec['n_slices'], rec['n_tiles']
    out = {k: _lib.device_to_numpy(rec['d_' + k], ns + (1 if k.endswith('_off') else 0), dt) for k, dt in DEV}
    out['bytes'] = _lib.device_to_numpy(rec['d_bytes'], rec['n_bytes'], np.uint8)
    out['names'] = _lib.device_to_numpy(rec['d_names'], rec['n_name_bytes'], np.uint8)
    out['map_bytes'] = _lib.device_to_numpy(rec['d_map_bytes'], 20 * nt, np.uint8)
    return out


def plain(rec):
    return {k: v for k, v in rec.items() if not k.startswith('d_')}


def on_device(rec, shift):
    """The records with every array in HBM, the bytes `shift` bytes into their allocation."""
    keep = []

    def up(a, sh=0):
        a = np.ascontiguousarray(a)
        t = torch.zeros(a.nbytes + sh + 8, dtype=torch.uint8, device='cuda')
        if a.nbytes:
            t[sh:sh + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
        keep.append(t)
        return t.data_ptr() + sh
    d = {'n_slices': rec['n_slices'], 'n_bytes': rec['n_bytes'], 'n_tiles': rec['n_tiles'],
         'slice_size': rec['slice_size']}
    for k, dt in DEV[:4]:
        d['d_' + k] = up(np.ascontiguousarray(rec[k], dt))
    d['d_bytes'] = up(rec['bytes'], shift)
    d['d_map_bytes'] = None if rec.get('map_bytes') is None else up(rec['map_bytes'], shift)
    torch.cuda.synchronize()
    return d, keep


def snap_arrays(s):
    return {k: s[k] for k in ('rows', 't0', 't1', 'n_rows', 'flags', 'quantisation')}


out = {}
adds = TS.script_adds()
if job == 'export':
    tiny()
    m = M.Matcher()
    for timed in (True, False):
        m.tile_store_open(1 << 16, Q, 2, times=timed)
        got = {'exports': [], 'flushes': [], 'adds': []}
        for i, a in enumerate(adds):
            got['adds'].append(m.tile_store_add_reports(a))
            if i in TS.SCRIPT_FLUSH_AFTER:
                if timed:
                    per = {}
                    for S in SIZES:
                        e = m.tile_store_export_records(S)
                        per[S] = (plain(e), device_copies(e))
                    got['exports'].append(per)
                got['flushes'].append(m.tile_store_flush())
        if timed:
            got['export_empty'] = plain(m.tile_store_export_records(3))
        m.tile_store_close()
        out['timed' if timed else 'plain'] = got
    for n in (257, 20001):
        m.tile_store_open(1 << 16, Q, 1, times=True)
        m.tile_store_add_reports(X.synthetic_file(n))
        e = m.tile_store_export_records(20000)
        out[n] = (plain(e), device_copies(e))
        m.tile_store_close()
elif job == 'restore':
    tiny()
    m = M.Matcher()
    m.tile_store_open(1 << 16, Q, 2, times=True)
    for a in adds[:3]:
        m.tile_store_add_reports(a)
    exports = {S: plain(m.tile_store_export_records(S)) for S in SIZES}
    out['flush'] = m.tile_store_flush()
    m.tile_store_add_reports(X.synthetic_file(20001))
    exports['synthetic'] = plain(m.tile_store_export_records(20000))
    out['flush_synthetic'] = m.tile_store_flush()
    m.tile_store_close()
    out['exports'] = exports
    for name, rec in exports.items():
        for timed in (True, False):
            sources = ['host'] + list(SHIFTS if name != 'synthetic' else (1,))
            for src in sources:
                m.tile_store_open(1 << 16, Q, 2, times=timed)
                if src == 'host':
                    res = m.tile_store_restore_records(rec)
                else:
                    d, keep = on_device(rec, src)
                    res = m.tile_store_restore_records(d, device=True)
                again = plain(m.tile_store_export_records(rec['slice_size'])) if timed else None
                out[(name, timed, src)] = (res, again, m.tile_store_flush())
                m.tile_store_close()
    # into a store that already holds rows
    m.tile_store_open(1 << 16, Q, 1, times=True)
    m.tile_store_add_reports(adds[3])
    out['append_result'] = m.tile_store_restore_records(exports[3])
    out['append_snapshot'] = snap_arrays(m.tile_store_snapshot())
    m.tile_store_close()
elif job == 'refusals':
    tiny()
    m = M.Matcher()
    pre = adds[4]
    n_pre = len(TS.rows_of(pre, Q))
    for name, rec, max_rows, reason, bad_slice, bad_tile in X.refusal_cases():
        for memory in ('host', 'device'):
            m.tile_store_open(max_rows + n_pre, Q, 1, times=True)
            m.tile_store_add_reports(pre)
            before = snap_arrays(m.tile_store_snapshot())
            if memory == 'host':
                r = refused(m.tile_store_restore_records, rec)
            else:
                d, keep = on_device(rec, 3)
                r = refused(m.tile_store_restore_records, d, device=True)
            out[(name, memory)] = (r, before, snap_arrays(m.tile_store_snapshot()))
            m.tile_store_close()
    # E_ROW: rows that are not what their reports give
    held = X.held_of(adds[:1], Q)
    m.tile_store_open(1 << 12, Q, 1, times=True)
    m.tile_store_add_reports(pre)
    before = snap_arrays(m.tile_store_snapshot())
    rows = {}
    for what in ('duration', 'bucket', 'invalid', 'two', 'no_times'):
        s = {'rows': held[0].copy(), 't0': held[1].copy(), 't1': held[2].copy()}
        if what == 'duration':
            s['rows']['duration'][5] += 1
        elif what == 'bucket':
            s['rows']['file'][7] += np.uint64(5 << 25)
        elif what == 'invalid':
            s['t1'][9] = s['t0'][9]
        elif what == 'two':
            s['rows']['speed_bin'][30] += 1
            s['rows']['start'][11] -= 1
        else:
            s['t0'] = s['t1'] = None
        rows[what] = refused(m.tile_store_restore, s)
    out['rows'] = (rows, before, snap_arrays(m.tile_store_snapshot()))
    out['add_rows_timed'] = refused(m.tile_store_add_rows, held[0])
    m.tile_store_close()
    m.tile_store_open(len(held[0]) + n_pre - 1, Q, 1, times=True)
    m.tile_store_add_reports(pre)
    out['rows_full'] = refused(m.tile_store_restore, {'rows': held[0], 't0': held[1], 't1': held[2]})
    out['rows_full_after'] = m.tile_store_snapshot()['n_rows']
    m.tile_store_close()
    m.tile_store_open(1 << 12, Q, 1)
    m.tile_store_add_reports(pre)
    out['export_plain'] = refused(m.tile_store_export_records, 3)
    m.tile_store_close()
    m.tile_store_open(1 << 12, Q, 1, times=True)
    out['bad_slice_size'] = refused(m.tile_store_export_records, 0)
    m.tile_store_close()
elif job == 'map':
    tiny()
    m = M.Matcher()
    for name, rec, use_map, want in X.map_cases():
        for memory in ('host', 'device'):
            m.tile_store_open(1 << 12, Q, 1, times=True)
            if memory == 'host':
                res = m.tile_store_restore_records(rec, use_map=use_map)
            else:
                d, keep = on_device(rec, 5)
                res = m.tile_store_restore_records(d, device=True, use_map=use_map)
            out[(name, memory)] = (res, snap_arrays(m.tile_store_snapshot()))
            m.tile_store_close()
elif job == 'snapshot':
    tiny()
    m = M.Matcher()
    m.tile_store_open(1 << 12, Q, 2, times=True)
    out['empty'] = snap_arrays(m.tile_store_snapshot())
    for a in adds[:3]:
        m.tile_store_add_reports(a)
    snap = m.tile_store_snapshot()
    out['snapshot'] = snap_arrays(snap)
    out['device'] = {k: _lib.device_to_numpy(snap['d_' + k], snap['n_rows'], dt)
                     for k, dt in (('rows', _lib.TILE_ROW), ('t0', np.float64), ('t1', np.float64))}
    nohost = m.tile_store_snapshot(host=False)
    out['nohost_keys'] = sorted(nohost)
    # into a second matcher's store straight from the first one's device copies
    m2 = M.Matcher()
    m2.tile_store_open(1 << 12, Q, 2, times=True)
    out['device_restore'] = m2.tile_store_restore(nohost, device=True)
    out['device_flush'] = m2.tile_store_flush()
    m2.tile_store_close()
    out['untouched'] = snap_arrays(m.tile_store_snapshot())
    out['flush'] = m.tile_store_flush()
    m.tile_store_close()
    for timed in (True, False):
        m.tile_store_open(1 << 12, Q, 2, times=timed)
        out[('restore', timed)] = m.tile_store_restore(snap)
        s2 = m.tile_store_snapshot()
        out[('snapshot', timed)] = snap_arrays(s2)
        out[('null_times', timed)] = (s2['d_t0'] == 0 and s2['d_t1'] == 0, s2['d_rows'] != 0)
        out[('flush', timed)] = m.tile_store_flush()
        m.tile_store_close()
else:   # restart
    import os, tempfile
    path, pts = R.city_stream(graph_dir)
    M.configure(M.default_config(path, **mref.OPTIONS['gtt']))
    shift = TS.CITY_SHIFT
    moved = dict(pts, time=pts['time'] + shift, timestamp=pts['timestamp'] + 1000 * shift)
    n = len(pts['key'])
    cuts = list(range(0, n, 7)) + [n]
    chunks = [(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1)]
    end_ts = int(moved['timestamp'].max()) + R.CITY['session_gap'] + 1
    middle = len(chunks) // 2

    def opened():
        m = M.Matcher()
        m.sessions_open(**R.CITY)
        m.tile_store_open(1 << 16, Q, 1, times=True)   # privacy 1: the stream's three reports are three pairs
        return m

    def run(m, part):
        for a, b in part:
            m.sessions_push(R.take(moved, a, b))
            m.tile_store_add_session()

    def finish(m):
        m.sessions_punctuate(end_ts)
        m.tile_store_add_session()
        return sr.stream_tile_payloads(m.tile_store_flush(), 'auto', 'reporter')

    m = opened()
    run(m, chunks)
    out['whole'] = finish(m)
    m.close()
    m = opened()
    run(m, chunks[:middle + 1])
    out['held_at_stop'] = m.tile_store_snapshot()['n_rows']
    tmp = tempfile.mkdtemp()
    out['saved'] = (sr.save_sessions(m, os.path.join(tmp, 's.npz')), sr.save_tiles(m, os.path.join(tmp, 't.npz')))
    m.close()
    m = opened()
    out['loaded'] = (sr.load_sessions(m, os.path.join(tmp, 's.npz')), sr.load_tiles(m, os.path.join(tmp, 't.npz')))
    m.tile_store_close()
    m.tile_store_open(1 << 16, 120, 1, times=True)
    out['other_quantisation'] = refused(sr.load_tiles, m, os.path.join(tmp, 't.npz'))
    m.tile_store_close()
    m.tile_store_open(1 << 16, Q, 1, times=True)
    sr.load_tiles(m, os.path.join(tmp, 't.npz'))
    run(m, chunks[middle + 1:])
    out['resumed'] = finish(m)
    out['chunks'] = (len(chunks), middle)
    m.close()
pickle.dump(out, open(dst, 'wb'))
print('tile records ok')
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
            dst = str(tmp_path_factory.mktemp('tile_records') / (job + '.pkl'))
            t0 = time.perf_counter()
            p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, dst, job)], env=env,
                               capture_output=True, text=True, timeout=240)
            assert p.returncode == 0 and 'tile records ok' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
            print('child %s: %.1f s' % (job, time.perf_counter() - t0))
            with open(dst, 'rb') as f:
                _RUNS[job] = pickle.load(f)
        return _RUNS[job]
    return get


def _same_records(got, want):
    bad = X.records_differing(got, want)
    assert not bad, bad


def _same_flush(got, want):
    bad = TS.differing(got, want)
    assert not bad, bad


def _same_held(got, want):
    assert got['n_rows'] == len(want[0])
    assert got['rows'].tobytes() == np.ascontiguousarray(want[0]).tobytes()
    if got['t0'] is not None:
        assert got['t0'].tobytes() == want[1].tobytes() and got['t1'].tobytes() == want[2].tobytes()


def _held_before_flush(k):
    """The script's held rows before its k-th flush."""
    adds = TS.script_adds()
    first = 0 if k == 0 else TS.SCRIPT_FLUSH_AFTER[k - 1] + 1
    return X.held_of(adds[first:TS.SCRIPT_FLUSH_AFTER[k] + 1], Q)


def test_export(run_job):
    """The script on a store with the times, exported before each flush at every slice size: every
    array equals the restatement's byte for byte, the device copies equal the host copies, and
    the flushes equal the plain store's and the restatement's (the times change nothing)."""
    r = run_job('export')
    timed, plain = r['timed'], r['plain']
    _, want_flushes = TS.script_flushes(2)
    assert len(timed['exports']) == len(timed['flushes']) == len(plain['flushes']) == 3
    for k in range(3):
        held = _held_before_flush(k)
        for S in SIZES:
            host, dev = timed['exports'][k][S]
            want = X.export(held, Q, S)
            _same_records(host, want)
            _same_records(dict(host, **dev), want)
        _same_flush(timed['flushes'][k], plain['flushes'][k])
        _same_flush(timed['flushes'][k], want_flushes[k])
    for a, b in zip(timed['adds'], plain['adds']):
        assert {k: a[k] for k in ('n_reports', 'n_valid', 'n_rows_added', 'n_rows')} == \
            {k: b[k] for k in ('n_reports', 'n_valid', 'n_rows_added', 'n_rows')}
    e = timed['export_empty']
    assert e['n_slices'] == 0 and e['n_tiles'] == 0 and e['rec_off'].tolist() == [0] and e['n_bytes'] == 0
    for n in (257, 20001):
        host, dev = r[n]
        want = X.export(X.held_of([X.synthetic_file(n)], Q), Q, 20000)
        assert want['n_slices'] == (1 if n == 257 else 2)
        _same_records(host, want)
        _same_records(dict(host, **dev), want)


def test_restore(run_job):
    """Each export into a fresh store with the times and into a fresh plain store, from host
    memory and from device memory at byte shifts 0, 1, 4 and 7: the flush equals the original's,
    the export again equals the export, and a store that already holds rows keeps them in front."""
    r = run_job('restore')
    held = _held_before_flush(0)
    for name, rec in r['exports'].items():
        synthetic = name == 'synthetic'
        want_flush = r['flush_synthetic' if synthetic else 'flush']
        n = 20001 if synthetic else len(held[0])
        exact = X.restore_records(X.empty_held(), rec, Q, 1 << 16)[1]['n_missing_slices']
        for timed in (True, False):
            for src in ['host'] + list((1,) if synthetic else SHIFTS):
                res, again, flush = r[(name, timed, src)]
                assert (res['n_rows'], res['n_slices'], res['n_rows_held']) == (n, rec['n_slices'], n), (name, timed, src)
                assert (res['n_unreferenced_slices'], res['n_missing_slices'], res['bad_reason']) == (0, exact, 0)
                _same_flush(flush, want_flush)
                if timed:
                    _same_records(again, rec)
    _same_records(r['exports'][3], X.export(held, Q, 3))
    first = X.held_of(TS.script_adds()[3:4], Q)
    want, counts = X.restore_records(first, r['exports'][3], Q, 1 << 16)
    _same_held(r['append_snapshot'], want)
    assert r['append_snapshot']['rows'][:len(first[0])].tobytes() == first[0].tobytes() and len(first[0]) > 0
    assert r['append_result']['n_rows_held'] == len(want[0]) and r['append_result']['n_rows'] == counts['n_rows']


def test_refusals(run_job):
    """Every reason of the record restore from host and device memory (bytes at shift 3), the
    lowest index and the lowest of its reasons; E_ROW of the snapshot restore; after each refusal
    the store's snapshot equals the one before it; add_rows on a store with the times and the
    export on a plain store are refused."""
    r = run_job('refusals')
    cases = X.refusal_cases()
    assert {c[3] for c in cases} == {X.E_LAYOUT, X.E_KEY, X.E_COUNT, X.E_SEGMENT, X.E_DUPLICATE, X.E_MAP, X.E_FULL}
    for name, rec, max_rows, reason, bad_slice, bad_tile in cases:
        for memory in ('host', 'device'):
            got, before, after = r[(name, memory)]
            assert got is not None, (name, memory, 'not refused')
            res = got[1]
            assert res is not None and (res['bad_reason'], res['bad_slice'], res['bad_tile']) == \
                (reason, bad_slice, bad_tile), (name, memory, got)
            assert before['n_rows'] > 0
            _same_held(after, (before['rows'], before['t0'], before['t1']))
    rows, before, after = r['rows']
    for what, index in (('duration', 5), ('bucket', 7), ('invalid', 9), ('two', 11)):
        assert rows[what] is not None and rows[what][1] is not None, what
        assert (rows[what][1]['bad_reason'], rows[what][1]['bad_slice']) == (X.E_ROW, index), (what, rows[what])
    assert rows['no_times'] is not None and 'OTR_TILE_STORE_TIMES' in rows['no_times'][0]
    _same_held(after, (before['rows'], before['t0'], before['t1']))
    assert r['rows_full'] is not None and r['rows_full'][1]['bad_reason'] == X.E_FULL and r['rows_full'][1]['bad_slice'] == -1
    assert r['rows_full_after'] == before['n_rows']
    assert r['add_rows_timed'] is not None and 'otr_tile_store_restore' in r['add_rows_timed'][0]
    assert r['export_plain'] is not None and 'OTR_TILE_STORE_TIMES' in r['export_plain'][0]
    assert r['bad_slice_size'] is not None and 'slice_size' in r['bad_slice_size'][0]


def test_map(run_job):
    """Unreferenced and missing slices, no map, an empty map: the counts and what gets restored."""
    r = run_job('map')
    for name, rec, use_map, want in X.map_cases():
        held, counts = X.restore_records(X.empty_held(), rec, Q, 1 << 12, use_map=use_map)
        assert {k: counts[k] for k in want} == want
        for memory in ('host', 'device'):
            res, snap = r[(name, memory)]
            assert {k: res[k] for k in want} == want, (name, memory, res)
            assert res['n_rows_held'] == want['n_rows'] and res['bad_reason'] == 0
            _same_held(snap, held)


def test_snapshot(run_job):
    """Snapshot, close, open, restore: the same flush; the snapshot is the held rows with their
    times in arrival order, host and device copies; it leaves the store untouched; a plain store's
    snapshot has null times."""
    r = run_job('snapshot')
    held = _held_before_flush(0)
    assert r['empty']['n_rows'] == 0 and len(r['empty']['rows']) == 0
    _same_held(r['snapshot'], held)
    assert r['snapshot']['flags'] == 1 and r['snapshot']['quantisation'] == Q
    _same_held(dict(r['device'], n_rows=len(held[0])), held)
    assert 'rows' not in r['nohost_keys'] and 'd_rows' in r['nohost_keys']
    _same_held(r['untouched'], held)
    _, want = TS.script_flushes(2)
    _same_flush(r['flush'], want[0])
    assert r['device_restore']['n_rows'] == len(held[0])
    _same_flush(r['device_flush'], want[0])
    for timed in (True, False):
        assert r[('restore', timed)]['n_rows'] == r[('restore', timed)]['n_rows_held'] == len(held[0])
        _same_flush(r[('flush', timed)], want[0])
        snap = r[('snapshot', timed)]
        assert snap['rows'].tobytes() == held[0].tobytes()
        if timed:
            _same_held(snap, held)
            assert r[('null_times', timed)] == (False, True)
        else:
            assert snap['t0'] is None and snap['t1'] is None and snap['flags'] == 0
            assert r[('null_times', timed)] == (True, True)


def test_restart(run_job):
    """The shifted city stream through sessions_push + tile_store_add_session per chunk, stopped
    after the middle chunk: save_sessions + save_tiles, the matcher freed, a new matcher with
    load_sessions + load_tiles runs the rest.  Its payloads equal an uninterrupted run's, text for
    text, and the store held rows at the stop."""
    r = run_job('restart')
    assert r['held_at_stop'] >= 1, r['chunks']
    assert r['saved'][1] == r['held_at_stop'] == r['loaded'][1]['n_rows']
    assert r['other_quantisation'] is not None and 'quantisation' in r['other_quantisation'][0]
    assert len(r['whole']) > 0 and r['resumed'] == r['whole']
    print('restart: %d chunks, stopped after chunk %d with %d rows and %d sessions, %d files'
          % (r['chunks'] + (r['held_at_stop'], r['saved'][0], len(r['whole']))))
