"""Restore, export and move of the session store in HBM (K17, include/otr.h otr_sessions_restore,
otr_sessions_restore_records, otr_sessions_export_records, otr_sessions_take) against the
restatement tests/session_records_ref.py over tests/sessions_ref.py: a fresh store restored at
every cut of the scripted stream goes on exactly as the restatement does (from host arrays, from
device arrays and from Batch.Serder's bytes); the export is those bytes; records at an odd device
address; a store split in two parts and continued apart; restores over dead table entries and
through rebuilds; the cap on a restored session; every refusal with the store untouched; and the
city stream cut in half with real matching, through records and through a file.  What the streams
cover is pinned by tests/test_session_restore_cpu.py.  One child process per job."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import session_records_ref as S
from tests import sessions_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = dict(report_dist=1e9, report_count=99, report_time=0)   # gates that never pass
CHILD = r'''
import sys, pickle, os
sys.path.insert(0, %r)
graph_dir, dst, job = %r, %r, %r
import numpy as np
import torch
from reporter_amd import matcher as M
from reporter_amd import _lib
from reporter_amd import simple_reporter as SR
from reporter_amd.tools import gen
from tests import matched_points_ref as mref
from tests import sessions_ref as R
from tests import session_records_ref as S

NEVER = dict(report_dist=1e9, report_count=99, report_time=0)


def batch_arrays(b):
    nt = int(b.n_traces)
    off = _lib.device_to_numpy(b.trace_offsets, nt + 1, np.int64)
    n = int(off[-1])
    return {'trace_offsets': off, 'lat': _lib.device_to_numpy(b.lat, n, np.float64),
            'lon': _lib.device_to_numpy(b.lon, n, np.float64), 'time': _lib.device_to_numpy(b.time, n, np.int64),
            'accuracy': _lib.device_to_numpy(b.accuracy, n, np.float32),
            'mode': _lib.device_to_numpy(b.mode, nt, np.uint8), 'memory': int(b.memory)}


def refused(f, *a, **kw):
    try:
        f(*a, **kw)
    except ValueError as e:
        return str(e)
    return None


def run_chunk(m, pts, arrival=None, snapshots=True):
    """A chunk through advance / commit with the scripted answers (of the arrival index when the
    chunk is a filtered one): the rounds as the existing scripted job records them."""
    rounds = []
    b, win = m.sessions_advance(pts)
    while b.n_traces > 0:
        arrays = batch_arrays(b)
        trig = [int(t) if arrival is None else int(arrival[int(t)]) for t in win['trigger']]
        ans = [R.scripted_match([None] * int(n), k, t) for k, t, n in zip(win['key'], trig, win['n_points'])]
        done = m.sessions_commit([a[0] if a[0] is not None else 0 for a in ans], [0 if a[1] else 500 for a in ans])
        rounds.append({'batch': arrays, 'windows': done, 'snapshot': m.sessions_snapshot() if snapshots else None})
        b, win = m.sessions_advance(None)
    return rounds, batch_arrays(b)


def chunk_and_punctuate(m, q, **kw):
    pts, ts = R.scripted_chunk(q)
    rounds, end = run_chunk(m, pts, **kw)
    return {'rounds': rounds, 'end_batch': end, 'snapshot': m.sessions_snapshot(),
            'punctuate': m.sessions_punctuate(ts), 'after': m.sessions_snapshot()}


KEEP = []


def to_device(a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
    KEEP.append(t)
    return t.data_ptr()


def restore(m, snap, how):
    if how == 'host':
        return m.sessions_restore(snap)
    if how == 'device':
        d = {k: to_device(snap[k]) for k in R.SNAPSHOT_FIELDS}
        d['n_sessions'], d['n_points'] = len(snap['key']), len(snap['time'])
        torch.cuda.synchronize()
        return m.sessions_restore(d, device=True)
    return m.sessions_restore_records(*S.encode(snap))


out = {}
tiny = job not in ('city',)
if tiny:
    M.configure(M.default_config(gen.graph_path('tiny', graph_dir)))
    m = M.Matcher()
if job.startswith('resume_'):
    out['cuts'] = []
    for (kind, p), snap in S.scripted_cuts():
        m.sessions_open(**R.SCRIPT)
        rec = {'restore': restore(m, snap, job[7:]), 'restored': m.sessions_snapshot(), 'chunks': []}
        if kind == 'push':
            rec['punctuate'] = m.sessions_punctuate(R.scripted_chunk(p)[1])
            rec['after'] = m.sessions_snapshot()
        for q in range(p + 1, R.SCRIPT_CHUNKS):
            rec['chunks'].append(chunk_and_punctuate(m, q))
        m.sessions_close()
        out['cuts'].append(rec)
elif job == 'records':
    def export():
        r = m.sessions_export_records()
        d = r.pop('device')
        n, nb = len(r['key']), len(r['bytes'])
        r['d_key'] = _lib.device_to_numpy(d.d_key, n, np.uint64)
        r['d_rec_off'] = _lib.device_to_numpy(d.d_rec_off, n + 1, np.int64)
        r['d_bytes'] = _lib.device_to_numpy(d.d_bytes, nb, np.uint8)
        r['memory'] = int(d.memory)
        return r

    m.sessions_open(**R.SCRIPT)
    out['empty'] = export()
    out['cuts'] = []
    for p in range(R.SCRIPT_CHUNKS):
        pts, ts = R.scripted_chunk(p)
        run_chunk(m, pts, snapshots=False)
        out['cuts'].append(export())
        m.sessions_punctuate(ts)
        out['cuts'].append(export())
    m.sessions_close()
    # the records of the cut after chunk 4's push, one byte into an aligned device buffer
    key, rec_off, data = S.encode(S.scripted_cuts()[8][1])
    buf = torch.zeros(len(data) + 1, dtype=torch.uint8, device='cuda')
    buf[1:] = torch.from_numpy(np.frombuffer(data, np.uint8).copy())
    torch.cuda.synchronize()
    assert buf.data_ptr() %% 16 == 0
    m.sessions_open(**R.SCRIPT)
    out['unaligned_restore'] = m.sessions_restore_records(to_device(key), to_device(rec_off), buf.data_ptr() + 1,
                                                          device=True, n_records=len(key), n_bytes=len(data))
    out['unaligned'] = m.sessions_snapshot()
    m.sessions_close()
    m.sessions_open(**R.SCRIPT)
    host = np.frombuffer(b'\0' + data, np.uint8)[1:]
    m.sessions_restore_records(key, rec_off, host)
    out['unaligned_host'] = m.sessions_snapshot()
elif job == 'move':
    m.sessions_open(**R.SCRIPT)
    for p in range(2):
        chunk_and_punctuate(m, p, snapshots=False)
    pts2, ts2 = R.scripted_chunk(2)
    run_chunk(m, pts2, snapshots=False)
    out['cut'] = m.sessions_snapshot()
    out['keep'] = m.sessions_take(1, 0, remove=False)
    out['after_keep'] = m.sessions_snapshot()
    out['parts'] = [m.sessions_take(2, r) for r in (0, 1)]
    out['after_take'] = m.sessions_snapshot()
    out['live_after_take'] = m.sessions_punctuate(-10 ** 12)['n_live']
    out['runs'] = []
    for r in (0, 1):
        m.sessions_close()
        m.sessions_open(**R.SCRIPT)
        run = {'restore': m.sessions_restore(out['parts'][r]), 'punctuate2': m.sessions_punctuate(ts2),
               'after2': m.sessions_snapshot(), 'chunks': []}
        for q in range(3, R.SCRIPT_CHUNKS):
            pts, ts = R.scripted_chunk(q)
            idx = np.nonzero(pts['key'] %% np.uint64(2) == np.uint64(r))[0]
            rounds, _ = run_chunk(m, {k: pts[k][idx] for k, _ in R.POINT_TYPES}, arrival=idx, snapshots=False)
            run['chunks'].append({'windows': [x['windows'] for x in rounds], 'arrival': idx,
                                  'snapshot': m.sessions_snapshot(), 'punctuate': m.sessions_punctuate(ts),
                                  'after': m.sessions_snapshot()})
        out['runs'].append(run)
elif job == 'dead':
    m.sessions_open(4, 4, session_gap=1000, **NEVER)
    a, _ = run_chunk(m, S.DEAD_FIRST)
    out['first'] = {'rounds': a, 'snapshot': m.sessions_snapshot()}
    out['punctuate'] = m.sessions_punctuate(S.DEAD_TS)
    out['after_punctuate'] = m.sessions_snapshot()
    out['restore'] = m.sessions_restore(S.DEAD_RESTORE)
    out['restored'] = m.sessions_snapshot()
    b, _ = run_chunk(m, S.DEAD_SECOND)
    out['second'] = {'rounds': b, 'snapshot': m.sessions_snapshot()}
    out['rebuilds_before'] = m.sessions_punctuate(0)['n_rebuilds']
    for _ in range(8):
        m.sessions_restore(m.sessions_take(1, 0))
    out['cycled'] = m.sessions_snapshot()
    out['rebuilds_after'] = m.sessions_punctuate(0)['n_rebuilds']
    c, _ = run_chunk(m, S.DEAD_THIRD)
    out['third'] = {'rounds': c, 'snapshot': m.sessions_snapshot()}
elif job == 'cap':
    for name, tm in (('forward', 1003), ('backward', 900)):
        m.sessions_open(4, 4, session_gap=60000, **NEVER)
        m.sessions_restore(S.CAP_SESSION)
        out[name] = m.sessions_push(S.cap_point(tm))
        out[name + '_after'] = m.sessions_snapshot()
        m.sessions_close()
elif job == 'refusals':
    one = S.still_snapshot([40], [1])
    out['no_store'] = [refused(m.sessions_restore, one), refused(m.sessions_restore_records, *S.encode(one)),
                       refused(m.sessions_take, 1, 0), refused(m.sessions_export_records)]
    out['cases'] = {}
    for name, (live, snap, ms, want) in S.REFUSALS.items():
        m.sessions_open(ms, 4, session_gap=60000, **NEVER)
        if live:
            m.sessions_push(R.refusal_points(list(live)))
        c = {'before': m.sessions_snapshot(), 'soa': refused(m.sessions_restore, snap)}
        c['after_soa'] = m.sessions_snapshot()
        if 'layout' not in name:
            c['device'] = refused(restore, m, snap, 'device')
            c['after_device'] = m.sessions_snapshot()
            c['records'] = refused(m.sessions_restore_records, *S.encode(snap))
            c['after_records'] = m.sessions_snapshot()
        c['then'] = m.sessions_restore(one)
        c['after_then'] = m.sessions_snapshot()
        m.sessions_close()
        out['cases'][name] = c
    out['layout'] = {}
    for name, (key, rec_off, data, want) in S.record_layout_cases().items():
        m.sessions_open(4, 4, session_gap=60000, **NEVER)
        m.sessions_push(R.refusal_points([9]))
        c = {'before': m.sessions_snapshot(), 'records': refused(m.sessions_restore_records, key, rec_off, data)}
        c['after'] = m.sessions_snapshot()
        m.sessions_close()
        out['layout'][name] = c
    # live + given == max_sessions is accepted
    m.sessions_open(4, 4, session_gap=60000, **NEVER)
    m.sessions_push(R.refusal_points([8]))
    out['brim'] = m.sessions_restore(S.BRIM)
    out['brim_after'] = m.sessions_snapshot()
    m.sessions_close()
    # an open advance / commit sequence, then an open chunk
    m.sessions_open(4, 4, session_gap=60000, **NEVER)
    b, win = m.sessions_advance(R.refusal_points([3, 3, 3, 3]))
    assert b.n_traces == 1
    out['pending'] = [refused(m.sessions_restore, one), refused(m.sessions_restore_records, *S.encode(one)),
                      refused(m.sessions_take, 1, 0)]
    m.sessions_commit([1], [0])
    out['chunk_open'] = [refused(m.sessions_restore, one), refused(m.sessions_restore_records, *S.encode(one)),
                         refused(m.sessions_take, 1, 0)]
    b, win = m.sessions_advance(None)
    assert b.n_traces == 0
    out['sequence_closed'] = m.sessions_restore(one)
    out['sequence_after'] = m.sessions_snapshot()
else:
    path, pts = R.city_stream(graph_dir)
    M.configure(M.default_config(path, **mref.OPTIONS['gtt']))
    m = M.Matcher()
    n = len(pts['key'])
    half = n // 2
    m.sessions_open(**R.CITY)
    out['one'] = {'result': R.by_trigger(m.sessions_push(pts)), 'snapshot': m.sessions_snapshot()}
    m.sessions_close()
    for how in ('records', 'file'):
        m.sessions_open(**R.CITY)
        first = m.sessions_push(R.take(pts, 0, half))
        mid = m.sessions_snapshot()
        if how == 'records':
            r = m.sessions_export_records()
        else:
            f = os.path.join(os.path.dirname(dst), 'sessions.npz')
            saved = SR.save_sessions(m, f)
        m.sessions_close()
        m.sessions_open(**R.CITY)
        if how == 'records':
            got = m.sessions_restore_records(r['key'], r['rec_off'], r['bytes'])
        else:
            got = SR.load_sessions(m, f)
            assert saved == got['n_sessions']
        restored = m.sessions_snapshot()
        second = m.sessions_push(R.take(pts, half, n))
        out[how] = {'result': R.by_trigger(R.concat([first, second], [0, half])), 'snapshot': m.sessions_snapshot(),
                    'mid': mid, 'restored': restored, 'restore': got}
        m.sessions_close()
pickle.dump(out, open(dst, 'wb'))
print('restore ok')
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
            dst = str(tmp_path_factory.mktemp('restore') / (job + '.pkl'))
            t0 = time.perf_counter()
            p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, dst, job)], env=env,
                               capture_output=True, text=True, timeout=240)
            assert p.returncode == 0 and 'restore ok' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
            print('child %s: %.1f s' % (job, time.perf_counter() - t0))
            with open(dst, 'rb') as f:
                _RUNS[job] = pickle.load(f)
        return _RUNS[job]
    return get


@pytest.fixture(scope='module')
def cuts():
    return S.scripted_cuts()


def _same(got, want, fields, what=''):
    bad = R.differing(got, want, fields)
    assert not bad, (what, bad)


class _Script:
    """The restatement with the scripted answers, remembering what it sent to the matcher."""

    def __init__(self, **cfg):
        self.seen = []
        self.ref = R.Store(self.match, **cfg)

    def match(self, points, key, trigger):
        self.seen.append((trigger, points))
        return R.scripted_match(points, key, trigger)

    def check_rounds(self, pts, rounds, what):
        """The device store's rounds of one chunk against the restatement consumed in rounds:
        windows, the emitted batch and the snapshot after every commit."""
        rounds = list(rounds)
        n = 0
        for wins in R.push_rounds(self.ref, pts):
            assert rounds, '%s: the device store ran out of rounds' % (what,)
            g = rounds.pop(0)
            _same(g['windows'], R.windows_to_arrays(wins), [k for k, _ in R.WINDOW_FIELDS], what)
            b = g['batch']
            sent = [w for _, w in sorted(self.seen, key=lambda x: x[0])]
            flat = [q for w in sent for q in w]
            assert b['memory'] == 1 and b['mode'].tolist() == [0] * len(wins)
            assert b['trace_offsets'].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in sent])]).tolist()
            _same(b, {'lat': np.array([q[0] for q in flat], np.float64), 'lon': np.array([q[1] for q in flat], np.float64),
                      'time': np.array([q[2] for q in flat], np.int64),
                      'accuracy': np.array([q[3] for q in flat], np.float32)}, ('lat', 'lon', 'time', 'accuracy'), what)
            del self.seen[:]
            _same(g['snapshot'], self.ref.snapshot(), R.SNAPSHOT_FIELDS, what)
            n += len(wins)
        assert not rounds, what
        return n

    def check_punctuate(self, ts, pun, after, what):
        ev, ne = self.ref.punctuate(ts)
        del self.seen[:]
        assert pun['n_evicted'] == ne and pun['n_live'] == len(self.ref.sessions), what
        _same(pun, R.windows_to_arrays(ev), ('key', 'trigger', 'n_points', 'trimmed'), what)
        _same(after, self.ref.snapshot(), R.SNAPSHOT_FIELDS, what)


@pytest.mark.parametrize('how', ['host', 'device', 'records'])
def test_resume_at_every_cut(how, run_job, cuts):
    """A fresh store restored with the restatement's snapshot of a cut, then the rest of the stream
    through advance / commit / punctuate: batches, windows and the snapshot after every commit
    (max_sep by bits) equal the restatement continued from the cut."""
    got = run_job('resume_' + how)['cuts']
    assert len(got) == len(cuts) == 2 * R.SCRIPT_CHUNKS
    n_windows = 0
    for ((kind, p), snap), g in zip(cuts, got):
        what = (how, kind, p)
        s = _Script(**{k: v for k, v in R.SCRIPT.items() if k != 'max_sessions'})
        assert S.restore(s.ref, snap, R.SCRIPT['max_sessions']) == (-1, 0)
        r = g['restore']
        assert (r['n_sessions'], r['n_points'], r['n_live']) == (len(snap['key']), len(snap['time']), len(snap['key']))
        _same(g['restored'], snap, R.SNAPSHOT_FIELDS, what)
        if kind == 'push':
            s.check_punctuate(R.scripted_chunk(p)[1], g['punctuate'], g['after'], what)
        assert len(g['chunks']) == R.SCRIPT_CHUNKS - 1 - p
        for q, c in zip(range(p + 1, R.SCRIPT_CHUNKS), g['chunks']):
            pts, ts = R.scripted_chunk(q)
            n_windows += s.check_rounds(pts, c['rounds'], what + (q,))
            assert c['end_batch']['trace_offsets'].tolist() == [0]
            _same(c['snapshot'], s.ref.snapshot(), R.SNAPSHOT_FIELDS, what)
            s.check_punctuate(ts, c['punctuate'], c['after'], what + (q,))
    print('resume %s: %d windows after the cuts' % (how, n_windows))
    assert n_windows > 300


def test_export_is_the_serder_bytes(run_job, cuts):
    """At every cut of an uninterrupted device run the exported records are the restatement's
    snapshot encoded, byte for byte, in host memory and in HBM."""
    r = run_job('records')
    e = r['empty']
    assert len(e['key']) == 0 and e['rec_off'].tolist() == [0] and len(e['bytes']) == 0 and e['d_rec_off'].tolist() == [0]
    assert len(r['cuts']) == len(cuts)
    for (name, snap), g in zip(cuts, r['cuts']):
        key, rec_off, data = S.encode(snap)
        assert g['memory'] == 0
        for pre in ('', 'd_'):
            assert g[pre + 'key'].tolist() == key.tolist(), (name, pre)
            assert g[pre + 'rec_off'].tolist() == rec_off.tolist(), (name, pre)
            assert g[pre + 'bytes'].tobytes() == data, (name, pre)


def test_records_at_an_odd_address(run_job, cuts):
    r = run_job('records')
    snap = cuts[8][1]
    assert 15 in np.diff(snap['point_off']) and 1 in np.diff(snap['point_off'])
    assert r['unaligned_restore']['n_sessions'] == len(snap['key'])
    assert r['unaligned_restore']['n_points'] == len(snap['time'])
    _same(r['unaligned'], snap, R.SNAPSHOT_FIELDS)
    _same(r['unaligned_host'], snap, R.SNAPSHOT_FIELDS)


def test_move_in_two_parts(run_job, cuts):
    """The store after chunk 2's push taken apart by key % 2, each part restored into a fresh store
    and fed its share of the rest of the stream: together the two runs emit the uninterrupted
    restatement's windows."""
    r = run_job('move')
    (kind, p), snap = cuts[4]
    assert (kind, p) == ('push', 2)
    _same(r['cut'], snap, R.SNAPSHOT_FIELDS)
    _same(r['keep'], snap, R.SNAPSHOT_FIELDS)
    _same(r['after_keep'], snap, R.SNAPSHOT_FIELDS)
    ref = R.Store(R.scripted_match, **{k: v for k, v in R.SCRIPT.items() if k != 'max_sessions'})
    for q in range(3):
        pts, ts = R.scripted_chunk(q)
        ref.push(pts)
        if q < 2:
            ref.punctuate(ts)
    for part in (0, 1):
        want = S.take(ref, 2, part, False)
        assert len(want['key']) > 0
        _same(r['parts'][part], want, R.SNAPSHOT_FIELDS, part)
        assert r['runs'][part]['restore']['n_sessions'] == len(want['key'])
    assert len(r['after_take']['key']) == 0 and r['live_after_take'] == 0

    def evictions(which, ts):
        ev, ne = ref.punctuate(ts)
        want = R.windows_to_arrays(ev)
        got = [which(run) for run in r['runs']]
        assert sum(g['n_evicted'] for g in got) == ne
        order = np.argsort(np.concatenate([g['key'] for g in got]), kind='stable')
        for k in ('key', 'n_points', 'trimmed'):
            assert np.concatenate([g[k] for g in got])[order].tolist() == want[k].tolist(), (k, ts)
        assert all((np.diff(g['trigger']) < 0).all() and (g['trigger'] < 0).all() for g in got)

    evictions(lambda run: run['punctuate2'], R.scripted_chunk(2)[1])
    n_windows = 0
    for i, q in enumerate(range(3, R.SCRIPT_CHUNKS)):
        pts, ts = R.scripted_chunk(q)
        want = R.windows_to_arrays(ref.push(pts))
        rows = []
        for run in r['runs']:
            c = run['chunks'][i]
            for w in c['windows']:
                for j in range(len(w['key'])):
                    rows.append(tuple(int(c['arrival'][w['trigger'][j]]) if k == 'trigger' else int(w[k][j])
                                      for k, _ in R.WINDOW_FIELDS))
        rows.sort(key=lambda x: x[1])
        _same({k: np.array([x[j] for x in rows], dt) for j, (k, dt) in enumerate(R.WINDOW_FIELDS)}, want,
              [k for k, _ in R.WINDOW_FIELDS], q)
        n_windows += len(rows)
        for part, run in enumerate(r['runs']):
            _same(run['chunks'][i]['snapshot'], S.take(ref, 2, part, False), R.SNAPSHOT_FIELDS, (q, part))
        evictions(lambda run: run['chunks'][i]['punctuate'], ts)
        for part, run in enumerate(r['runs']):
            _same(run['chunks'][i]['after'], S.take(ref, 2, part, False), R.SNAPSHOT_FIELDS, (q, part))
    assert n_windows > 50


def test_same_store_dead_entries_and_rebuilds(run_job):
    """On the 4 x 4 store: keys pushed, some punctuated away, one of them restored beside a new key
    and both pushed onto; then take / restore cycles until the key table is rebuilt."""
    r = run_job('dead')
    s = _Script(max_points=4, session_gap=1000, **NEVER)
    assert s.check_rounds(S.DEAD_FIRST, r['first']['rounds'], 'first') == 0
    _same(r['first']['snapshot'], s.ref.snapshot(), R.SNAPSHOT_FIELDS)
    s.check_punctuate(S.DEAD_TS, r['punctuate'], r['after_punctuate'], 'punctuate')
    assert r['after_punctuate']['key'].tolist() == [3] and r['punctuate']['n_evicted'] == 2
    assert S.restore(s.ref, S.DEAD_RESTORE, 4) == (-1, 0)
    assert r['restore']['n_live'] == 3
    _same(r['restored'], s.ref.snapshot(), R.SNAPSHOT_FIELDS)
    assert r['restored']['key'].tolist() == [1, 3, 7]
    assert s.check_rounds(S.DEAD_SECOND, r['second']['rounds'], 'second') == 2   # both reach the cap
    _same(r['second']['snapshot'], s.ref.snapshot(), R.SNAPSHOT_FIELDS)
    _same(r['cycled'], s.ref.snapshot(), R.SNAPSHOT_FIELDS)
    assert r['rebuilds_after'] > r['rebuilds_before']
    s.check_rounds(S.DEAD_THIRD, r['third']['rounds'], 'third')
    _same(r['third']['snapshot'], s.ref.snapshot(), R.SNAPSHOT_FIELDS)
    assert len(r['third']['snapshot']['key']) > 0


def test_cap_on_a_restored_session(run_job):
    """A restored session of max_points - 1 points: the next point reaches the cap, reported by
    force with a forward clock, cleared with a backward one."""
    r = run_job('cap')
    for name, tm, counts in (('forward', 1003, (1, 0, 1)), ('backward', 900, (0, 1, 0))):
        ref = R.Store(lambda points, key, trigger: (None, True, []), 4, session_gap=60000, **NEVER)
        assert S.restore(ref, S.CAP_SESSION, 4) == (-1, 0)
        wins = ref.push(S.cap_point(tm))
        g = r[name]
        assert (g['n_forced'], g['n_dropped'], g['n_windows']) == counts == (ref.n_forced, ref.n_dropped, len(wins))
        _same(g, R.windows_to_arrays(wins), ('key', 'trigger', 'n_points'), name)
    assert r['forward']['n_points'].tolist() == [4] and r['forward']['key'].tolist() == [5]
    assert len(r['backward_after']['key']) == 0 and r['backward']['n_live'] == 0


def _message(want):
    bad, reason = want
    names = {S.E_LAYOUT: 'layout', S.E_KEY: 'key', S.E_COUNT: 'count', S.E_DUPLICATE: 'duplicate', S.E_LIVE: 'live',
             S.E_FULL: 'full'}
    return 'refused: %s%s (' % ('session %d: ' % bad if bad >= 0 else '', names[reason])


def test_refusals_leave_the_store_untouched(run_job):
    r = run_job('refusals')
    assert all(e and 'otr_sessions_open' in e for e in r['no_store'])
    assert set(r['cases']) == set(S.REFUSALS)
    reasons = set()
    for name, (live, snap, ms, want) in S.REFUSALS.items():
        c = r['cases'][name]
        assert sorted(c['before']['key'].tolist()) == sorted(live)
        assert S.restore(S.small_store(live), snap, ms) == want
        reasons.add(want[1])
        for how in ('soa', 'device', 'records'):
            if how in c:
                assert c[how] and _message(want) in c[how], (name, how, c[how])
                _same(c['after_' + how], c['before'], R.SNAPSHOT_FIELDS, (name, how))
        assert c['then']['n_sessions'] == 1 and c['then']['n_live'] == len(live) + 1
        assert sorted(c['after_then']['key'].tolist()) == sorted(live + (40,))
    assert reasons == {S.E_LAYOUT, S.E_KEY, S.E_COUNT, S.E_DUPLICATE, S.E_LIVE, S.E_FULL}
    for name, (key, rec_off, data, want) in S.record_layout_cases().items():
        c = r['layout'][name]
        assert c['records'] and _message(want) in c['records'], (name, c['records'])
        _same(c['after'], c['before'], R.SNAPSHOT_FIELDS, name)
    # the boundary: live + given == max_sessions
    ref = R.Store(lambda points, key, trigger: (None, True, []), 4, session_gap=60000, **NEVER)
    ref.push(R.refusal_points([8]))
    assert S.restore(ref, S.BRIM, 4) == (-1, 0) and len(ref.sessions) == 4
    assert r['brim']['n_live'] == 4 and r['brim']['n_sessions'] == 3
    _same(r['brim_after'], ref.snapshot(), R.SNAPSHOT_FIELDS)
    for k in ('pending', 'chunk_open'):
        assert all(e and 'sequence is open' in e for e in r[k]), r[k]
    assert r['sequence_closed']['n_sessions'] == 1 and 40 in r['sequence_after']['key'].tolist()


def test_city_stream_cut_in_half(run_job):
    """Real matching: the first half pushed, the sessions exported, the store closed and opened
    again, the records restored and the second half pushed give the windows, reports and final
    snapshot of the one-push run; the same through save_sessions / load_sessions."""
    r = run_job('city')
    one = r['one']
    assert len(one['result']['key']) > 100 and len(one['result']['id']) > 0
    for how in ('records', 'file'):
        g = r[how]
        assert len(g['mid']['key']) > 5 and g['restore']['n_sessions'] == len(g['mid']['key'])
        _same(g['restored'], g['mid'], R.SNAPSHOT_FIELDS, how)
        _same(g['result'], one['result'], R.RESULT_FIELDS, how)
        _same(g['snapshot'], one['snapshot'], R.SNAPSHOT_FIELDS, how)
