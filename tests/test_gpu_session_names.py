"""The session store's uuid directory in HBM (K18, include/otr.h otr_sessions_open_named ...)
against the restatement tests/session_names_ref.py: the scripted stream through a named store
beside a plain one; every name refusal with the store and the directory untouched and the refused
chunk's claims rolled back; slot reuse, key reuse, table rebuilds; take / restore_named in two
parts and records with names at an odd device address; a collision across a restore found through
otr_sessions_push_text; evictions in name order; and the city stream through stream_text_tiles on
a named store with save_sessions / load_sessions in between.  One child process per job, scripted
matching through advance / commit except in the last."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import formatter_ref as F
from tests import session_names_ref as N
from tests import session_records_ref as S
from tests import sessions_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = dict(report_dist=1e9, report_count=99, report_time=0)   # gates that never pass
UB = N.UUID_BYTES
SMALL = dict(max_sessions=8, max_points=4, session_gap=60000, **NEVER)


def whole(points, key, trigger):
    """The scripted answer of the reuse job: every window is used up."""
    return len(points), True, []


# the reuse job's steps: (op, arguments); pushes are rows of (key, time, timestamp) and names
REUSE = dict(max_sessions=4, max_points=4, session_gap=1000, **NEVER)
REUSE_STEPS = [
    ('push', [(1, 100 + i, 1000 + i) for i in range(4)], [b'z' * 20] * 4),        # forced at the cap, trimmed to empty
    ('push', [(9, 200, 2000), (3, 201, 2001)], [b'abc', b'abc\x01']),             # key 9 takes key 1's slot
    ('push', [(9, 202, 2002), (3, 203, 2003)], [b'abc', b'abc\x01']),             # accepted: no stale tail
    ('punctuate', 10 ** 6),                                                        # 'abc' (key 9) before 'abc\x01' (key 3)
    ('push', [(9, 300, 2 * 10 ** 6)], [b'other']),                                 # the evicted key under another name
    ('cycle', 8),                                                                  # take / restore_named until a rebuild
    ('restore', S.still_snapshot([1], [2]), [b'back']),                            # over key 1's dead entry (or a rebuilt table)
    ('push', [(9, 301, 2 * 10 ** 6 + 1), (1, 302, 2 * 10 ** 6 + 2), (7, 303, 2 * 10 ** 6 + 3)], [b'other', b'back', b'new']),
    ('refused', [(1, 304, 2 * 10 ** 6 + 4)], [b'wrong']),
]

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
from tests import formatter_ref as F
from tests import matched_points_ref as mref
from tests import sessions_ref as R
from tests import session_records_ref as S
from tests import session_names_ref as N
from tests import test_gpu_session_names as T

UB = N.UUID_BYTES
KEEP = []


def batch_arrays(b):
    nt = int(b.n_traces)
    off = _lib.device_to_numpy(b.trace_offsets, nt + 1, np.int64)
    n = int(off[-1])
    return {'trace_offsets': off, 'lat': _lib.device_to_numpy(b.lat, n, np.float64),
            'lon': _lib.device_to_numpy(b.lon, n, np.float64), 'time': _lib.device_to_numpy(b.time, n, np.int64),
            'accuracy': _lib.device_to_numpy(b.accuracy, n, np.float32),
            'mode': _lib.device_to_numpy(b.mode, nt, np.uint8), 'memory': int(b.memory)}


def refused(f, *a, **kw):
    """None, or what the refusal says: (text, point, reason, message) of a name refusal."""
    try:
        f(*a, **kw)
    except M.NameRefusal as e:
        return (str(e), e.point, e.reason, e.message)
    except ValueError as e:
        return (str(e), None, None, None)
    return None


def to_device(a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
    KEEP.append(t)
    return t.data_ptr()


def device_names(names):
    d = {k: to_device(names[k]) for k in ('bytes', 'off', 'len')}
    d['n_bytes'] = int(names['n_bytes'])
    return d


def device_points(pts):
    d = {k: to_device(pts[k]) for k, _ in R.POINT_TYPES}
    d['n'] = len(pts['key'])
    return d


def run_chunk(m, pts, names, answer=R.scripted_match, arrival=None, snapshots=True):
    rounds = []
    b, win = m.sessions_advance(pts, names=names)
    while b.n_traces > 0:
        arrays = batch_arrays(b)
        trig = [int(t) if arrival is None else int(arrival[int(t)]) for t in win['trigger']]
        ans = [answer([None] * int(n), k, t) for k, t, n in zip(win['key'], trig, win['n_points'])]
        done = m.sessions_commit([a[0] if a[0] is not None else 0 for a in ans], [0 if a[1] else 500 for a in ans])
        rounds.append({'batch': arrays, 'windows': done, 'snapshot': m.sessions_snapshot() if snapshots else None})
        b, win = m.sessions_advance(None)
    return rounds, batch_arrays(b)


def state(m):
    return {'snapshot': m.sessions_snapshot(), 'names': m.sessions_names()}


out = {}
if job != 'city':
    M.configure(M.default_config(gen.graph_path('tiny', graph_dir)))
    m = M.Matcher()
if job == 'baseline':
    for kind in ('named', 'plain'):
        m.sessions_open(uuid_bytes=UB if kind == 'named' else 0, **R.SCRIPT)
        recs = []
        for p in range(R.SCRIPT_CHUNKS):
            pts, ts = R.scripted_chunk(p)
            names = N.names_for(pts['key']) if kind == 'named' else None
            rounds, end = run_chunk(m, pts, names)
            rec = {'rounds': rounds, 'end_batch': end, 'snapshot': m.sessions_snapshot()}
            if kind == 'named':
                rec['names'] = m.sessions_names()
            rec['punctuate'] = m.sessions_punctuate(ts)
            rec['after'] = m.sessions_snapshot()
            if kind == 'named':
                rec['after_names'] = m.sessions_names()
            recs.append(rec)
        out[kind] = recs
        m.sessions_close()
elif job == 'refusals':
    out['cases'] = {}
    stored_keys = sorted(N.STORED)
    for name, (keys, names, want) in N.refusal_cases().items():
        m.sessions_open(uuid_bytes=UB, **T.SMALL)
        m.sessions_push(R.refusal_points(stored_keys), names=N.raw([N.STORED[k] for k in stored_keys]))
        pts = R.refusal_points(keys)
        c = {'before': state(m)}
        for how in ('host', 'device', 'advance'):
            if how == 'host':
                c[how] = refused(m.sessions_push, pts, names=names)
            elif how == 'device':
                dp, dn = device_points(pts), device_names(names)
                torch.cuda.synchronize()
                c[how] = refused(m.sessions_push, dp, device=True, names=dn)
            else:
                c[how] = refused(m.sessions_advance, pts, names=names)
            c['last_' + how] = m.sessions_last_refusal()
            c['after_' + how] = state(m)
        c['then'] = m.sessions_push(R.refusal_points(N.THEN_KEYS), names=N.THEN_NAMES)
        c['last_then'] = m.sessions_last_refusal()
        c['after_then'] = state(m)
        m.sessions_close()
        out['cases'][name] = c
    # the store's own refusals keep their precedence and messages
    m.sessions_open(uuid_bytes=UB, **dict(T.SMALL, max_sessions=2))
    bad_names = N.raw([b'x' * (UB + 1)] * 3)
    out['own'] = [refused(m.sessions_push, R.refusal_points([1, R.NO_ID, 2]), names=bad_names),
                  refused(m.sessions_push, R.refusal_points([1, 2, 3]), names=bad_names)]
    out['own_last'] = m.sessions_last_refusal()
    out['own_after'] = state(m)
    # which calls a store takes
    one = S.still_snapshot([40], [1])
    pts = R.refusal_points([1])
    out['unnamed_on_named'] = [refused(m.sessions_push, pts), refused(m.sessions_advance, pts),
                               refused(m.sessions_restore, one), refused(m.sessions_restore_records, *S.encode(one))]
    out['no_listing'] = refused(m.sessions_names)
    m.sessions_punctuate(0)
    m.sessions_close()
    m.sessions_open(**T.SMALL)
    out['named_on_plain'] = [refused(m.sessions_push, pts, names=[b'a']), refused(m.sessions_advance, pts, names=[b'a']),
                             refused(m.sessions_restore, one, names=[b'a']),
                             refused(m.sessions_restore_records, *S.encode(one), names=[b'a'])]
    m.sessions_snapshot()
    out['names_on_plain'] = refused(m.sessions_names)
    out['plain_after'] = m.sessions_snapshot()
    m.sessions_close()
    out['bad_uuid_bytes'] = [refused(m.sessions_open, uuid_bytes=b, **T.SMALL) for b in (-1, 256)]
    m.sessions_open(uuid_bytes=255, **T.SMALL)
    m.sessions_push(R.refusal_points([1, 2]), names=[b'q' * 255, b''])
    out['widest'] = state(m)
    m.sessions_close()
elif job == 'reuse':
    m.sessions_open(uuid_bytes=UB, **T.REUSE)
    steps = []
    for step in T.REUSE_STEPS:
        op = step[0]
        rec = {}
        if op == 'push':
            rounds, _ = run_chunk(m, R._still(step[1]), N.raw(step[2]), answer=T.whole)
            rec['windows'] = [r['windows'] for r in rounds]
        elif op == 'refused':
            rec['refused'] = refused(m.sessions_push, R._still(step[1]), names=N.raw(step[2]))
        elif op == 'punctuate':
            rec['punctuate'] = m.sessions_punctuate(step[1])
        elif op == 'cycle':
            rec['rebuilds_before'] = m.sessions_punctuate(0)['n_rebuilds']
            for _ in range(step[1]):
                snap = m.sessions_take(1, 0)
                m.sessions_restore(snap, names=m.sessions_names())
            rec['rebuilds_after'] = m.sessions_punctuate(0)['n_rebuilds']
        else:
            rec['restore'] = m.sessions_restore(step[1], names=step[2])
        rec.update(state(m))
        steps.append(rec)
    out['steps'] = steps
elif job == 'move':
    m.sessions_open(uuid_bytes=UB, **R.SCRIPT)
    for p in range(3):
        pts, ts = R.scripted_chunk(p)
        run_chunk(m, pts, N.names_for(pts['key']), snapshots=False)
        if p < 2:
            m.sessions_punctuate(ts)
    out['cut'] = state(m)
    exp = m.sessions_export_records()
    exp.pop('device')
    exp['names'] = m.sessions_names()
    out['export'] = exp
    out['parts'] = []
    for r in (0, 1):
        snap = m.sessions_take(2, r)
        out['parts'].append({'snapshot': snap, 'names': m.sessions_names()})
    out['after_take'] = state(m)
    out['runs'] = []
    pts3, ts3 = R.scripted_chunk(3)
    for r in (0, 1):
        m.sessions_close()
        m.sessions_open(uuid_bytes=UB, **R.SCRIPT)
        run = {'restore': m.sessions_restore(out['parts'][r]['snapshot'], names=out['parts'][r]['names'])}
        run['restored'] = state(m)
        idx = np.nonzero(pts3['key'] %% np.uint64(2) == np.uint64(r))[0]
        sub = {k: pts3[k][idx] for k, _ in R.POINT_TYPES}
        rounds, _ = run_chunk(m, sub, N.names_for(sub['key']), arrival=idx, snapshots=False)
        run.update({'windows': [x['windows'] for x in rounds], 'arrival': idx, 'after': state(m),
                    'punctuate': m.sessions_punctuate(ts3), 'end': state(m)})
        out['runs'].append(run)
    # the export's records and names, each one byte into an aligned device buffer
    m.sessions_close()
    m.sessions_open(uuid_bytes=UB, **R.SCRIPT)
    data, off, ln = _lib.pack_names(exp['names'])
    bufs = []
    for a in (exp['bytes'], data):
        b = torch.zeros(len(a) + 1, dtype=torch.uint8, device='cuda')
        b[1:] = torch.from_numpy(np.ascontiguousarray(a, np.uint8).copy())
        assert b.data_ptr() %% 16 == 0
        bufs.append(b)
    dn = {'bytes': bufs[1].data_ptr() + 1, 'n_bytes': len(data), 'off': to_device(off), 'len': to_device(ln)}
    dk, do = to_device(exp['key']), to_device(exp['rec_off'])
    torch.cuda.synchronize()
    out['records_restore'] = m.sessions_restore_records(dk, do, bufs[0].data_ptr() + 1, device=True,
                                                        n_records=len(exp['key']), n_bytes=len(exp['bytes']), names=dn)
    out['records_restored'] = state(m)
    m.sessions_close()
    # restore refusals
    m.sessions_open(uuid_bytes=UB, **T.SMALL)
    m.sessions_push(R.refusal_points([2]), names=[b'two'])
    snap = S.still_snapshot([1, 3], [1, 1])
    before = state(m)
    lay = N.raw([b'one', b'three'])
    lay['off'][1] = 5
    out['restore_refusals'] = {
        'long': refused(m.sessions_restore, snap, names=[b'one', b'x' * (UB + 1)]),
        'layout': refused(m.sessions_restore, snap, names=lay),
        'records_long': refused(m.sessions_restore_records, *S.encode(snap), names=[b'x' * (UB + 1), b'three']),
        'live_first': refused(m.sessions_restore, S.still_snapshot([2, 3], [1, 1]), names=[b'x' * (UB + 1), b'three']),
        'before_full': refused(m.sessions_restore, S.still_snapshot(list(range(10, 19)), [1] * 9),
                               names=[b'n'] * 8 + [b'x' * (UB + 1)]),
        'full': refused(m.sessions_restore, S.still_snapshot(list(range(10, 19)), [1] * 9), names=[b'n'] * 9)}
    out['restore_refusals_untouched'] = (before, state(m))
    out['restore_ok'] = m.sessions_restore(snap, names=[b'one', b'x' * UB])
    out['restore_ok_state'] = state(m)
elif job == 'text':
    csv = F.FORMATS['csv']
    m.sessions_open(uuid_bytes=UB, **T.SMALL)
    snap = S.still_snapshot([M.session_key(b'veh-A')], [1])
    m.sessions_restore(snap, names=[b'veh-B'])
    out['before'] = state(m)
    lines = [b'garbage', b'veh-C,52.5,13.4,100,4', b'veh-A,52.5,13.4,101,4', b'veh-C,52.5,13.4,102,4']
    out['refused'] = refused(m.sessions_push_text, b'\n'.join(lines), csv, timestamp=1000)
    out['last'] = m.sessions_last_refusal()
    out['after'] = state(m)
    f, s = m.sessions_push_text(b'\n'.join(lines[:2] + lines[3:]), csv, timestamp=1000)
    out['then'] = (f['n_points'], s['n_live'])
    out['then_last'] = m.sessions_last_refusal()
    out['then_state'] = state(m)
elif job == 'evict':
    rows = []
    for j in range(2):
        rows += [(k, 100 + j, 1000 + j) for k in N.EVICT_KEYS]
    pts = R._still(rows)
    for kind in ('named', 'plain'):
        m.sessions_open(uuid_bytes=UB if kind == 'named' else 0, **dict(T.SMALL, max_sessions=16))
        m.sessions_push(pts, names=N.raw(N.EVICT_NAMES * 2) if kind == 'named' else None)
        snap = m.sessions_snapshot()
        out[kind] = {'snapshot': snap, 'names': m.sessions_names() if kind == 'named' else None,
                     'punctuate': m.sessions_punctuate(10 ** 9), 'after': m.sessions_snapshot()}
        m.sessions_close()
else:
    path, pts = R.city_stream(graph_dir)
    M.configure(M.default_config(path, **mref.OPTIONS['gtt']))
    m = M.Matcher()
    csv = F.FORMATS['csv']
    msgs = F.render_sv(pts, csv)
    ts = np.asarray(pts['timestamp'], np.int64)
    n = len(msgs)
    half = n // 2
    end_ts = int(ts.max()) + R.CITY['session_gap'] + 1
    chunk = lambda a, b: (b'\n'.join(msgs[a:b]) + b'\n', None, ts[a:b])
    # the plain store, uninterrupted
    m.sessions_open(**R.CITY)
    m.tile_store_open(1 << 16, 3600, 1)
    one = SR.stream_text_tiles(m, [chunk(0, half), chunk(half, n)], csv, end_ts)
    out['plain'] = {'payloads': one['payloads'], 'counts': one['counts']}
    m.tile_store_close()
    m.sessions_close()
    # the named store: the first half, saved, closed, opened, loaded, the second half
    f = os.path.join(os.path.dirname(dst), 'named_sessions.npz')
    m.sessions_open(uuid_bytes=UB, **R.CITY)
    m.tile_store_open(1 << 16, 3600, 1)
    fs, s1 = m.sessions_push_text(chunk(0, half)[0], csv, timestamp=ts[:half], arrays=False)
    m.tile_store_add_session()
    out['mid'] = state(m)
    saved = SR.save_sessions(m, f)
    m.sessions_close()
    m.sessions_open(uuid_bytes=UB, **R.CITY)
    got = SR.load_sessions(m, f)
    assert saved == got['n_sessions']
    out['loaded'] = state(m)
    two = SR.stream_text_tiles(m, [chunk(half, n)], csv, end_ts)
    out['named'] = {'payloads': two['payloads'], 'windows': two['counts']['windows'] + s1['n_windows'],
                    'reports': two['counts']['reports'] + s1['n_reports']}
    m.tile_store_close()
    m.sessions_close()
    # a names file does not load into a plain store, nor a plain file into a named one
    m.sessions_open(**R.CITY)
    out['names_into_plain'] = refused(SR.load_sessions, m, f)
    m.sessions_close()
    out['point_keys'] = np.asarray(pts['key'])
pickle.dump(out, open(dst, 'wb'))
print('names ok')
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
            dst = str(tmp_path_factory.mktemp('names') / (job + '.pkl'))
            t0 = time.perf_counter()
            p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, dst, job)], env=env,
                               capture_output=True, text=True, timeout=240)
            assert p.returncode == 0 and 'names ok' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
            print('child %s: %.1f s' % (job, time.perf_counter() - t0))
            with open(dst, 'rb') as f:
                _RUNS[job] = pickle.load(f)
        return _RUNS[job]
    return get


def _same(got, want, fields, what=''):
    bad = R.differing(got, want, fields)
    assert not bad, (what, bad)


def _state(got, ref, what=''):
    """A device store's snapshot and names against the restatement's."""
    _same(got['snapshot'], ref.snapshot(), R.SNAPSHOT_FIELDS, what)
    assert got['names'] == ref.snapshot_names(), (what, got['names'], ref.snapshot_names())


class _Script:
    """The named restatement with scripted answers, remembering what it sent to the matcher."""

    def __init__(self, answer=R.scripted_match, uuid_bytes=UB, **cfg):
        self.seen = []
        self.answer = answer
        cfg = dict(cfg)
        cfg.pop('max_sessions', None)
        self.ref = N.Store(self.match, cfg.pop('max_points'), uuid_bytes, **cfg)

    def match(self, points, key, trigger):
        self.seen.append((trigger, points))
        return self.answer(points, key, trigger)

    def check_rounds(self, pts, names, rounds, what, batches=True):
        """The device store's rounds of one named chunk against the restatement consumed in rounds."""
        assert self.ref.begin(pts['key'], names) == (-1, 0), what
        rounds = list(rounds)
        n = 0
        for wins in R.push_rounds(self.ref, pts):
            assert rounds, '%s: the device store ran out of rounds' % (what,)
            g = rounds.pop(0)
            _same(g['windows'], R.windows_to_arrays(wins), [k for k, _ in R.WINDOW_FIELDS], what)
            if batches:
                b = g['batch']
                sent = [w for _, w in sorted(self.seen, key=lambda x: x[0])]
                flat = [q for w in sent for q in w]
                assert b['trace_offsets'].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in sent])]).tolist()
                _same(b, {'lat': np.array([q[0] for q in flat], np.float64), 'lon': np.array([q[1] for q in flat], np.float64),
                          'time': np.array([q[2] for q in flat], np.int64),
                          'accuracy': np.array([q[3] for q in flat], np.float32)}, ('lat', 'lon', 'time', 'accuracy'), what)
                _same(g['snapshot'], self.ref.snapshot(), R.SNAPSHOT_FIELDS, what)
            del self.seen[:]
            n += len(wins)
        assert not rounds, what
        self.ref.sync()
        return n

    def check_punctuate(self, ts, pun, what):
        ev, ne = self.ref.punctuate(ts)
        del self.seen[:]
        assert pun['n_evicted'] == ne and pun['n_live'] == len(self.ref.sessions), what
        _same(pun, R.windows_to_arrays(ev), ('key', 'trigger', 'n_points', 'trimmed'), what)
        return len(ev)


def _script_cfg():
    return {k: v for k, v in R.SCRIPT.items() if k != 'max_sessions'}


def test_baseline_beside_the_plain_store(run_job):
    """Job 1: the scripted stream with name = b'veh-%d' % key.  Rounds, batches and snapshots equal
    the restatement's and the plain store's; the names of every listing equal the restatement's;
    the evictions come in name order where the plain store's come in key order."""
    r = run_job('baseline')
    s = _Script(**_script_cfg())
    n_windows = n_evictions = reordered = 0
    for p, (g, q) in enumerate(zip(r['named'], r['plain'])):
        pts, ts = R.scripted_chunk(p)
        n_windows += s.check_rounds(pts, N.names_for(pts['key']), g['rounds'], p)
        assert len(g['rounds']) == len(q['rounds'])
        for a, b in zip(g['rounds'], q['rounds']):
            _same(a['windows'], b['windows'], [k for k, _ in R.WINDOW_FIELDS], p)
            _same(a['snapshot'], b['snapshot'], R.SNAPSHOT_FIELDS, p)
        _same(g['snapshot'], q['snapshot'], R.SNAPSHOT_FIELDS, p)
        _state(g, s.ref, p)
        n_evictions += s.check_punctuate(ts, g['punctuate'], p)
        _state({'snapshot': g['after'], 'names': g['after_names']}, s.ref, p)
        _same(g['after'], q['after'], R.SNAPSHOT_FIELDS, p)
        # the same sessions leave the plain store, in key order
        a, b = g['punctuate'], q['punctuate']
        assert sorted(a['key'].tolist()) == b['key'].tolist() and a['n_evicted'] == b['n_evicted']
        assert a['trigger'].tolist() == sorted(a['trigger'].tolist(), reverse=True)
        reordered += a['key'].tolist() != b['key'].tolist()
    assert n_windows > 30 and n_evictions > 10 and reordered > 0


def _refusal_text(want):
    return 'point %d: name %s (' % (want[0], {1: 'long', 2: 'collision', 3: 'layout'}[want[1]])


def test_refusals_leave_store_and_directory_untouched(run_job):
    """Job 2: every refusal case from host arrays, from device arrays and through advance_named:
    the point and the reason of the restatement, snapshot and names as before, and the chunk that
    follows (whose new keys the refused chunk had claimed) behaves as the restatement's."""
    r = run_job('refusals')
    cases = N.refusal_cases()
    assert set(r['cases']) == set(cases)
    for name, (keys, names, want) in cases.items():
        c = r['cases'][name]
        st = N.small_store({})
        stored = sorted(N.STORED)
        assert st.push_named(R.refusal_points(stored), N.raw([N.STORED[k] for k in stored])) == ((-1, 0), [])
        assert st.begin(keys, names) == want
        _state(c['before'], st, name)
        for how in ('host', 'device', 'advance'):
            assert c[how] and _refusal_text(want) in c[how][0] and c[how][1:] == (want[0], want[1], -1), (name, how, c[how])
            assert c['last_' + how] == {'point': want[0], 'message': -1, 'reason': want[1]}, (name, how)
            _state(c['after_' + how], st, (name, how))
        bad, wins = st.push_named(R.refusal_points(N.THEN_KEYS), N.THEN_NAMES)
        assert bad == (-1, 0) and not wins and c['then']['n_windows'] == 0 and c['then']['n_live'] == len(st.sessions) == 4
        assert c['last_then'] == {'point': -1, 'message': -1, 'reason': 0}
        _state(c['after_then'], st, name)
    assert {w[1] for _, _, w in cases.values()} == {N.E_LONG, N.E_COLLISION, N.E_LAYOUT}
    # the store's own refusals come first, with their messages
    assert 'OTR_NO_ID' in r['own'][0][0] and 'beyond max_sessions' in r['own'][1][0]
    assert all(x[1] is None for x in r['own']) and r['own_last']['reason'] == 0
    assert len(r['own_after']['snapshot']['key']) == 0 and r['own_after']['names'] == []
    assert all(x and 'uuid directory' in x[0] for x in r['unnamed_on_named']), r['unnamed_on_named']
    assert all(x and 'no uuid directory' in x[0] for x in r['named_on_plain']), r['named_on_plain']
    assert r['no_listing'] and 'no listing' in r['no_listing'][0]
    assert r['names_on_plain'] and 'no uuid directory' in r['names_on_plain'][0] and len(r['plain_after']['key']) == 0
    assert all(x and 'uuid_bytes' in x[0] for x in r['bad_uuid_bytes'])
    assert r['widest']['names'] == [b'q' * 255, b''] and r['widest']['snapshot']['key'].tolist() == [1, 2]


def test_slot_reuse_key_reuse_and_rebuilds(run_job):
    """Jobs 3 to 5: a 20-byte name's slot reused under a 3-byte name (the listing shows 3 bytes, a
    later point under it is accepted, and the eviction order sees no stale tail); an evicted key
    back under another name; names through take / restore_named cycles that rebuild the table and
    a restore over a dead entry."""
    steps = run_job('reuse')['steps']
    s = _Script(answer=whole, **REUSE)
    assert len(steps) == len(REUSE_STEPS)
    for i, (step, g) in enumerate(zip(REUSE_STEPS, steps)):
        op = step[0]
        if op == 'push':
            rounds = [{'windows': w} for w in g['windows']]
            n = s.check_rounds(R._still(step[1]), N.raw(step[2]), rounds, i, batches=False)
            assert (n == 1) == (i == 0)
        elif op == 'refused':
            assert s.ref.begin(R._still(step[1])['key'], N.raw(step[2])) == (0, N.E_COLLISION)
            assert g['refused'][1:3] == (0, N.E_COLLISION)
        elif op == 'punctuate':
            assert s.check_punctuate(step[1], g['punctuate'], i) == 2
            assert g['punctuate']['key'].tolist() == [9, 3] and g['punctuate']['trigger'].tolist() == [-1, -2]
        elif op == 'cycle':
            assert g['rebuilds_after'] > g['rebuilds_before']
        else:
            assert N.restore_named(s.ref, step[1], N.raw(step[2]), REUSE['max_sessions']) == (-1, 0)
            assert g['restore']['n_sessions'] == 1
        _state(g, s.ref, i)
    assert steps[0]['names'] == [] and steps[1]['names'] == [b'abc\x01', b'abc']
    assert steps[4]['names'] == [b'other'] and steps[-1]['names'] == [b'back', b'new', b'other']


def test_take_and_restore_named_in_two_parts(run_job):
    """Job 6: the named store after chunk 2's push taken apart by key % 2 with its names, each part
    restored into a fresh named store and fed its share of chunk 3; the export's records and names
    restored from odd device addresses; the restore's refusals."""
    r = run_job('move')
    s = _Script(**_script_cfg())
    for p in range(3):
        pts, ts = R.scripted_chunk(p)
        assert s.ref.push_named(pts, N.names_for(pts['key']))[0] == (-1, 0)
        if p < 2:
            s.ref.punctuate(ts)
    _state(r['cut'], s.ref)
    key, rec_off, data = S.encode(s.ref.snapshot())
    e = r['export']
    assert e['key'].tolist() == key.tolist() and e['rec_off'].tolist() == rec_off.tolist() and e['bytes'].tobytes() == data
    assert e['names'] == s.ref.snapshot_names() and len(e['names']) > 10
    _state(r['records_restored'], s.ref, 'records')
    assert r['records_restore']['n_sessions'] == len(key)
    parts = [N.take(s.ref, 2, part, False) for part in (0, 1)]
    for part in (0, 1):
        want_snap, want_names = parts[part]
        assert len(want_names) > 0
        _same(r['parts'][part]['snapshot'], want_snap, R.SNAPSHOT_FIELDS, part)
        assert r['parts'][part]['names'] == want_names
        _same(r['runs'][part]['restored']['snapshot'], want_snap, R.SNAPSHOT_FIELDS, part)
        assert r['runs'][part]['restored']['names'] == want_names
    assert len(r['after_take']['snapshot']['key']) == 0 and r['after_take']['names'] == []
    pts3, ts3 = R.scripted_chunk(3)
    bad, wins = s.ref.push_named(pts3, N.names_for(pts3['key']))
    assert bad == (-1, 0)
    want = R.windows_to_arrays(wins)
    rows = []
    for run in r['runs']:
        for w in run['windows']:
            for j in range(len(w['key'])):
                rows.append(tuple(int(run['arrival'][w['trigger'][j]]) if k == 'trigger' else int(w[k][j])
                                  for k, _ in R.WINDOW_FIELDS))
    rows.sort(key=lambda x: x[1])
    _same({k: np.array([x[j] for x in rows], dt) for j, (k, dt) in enumerate(R.WINDOW_FIELDS)}, want,
          [k for k, _ in R.WINDOW_FIELDS])
    assert len(rows) > 10
    for part, run in enumerate(r['runs']):
        snap, names = N.take(s.ref, 2, part, False)
        _same(run['after']['snapshot'], snap, R.SNAPSHOT_FIELDS, part)
        assert run['after']['names'] == names
    ev, ne = s.ref.punctuate(ts3)
    assert sum(run['punctuate']['n_evicted'] for run in r['runs']) == ne
    for part, run in enumerate(r['runs']):   # each part evicts its share, in name order
        mine = [w['key'] for w in ev if w['key'] % 2 == part]
        assert run['punctuate']['key'].tolist() == mine
        snap, names = N.take(s.ref, 2, part, False)
        _same(run['end']['snapshot'], snap, R.SNAPSHOT_FIELDS, part)
        assert run['end']['names'] == names
    f = r['restore_refusals']
    for k, where, reason in (('long', 'session 1: ', 'name'), ('layout', 'session 1: ', 'name'),
                             ('records_long', 'session 0: ', 'name'), ('live_first', 'session 0: ', 'live'),
                             ('before_full', 'session 8: ', 'name'), ('full', '', 'full')):
        assert f[k] and 'refused: %s%s (' % (where, reason) in f[k][0], (k, f[k])
    before, after = r['restore_refusals_untouched']
    _same(after['snapshot'], before['snapshot'], R.SNAPSHOT_FIELDS)
    assert after['names'] == before['names'] == [b'two']
    assert r['restore_ok']['n_sessions'] == 2 and r['restore_ok_state']['names'] == [b'one', b'two', b'x' * UB]


def test_collision_across_a_restore_through_text(run_job):
    """Job 7: a session restored under key otr_uuid_key(b'veh-A') with the name b'veh-B'; a message
    of uuid veh-A is then refused, with its arrival index among the messages, the store untouched."""
    r = run_job('text')
    assert F.uuid_hash(b'veh-A') == int(r['before']['snapshot']['key'][0]) and r['before']['names'] == [b'veh-B']
    assert r['refused'] and r['refused'][1:] == (1, N.E_COLLISION, 2), r['refused']
    assert r['last'] == {'point': 1, 'message': 2, 'reason': N.E_COLLISION}
    _same(r['after']['snapshot'], r['before']['snapshot'], R.SNAPSHOT_FIELDS)
    assert r['after']['names'] == [b'veh-B']
    assert r['then'] == (2, 2) and r['then_last']['reason'] == 0
    want = sorted([(F.uuid_hash(b'veh-A'), b'veh-B'), (F.uuid_hash(b'veh-C'), b'veh-C')])
    assert r['then_state']['snapshot']['key'].tolist() == [k for k, _ in want]
    assert r['then_state']['names'] == [nm for _, nm in want]


def test_evictions_in_name_order(run_job):
    """Job 8: the key order is the reverse of the name order; a prefix pair, pairs first differing
    at byte 9 and at byte uuid_bytes (three sort words).  Windows, triggers and ranks as the
    restatement's; the plain store still goes by key."""
    r = run_job('evict')
    rows = []
    for j in range(2):
        rows += [(k, 100 + j, 1000 + j) for k in N.EVICT_KEYS]
    cfg = dict(SMALL)
    cfg.pop('max_sessions')
    st = N.Store(lambda points, key, trigger: (None, True, []), cfg.pop('max_points'), UB, **cfg)
    assert st.push_named(R._still(rows), N.raw(N.EVICT_NAMES * 2))[0] == (-1, 0)
    g = r['named']
    _state(g, st)
    ev, ne = st.punctuate(10 ** 9)
    assert ne == len(N.EVICT_KEYS) == len(ev) == g['punctuate']['n_evicted']
    _same(g['punctuate'], R.windows_to_arrays(ev), ('key', 'trigger', 'n_points', 'trimmed'))
    assert g['punctuate']['key'].tolist() == N.EVICT_KEYS
    assert g['punctuate']['trigger'].tolist() == [-1 - i for i in range(ne)]
    assert len(g['after']['key']) == 0
    q = r['plain']
    assert q['punctuate']['key'].tolist() == sorted(N.EVICT_KEYS)
    assert q['punctuate']['trigger'].tolist() == [-1 - i for i in range(ne)]
    _same(q['snapshot'], g['snapshot'], R.SNAPSHOT_FIELDS)


def test_city_stream_on_a_named_store(run_job):
    """Job 9, real matching: the city stream as messages through stream_text_tiles on a named store,
    saved and loaded half way, gives the payloads and counts of the uninterrupted plain store; the
    names of the live sessions are their uuids, through the file too."""
    r = run_job('city')
    assert r['named']['payloads'] == r['plain']['payloads'] and len(r['plain']['payloads']) > 0
    assert (r['named']['windows'], r['named']['reports']) == (r['plain']['counts']['windows'], r['plain']['counts']['reports'])
    assert r['plain']['counts']['windows'] > 100
    uuid = {F.uuid_hash(F.uuid_of_key(k)): F.uuid_of_key(k) for k in set(r['point_keys'].tolist())}
    mid = r['mid']
    assert len(mid['names']) > 5 and mid['names'] == [uuid[int(k)] for k in mid['snapshot']['key']]
    _same(r['loaded']['snapshot'], mid['snapshot'], R.SNAPSHOT_FIELDS)
    assert r['loaded']['names'] == mid['names']
    assert r['names_into_plain'] and 'no uuid directory' in r['names_into_plain'][0]
