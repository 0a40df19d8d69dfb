"""The session store in HBM (K14, include/otr.h otr_sessions_*) against its restatement
tests/sessions_ref.py: scripted rounds through advance / commit with the snapshot compared after
every commit (max_sep by bits) and the emitted batches too; real matching on the city stream,
where any chunking gives the same windows, reports and snapshot, equal to the restatement driven
by match_batch on each window alone; punctuate; capacity and refusals; and match_batch itself
unmoved by a store.  What the streams cover is pinned by tests/test_sessions_cpu.py.  One child
process per job."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import sessions_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOBS = ('scripted', 'city_gtt', 'city_deployed', 'punctuate', 'refusals', 'unmoved')
CHILD = r'''
import sys, pickle, ctypes
sys.path.insert(0, %r)
graph_dir, dst, job = %r, %r, %r
import numpy as np
import torch
from reporter_amd import matcher as M
from reporter_amd import _lib
from reporter_amd.tools import gen
from tests import matched_points_ref as mref
from tests import sessions_ref as R


class DevArr:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {'shape': (n,), 'typestr': typestr, 'data': (int(ptr), False), 'version': 2}


def dev(ptr, n, dt):
    if n == 0:
        return np.zeros(0, dt)
    return torch.as_tensor(DevArr(ptr, n, np.dtype(dt).str), device='cuda').clone().cpu().numpy()


def batch_arrays(b):
    nt = int(b.n_traces)
    off = dev(b.trace_offsets, nt + 1, np.int64)
    n = int(off[-1])
    return {'trace_offsets': off, 'lat': dev(b.lat, n, np.float64), 'lon': dev(b.lon, n, np.float64),
            'time': dev(b.time, n, np.int64), 'accuracy': dev(b.accuracy, n, np.float32),
            'mode': dev(b.mode, nt, np.uint8), 'memory': int(b.memory)}


def refused(f, *a):
    try:
        f(*a)
    except ValueError as e:
        return str(e)
    return None


out = {}
if job == 'scripted':
    M.configure(M.default_config(gen.graph_path('tiny', graph_dir)))
    m = M.Matcher()
    m.sessions_open(**R.SCRIPT)
    out['chunks'] = []
    for p in range(R.SCRIPT_CHUNKS):
        pts, ts = R.scripted_chunk(p)
        rounds = []
        b, win = m.sessions_advance(pts)
        while b.n_traces > 0:
            arrays = batch_arrays(b)
            ans = [R.scripted_match([None] * int(n), k, t) for k, t, n in zip(win['key'], win['trigger'], win['n_points'])]
            done = m.sessions_commit([a[0] if a[0] is not None else 0 for a in ans], [0 if a[1] else 500 for a in ans])
            rounds.append({'batch': arrays, 'windows': done, 'snapshot': m.sessions_snapshot()})
            b, win = m.sessions_advance(None)
        out['chunks'].append({'rounds': rounds, 'end_batch': batch_arrays(b), 'snapshot': m.sessions_snapshot(),
                              'punctuate': m.sessions_punctuate(ts), 'after': m.sessions_snapshot()})
elif job.startswith('city'):
    cfg = job[5:]
    path, pts = R.city_stream(graph_dir)
    M.configure(M.default_config(path, **mref.OPTIONS[cfg]))
    m = M.Matcher()
    n = len(pts['key'])
    second = [0] + [i for i in range(1, n) if pts['time'][i] != pts['time'][i - 1]] + [n]
    cuts = {'one': [0, n], 'second': second, 'seven': list(range(0, n, 7)) + [n], 'split': [0, n]}
    end_ts = int(pts['timestamp'].max()) + R.CITY['session_gap'] + 1
    for name, c in cuts.items():
        m.sessions_open(batch_probes=100 if name == 'split' else 0, **R.CITY)
        res = [m.sessions_push(R.take(pts, c[i], c[i + 1])) for i in range(len(c) - 1)]
        out[name] = {'result': R.by_trigger(R.concat(res, c[:-1])), 'snapshot': m.sessions_snapshot(),
                     'rounds': sum(r['n_rounds'] for r in res), 'punctuate': m.sessions_punctuate(end_ts),
                     'after': m.sessions_snapshot(), 'ms': sum(r['device_ms'] for r in res)}
        m.sessions_close()

    def match(points, key, trigger):
        r = m.match_batch(R.window_traces(points), copy_out=True)
        return R.result_to_match(_lib.result_to_numpy(r), int(r.trace_status[0]))

    ref = R.Store(match, **{k: v for k, v in R.CITY.items() if k != 'max_sessions'})
    out['want'] = {'result': R.windows_to_arrays(ref.push(pts)), 'snapshot': ref.snapshot()}
    ev, ne = ref.punctuate(end_ts)
    out['want']['punctuate'] = R.windows_to_arrays(ev)
    out['want']['n_evicted'] = ne
elif job == 'punctuate':
    M.configure(M.default_config(gen.graph_path('tiny', graph_dir)))
    m = M.Matcher()
    m.sessions_open(8, 8, report_dist=1e9, report_count=99, report_time=0, session_gap=60000)
    out['pushed'] = m.sessions_push(R.PUNCTUATE_POINTS)
    out['steps'] = []
    for ts in R.PUNCTUATE_TS:
        out['steps'].append({'result': m.sessions_punctuate(ts), 'snapshot': m.sessions_snapshot()})
elif job == 'refusals':
    M.configure(M.default_config(gen.graph_path('tiny', graph_dir)))
    m = M.Matcher()
    empty = {k: np.zeros(0, dt) for k, dt in R.POINT_TYPES}
    out['no_store'] = [refused(m.sessions_push, empty), refused(m.sessions_punctuate, 0), refused(m.sessions_snapshot)]
    m.sessions_open(4, 4, report_dist=500.0, report_count=3, report_time=0, session_gap=60000)
    out['twice'] = refused(m.sessions_open, 4, 4)
    out['first'] = m.sessions_push(R.refusal_points([1, 2, 3, 1, 2]))
    out['before'] = m.sessions_snapshot()
    out['too_many'] = refused(m.sessions_push, R.refusal_points([1, 4, 5, 2]))
    out['after_too_many'] = m.sessions_snapshot()
    out['no_id'] = refused(m.sessions_push, R.refusal_points([1, R.NO_ID]))
    out['after_no_id'] = m.sessions_snapshot()
    out['fits'] = m.sessions_push(R.refusal_points([4, 1]))
    out['after_fits'] = m.sessions_snapshot()
    out['forced'] = m.sessions_push(R.refusal_points([3, 3, 3]))
    out['empty'] = m.sessions_push(empty)
    b, win = m.sessions_advance(empty)
    out['empty_batch'] = batch_arrays(b)
    out['empty_windows'] = win
    out['commit_nothing'] = refused(m.sessions_commit, [])
else:
    from tests import ragged
    path, tr = ragged.ragged_city(graph_dir)
    M.configure(ragged.engine_config(path, 'gtt'))
    m = M.Matcher()
    out['before'] = {k: np.asarray(v) for k, v in m.match_batch_numpy(tr).items()}
    m.sessions_open(**R.CITY)
    _, pts = R.city_stream(graph_dir)
    out['windows'] = m.sessions_push(pts)['n_windows']
    out['after'] = {k: np.asarray(v) for k, v in m.match_batch_numpy(tr).items()}
    m.sessions_close()
    out['closed'] = {k: np.asarray(v) for k, v in m.match_batch_numpy(tr).items()}
pickle.dump(out, open(dst, 'wb'))
print('sessions ok')
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
            dst = str(tmp_path_factory.mktemp('sessions') / (job + '.pkl'))
            t0 = time.perf_counter()
            p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, dst, job)], env=env,
                               capture_output=True, text=True, timeout=240)
            assert p.returncode == 0 and 'sessions ok' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
            print('child %s: %.1f s' % (job, time.perf_counter() - t0))
            with open(dst, 'rb') as f:
                _RUNS[job] = pickle.load(f)
        return _RUNS[job]
    return get


def _same(got, want, fields):
    bad = R.differing(got, want, fields)
    assert not bad, bad


def test_scripted_rounds(run_job):
    """advance / commit with scripted shape_used, no matcher in the loop: batches, windows and the
    snapshot after every commit equal the restatement consumed in rounds; the key table (32
    entries, 56 keys passing through) is rebuilt on the way."""
    chunks = run_job('scripted')['chunks']
    seen = []

    def match(points, key, trigger):
        seen.append((trigger, points))
        return R.scripted_match(points, key, trigger)

    ref = R.Store(match, **{k: v for k, v in R.SCRIPT.items() if k != 'max_sessions'})
    n_rounds = n_windows = 0
    for p, got in enumerate(chunks):
        pts, ts = R.scripted_chunk(p)
        rounds = list(got['rounds'])
        for wins in R.push_rounds(ref, pts):
            assert rounds, 'chunk %d: the device store ran out of rounds' % p
            g = rounds.pop(0)
            want = R.windows_to_arrays(wins)
            _same(g['windows'], want, [k for k, _ in R.WINDOW_FIELDS])
            assert np.all(np.diff(g['windows']['trigger']) > 0)
            # the batch: offsets, six-decimal coordinates, times, float accuracies, mode auto, in HBM
            b = g['batch']
            sent = [w for _, w in sorted(seen, key=lambda x: x[0])]   # the round's windows by trigger
            flat = [q for w in sent for q in w]
            assert b['memory'] == 1 and b['mode'].tolist() == [0] * len(wins)
            assert b['trace_offsets'].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in sent])]).tolist()
            _same(b, {'lat': np.array([q[0] for q in flat], np.float64), 'lon': np.array([q[1] for q in flat], np.float64),
                      'time': np.array([q[2] for q in flat], np.int64),
                      'accuracy': np.array([q[3] for q in flat], np.float32)}, ('lat', 'lon', 'time', 'accuracy'))
            del seen[:]
            _same(g['snapshot'], ref.snapshot(), R.SNAPSHOT_FIELDS)
            n_rounds += 1
            n_windows += len(wins)
        assert not rounds and got['end_batch']['trace_offsets'].tolist() == [0]
        _same(got['snapshot'], ref.snapshot(), R.SNAPSHOT_FIELDS)
        ev, ne = ref.punctuate(ts)
        del seen[:]
        pun = got['punctuate']
        assert pun['n_evicted'] == ne and pun['n_live'] == len(ref.sessions)
        _same(pun, R.windows_to_arrays(ev), ('key', 'trigger', 'n_points', 'trimmed'))
        _same(got['after'], ref.snapshot(), R.SNAPSHOT_FIELDS)
    print('scripted: %d rounds, %d windows, %d rebuilds' % (n_rounds, n_windows, chunks[-1]['punctuate']['n_rebuilds']))
    assert n_windows > 100 and chunks[-1]['punctuate']['n_rebuilds'] >= 1


@pytest.mark.parametrize('cfg', ['gtt', 'deployed'])
def test_real_matching_any_chunking(cfg, run_job):
    r = run_job('city_' + cfg)
    want = r['want']
    print('city %s: %d windows, %d reports; rounds %s; device ms %s' % (
        cfg, len(want['result']['key']), len(want['result']['id']),
        {k: r[k]['rounds'] for k in ('one', 'second', 'seven', 'split')},
        {k: round(r[k]['ms'], 1) for k in ('one', 'second', 'seven', 'split')}))
    assert len(want['result']['key']) > 100 and len(want['result']['id']) > 0
    for name in ('one', 'second', 'seven', 'split'):
        _same(r[name]['result'], want['result'], R.RESULT_FIELDS)
        _same(r[name]['snapshot'], want['snapshot'], R.SNAPSHOT_FIELDS)
        pun = r[name]['punctuate']
        _same(pun, want['punctuate'], R.RESULT_FIELDS)
        assert pun['n_evicted'] == want['n_evicted'] > pun['n_windows'] > 0
        assert len(r[name]['after']['key']) == 0 and pun['n_live'] == 0
    assert r['one']['rounds'] > 1


def test_punctuate(run_job):
    """Stale and fresh sessions mixed: evictions in ascending key order, reporting (n >= 2, elapsed
    >= 0) or not, a session exactly at the gap stays, and the evicted keys are gone."""
    r = run_job('punctuate')
    ref = R.Store(lambda points, key, trigger: (None, True, []), 8, 1e9, 99, 0, 60000)
    assert ref.push(R.PUNCTUATE_POINTS) == [] and r['pushed']['n_windows'] == 0
    for ts, got in zip(R.PUNCTUATE_TS, r['steps']):
        ev, ne = ref.punctuate(ts)
        assert got['result']['n_evicted'] == ne and got['result']['n_live'] == len(ref.sessions)
        _same(got['result'], R.windows_to_arrays(ev), ('key', 'trigger', 'n_points', 'trimmed'))
        _same(got['snapshot'], ref.snapshot(), R.SNAPSHOT_FIELDS)
    first = r['steps'][0]['result']
    assert first['key'].tolist() == [5, 12] and first['trigger'].tolist() == [-3, -4] and first['n_evicted'] == 4
    assert r['steps'][0]['snapshot']['key'].tolist() == [9, 11]
    assert r['steps'][1]['result']['n_evicted'] == 1 and r['steps'][1]['snapshot']['key'].tolist() == [9]
    assert len(r['steps'][2]['snapshot']['key']) == 0


def test_capacity_and_refusals(run_job):
    r = run_job('refusals')
    assert all(e and 'otr_sessions_open' in e for e in r['no_store'])
    assert r['twice'] and 'already' in r['twice']
    assert r['first']['n_windows'] == 0 and r['first']['n_live'] == 3
    assert r['too_many'] and 'max_sessions' in r['too_many']
    _same(r['after_too_many'], r['before'], R.SNAPSHOT_FIELDS)
    assert r['no_id'] and 'OTR_NO_ID' in r['no_id']
    _same(r['after_no_id'], r['before'], R.SNAPSHOT_FIELDS)
    # the store still works: key 4 fits, key 1 goes on
    assert r['fits']['n_live'] == 4 and r['after_fits']['key'].tolist() == [1, 2, 3, 4]
    assert np.diff(r['after_fits']['point_off']).tolist() == [3, 2, 1, 1]
    # key 3 stands still: its 4th point reaches the cap and is reported by force
    f = r['forced']
    assert (f['n_forced'], f['n_dropped'], f['n_windows']) == (1, 0, 1)
    assert f['key'].tolist() == [3] and f['trigger'].tolist() == [2] and f['n_points'].tolist() == [4]
    e = r['empty']
    assert (e['n_windows'], e['n_rounds'], e['rep_off'].tolist()) == (0, 0, [0])
    assert r['empty_batch']['trace_offsets'].tolist() == [0] and r['empty_windows']['n_windows'] == 0
    assert r['commit_nothing'] and 'commit' in r['commit_nothing']


def test_match_batch_unmoved(run_job):
    """match_batch on the ragged batch before a store exists, after it was used and after it was
    closed: bit-identical (candidate slots past cand_count are workspace, not results)."""
    r = run_job('unmoved')
    assert r['windows'] > 0

    def defined(res):
        out = dict(res)
        live = np.arange(res['cand_edge'].shape[1])[None, :] < res['cand_count'][:, None]
        for k in ('cand_edge', 'cand_p', 'cand_sqd'):
            out[k] = np.where(live, res[k], 0)
        return out

    before = defined(r['before'])
    for other in ('after', 'closed'):
        got = defined(r[other])
        for k, a in before.items():
            b = got[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (other, k)
