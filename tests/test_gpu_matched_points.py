"""k_matched_points (K12) against its restatement tests/matched_points_ref.py, bit for bit on
all eight per-probe arrays, the reference computed from the same GPU result (compare() holds
that result equal to the oracle's): the city 1 Hz batch under deployed and gtt at the default
interpolation distance and at 250 m (gaps of more than 64 probes, 9 pieces), the ragged batch
(empty and one-probe traces, no active state, forced steps, more than 60 sub-paths), an arc
of more than 100 shape segments and the known-answer road.  On the ragged batch also: the
flag changes nothing else, no flag means OTR_BAD_REQUEST, a trace's points do not depend on
its neighbours, and device inputs without a copy-out give the same arrays in HBM.  What the
batches cover is pinned by tests/test_matched_points_cpu.py.  One child process per
configuration."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle.compare import compare
from tests import matched_points_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# job -> (batch, configuration: tests/ragged.py CONFIGS for 'ragged', ref.OPTIONS otherwise)
JOBS = {
    'city_deployed': ('city', 'deployed'), 'city_gtt': ('city', 'gtt'),
    'city_deployed250': ('city', 'deployed250'), 'city_gtt250': ('city', 'gtt250'),
    'ragged_gtt': ('ragged', 'gtt'), 'arc': ('arc', 'gtt50'), 'kat': ('kat', 'gtt50'),
}
CHILD = r'''
import sys, pickle, ctypes
sys.path.insert(0, %r)
graph_dir, dst, batch, cfg = %r, %r, %r, %r
import numpy as np
import torch
from reporter_amd import matcher as M
from reporter_amd import _lib
from tests import matched_points_ref as ref
from tests import ragged

TYPES = {'kind': '|u1', 'edge': '<u4', 'frac': '<f8', 'lat': '<f8', 'lon': '<f8', 'dist': '<f8', 'state': '<i8',
         'pos_mm': '<i8'}


class DevArr:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {'shape': (n,), 'typestr': typestr, 'data': (int(ptr), False), 'version': 2}


def run(m, tr, **kw):
    r = m.match_batch(tr, copy_out=True, matched_points=True, timing=True, **kw)
    pr = m.matched_points_result()
    return {'res': {k: np.asarray(v) for k, v in _lib.result_to_numpy(r).items()}, 'status': int(r.status),
            'pts': _lib.points_to_numpy(pr), 'n': int(pr.n_probes), 'ms': float(pr.kernel_ms)}


if batch == 'ragged':
    path, tr = ragged.ragged_city(graph_dir)
    M.configure(ragged.engine_config(path, cfg))
else:
    built = getattr(ref, batch)(graph_dir)
    path, tr = built[0], built[1]
    M.configure(M.default_config(path, **ref.OPTIONS[cfg]))
m = M.Matcher()
out = {'flagged': run(m, tr)}
if batch == 'ragged':
    # without the flag: the same result, and no points
    r = m.match_batch(tr, copy_out=True)
    out['plain'] = {k: np.asarray(v) for k, v in _lib.result_to_numpy(r).items()}
    pr = _lib.PointResult()
    out['plain_rc'] = int(_lib.lib().otr_matched_points(m._h, ctypes.byref(pr)))
    out['plain_error'] = _lib.last_error()
    out['shuffled'] = run(m, ragged.reorder(tr, ragged.PERMS['shuffled']))
    # device inputs, no copy-out: the d_* arrays
    dev = {'trace_offsets': torch.from_numpy(np.ascontiguousarray(tr.offsets, np.int64)).cuda(),
           'lat': torch.from_numpy(np.ascontiguousarray(tr.lat, np.float64)).cuda(),
           'lon': torch.from_numpy(np.ascontiguousarray(tr.lon, np.float64)).cuda(),
           'time': torch.from_numpy(np.ascontiguousarray(tr.time, np.int64)).cuda(),
           'mode': torch.from_numpy(np.ascontiguousarray(tr.mode, np.uint8)).cuda()}
    torch.cuda.synchronize()
    m.match_batch(tr, copy_out=False, matched_points=True,
                  device_arrays={k: v.data_ptr() for k, v in dev.items()})
    pr = m.matched_points_result()
    n = int(pr.n_probes)
    out['device_host_null'] = not pr.kind and not pr.pos_mm
    out['device'] = {k: torch.as_tensor(DevArr(getattr(pr, 'd_' + k), n, t), device='cuda').clone().cpu().numpy()
                     for k, t in TYPES.items()}
pickle.dump(out, open(dst, 'wb'))
print('matched points ok')
'''

_RUNS = {}


@pytest.fixture(scope='module')
def run_job(graph_dir, tmp_path_factory):
    def get(job):
        if job not in _RUNS:
            batch, cfg = JOBS[job]
            env = dict(os.environ)
            for k in ('OTR_VIT_SPLIT', 'OTR_TIERS', 'OTR_EST_K', 'OTR_LIB', 'OTR_SMALL_KEYS', 'OTR_SMALL_PATH_KEYS',
                      'OTR_TINY_KEYS'):
                env.pop(k, None)
            dst = str(tmp_path_factory.mktemp('matched_points') / (job + '.pkl'))
            t0 = time.perf_counter()
            p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, dst, batch, cfg)], env=env,
                               capture_output=True, text=True, timeout=240)
            assert p.returncode == 0 and 'matched points ok' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
            print('child %s: %.1f s' % (job, time.perf_counter() - t0))
            with open(dst, 'rb') as f:
                _RUNS[job] = pickle.load(f)
        return _RUNS[job]
    return get


def _batch(job, graph_dir):
    from reporter_amd.graphfile import GraphFile
    batch, _ = JOBS[job]
    if batch == 'ragged':
        from tests import ragged
        path, tr = ragged.ragged_city(graph_dir)
    else:
        built = getattr(ref, batch)(graph_dir)
        path, tr = built[0], built[1]
    return GraphFile(path), tr


def _report(got, want):
    """The first differing probes of every array that differs."""
    msg = []
    for k in ref.same_bits(got, want):
        i = np.flatnonzero(np.asarray(got[k]) != np.asarray(want[k]))[:5]
        msg.append('%s: %d differ, first %s got %s want %s' % (k, len(i), i.tolist(), got[k][i].tolist(),
                                                               want[k][i].tolist()))
    return msg


@pytest.mark.parametrize('job', list(JOBS))
def test_bit_exact(job, run_job, graph_dir):
    got = run_job(job)['flagged']
    G, tr = _batch(job, graph_dir)
    assert got['status'] == 0 and got['n'] == tr.n_probes
    want = ref.matched_points(got['res'], tr, G)
    kinds = np.bincount(got['pts']['kind'], minlength=3)
    print('%s: kinds %s, K12 %.3f ms' % (job, kinds.tolist(), got['ms']))
    assert not _report(got['pts'], want)
    assert kinds[1] > 0 and got['ms'] > 0.0


def test_flag_changes_nothing_else(run_job):
    r = run_job('ragged_gtt')
    errors, stats = compare(r['flagged']['res'], r['plain'])
    assert not errors and all(stats.values()), (errors, stats)
    assert r['plain_rc'] == 400 and 'OTR_BATCH_MATCHED_POINTS' in r['plain_error']


def test_points_do_not_depend_on_neighbours(run_job, graph_dir):
    from tests import ragged
    r = run_job('ragged_gtt')
    _, tr = ragged.ragged_city(graph_dir)
    p = ragged.PERMS['shuffled']
    moved = ragged.reorder(tr, p)
    pos = np.argsort(np.asarray(p))   # trace t of the original is trace pos[t] of the shuffled batch
    sel = np.concatenate([np.arange(moved.offsets[q], moved.offsets[q + 1]) for q in pos] + [np.zeros(0, np.int64)])
    got, want = r['shuffled']['pts'], r['flagged']['pts']
    # states are numbered through the batch: compare them relative to their trace's first state
    soff_m, soff = r['shuffled']['res']['trace_state_off'], r['flagged']['res']['trace_state_off']
    back = {k: np.asarray(got[k])[sel] for k in ref.FIELDS}
    shift = np.concatenate([np.full(int(tr.offsets[t + 1] - tr.offsets[t]), int(soff[t]) - int(soff_m[pos[t]]), np.int64)
                            for t in range(tr.n_traces)] + [np.zeros(0, np.int64)])
    back['state'] = np.where(back['state'] >= 0, back['state'] + shift, -1)
    assert not _report(back, want)


def test_device_inputs_without_copy_out(run_job):
    r = run_job('ragged_gtt')
    assert r['device_host_null']
    assert not _report(r['device'], r['flagged']['pts'])
