"""k_edge_traversals (K13) against its restatement tests/edge_traversals_ref.py, bit for bit on
all eleven arrays, the reference computed from the same GPU result: the ragged batch under gtt
and deployed (traces with more than 128 traversals and with none, zero-length traversals, steps
back onto the edge just left, one-traversal sub-paths), the city 1 Hz batch and the two
known-answer roads.  The speed entries by composition: otr_edge_observations reduced by
otr_hist_reduce equals the oracle's reduction of the restatement's entries.  On the ragged
batch also: the flag changes nothing else, no flag means OTR_BAD_REQUEST, it does not disturb
the matched points (K12) nor they it, a trace's traversals do not depend on its neighbours,
device inputs without a copy-out give the same arrays in HBM, and an empty batch has no
traversal.  What the batches cover is pinned by tests/test_edge_traversals_cpu.py.  One child
process per job."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle import hist as oh
from oracle.compare import compare
from tests import edge_traversals_ref as ref
from tests import matched_points_ref as mref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# job -> (batch, configuration: tests/ragged.py CONFIGS for 'ragged', matched_points_ref.OPTIONS otherwise)
JOBS = {
    'ragged_gtt': ('ragged', 'gtt'), 'ragged_deployed': ('ragged', 'deployed'), 'city_gtt': ('city', 'gtt'),
    'kat': ('kat', 'gtt50'), 'kat3': ('kat3', 'gtt50'),
}
CHILD = r'''
import sys, pickle, ctypes
sys.path.insert(0, %r)
graph_dir, dst, batch, cfg = %r, %r, %r, %r
import numpy as np
import torch
from reporter_amd import matcher as M
from reporter_amd import _lib
from reporter_amd import simple_reporter as sr
from tests import edge_traversals_ref as ref
from tests import matched_points_ref as mref
from tests import ragged


class DevArr:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {'shape': (n,), 'typestr': typestr, 'data': (int(ptr), False), 'version': 2}


def run(m, tr, **kw):
    r = m.match_batch(tr, copy_out=True, edge_traversals=True, timing=True, **kw)
    tv = m.edge_traversals_result()
    out = {'res': {k: np.asarray(v) for k, v in _lib.result_to_numpy(r).items()}, 'status': int(r.status),
           'trav': _lib.traversals_to_numpy(tv), 'n': int(tv.n_traversals), 'n_traces': int(tv.n_traces),
           'ms': float(tv.kernel_ms)}
    ptr, n = m.edge_observations(3600)
    out['n_obs'] = n
    # (hist_reduce copies its input first: the entries stay the matcher's for the second call)
    out['reduced'] = {p: sr.hist_reduce(m, ptr, n, privacy=p) for p in (1, 2)}
    return out


if batch == 'ragged':
    path, tr = ragged.ragged_city(graph_dir)
    M.configure(ragged.engine_config(path, cfg))
else:
    built = (ref.kat3 if batch == 'kat3' else getattr(mref, batch))(graph_dir)
    path, tr = built[0], built[1]
    M.configure(M.default_config(path, **mref.OPTIONS[cfg]))
m = M.Matcher()
out = {'flagged': run(m, tr)}
if (batch, cfg) == ('ragged', 'gtt'):
    # without the flag: the same result, and no traversals
    r = m.match_batch(tr, copy_out=True)
    out['plain'] = {k: np.asarray(v) for k, v in _lib.result_to_numpy(r).items()}
    tv = _lib.TraversalResult()
    out['plain_rc'] = int(_lib.lib().otr_edge_traversals(m._h, ctypes.byref(tv)))
    out['plain_error'] = _lib.last_error()
    ptr, n = ctypes.c_void_p(), ctypes.c_int64()
    out['plain_obs_rc'] = int(_lib.lib().otr_edge_observations(m._h, 3600, ctypes.byref(ptr), ctypes.byref(n)))
    out['plain_obs_error'] = _lib.last_error()
    # the matched points alone, then both flags together
    m.match_batch(tr, copy_out=True, matched_points=True)
    out['points_alone'] = m.matched_points()
    out['both'] = run(m, tr, matched_points=True)
    out['both']['points'] = m.matched_points()
    out['shuffled'] = run(m, ragged.reorder(tr, ragged.PERMS['shuffled']))
    # device inputs, no copy-out: the d_* arrays
    dev = {'trace_offsets': torch.from_numpy(np.ascontiguousarray(tr.offsets, np.int64)).cuda(),
           'lat': torch.from_numpy(np.ascontiguousarray(tr.lat, np.float64)).cuda(),
           'lon': torch.from_numpy(np.ascontiguousarray(tr.lon, np.float64)).cuda(),
           'time': torch.from_numpy(np.ascontiguousarray(tr.time, np.int64)).cuda(),
           'mode': torch.from_numpy(np.ascontiguousarray(tr.mode, np.uint8)).cuda()}
    torch.cuda.synchronize()
    m.match_batch(tr, copy_out=False, edge_traversals=True,
                  device_arrays={k: v.data_ptr() for k, v in dev.items()})
    tv = m.edge_traversals_result()
    n = int(tv.n_traversals)
    out['device_host_null'] = all(not getattr(tv, k) for k in ref.FIELDS)
    # (seg_id crosses as int64 words: the same bits)
    out['device'] = {k: torch.as_tensor(DevArr(getattr(tv, 'd_' + k), int(tv.n_traces) + 1 if k == 'trace_off' else n,
                                               '<i8' if k == 'seg_id' else np.dtype(t).str),
                                        device='cuda').clone().cpu().numpy().view(t)
                     for k, t in ref.TYPES.items()}
    # an empty batch: no traversal, a trace_off of one zero, no entry
    from reporter_amd.tools.gen import Traces
    m.match_batch(Traces(np.zeros(0), np.zeros(0), np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.uint8)),
                  copy_out=True, edge_traversals=True)
    tv = m.edge_traversals_result()
    out['empty'] = {'n': int(tv.n_traversals), 'n_traces': int(tv.n_traces), 'trav': _lib.traversals_to_numpy(tv),
                    'd_trace_off': torch.as_tensor(DevArr(tv.d_trace_off, 1, '<i8'), device='cuda').clone().cpu().numpy(),
                    'n_obs': m.edge_observations()[1]}
pickle.dump(out, open(dst, 'wb'))
print('edge traversals ok')
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
            dst = str(tmp_path_factory.mktemp('edge_traversals') / (job + '.pkl'))
            t0 = time.perf_counter()
            p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, dst, batch, cfg)], env=env,
                               capture_output=True, text=True, timeout=240)
            assert p.returncode == 0 and 'edge traversals ok' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
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
        built = (ref.kat3 if batch == 'kat3' else getattr(mref, batch))(graph_dir)
        path, tr = built[0], built[1]
    return GraphFile(path), tr


def _report(got, want):
    """The first differing entries of every array that differs."""
    msg = []
    for k in ref.same_bits(got, want):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype:
            msg.append('%s: got %s %s, want %s %s' % (k, a.dtype, a.shape, b.dtype, b.shape))
            continue
        i = np.flatnonzero(a != b)[:5]
        msg.append('%s: %d differ, first %s got %s want %s' % (k, len(i), i.tolist(), a[i].tolist(), b[i].tolist()))
    return msg


@pytest.mark.parametrize('job', list(JOBS))
def test_bit_exact(job, run_job, graph_dir):
    got = run_job(job)['flagged']
    G, tr = _batch(job, graph_dir)
    assert got['status'] == 0 and got['n_traces'] == tr.n_traces
    want = ref.traversals(got['res'], tr, G)
    print('%s: %d traversals, K13 %.3f ms' % (job, got['n'], got['ms']))
    assert not _report(got['trav'], want)
    assert got['n'] == len(want['edge']) > 0 and got['ms'] > 0.0


@pytest.mark.parametrize('job', list(JOBS))
def test_entries_reduce_to_the_oracles_reduction(job, run_job, graph_dir):
    got = run_job(job)['flagged']
    G, tr = _batch(job, graph_dir)
    obs = ref.observations(ref.traversals(got['res'], tr, G), G, 3600)
    print('%s: %d entries, bins %s' % (job, len(obs), np.bincount(obs['speed_bin'], minlength=8).tolist()))
    assert got['n_obs'] == len(obs)
    for p in (1, 2):
        assert np.array_equal(got['reduced'][p], oh.reduce(obs, p)), p
    assert int(got['reduced'][1]['count'].sum()) == len(obs)
    if job == 'kat3':
        assert len(obs) == 2 and obs['speed_bin'].tolist() == [2, 4]
    elif job == 'kat':
        assert len(obs) == 0   # (no traversal of its two edges is complete)
    else:
        assert len(obs) > 0


def test_flag_changes_nothing_else(run_job):
    r = run_job('ragged_gtt')
    errors, stats = compare(r['flagged']['res'], r['plain'])
    assert not errors and all(stats.values()), (errors, stats)
    assert r['plain_rc'] == 400 and 'OTR_BATCH_EDGE_TRAVERSALS' in r['plain_error']
    assert r['plain_obs_rc'] == 400 and 'OTR_BATCH_EDGE_TRAVERSALS' in r['plain_obs_error']


def test_together_with_matched_points(run_job):
    r = run_job('ragged_gtt')
    assert not _report(r['both']['trav'], r['flagged']['trav'])
    assert not mref.same_bits(r['both']['points'], r['points_alone'])
    assert r['both']['n_obs'] == r['flagged']['n_obs']
    assert np.array_equal(r['both']['reduced'][2], r['flagged']['reduced'][2])


def test_traversals_do_not_depend_on_neighbours(run_job, graph_dir):
    from tests import ragged
    r = run_job('ragged_gtt')
    _, tr = ragged.ragged_city(graph_dir)
    p = ragged.PERMS['shuffled']
    pos = np.argsort(np.asarray(p))   # trace t of the original is trace pos[t] of the shuffled batch
    got, want = r['shuffled']['trav'], r['flagged']['trav']
    soff_m, soff = r['shuffled']['res']['trace_state_off'], r['flagged']['res']['trace_state_off']
    goff = got['trace_off']
    sel = np.concatenate([np.arange(goff[q], goff[q + 1]) for q in pos] + [np.zeros(0, np.int64)]).astype(np.int64)
    back = {k: np.asarray(got[k])[sel] for k in ref.FIELDS[1:]}
    per = np.diff(goff)[pos]
    back['trace_off'] = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    # states are numbered through the batch: compare them relative to their trace's first state
    shift = np.concatenate([np.full(int(per[t]), int(soff[t]) - int(soff_m[pos[t]]), np.int64)
                            for t in range(tr.n_traces)] + [np.zeros(0, np.int64)])
    back['first_state'] = back['first_state'] + shift
    assert not _report(back, want)


def test_empty_batch(run_job):
    e = run_job('ragged_gtt')['empty']
    assert (e['n'], e['n_traces'], e['n_obs']) == (0, 0, 0)
    assert e['trav']['trace_off'].tolist() == [0] and e['d_trace_off'].tolist() == [0]
    assert all(len(e['trav'][k]) == 0 for k in ref.FIELDS[1:])


def test_device_inputs_without_copy_out(run_job):
    r = run_job('ragged_gtt')
    assert r['device_host_null']
    assert not _report(r['device'], r['flagged']['trav'])
