"""The per-trace stages (k_link, k_viterbi, k_segments, k_histogram) on the ragged batches of
tests/ragged.py, through all three k_viterbi instances: two traces per wave (k_viterbi<2>,
the kernel of the large batches, reached here with OTR_VIT_SPLIT=0), one trace per wave with
the split predecessor scan (k_viterbi<1, true>, the default below 8,192 traces) and one trace
per wave for more than 32 candidates (k_viterbi<1>).  Each result equals the oracle field by
field, the two K <= 32 instances agree bit for bit, a trace's result does not depend on the
traces around it (the batch reversed and shuffled), and the device histogram equals its
restatement.  What the batches cover is pinned by tests/test_trace_stage_cases_cpu.py.
Runs in one child process per setting (the knob is read once per process); the result says
which instance ran (otr.h OTR_VITERBI_VARIANT)."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle.compare import compare, subset
from tests import ragged

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = {'two_per_wave': '0', 'split': None}  # OTR_VIT_SPLIT
JOBS = [(case, cfg) for case, (_, cfgs) in ragged.CASES.items() for cfg in cfgs]
HIST_HOURS = 3
CHILD = r'''
import sys, pickle
sys.path.insert(0, %r)
graph_dir, dst = %r, %r
import numpy as np
import torch
from reporter_amd import matcher as M
from reporter_amd import _lib
from reporter_amd.tools import gen
from tests import ragged


class DevArr:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {'shape': (n,), 'typestr': '<i4', 'data': (int(ptr), False), 'version': 2}


def run(path, cfg, tr, **kw):
    M.configure(ragged.engine_config(path, cfg))
    r = M.Matcher().match_batch(tr, copy_out=True, **kw)
    out = {'res': {k: np.asarray(v) for k, v in _lib.result_to_numpy(r).items()},
           'variant': float(r.kernel_ms[_lib.VITERBI_VARIANT]), 'status': int(r.status)}
    if kw.get('hist_hours'):
        n = int(r.hist_len)
        torch.cuda.synchronize()
        out['hist'] = torch.as_tensor(DevArr(r.d_hist, n), device='cuda').clone().cpu().numpy()
    return out


out = {}
for case, (build, cfgs) in ragged.CASES.items():
    path, tr = build(graph_dir)
    for cfg in cfgs:
        out[(case, cfg)] = run(path, cfg, tr)
    if case == 'ragged_city':
        for name, perm in ragged.PERMS.items():
            out[('perm', name)] = run(path, 'gtt', ragged.reorder(tr, perm))
        out['hist'] = run(path, 'gtt', tr, hist_hours=%d, hist_base_time=gen.T_BEGIN)
pickle.dump(out, open(dst, 'wb'))
print('trace stages ok')
'''


@pytest.fixture(scope='module')
def runs(graph_dir, tmp_path_factory):
    """{setting: {job: result}}: every batch matched on the GPU, one child process per setting."""
    res = {}
    for name, split in SETTINGS.items():
        env = dict(os.environ)
        for k in ('OTR_VIT_SPLIT', 'OTR_TIERS', 'OTR_EST_K', 'OTR_LIB', 'OTR_SMALL_KEYS', 'OTR_SMALL_PATH_KEYS',
                  'OTR_TINY_KEYS'):
            env.pop(k, None)
        if split is not None:
            env['OTR_VIT_SPLIT'] = split
        dst = str(tmp_path_factory.mktemp('trace_stages') / (name + '.pkl'))
        t0 = time.perf_counter()
        p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, dst, HIST_HOURS)], env=env,
                           capture_output=True, text=True, timeout=240)
        assert p.returncode == 0 and 'trace stages ok' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
        print('child %s: %.1f s' % (name, time.perf_counter() - t0))
        with open(dst, 'rb') as f:
            res[name] = pickle.load(f)
    return res


def test_variant_codes(runs):
    """11 k_viterbi<1, true>, 20 k_viterbi<2>, 10 k_viterbi<1>."""
    for setting, k32_code in (('two_per_wave', 20), ('split', 11)):
        for case, cfg in JOBS:
            want = 10 if case == 'wide_K' else k32_code
            assert runs[setting][(case, cfg)]['variant'] == want, (setting, case, cfg)
        for job in (('perm', 'reversed'), ('perm', 'shuffled'), 'hist'):
            assert runs[setting][job]['variant'] == k32_code, (setting, job)


@pytest.mark.parametrize('case,cfg', JOBS)
@pytest.mark.parametrize('setting', list(SETTINGS))
def test_oracle_parity(setting, case, cfg, runs, graph_dir):
    got = runs[setting][(case, cfg)]
    _, _, want, _ = ragged.oracle_result(case, cfg, graph_dir)
    errors, stats = compare(got['res'], want)
    assert not errors, errors
    assert got['status'] == 0 and got['res']['status'] == 0
    assert stats['n_seg'] > 0 and stats['n_rep'] > 0


@pytest.mark.parametrize('case,cfg', JOBS)
def test_variants_agree_bit_for_bit(case, cfg, runs):
    errors, stats = compare(runs['two_per_wave'][(case, cfg)]['res'], runs['split'][(case, cfg)]['res'])
    assert not errors and all(stats.values()), (errors, stats)


@pytest.mark.parametrize('perm', list(ragged.PERMS))
@pytest.mark.parametrize('setting', list(SETTINGS))
def test_trace_does_not_depend_on_its_neighbours(setting, perm, runs, graph_dir):
    """No oracle: the permuted batch's results, put back in order, are the original batch's."""
    _, tr = ragged.ragged_city(graph_dir)
    p = ragged.PERMS[perm]
    moved = ragged.reorder(tr, p)
    pos = np.argsort(np.asarray(p))  # trace t of the original is trace pos[t] of the permuted batch
    back = subset(runs[setting][('perm', perm)]['res'], pos, moved.offsets)
    errors, stats = compare(back, runs[setting][('ragged_city', 'gtt')]['res'])
    assert not errors and all(stats.values()), (errors, stats)


@pytest.mark.parametrize('setting', list(SETTINGS))
def test_device_histogram(setting, runs, graph_dir):
    """k_histogram, one wave per trace, on ragged_city's traces of 0 to 49 ('gtt'; 51 under
    'deployed') reports: one stride of 64 lanes.  Traces of more reports, other quantisations
    and other windows: tests/test_gpu_tile_stages.py."""
    from oracle.hist import histogram
    from reporter_amd import _lib
    from reporter_amd.graphfile import GraphFile
    from reporter_amd.tools import gen
    path, tr = ragged.ragged_city(graph_dir)
    got = runs[setting]['hist']
    res = got['res']
    errors, stats = compare(res, runs[setting][('ragged_city', 'gtt')]['res'])  # (the histogram changes no result)
    assert not errors and all(stats.values()), (errors, stats)
    G = GraphFile(path)
    n = np.diff(tr.offsets)
    first = np.where(n > 0, tr.time[np.minimum(tr.offsets[:-1], len(tr.time) - 1)], 0)
    last = np.where(n > 0, tr.time[np.maximum(tr.offsets[1:] - 1, 0)], 0)
    idx = {int(s): i for i, s in enumerate(G.seg_id)}
    want, rows = histogram(res, first, last, idx, len(G.seg_id), gen.T_BEGIN, HIST_HOURS)
    assert rows == res['n_rows'] and rows > 0 and want.sum() > 0
    assert np.array_equal(got['hist'].reshape(HIST_HOURS, len(G.seg_id), _lib.HIST_BINS), want)
