"""The Viterbi stage (K5) on exact cost ties (the lowest index among equal
minima, for a predecessor and for the winner where a sub-path ends), in its three instances:
k_viterbi<2> (vit_scan<., 8>, reached with OTR_VIT_SPLIT=0), k_viterbi<1, true> (vit_scan_half
and vit_pair, the default below 8,192 traces) and k_viterbi<1> (vit_scan<., 16> and the global
backtrack, under the 'wide' configuration).  The batches are those of tests/viterbi_cases.py:
every case alone, all cases as one batch, that batch reversed and under one fixed shuffle.
What each trace reaches is pinned on the CPU by tests/test_viterbi_cases_cpu.py.

Every batch equals the oracle field by field (oracle.compare.compare: the tied winner decides the
matched edge, the route, the segments and the reports), the two K <= 32 instances agree bit for
bit, the permuted batches put back in order equal the unpermuted one, and the route work counters
change nothing.  One child process per setting (OTR_VIT_SPLIT is read once per process), one after
another."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle.compare import compare, subset
from tests import viterbi_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# setting -> (suite, OTR_VIT_SPLIT, the k_viterbi instance code of otr.h OTR_VITERBI_VARIANT)
SETTINGS = {'two_per_wave': ('k32', '0', 20), 'split': ('k32', None, 11), 'wide': ('wide', None, 10)}
CFGS = {'k32': ('gtt', 'deployed', 'mixed'), 'wide': ('wide',)}
BATCHES = {'k32': ('pred_pairs', 'end_ties', 'both', 'ragged_K', 'unreachable', 'route_tie', 'long', 'all',
                   'reversed', 'shuffled'),
           'wide': ('pred_wide', 'end_wide', 'all', 'reversed', 'shuffled')}
JOBS = [(setting, cfg, batch) for setting, (suite, _, _) in SETTINGS.items() for cfg in CFGS[suite]
        for batch in BATCHES[suite]]
CHILD = r'''
import sys, pickle
sys.path.insert(0, %r)
graph_dir, suite, dst = %r, %r, %r
import numpy as np
from reporter_amd import matcher as M
from reporter_amd import _lib
from tests import ragged
from tests import viterbi_cases as C

s = C.suite(suite, graph_dir)
out = {}
for cfg in s.cfgs:
    M.configure(ragged.engine_config(s.path, cfg))
    for name, names in s.batches().items():
        tr = s.batch(names)
        for work in (True, False):
            r = M.Matcher().match_batch(tr, copy_out=True, route_work=work)
            out[(cfg, name, work)] = {'res': {k: np.asarray(v) for k, v in _lib.result_to_numpy(r).items()},
                                      'variant': float(r.kernel_ms[_lib.VITERBI_VARIANT]), 'status': int(r.status)}
pickle.dump(out, open(dst, 'wb'))
print('viterbi ties ok')
'''


def exact(stats):
    """Every float field of compare()'s stats is bit-exact (and there are some)."""
    flags = [v for k, v in stats.items() if k.endswith('_bitexact')]
    return bool(flags) and all(flags)


@pytest.fixture(scope='module')
def runs(graph_dir, tmp_path_factory):
    """{setting: {(cfg, batch, route_work): result}}: every batch matched on the GPU."""
    res = {}
    for name, (suite, split, _) in SETTINGS.items():
        env = dict(os.environ)
        for k in ('OTR_VIT_SPLIT', 'OTR_TIERS', 'OTR_EST_K', 'OTR_LIB', 'OTR_SMALL_KEYS', 'OTR_SMALL_PATH_KEYS',
                  'OTR_TINY_KEYS'):
            env.pop(k, None)
        if split is not None:
            env['OTR_VIT_SPLIT'] = split
        dst = str(tmp_path_factory.mktemp('viterbi_ties') / (name + '.pkl'))
        t0 = time.perf_counter()
        p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, suite, dst)], env=env,
                           capture_output=True, text=True, timeout=240)
        assert p.returncode == 0 and 'viterbi ties ok' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
        print('child %s: %.1f s' % (name, time.perf_counter() - t0))
        with open(dst, 'rb') as f:
            res[name] = pickle.load(f)
    return res


def test_batches_are_the_suites(graph_dir):
    for suite in CFGS:
        s = C.suite(suite, graph_dir)
        assert tuple(s.cfgs) == CFGS[suite] and sorted(s.batches()) == sorted(BATCHES[suite])


def test_variant_codes(runs):
    """20 k_viterbi<2>, 11 k_viterbi<1, true>, 10 k_viterbi<1>."""
    for setting, (_, _, code) in SETTINGS.items():
        assert runs[setting] and all(r['variant'] == code for r in runs[setting].values()), setting


@pytest.mark.parametrize('setting,cfg,batch', JOBS)
def test_oracle_parity(setting, cfg, batch, runs, graph_dir):
    _, _, want = C.oracle_result(SETTINGS[setting][0], cfg, batch, graph_dir)
    got = runs[setting][(cfg, batch, True)]
    errors, stats = compare(got['res'], want)
    assert not errors, errors
    assert got['status'] == 0 and got['res']['status'] == 0 and stats['n_seg'] > 0


@pytest.mark.parametrize('setting,cfg,batch', JOBS)
def test_route_work_counters_change_nothing(setting, cfg, batch, runs):
    off = runs[setting][(cfg, batch, False)]
    errors, stats = compare(off['res'], runs[setting][(cfg, batch, True)]['res'])
    assert not errors and exact(stats) and off['status'] == 0, (errors, stats)


@pytest.mark.parametrize('cfg,batch', [(c, b) for c in CFGS['k32'] for b in BATCHES['k32']])
def test_variants_agree_bit_for_bit(cfg, batch, runs):
    errors, stats = compare(runs['two_per_wave'][(cfg, batch, True)]['res'], runs['split'][(cfg, batch, True)]['res'])
    assert not errors and exact(stats), (errors, stats)


@pytest.mark.parametrize('perm', ['reversed', 'shuffled'])
@pytest.mark.parametrize('setting,cfg', [(s, c) for s, (suite, _, _) in SETTINGS.items() for c in CFGS[suite]])
def test_trace_does_not_depend_on_its_neighbours(setting, cfg, perm, runs, graph_dir):
    """No oracle: the permuted batch's results, put back in order, are the all-cases batch's."""
    s = C.suite(SETTINGS[setting][0], graph_dir)
    b = s.batches()
    moved = s.batch(b[perm])
    pos = np.asarray([b[perm].index(n) for n in b['all']])  # trace t of 'all' is trace pos[t] of the permuted batch
    back = subset(runs[setting][(cfg, perm, True)]['res'], pos, moved.offsets)
    errors, stats = compare(back, runs[setting][(cfg, 'all', True)]['res'])
    assert not errors and exact(stats), (errors, stats)
