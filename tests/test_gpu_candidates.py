"""k_candidates (K1) against the grid-free brute force of tests/candidates_ref.py, bit for bit:
every case, option set and probe order through match_batch, once as configured (the option sets
within Batch::candidates' rule run k_candidates<2>, the others <1>) and once under OTR_CAND_G=1
(everything runs <1>).  Also: the whole result equals the oracle's, a state's candidates do not
depend on its wave partner (three orders and a batch of one), and the two instances agree.  What
the cases cover (the cell-by-cell path and its first and last cell, cuts inside ties, several
compactions, the hand-over to shape_ll, a distance exactly at the radius, per-probe accuracies,
mixed waves, ...) is pinned by tests/test_candidates_cases_cpu.py.  One child process per
instance.

Each of these edits to k_candidates / project_edge was seen to fail the named cases: the edge-id
tie-break of cand_less reversed (star, dense, border, modes); best < r2 for best <= r2
(exact_radius); the per-probe accuracy ignored (modes); the cell-by-cell loop one cell short
(corner); the second preloaded shape point taken for the first (every case)."""
import os
import pickle
import subprocess
import sys
import time

import pytest

from oracle import pyoracle as po
from oracle.compare import compare
from tests import candidates_ref as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILDREN = {'default': None, 'g1': '1'}   # name -> OTR_CAND_G
CHILD = r'''
import sys, pickle
sys.path.insert(0, %r)
graph_dir, dst = %r, %r
from reporter_amd import matcher as M
from tests import candidates_ref as cr

out = {}
for case in cr.CASES:
    for run in cr.runs_of(case, graph_dir):
        M.configure(run.engine_config())
        m = M.Matcher()
        for name, order in cr.batches(run):
            out[(run.name, name)] = m.match_batch_numpy(run.traces(order))
        m.close()
pickle.dump(out, open(dst, 'wb'))
print('candidates ok')
'''

_RUNS = {}
_ORACLE = {}


@pytest.fixture(scope='module')
def child(graph_dir, tmp_path_factory):
    def get(which):
        if which not in _RUNS:
            # (a child that died is not followed by another GPU process)
            assert all(r is not None for r in _RUNS.values()), 'an earlier child failed'
            _RUNS[which] = None
            env = dict(os.environ)
            for k in ('OTR_VIT_SPLIT', 'OTR_TIERS', 'OTR_EST_K', 'OTR_LIB', 'OTR_SMALL_KEYS', 'OTR_SMALL_PATH_KEYS',
                      'OTR_TINY_KEYS', 'OTR_CAND_G'):
                env.pop(k, None)
            if CHILDREN[which] is not None:
                env['OTR_CAND_G'] = CHILDREN[which]
            dst = str(tmp_path_factory.mktemp('candidates') / (which + '.pkl'))
            t0 = time.perf_counter()
            p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, dst)], env=env, capture_output=True,
                               text=True, timeout=240)
            assert p.returncode == 0 and 'candidates ok' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
            print('child %s: %.1f s' % (which, time.perf_counter() - t0))
            with open(dst, 'rb') as f:
                _RUNS[which] = pickle.load(f)
        assert _RUNS[which] is not None, 'the child %s failed' % which
        return _RUNS[which]
    return get


def _oracle(run, name, order):
    key = (run.name, name)
    if key not in _ORACLE:
        _ORACLE[key] = po.match_batch(po.Graph(run.path), run.traces(order), run.oracle_params())
    return _ORACLE[key]


@pytest.mark.parametrize('which', list(CHILDREN))
@pytest.mark.parametrize('case', cr.CASES)
def test_equals_brute_force(case, which, child, graph_dir):
    got = child(which)
    bad, n = [], 0
    for run in cr.runs_of(case, graph_dir):
        for name, order in cr.batches(run):
            res = got[(run.name, name)]
            if int(res['status']) != 0:
                bad.append('%s %s: status %d' % (run.name, name, int(res['status'])))
            bad += ['%s: %s' % (name, d) for d in cr.differences(run, order, res)]
            n += len(order)
    print('%s %s: %d states, %d differ' % (case, which, n, len(bad)))
    assert not bad, bad[:5]
    assert n > 0


@pytest.mark.parametrize('which', list(CHILDREN))
@pytest.mark.parametrize('case', cr.CASES)
def test_equals_oracle(case, which, child, graph_dir):
    got = child(which)
    for run in cr.runs_of(case, graph_dir):
        for name, order in cr.batches(run):
            errors, stats = compare(got[(run.name, name)], _oracle(run, name, order))
            assert not errors, (run.name, name, errors)
            assert all(v for k, v in stats.items() if k.endswith('_bitexact')), (run.name, name, stats)
            assert stats['n_states'] == len(order)


@pytest.mark.parametrize('which', list(CHILDREN))
@pytest.mark.parametrize('case', cr.CASES)
def test_candidates_do_not_depend_on_the_wave_partner(case, which, child, graph_dir):
    got = child(which)
    for run in cr.runs_of(case, graph_dir):
        rows = {}   # probe -> {order name: its row}
        for name, order in cr.batches(run):
            for s, row in enumerate(cr.rows_of(got[(run.name, name)])):
                rows.setdefault(order[s], {})[name + '@%d' % s] = row
        assert sorted(rows) == list(range(len(run.probes)))
        for i, by in rows.items():
            first = next(iter(by.values()))
            assert len(by) >= 3 and all(cr.same_row(r, first) for r in by.values()), (run.name, i, by)
        if run.name == cr.ALONE:
            assert any(k.startswith('alone') for k in rows[0])


@pytest.mark.parametrize('case', cr.CASES)
def test_the_two_instances_agree(case, child, graph_dir):
    a, b = child('default'), child('g1')
    assert sorted(a) == sorted(b)
    for run in cr.runs_of(case, graph_dir):
        for name, order in cr.batches(run):
            x, y = a[(run.name, name)], b[(run.name, name)]
            errors, stats = compare(x, y)
            assert not errors and all(v for k, v in stats.items() if k.endswith('_bitexact')), (run.name, name, errors)
            assert int(x['status']) == int(y['status']) == 0 and int(x['n_overflow']) == int(y['n_overflow']) == 0
            for s, (p, q) in enumerate(zip(cr.rows_of(x), cr.rows_of(y))):
                assert cr.same_row(p, q), (run.name, name, s)
