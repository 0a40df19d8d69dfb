"""The edge-state route search (turn costs: k_route_e1<360> -> <512> -> <1024>, k_general, the
winner paths of k_paths_edge, the turn-mode Viterbi) on the hand-built graphs of
tests/edge_state_cases.py, field by field against the oracle, in every library setting:

    product library                        the tiers as they fall
    libotr_tiercheck.so, OTR_FORCE_EDGE 1   every route search in the 512-state table
                                       3   ... in the 1,024-state table
                                       7   ... in k_general
                                      24   every winner path in k_general
                                      96   every search stops after 2 / 4 rounds and resumes from its dump
    libotr_generalcheck.so                 everything in k_general

One child process per setting runs all cases; the traces of a case also run as batches of 1, 2,
3, .. of them (1, fewer than 8 and more than 8 tasks meet the per-XCD queues).  Every batch runs
with route_work on (status 0, compare() against the oracle without errors) and off (equal to the
first run bit for bit).  What each case reaches is pinned on the CPU by
tests/test_edge_state_cases_cpu.py; here a case that does not get there fails:

  hub      the CSR-tail pass: the tier that did the work relaxed more edges than four per
           settled state can give (the restatement's count for the same searches), hub5 and hub9;
           not so hub4.  k_general (setting 7, generalcheck) the same against its exhaustive
           searches.
  tree4    product library: searches ended in the 360-, 512- and 1,024-state tables and in
           k_general, which settled the whole tree; the batches without trace 3 dump nothing (the
           tables fill inside a round: restart), trace 3 passes the 512-state table's load limit
           between two rounds: one dump, resumed.  Setting 96: dumped and resumed.
  stair_steep  setting 96: at least two dumps (after round 2, and 4 rounds later), each holding a
           key without a label (the rounds are pinned on the CPU), ended in the 1,024-state table.
  stair    the cap at its edge (compare() holds it): 77 right angles and one more straight pass are
           matched, which only the labelled state behind the 77th turn offers; 78, or a slant 628 mm
           over the cap, break the trace.
  wide     product library: wide34 (34 candidates) runs in k_general, wide32 does not.
  star70, ties  the matched route holds the in-edge of the centre / the branch edge the oracle
           takes (compare() holds the whole route).

Work counters are asserted as inequalities only (the order of the pending list depends on LDS
atomics).  Runs in child processes (one library per process)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def batch_sizes(n):
    """1, 2, 3, .. for short cases; 1, 2, 3, all but one and all for the longer ones."""
    return list(range(1, n + 1)) if n <= 4 else sorted({1, 2, 3, n - 1, n})


CHILD = r'''
import sys
sys.path.insert(0, %r)
from oracle import pyoracle as po
from oracle.compare import compare
from reporter_amd import _lib
from reporter_amd import matcher as M
from tests import edge_state_cases as C
from tests import edge_state_ref as R
from tests import test_gpu_edge_state as T
gdir, force, general = %r, %d, %r
E1 = (10, 9, 11)  # the 360-, 512- and 1,024-state tables' slots; 6: k_general
for name in sorted(C.BUILDERS):
    c = C.build(name, gdir)
    M.configure(C.engine_config(c.path, c.cfg))
    prm = C.oracle_params(c.cfg)
    g = po.Graph(c.path)
    for n in T.batch_sizes(len(c.traces)):
        b = c.batch(n)
        want = po.match_batch(g, b, prm)
        r = M.Matcher().match_batch(b, copy_out=True, route_work=True)
        assert r.status == 0, (name, n, r.status)
        cn = [int(r.counters[k]) for k in range(24)]
        w = [[int(r.route_tier_work[t][k]) for k in range(4)] for t in range(16)]
        got = _lib.result_to_numpy(r)
        errors, stats = compare(got, want)
        assert not errors, (name, n, errors)
        r2 = M.Matcher().match_batch(b, copy_out=True, route_work=False)
        assert r2.status == 0, (name, n, r2.status)
        errors, stats = compare(_lib.result_to_numpy(r2), got)
        exact = [v for k, v in stats.items() if k.endswith('_bitexact')]
        assert not errors and exact and all(exact), (name, n, errors, stats)
        print(name, n, 'force', force, 'searches/settled/relaxed 360', w[10][:3], '512', w[9][:3], '1024', w[11][:3],
              'general', w[6][:3], 'node tiers', [w[t][0] for t in (0, 1, 2, 3, 4, 5, 12, 13)], 'resumed', cn[22],
              'dumped', cn[23])
        turn_traces = [t for t in range(n) if prm[int(b.mode[t])].turn_penalty_factor > 0]
        ran = sum(w[t][0] for t in E1) + w[6][0]
        route = [int(e) for e in got['route_edge']]
        # ---- which tier did the work
        if general:
            assert cn[3] == 0 and sum(w[t][0] for t in E1) == 0, (name, n, w)
        elif force & 1:
            assert w[10][0] == 0, (name, n, w)
            if (force & 7) == 1 and ran:
                assert w[9][0] + w[6][0] > 0 and (w[9][0] > 0 or name == 'wide34'), (name, n, w)
            if (force & 7) == 3:
                assert w[9][0] == 0 and (not ran or w[11][0] > 0 or name == 'wide34'), (name, n, w)
            if (force & 7) == 7:
                assert w[9][0] == 0 and w[11][0] == 0 and (not ran or w[6][0] > 0), (name, n, w)
        # ---- the cases' branches
        if name.startswith('hub') and (general or force in (0, 1, 3, 7)):
            exhaustive = general or force == 7
            G = R.RefGraph(c.path, prm, 0)
            full = cap4 = 0
            for t, st, i, S in R.batch_searches(c.path, prm, b, want, exhaustive):
                f, c4 = R.relax_counts(G, S)
                full, cap4 = full + f, cap4 + c4
            relaxed = w[6][2] if exhaustive else sum(w[t][2] for t in E1)
            print('   relaxed', relaxed, 'four per state give', cap4, 'all out-edges', full)
            if name == 'hub4':
                assert full == cap4 and relaxed <= cap4, (name, n, relaxed, cap4)
            else:
                assert full > cap4 and relaxed > cap4, (name, n, relaxed, cap4, full)  # the tail pass ran
        if name == 'tree4' and force == 0 and not general:
            assert w[10][0] > 0 and w[6][0] > 0 and w[6][1] >= c.info['n_tree'], (n, w)
            if n <= 3:
                assert cn[22] == 0 and cn[23] == 0, (n, cn)  # the tables filled inside a round: restarts, no dump
            if n >= 3:
                assert w[9][0] > 0, (n, w)   # trace 2: 426 keys end in the 512-state table
            if n == 4:
                assert w[11][0] > 0 and cn[23] > 0 and cn[22] > 0, (n, w, cn)  # trace 3: dumped at 490 keys, resumed
        if name == 'tree4' and force == 96:
            # (a search counts as resumed where it ends: traces 2 and 3 end in the 1,024-state table)
            assert cn[23] > 0 and w[6][0] > 0 and (n < 3 or cn[22] > 0), (n, w, cn)
        if name == 'stair_steep' and force == 96:
            # the feeder's search runs 9 rounds: stopped after round 2 and after round 6, ended at 1,024 states
            assert cn[23] >= 2 and cn[22] >= 1 and w[11][0] > 0, (n, w, cn)
        if name in ('stair', 'stair_near', 'stair_early', 'stair_late') and force == 96:
            assert cn[23] >= 2 and cn[22] >= 1 and w[11][0] > 0, (name, n, w, cn)
        if force == 0 and not general:
            if name == 'wide34':
                assert w[6][0] > 0 and sum(w[t][0] for t in E1) == 0, (n, w)
            if name == 'wide32':
                assert w[6][0] == 0 and w[10][0] > 0, (n, w)
            if name not in ('wide34', 'tree4') and turn_traces:
                assert w[6][0] == 0, (name, n, w)  # the lean tiers hold every other case
        if name == 'star70':
            for t, (a, bb) in enumerate(c.info['pairs'][:n]):
                assert c.info['ids']['in%%d' %% a] in route and c.info['ids']['out%%d' %% bb] in route, (n, t)
        if name in ('ties', 'ties_mirror'):
            ids = c.info['ids']
            assert min(ids['PT'], ids['QT']) in route and max(ids['PT'], ids['QT']) not in route, route
        if name == 'ties_key':
            assert (c.info['ids']['PT'] in route) != (c.info['ids']['QT'] in route), route
print('edge state ok')
'''

SETTINGS = [('product', None, 0), ('tiercheck', 'libotr_tiercheck.so', 1), ('tiercheck', 'libotr_tiercheck.so', 3),
            ('tiercheck', 'libotr_tiercheck.so', 7), ('tiercheck', 'libotr_tiercheck.so', 24),
            ('tiercheck', 'libotr_tiercheck.so', 96), ('generalcheck', 'libotr_generalcheck.so', 0)]


@pytest.mark.parametrize('kind,lib,force', SETTINGS, ids=['%s-%d' % (s[0], s[2]) for s in SETTINGS])
def test_edge_state_cases_equal_oracle(graph_dir, kind, lib, force):
    env = dict(os.environ)
    for k in ('OTR_LIB', 'OTR_TIERS', 'OTR_EST_K', 'OTR_FORCE_EDGE', 'OTR_NDUMP_GB', 'OTR_OPT_RESERVE_GB',
              'OTR_SMALL_KEYS', 'OTR_TINY_KEYS', 'OTR_ROUTE_G', 'OTR_E1RESUME', 'OTR_SORT'):
        env.pop(k, None)
    if lib:
        path = os.path.join(ROOT, 'reporter_amd', lib)
        assert os.path.exists(path), 'build first: python -m reporter_amd.build'
        env['OTR_LIB'] = path
    if force:
        env['OTR_FORCE_EDGE'] = str(force)
    p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, force, kind == 'generalcheck')], env=env,
                       capture_output=True, text=True, timeout=240)
    print(p.stdout[-20000:])
    assert p.returncode == 0 and 'edge state ok' in p.stdout, p.stdout[-3000:] + p.stderr[-4000:]
