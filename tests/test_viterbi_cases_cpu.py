"""The traces of tests/viterbi_cases.py reach the exact cost ties they were built for (CPU only:
the oracle and the restatement of tests/viterbi_ref.py).  These are requirements on the inputs of
tests/test_gpu_viterbi_ties.py, not measurements: a class of CLASSES that nobody reaches fails.

The restatement equals the oracle on every case and configuration and on ragged_city (a third
implementation on generated data); every tie class sits at the stated indices in the stated
state; every tie trace is discriminating (resolved towards the highest index its winners differ
from the oracle's); cand_sqd inside a bundle is bit-equal."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import ragged
from tests import viterbi_cases as C
from tests import viterbi_ref as R

ALL18, ALL20 = list(range(18)), list(range(20))
# (class, suite, trace, kind, state, the indices at the exact minimum).  kind 'pred': the
# predecessors of the winner of `state`, found in the state before it; 'end': the candidates of
# `state`, which ends a sub-path.
CLASSES = [
    ('the two halves of the split scan', 'k32', 'pred_0_1', 'pred', 1, [0, 1]),
    ('the lower index in the odd half', 'k32', 'pred_1_2', 'pred', 1, [1, 2]),
    ('both in the even half', 'k32', 'pred_0_2', 'pred', 1, [0, 2]),
    ('both in the odd half', 'k32', 'pred_1_3', 'pred', 1, [1, 3]),
    ('the U = 8 chunk boundary', 'k32', 'pred_7_8', 'pred', 1, [7, 8]),
    ('a chunk boundary inside the even half', 'k32', 'pred_14_16', 'pred', 1, [14, 16]),
    ('a chunk boundary inside the odd half', 'k32', 'pred_15_17', 'pred', 1, [15, 17]),
    ('both halves at the U = 16 chunk boundary', 'k32', 'pred_15_16', 'pred', 1, [15, 16]),
    ('a three-way tie', 'k32', 'pred_3_8_12', 'pred', 1, [3, 8, 12]),
    ('all 18 predecessors', 'k32', 'pred_all', 'pred', 1, ALL18),
    ('wide: the U = 16 chunk boundary', 'wide', 'pred_15_16', 'pred', 1, [15, 16]),
    ('wide: the second chunk boundary', 'wide', 'pred_31_32', 'pred', 1, [31, 32]),
    ('wide: inside the third chunk', 'wide', 'pred_32_33', 'pred', 1, [32, 33]),
    ('wide: the third chunk boundary', 'wide', 'pred_47_48', 'pred', 1, [47, 48]),
    ('end winner, butterfly distance 1', 'k32', 'end_0_1', 'end', 1, [0, 1]),
    ('end winner, distance 2', 'k32', 'end_1_3', 'end', 1, [1, 3]),
    ('end winner, distance 16', 'k32', 'end_0_16', 'end', 1, [0, 16]),
    ('end winner, distance 16 off lane 0', 'k32', 'end_3_19', 'end', 1, [3, 19]),
    ('winner at a break, distance 1', 'k32', 'brk_0_1', 'end', 1, [0, 1]),
    ('winner at a break, distance 2', 'k32', 'brk_1_3', 'end', 1, [1, 3]),
    ('winner at a break, distance 16', 'k32', 'brk_0_16', 'end', 1, [0, 16]),
    ('winner at a break, distance 16 off lane 0', 'k32', 'brk_3_19', 'end', 1, [3, 19]),
    ('a one-state sub-path on a bundle', 'k32', 'one_state_sub', 'end', 1, ALL20),
    ('a one-state trace on a bundle', 'k32', 'one_state_trace', 'end', 0, ALL20),
    ('wide: end winner, distance 32', 'wide', 'end_0_32', 'end', 1, [0, 32]),
    ('wide: end winner across lane 32', 'wide', 'end_31_32', 'end', 1, [31, 32]),
    ('wide: winner at a break, distance 32', 'wide', 'brk_0_32', 'end', 1, [0, 32]),
    ('wide: winner at a break across lane 32', 'wide', 'brk_31_32', 'end', 1, [31, 32]),
    ('both: the end tie', 'k32', 'both0', 'end', 1, [2, 7]),
    ('both: the predecessor tie behind it', 'k32', 'both0', 'pred', 1, [5, 9]),
    ('both: the end tie, high lanes', 'k32', 'both1', 'end', 1, [16, 18]),
    ('both: the predecessor tie behind it, across the halves', 'k32', 'both1', 'pred', 1, [1, 16]),
    ('ragged_K: 18 predecessors, 2 candidates', 'k32', 'rag0', 'pred', 1, [9, 17]),
    ('ragged_K: the end tie after 2 -> 18', 'k32', 'rag0', 'end', 2, [4, 6]),
    ('ragged_K: 2 predecessors, 18 candidates', 'k32', 'rag1', 'pred', 1, [0, 1]),
    ('ragged_K: 18 predecessors, 2 candidates, second step', 'k32', 'rag1', 'pred', 2, [2, 10]),
    ('long: state 3', 'k32', 'long104', 'pred', 4, [2, 11]),
    ('long: the end of 104 states (the LDS table of two traces per wave)', 'k32', 'long104', 'end', 103, [5, 14]),
    ('long: state 103 behind state 104 (105 states: global backtrack, two per wave)', 'k32', 'long105', 'pred', 104,
     [5, 14]),
    ('long: state 3 of 105 states', 'k32', 'long105', 'pred', 4, [2, 11]),
    ('long: state 103 inside 128 states', 'k32', 'long128', 'pred', 104, [5, 14]),
    ('long: the end of 128 states (the LDS table of one trace per wave)', 'k32', 'long128', 'end', 127, [9, 16]),
    ('long: state 127 behind state 128 (129 states: global backtrack)', 'k32', 'long129', 'pred', 128, [9, 16]),
    ('long: state 3 of 129 states', 'k32', 'long129', 'pred', 4, [2, 11]),
]
TIE_TRACES = sorted({(c[1], c[2]) for c in CLASSES})
SUITE_CFGS = [('k32', 'gtt'), ('k32', 'deployed'), ('k32', 'mixed'), ('wide', 'wide')]

_REF = {}


def ref(name, cfg, graph_dir, prefer='lowest'):
    """{trace name: the restatement's result} of the all-cases batch, once per process."""
    key = (name, cfg, prefer)
    if key not in _REF:
        s, tr, want = C.oracle_result(name, cfg, 'all', graph_dir)
        res = R.viterbi(po.Graph(s.path), tr, want, ragged.oracle_params(cfg), prefer)
        _REF[key] = (dict(zip(s.all_names(), res)), res)
    return _REF[key]


@pytest.mark.parametrize('name,cfg', SUITE_CFGS)
def test_restatement_equals_oracle_on_the_cases(name, cfg, graph_dir):
    s, tr, want = C.oracle_result(name, cfg, 'all', graph_dir)
    _, res = ref(name, cfg, graph_dir)
    assert np.array_equal(R.flat(res, 'winner'), want['winner'])
    assert np.array_equal(R.flat(res, 'subpath'), want['subpath'])
    assert len(want['seg_id']) > 0 and (want['winner'] >= 0).all()


@pytest.mark.parametrize('cfg', ['gtt', 'deployed'])
def test_restatement_equals_oracle_on_ragged_city(cfg, graph_dir):
    path, tr, want, _ = ragged.oracle_result('ragged_city', cfg, graph_dir)
    g, prm = po.Graph(path), ragged.oracle_params(cfg)
    res = R.viterbi(g, tr, want, prm)
    assert np.array_equal(R.flat(res, 'winner'), want['winner'])
    assert np.array_equal(R.flat(res, 'subpath'), want['subpath'])
    # the measurement, printed and not asserted: exact ties in generated data
    hi = R.viterbi(g, tr, want, prm, 'highest')
    differ = int((R.flat(hi, 'winner') != want['winner']).sum())
    traces = sum(1 for a, b in zip(res, hi) if a['winner'] != b['winner'])
    print('ragged_city %s: %d of %d predecessor minima and %d of %d sub-path ends are exact ties; resolved towards '
          'the highest index %d of %d winners in %d of %d traces differ' % (
              (cfg, R.count_ties(res)[0], sum(len(r['pred_ties']) for r in res), R.count_ties(res)[1],
               sum(len(r['end_ties']) for r in res), differ, len(want['winner']), traces, tr.n_traces)))


def test_route_step_is_route(graph_dir):
    """The whole-step routes the restatement reads are Graph.route's, pair by pair."""
    s, tr, want = C.oracle_result('k32', 'deployed', 'unreachable', graph_dir)
    g, prm = po.Graph(s.path), ragged.oracle_params('deployed')
    for a in range(len(want['winner']) - 1):
        Ka, Kb = int(want['cand_count'][a]), int(want['cand_count'][a + 1])
        se, sp = want['cand_edge'][a][:Ka], want['cand_p'][a][:Ka]
        de, dp = want['cand_edge'][a + 1][:Kb], want['cand_p'][a + 1][:Kb]
        d, t, c = g.route_step(se, sp, de, dp, 600.0, 240, prm, 0)
        for i in range(Ka):
            for j in range(Kb):
                one = g.route(int(se[i]), float(sp[i]), int(de[j]), float(dp[j]), 600.0, 240, prm, 0)
                assert (one is None and c[i][j] < 0) or one == (d[i][j], t[i][j], c[i][j]), (a, i, j, one)


CLASS_JOBS = [(cfg, c) for c in CLASSES for cfg in (('wide',) if c[1] == 'wide' else ('gtt', 'deployed', 'mixed'))]


@pytest.mark.parametrize('cfg,cls', CLASS_JOBS, ids=['%s-%s-%s-%s%d' % (cfg, c[1], c[2], c[3], c[4]) for cfg, c in CLASS_JOBS])
def test_tie_class_is_reached(cfg, cls, graph_dir):
    what, name, trace, kind, state, tied = cls
    r = ref(name, cfg, graph_dir)[0][trace]
    if kind == 'end':
        assert r['end_ties'].get(state) == tied, (what, r['end_ties'])
    else:
        assert r['pred_ties'].get((state, r['winner'][state])) == tied, (what, state, r['winner'][state])
        assert r['winner'][state - 1] == tied[0]


@pytest.mark.parametrize('name,cfg', SUITE_CFGS)
def test_every_tie_trace_is_discriminating(name, cfg, graph_dir):
    lo, hi = ref(name, cfg, graph_dir)[0], ref(name, cfg, graph_dir, 'highest')[0]
    s, tr, want = C.oracle_result(name, cfg, 'all', graph_dir)
    off = want['trace_state_off']
    for t, trace in enumerate(s.all_names()):
        assert lo[trace]['winner'] == [int(w) for w in want['winner'][off[t]:off[t + 1]]]
        if (name, trace) in TIE_TRACES:
            assert hi[trace]['winner'] != lo[trace]['winner'], trace
    assert all(tr_ in s.all_names() for n, tr_ in TIE_TRACES if n == name)


@pytest.mark.parametrize('name,cfg', SUITE_CFGS)
def test_bundles_project_bit_equal(name, cfg, graph_dir):
    """The premise: the duplicates of a bundle are consecutive candidates in edge-id order with
    bit-equal cand_sqd and cand_p."""
    s, tr, want = C.oracle_result(name, cfg, 'all', graph_dir)
    bundle = {}
    for (key, r), e in s.ids.items():
        bundle.setdefault(key, []).append(e)
    of_edge = {e: sorted(v) for v in bundle.values() if len(v) > 1 for e in v}
    seen = 0
    for st in range(len(want['winner'])):
        K = int(want['cand_count'][st])
        edges = [int(e) for e in want['cand_edge'][st][:K]]
        for e in set(edges) & set(of_edge):
            grp = of_edge[e]
            if e != grp[0]:
                continue
            at = edges.index(e)
            assert edges[at:at + len(grp)] == grp, (st, grp)
            sq, p = want['cand_sqd'][st][at:at + len(grp)], want['cand_p'][st][at:at + len(grp)]
            assert len(set(sq.tobytes()[8 * q:8 * q + 8] for q in range(len(grp)))) == 1 and len(set(p)) == 1
            seen += 1
    assert seen >= 8


@pytest.mark.parametrize('cfg', ['gtt', 'deployed', 'mixed'])
def test_unreachable_candidates(cfg, graph_dir):
    s, tr, want = C.oracle_result('k32', cfg, 'all', graph_dir)
    r = ref('k32', cfg, graph_dir)[0]['unreachable']
    t = s.all_names().index('unreachable')
    so = int(want['trace_state_off'][t])
    edge = lambda st, j: int(want['cand_edge'][so + st][j])
    ids = s.ids
    # state 1: the two stubs in front (no route from any predecessor: infinite cost, no break),
    # then the road and the spur, both reached
    assert r['K'] == [1, 4, 2, 3, 3] and r['breaks'] == [0, 3]
    assert [edge(1, j) for j in range(4)] == [ids[('stub0', 0)], ids[('stub1', 0)], ids[(('unr', 1), 0)],
                                              ids[('spur', 0)]]
    assert r['inf'] == {(1, 0), (1, 1)} and r['winner'][:3] == [0, 2, 0]
    # state 2: the stubs (infinite cost) have the shorter routes on, the spur (finite cost) has none
    g, prm = po.Graph(s.path), ragged.oracle_params(cfg)
    mode = s.mode['unreachable']
    route = lambda i, j: g.route(edge(1, i), float(want['cand_p'][so + 1][i]), edge(2, j),
                                 float(want['cand_p'][so + 2][j]), 600.0, C.DT, prm, mode)
    for j in range(2):
        assert route(0, j)[0] < route(2, j)[0] and route(1, j)[0] < route(2, j)[0]
        assert route(3, j) is None and (2, 3, j) in r['no_route'] and (2, 2, j) not in r['no_route']
        assert r['pred_ties'][(2, j)] == [2]
    # state 3: three candidates, none reached (no forced step): a break with K > 1
    assert all((3, i, j) in r['no_route'] for i in range(2) for j in range(3))


def test_ragged_K_and_long_positions(graph_dir):
    s = C.suite('k32', graph_dir)
    r = ref('k32', 'gtt', graph_dir)[0]
    assert r['rag0']['K'] == [18, 2, 18] and r['rag1']['K'] == [2, 18, 2]
    for names in (s.batches()['all'], s.batches()['ragged_K']):   # one wave: the neighbour's Kp is the larger one
        a, b = names.index('rag0'), names.index('rag1')
        assert a % 2 == 0 and b == a + 1
    rev = s.batches()['reversed']
    assert rev.index('rag1') % 2 == 0 and rev.index('rag0') == rev.index('rag1') + 1
    lds2, lds1 = ragged.LDS_STATES
    assert [len(r['long%d' % n]['K']) for n in C.LONG_LENS] == [lds2, lds2 + 1, lds1, lds1 + 1]
    assert max(max(r['long%d' % n]['K']) for n in C.LONG_LENS) <= 32 and r['long129']['breaks'] == [0]
    names = s.batches()['all']
    assert names.index('long104') % 2 == 0 and names.index('long128') % 2 == 0  # (104, 105) and (128, 129) share waves


def test_route_tie_walks_the_smaller_edge(graph_dir):
    for cfg in ('gtt', 'deployed'):
        s, tr, want = C.oracle_result('k32', cfg, 'route_tie', graph_dir)
        a, b = s.ids[(('rt', 1), 0)], s.ids[(('rt', 1), 1)]
        route = [int(e) for e in want['route_edge']]
        assert a < b and route == [s.ids[(('rt', 0), 0)], a, s.ids[(('rt', 2), 0)]], route


def test_modes_and_batches(graph_dir):
    """Under 'mixed' (turn costs for auto only) tied traces sit in both halves of a wave that
    holds one trace with turn costs and one without, in both orders; every tie trace is first
    and second in a wave over the three orders of the all-cases batch."""
    s = C.suite('k32', graph_dir)
    b = s.batches()
    ties = {t for n, t in TIE_TRACES if n == 'k32'}
    assert sorted(b['all']) == sorted(b['reversed']) == sorted(b['shuffled']) and len(b['all']) == 30
    assert b['shuffled'] != b['all'] and b['shuffled'] != b['reversed']
    halves = {t: set() for t in ties}
    mixed = set()
    for order in (b['all'], b['reversed'], b['shuffled']):
        for i, t in enumerate(order):
            if t in ties:
                halves[t].add(i % 2)
        for x, y in zip(order[0::2], order[1::2]):
            if x in ties and y in ties and (s.mode[x] == 0) != (s.mode[y] == 0):
                mixed.add(s.mode[x] == 0)
    assert all(h == {0, 1} for h in halves.values()), halves
    assert mixed == {True, False}
    assert {s.mode[t] for t in ties} == {0, 1, 2}
