"""What the cases of tests/edge_state_cases.py reach, pinned on the CPU (no GPU): for every case
the oracle's batch result and the restatement of tests/edge_state_ref.py.

  * the restatement's labels equal Graph.route's (length, time, turn cost) for every (source,
    target) pair of every step of every case;
  * the known answers of the staircase, the exact ties of the diamonds;
  * the coverage facts tests/test_gpu_edge_state.py relies on, each as an assertion: the hub
    centres' out-degrees, the star's in-degree and candidate counts, the tree's rounds and key
    counts around the table sizes, the offers beyond the turn-cost cap and their rounds, the
    candidate counts of the ladder, the mode-dependent route, the time bound at its limit, the
    target behind the source.

The edge-state tiers take no size estimate: every turn-mode task starts in the 360-state table
(Batch::route_edge), so no case depends on first_tier_estimate."""
import pytest

from oracle import pyoracle as po
from tests import edge_state_cases as C
from tests import edge_state_ref as R

NOEDGE = 0xFFFFFFFF
_CACHE = {}


def case(name, graph_dir):
    """(Case, oracle parameters, batch, the oracle's result), computed once per process."""
    if name not in _CACHE:
        c = C.build(name, graph_dir)
        prm = C.oracle_params(c.cfg)
        b = c.batch()
        _CACHE[name] = (c, prm, b, po.match_batch(po.Graph(c.path), b, prm))
    return _CACHE[name]


def searches(name, graph_dir, exhaustive=False):
    key = (name, 'searches', exhaustive)
    if key not in _CACHE:
        c, prm, b, want = case(name, graph_dir)
        _CACHE[key] = list(R.batch_searches(c.path, prm, b, want, exhaustive))
    return _CACHE[key]


def route_of_trace(want, t):
    a, b = int(want['trace_route_off'][t]), int(want['trace_route_off'][t + 1])
    return [int(e) for e in want['route_edge'][a:b]]


def longest(ss, t):
    """The searches of trace t's longest step."""
    mine = [x for x in ss if x[0] == t]
    g = max(x[1]['gcd'] for x in mine)
    return [x for x in mine if x[1]['gcd'] == g]


@pytest.mark.parametrize('name', sorted(C.BUILDERS))
def test_restatement_equals_oracle_routes(name, graph_dir):
    """Every (source, target) pair of every step: the restatement's target label, or the part of
    the common edge, equals Graph.route's (length, time, turn cost) - or both find no route."""
    c, prm, b, want = case(name, graph_dir)
    assert R.GraphFile(c.path).n_edges <= 4000 and len(b.lat) <= 48
    og = po.Graph(c.path)
    graphs, n = {}, 0
    for t, st, i, S in searches(name, graph_dir):
        md = int(b.mode[t])
        G = graphs.setdefault(md, R.RefGraph(c.path, prm, md))
        ei, pi = st['src'][i]
        for q, (ej, pj) in enumerate(st['dst']):
            o = og.route(ei, pi, ej, pj, st['bound'], st['dt'], prm, md)
            if ej == ei and pj >= pi:
                r = R.route(G, ei, pi, ej, pj, st['bmm'], st['bt'])
            else:
                r = None if S.targets[q] is None else (S.targets[q][1], S.targets[q][2],
                                                       S.targets[q][0] - S.targets[q][1])
            o = None if o is None else (int(round(o[0] * 1000.0)), int(o[1]), int(o[2]))
            assert o == r, (name, t, st['state'], (ei, pi), (ej, pj), o, r)
            n += 1
    assert n > 0 or name.startswith('modes'), name


# ---- hub ------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [4, 5, 9])
def test_hub_out_degree_and_tail_relaxations(n, graph_dir):
    c, prm, b, want = case('hub%d' % n, graph_dir)
    G = R.RefGraph(c.path, prm, 0)
    assert len(G.out_edges(c.info['centre'])) == n
    assert max(len(G.out_edges(v)) for v in range(G.gf.n_nodes)) == n
    assert want['subpath'].max() == 0  # every trace one sub-path
    full = cap4 = 0
    for t, st, i, S in searches(c.name, graph_dir):
        f, c4 = R.relax_counts(G, S)
        full, cap4 = full + f, cap4 + c4
    # the adjacency slots alone give cap4 relaxations; more than that needs the tail pass
    assert (full > cap4) == (n > 4), (n, full, cap4)
    # the traces into every spoke, the one through the centre, the one that turns back
    ids = c.info['ids']
    for k in range(n - 1):
        assert route_of_trace(want, k)[:2] == [ids['WC>'], ids['S%d>' % k]]
    assert route_of_trace(want, n - 1) == [ids['S0<'], ids['S%d>' % (n - 2)]]
    m = (n - 1) // 2
    assert route_of_trace(want, n) == [ids['X%d>' % m], ids['X%d<' % m], ids['S%d<' % m]]  # the U-turn at the dead end


# ---- star70 ---------------------------------------------------------------------------------
def test_star70_in_degree_and_winner_paths(graph_dir):
    c, prm, b, want = case('star70', graph_dir)
    G = R.RefGraph(c.path, prm, 0)
    assert len(G.in_edges(c.info['centre'])) == 70 > 64
    assert 8 <= want['cand_count'].min() and want['cand_count'].max() <= 16  # about a dozen, not more than 32
    ids = c.info['ids']
    for t, (a, bb) in enumerate(c.info['pairs']):
        # in on spoke a, out on spoke b: the walk back from out_b picks in_a among C's 70 in-edges
        assert route_of_trace(want, t) == [ids['in%d' % a], ids['out%d' % bb]]
    assert want['subpath'].max() == 0


# ---- tree4 ----------------------------------------------------------------------------------
def test_tree4_rounds_and_key_counts(graph_dir):
    c, prm, b, want = case('tree4', graph_dir)
    ss = searches('tree4', graph_dir)
    (t, st, i, S), = longest(ss, 0)
    assert st['src'][i][0] == c.info['root']
    # whole levels are final in one round
    assert S.final_per_round == [1, 5, 20, 80, 320, 1280, 1]
    assert [1] + S.keys_after[:5] == c.info['keys'] and S.keys_after[-1] == c.info['n_tree'] == 1707
    assert any(f > 32 for f in S.final_per_round) and any(f > 64 for f in S.final_per_round)
    k = [1] + S.keys_after
    assert any(k[r] <= 315 and k[r + 1] > 360 for r in range(len(k) - 1))   # the 360-state table fills in a round
    assert any(k[r] <= 448 and k[r + 1] > 512 for r in range(len(k) - 1))   # and the 512-state one
    # the spread of a level's keys: below the IN gap + tmin (one round per level) and below
    # len - gap (no state of the next level final beside a waiting one of this level)
    G = R.RefGraph(c.path, prm, 0)
    by_round = {}
    for s, r in S.final_round.items():
        by_round.setdefault(r, []).append(S.labels[s][0])
    spread = max(max(v) - min(v) for v in by_round.values())
    assert spread < 100000 - 65280 and spread < 65280 + G.tmin, spread
    # the search runs the tree dry: the unconnected candidate is never reached, the target edge is
    assert S.targets.count(None) == 2 and len(S.final) == 1707
    assert want['subpath'][:4].tolist() == [0, 0, 0, 0] and c.info['target'] in route_of_trace(want, 0)
    # the reversed trace: searches that end with nothing pending and no target reached
    for t1, st1, i1, S1 in longest(ss, 1):
        assert all(x is None for x in S1.targets) and len(S1.final) == len(S1.labels) <= 2
    # the time-bounded traces: 426 keys (ends in the 512-state table: limit 448), 746 keys (the
    # 512-state table's limit passed between two rounds, 426 -> 490 with 64 states per round:
    # a dump; ends in the 1,024-state table: limit 896)
    (_, _, _, S2), = longest(ss, 2)
    (_, _, _, S3), = longest(ss, 3)
    assert S2.keys_after[-1] == 426 and 106 in S2.keys_after and S2.targets == [None] * 3
    assert S3.keys_after[-1] == 746 and 426 in S3.keys_after and S3.final_per_round[-1] == 320
    assert 448 < 426 + 64 <= 512 and 746 <= 896


# ---- stair ----------------------------------------------------------------------------------
def test_stair_known_answers(graph_dir):
    c, prm, b, want = case('stair', graph_dir)
    og = po.Graph(c.path)
    ids = c.info['ids']
    far = 1.0e6
    tab = po.turn_table(prm)
    assert (tab[180], tab[90]) == (3663, 27067)
    src = (ids['feeder'], 1.0 - 40.0 / 300.0)  # 40 m of the feeder left
    r76 = og.route(src[0], src[1], ids['s76'], 0.5, far, 0, prm)
    r77 = og.route(src[0], src[1], ids['s77'], 0.5, far, 0, prm)
    r78 = og.route(src[0], src[1], ids['s78'], 0.5, far, 0, prm)
    assert r76 is not None and r76[2] == 2060755 == 3663 + 76 * 27067
    assert r77 is not None and r77[2] == 2087822 == 3663 + 77 * 27067 <= R.TC_CAP
    # 825 m: the exit part, 77 stair edges, half of edge 77
    assert int(round(r77[0] * 1000)) == 40000 + 77 * 10000 + 5000
    assert r78 is None and 3663 + 78 * 27067 > R.TC_CAP
    # trace 0 crosses 77 turns in one step; trace 1 breaks where every target lies behind the 78th
    assert want['subpath'].tolist() == [0, 0, 0, 0, 0, 0, 1, 1]
    rt = route_of_trace(want, 0)
    assert rt[:77] == [ids['feeder']] + [ids['s%d' % j] for j in range(76)] and NOEDGE not in rt
    # (the winner there stops short of edge 77: fewer turns weigh more than the distance to the
    # probe; with edge 77 / 78 the only candidate, stair_near, the winner crosses 77 turns exactly)
    cn, prmn, bn, wn = case('stair_near', graph_dir)
    assert wn['cand_count'].tolist() == [1] * 12 and wn['subpath'].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1]
    chain = [ids['feeder']] + [ids['s%d' % j] for j in range(78)]
    assert route_of_trace(wn, 0) == chain and route_of_trace(wn, 2) == chain + [ids['straight']]
    (_, stn, _, Sn), = longest(searches('stair_near', graph_dir), 1)
    assert stn['dst'][0][0] == ids['s78'] and Sn.targets == [None] and set(Sn.capped) == {ids['s78'], ids['slant']}
    # at the cap: straight on from edge 77 stays under it by 5,666 mm, the slant breaks it by 628 mm
    rs = og.route(src[0], src[1], ids['straight'], 0.5, far, 0, prm)
    assert rs is not None and rs[2] == 2091485 == 2087822 + tab[180] <= R.TC_CAP
    assert og.route(src[0], src[1], ids['slant'], 0.5, far, 0, prm) is None and 2087822 + tab[135] == R.TC_CAP + 628
    (_, st2, _, S2), = longest(searches('stair_near', graph_dir), 2)
    (_, st3, _, S3), = longest(searches('stair_near', graph_dir), 3)
    assert st2['dst'][0][0] == ids['straight'] and S2.targets[0][0] - S2.targets[0][1] == 2091485
    # (only the labelled state of edge 77 offers it)
    assert S2.labels[ids['s77']][0] - S2.labels[ids['s77']][1] == 2087822
    assert st3['dst'][0][0] == ids['slant'] and S3.targets == [None]
    assert route_of_trace(want, 1).count(NOEDGE) == 1
    ss = searches('stair', graph_dir)
    for t in (0, 1):
        capped = [S.capped for _, st, i, S in longest(ss, t) if st['src'][i][0] == ids['feeder']]
        assert capped and all(set(x) == {ids['s78'], ids['slant']} for x in capped), capped
    # from the feeder: one state per round, the cap-breaking offer in the round that settles edge 77
    S = [S for _, st, i, S in longest(ss, 0) if st['src'][i][0] == ids['feeder']][0]
    assert S.capped[ids['s78']] == S.final_round[ids['s77']] == 79 and ids['s78'] not in S.labels
    assert any(x is not None and x[0] - x[1] == 2087822 for x in S.targets)


@pytest.mark.parametrize('order', ['early', 'late'])
def test_stair_bypass_offers_in_both_orders(order, graph_dir):
    c, prm, b, want = case('stair_' + order, graph_dir)
    ids = c.info['ids']
    (t, st, i, S), = longest(searches(c.name, graph_dir), 0)
    s78 = ids['s78']
    assert s78 in S.capped and s78 in S.labels  # a cap-breaking and a feasible offer
    assert S.capped[s78] == S.final_round[ids['s77']]
    if order == 'early':
        assert S.final_round[s78] < S.capped[s78] - 50  # the label was final long before
    else:
        # a key without a label from the cap-breaking offer to the bypass's, rounds later
        assert S.capped[s78] == 79 and S.labelled[s78] == S.final_round[ids['bypass']] > 79
        assert S.labels[s78][0] - S.labels[s78][1] <= R.TC_CAP
    q = [k for k, (ej, pj) in enumerate(st['dst']) if ej == s78][0]
    assert S.targets[q] is not None and S.via[q] == ids['bypass'] and want['subpath'].max() == 0
    if order == 'early':
        assert route_of_trace(want, 0)[:2] == [ids['feeder'], ids['bypass']]


def test_stair_steep_caps_in_the_first_rounds(graph_dir):
    """Under turn_penalty_factor 2,000 the offers to the two side edges break the cap in round 2
    and in round 5 (between rounds 3 and 6): a search stopped after 2 rounds and again 4 rounds later (the
    forced stops of the test build) dumps a key without a label both times."""
    c, prm, b, want = case('stair_steep', graph_dir)
    ids = c.info['ids']
    ss = [x for x in longest(searches('stair_steep', graph_dir), 0) if x[1]['src'][x[2]][0] == ids['feeder']]
    assert ss
    for t, st, i, S in ss:
        assert S.capped[ids['side0']] == 2 and 2 < S.capped[ids['side3']] <= 6, S.capped
        assert ids['side0'] not in S.labels and ids['side3'] not in S.labels
        assert S.rounds > 6  # still running at both stops
    assert want['subpath'].max() == 0


# ---- ties -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ties', 'ties_mirror'])
def test_exact_tie_takes_the_smaller_in_edge(name, graph_dir):
    c, prm, b, want = case(name, graph_dir)
    ids = c.info['ids']
    G = R.RefGraph(c.path, prm, 0)
    S = [S for _, st, i, S in longest(searches(name, graph_dir), 0) if st['src'][i][0] == ids['WS']][0]
    assert S.labels[ids['PT']] == S.labels[ids['QT']]  # (key, length, time) equal
    assert G.turn_cost(ids['PT'], ids['TN']) == G.turn_cost(ids['QT'], ids['TN'])
    small = min(ids['PT'], ids['QT'])
    assert (small == ids['PT']) == (name == 'ties')  # the smaller id on the other branch in the mirror
    rt = route_of_trace(want, 0)
    assert small in rt and max(ids['PT'], ids['QT']) not in rt
    q = [k for k, (ej, pj) in enumerate(longest(searches(name, graph_dir), 0)[0][1]['dst']) if ej == ids['TN']][0]
    assert S.via[q] == small


def test_key_tie_decided_by_length(graph_dir):
    c, prm, b, want = case('ties_key', graph_dir)
    ids = c.info['ids']
    og = po.Graph(c.path)
    tab = po.turn_table(prm)
    G = R.RefGraph(c.path, prm, 0)

    def deg(a, bb):
        back = (og.edge_info(ids[a])[1] + 180) % 360
        td = (og.edge_info(ids[bb])[0] - back + 360) % 360
        return td if td <= 180 else 360 - td
    tp = tab[deg('WS', 'SP')] + tab[deg('SP', 'PT')] + tab[deg('PT', 'TN')]
    tq = tab[deg('WS', 'SQ')] + tab[deg('SQ', 'QT')] + tab[deg('QT', 'TN')]
    assert (tp, tq) == (c.info['turn_p'], c.info['turn_q']) and tp != tq
    assert G.len_mm[ids['SP']] - G.len_mm[ids['SQ']] == tq - tp  # the lengths differ by the turn sums' difference
    steps = longest(searches('ties_key', graph_dir), 0)
    S = [S for _, st, i, S in steps if st['src'][i][0] == ids['WS']][0]
    q = [k for k, (ej, pj) in enumerate(steps[0][1]['dst']) if ej == ids['TN']][0]
    kp = S.labels[ids['PT']][0] + G.turn_cost(ids['PT'], ids['TN'])
    kq = S.labels[ids['QT']][0] + G.turn_cost(ids['QT'], ids['TN'])
    assert kp == kq and S.labels[ids['PT']][1] != S.labels[ids['QT']][1]
    short = 'PT' if S.labels[ids['PT']][1] < S.labels[ids['QT']][1] else 'QT'
    assert S.via[q] == ids[short]
    rt = route_of_trace(want, 0)
    assert ids[short] in rt and ids['QT' if short == 'PT' else 'PT'] not in rt


# ---- modes ----------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', ['deployed', 'mixed'])
def test_modes_routes_differ(cfg, graph_dir):
    c, prm, b, want = case('modes_' + cfg, graph_dir)
    ids = c.info['ids']
    assert b.mode.tolist() == [0, 1, 2, 0, 1, 2]
    auto, bike, foot = (route_of_trace(want, t) for t in range(3))
    assert ids['AB>'] not in auto and ids['CD>'] in auto       # closed to auto: round the loop
    assert ids['AB>'] in bike and ids['AB>'] in foot and auto != bike
    assert ids['CD<'] in route_of_trace(want, 3) and ids['AB<'] in route_of_trace(want, 4)
    assert want['subpath'].max() == 0
    turn_modes = {int(b.mode[t]) for t, _, _, _ in searches(c.name, graph_dir)}
    assert turn_modes == ({0, 1, 2} if cfg == 'deployed' else {0})  # mixed: node and edge-state searches in one batch


# ---- wide -----------------------------------------------------------------------------------
def test_wide_candidate_counts(graph_dir):
    c32, prm, b, w32 = case('wide32', graph_dir)
    c34, _, _, w34 = case('wide34', graph_dir)
    assert set(w32['cand_count'].tolist()) == {32} and set(w34['cand_count'].tolist()) == {34}
    assert prm[0].turn_penalty_factor == 200.0 and prm[0].max_candidates == 64
    G = R.RefGraph(c32.path, prm, 0)
    for t, st, i, S in longest(searches('wide32', graph_dir), 0)[:1]:
        assert len(st['dst']) == 32 and len({G.src[ej] for ej, pj in st['dst']}) == 32  # 32 lanes, 32 target nodes
        assert all(S.need)
    assert w32['subpath'].max() == 0 and w34['subpath'].max() == 0


# ---- timed ----------------------------------------------------------------------------------
def test_timed_breaks_under_turn_costs(graph_dir):
    c, prm, b, want = case('timed', graph_dir)
    ids = c.info['ids']
    assert prm[0].turn_penalty_factor == 200.0
    assert want['subpath'].tolist() == [0] * 5 + [1] * 5 + [0] * 5 + [1] * 5
    assert route_of_trace(want, 0) == [ids['T0>'], ids['T1>'], NOEDGE, ids['T3>'], ids['T4>']]
    assert ids['T2>'] not in want['route_edge'] and ids['T2<'] not in want['route_edge']


def test_time_bound_at_its_limit(graph_dir):
    c, prm, b, want = case('tbmax', graph_dir)
    G = R.RefGraph(c.path, prm, 0)
    assert G.time_ds[0] == 7200
    ss = searches('tbmax', graph_dir)
    bt = [longest(ss, t)[0][1]['bt'] for t in range(3)]
    assert bt == [131060, None, 131060] and 131060 <= R.TB_MAX < 131080
    assert want['subpath'].tolist() == [0, 1, 0, 0, 0, 0]  # 131,760 breaks the applied bound; no bound; 130,680 holds
    assert len(route_of_trace(want, 1)) == 19 and len(route_of_trace(want, 2)) == 19


# ---- loop -----------------------------------------------------------------------------------
def test_target_behind_source_goes_round(graph_dir):
    c, prm, b, want = case('ring', graph_dir)
    ids = c.info['ids']
    assert want['cand_count'].tolist() == [1, 1, 1, 1] and want['subpath'].max() == 0
    ss = [x for x in searches('ring', graph_dir)]
    assert len(ss) == 1  # the forward steps need no search
    t, st, i, S = ss[0]
    (ei, pi), (ej, pj) = st['src'][i], st['dst'][0]
    assert ei == ej == ids['AB'] and pj < pi
    k, d, tt = S.targets[0]
    assert abs(d - 82000) <= 100 and k - d == 4 * 27067 and d <= st['bmm']
    assert route_of_trace(want, 0) == [ids['AB'], ids['BC'], ids['CD'], ids['DA'], ids['AB']]
    for name in ('square', 'block'):
        c2, prm2, b2, w2 = case(name, graph_dir)
        assert prm2[0].turn_penalty_factor == 200.0 and w2['subpath'].max() == 0
