"""Step 3 of the oracle's match_trace (oracle/oracle.c: transitions, Viterbi, breaks, end
winners, backtrack) restated in plain Python floats, in the oracle's
operation order, so that the exact cost ties show: the oracle's result holds no costs.  A
helper module (no tests, no fixtures): tests/test_viterbi_cases_cpu.py holds it equal to the
oracle and reads the tie sets.

The route triples come from pyoracle.Graph.route_step: Graph.route (orc_route) for every pair of
a step, with the step's bound and time difference.

viterbi(graph, traces, want, prm) takes the oracle's graph handle (pyoracle.Graph), the
gen.Traces that were matched, the oracle's result (its candidates are the input) and the
per-mode parameter array, and returns one dict per trace:

    winner, subpath   per state, as the oracle's result has them
    pred_ties         {(state, j): [i, ..]}: the predecessors of candidate j at the exact minimum
                      (every reachable candidate; a tie is a list longer than one)
    end_ties          {state: [j, ..]}: the candidates at the exact minimum where a sub-path ends
    inf               {(state, j)}: candidates that no predecessor reaches in a state that does
                      not break (infinite cost)
    no_route          {(state, i, j)}: pairs without a route in a step that is not forced
    breaks            [state]: the states that start a sub-path
    K                 per state, the candidate count

States are numbered within the trace.  prefer='highest' resolves every tie towards the highest
index instead: what a device that got the rule backwards would compute."""
import math

import numpy as np

from tests.matched_points_ref import gc_dist

INF = float('inf')


def _pick(idx, prefer):
    return idx[0] if prefer == 'lowest' else idx[-1]


def viterbi_trace(graph, tr, want, prm, t, prefer='lowest'):
    assert prefer in ('lowest', 'highest')
    mode = int(tr.mode[t]) if int(tr.mode[t]) < 3 else 0
    P = prm[mode]
    inv2s2 = 1.0 / (P.sigma_z * P.sigma_z * 2.0)
    inv_beta = 1.0 / P.beta
    so, eo = int(want['trace_state_off'][t]), int(want['trace_state_off'][t + 1])
    ns = eo - so
    K = [int(k) for k in want['cand_count'][so:eo]]
    probe = [int(p) for p in want['state_probe'][so:eo]]
    edge = want['cand_edge'][so:eo]
    frac = want['cand_p'][so:eo]
    sqd = want['cand_sqd'][so:eo]
    out = {'winner': [-1] * ns, 'subpath': [-1] * ns, 'pred_ties': {}, 'end_ties': {}, 'inf': set(),
           'no_route': set(), 'breaks': [], 'K': K}
    act = [s for s in range(ns) if K[s] > 0]
    na = len(act)
    if na == 0:
        return out
    bp = [None] * na
    brk = [False] * na
    end_winner = [None] * na

    def end_of(k, cost):
        best = min(cost)
        idx = [j for j, c in enumerate(cost) if c == best]
        out['end_ties'][act[k]] = idx
        end_winner[k] = _pick(idx, prefer)

    cost = [float(sqd[act[0]][j]) * inv2s2 for j in range(K[act[0]])]
    brk[0] = True
    for k in range(1, na):
        sa, sb = act[k - 1], act[k]
        ia, ib = probe[sa], probe[sb]
        Ka, Kb = K[sa], K[sb]
        gcd = gc_dist(float(tr.lat[ia]), float(tr.lon[ia]), float(tr.lat[ib]), float(tr.lon[ib]))
        forced = gcd > P.breakage_distance
        gfl = gcd if gcd > P.interpolation_distance else P.interpolation_distance
        bound = P.max_route_distance_factor * gfl
        if bound > P.breakage_distance:
            bound = P.breakage_distance
        dt = int(tr.time[ib]) - int(tr.time[ia])
        trans = [[INF] * Kb for _ in range(Ka)]
        if not forced:
            d, _, turn_mm = graph.route_step(edge[sa][:Ka], frac[sa][:Ka], edge[sb][:Kb], frac[sb][:Kb], bound, dt,
                                             prm, mode)
            for i in range(Ka):
                for j in range(Kb):
                    if turn_mm[i][j] < 0:
                        out['no_route'].add((sb, i, j))
                    else:
                        trans[i][j] = (float(turn_mm[i][j]) / 1000.0 + math.fabs(float(d[i][j]) - gcd)) * inv_beta
        ncost = [INF] * Kb
        b = [-1] * Kb
        for j in range(Kb):
            cs = [(cost[i] + trans[i][j], i) for i in range(Ka) if trans[i][j] != INF and cost[i] != INF]
            if cs:
                best = min(c for c, _ in cs)
                idx = [i for c, i in cs if c == best]
                out['pred_ties'][(sb, j)] = idx
                b[j] = _pick(idx, prefer)
                ncost[j] = best + float(sqd[sb][j]) * inv2s2
        if all(x < 0 for x in b):
            brk[k] = True
            ncost = [float(sqd[sb][j]) * inv2s2 for j in range(Kb)]
            end_of(k - 1, cost)
        else:
            out['inf'].update((sb, j) for j in range(Kb) if b[j] < 0)
        bp[k] = b
        cost = ncost
    end_of(na - 1, cost)
    cur = -1
    for k in range(na - 1, -1, -1):
        if k == na - 1 or brk[k + 1]:
            cur = end_winner[k]
        out['winner'][act[k]] = cur
        if not brk[k]:
            cur = bp[k][cur]
    sp = -1
    for k in range(na):
        if brk[k]:
            sp += 1
            out['breaks'].append(act[k])
        out['subpath'][act[k]] = sp
    return out


def viterbi(graph, tr, want, prm, prefer='lowest'):
    return [viterbi_trace(graph, tr, want, prm, t, prefer) for t in range(tr.n_traces)]


def flat(results, key):
    """The per-trace lists `key` ('winner', 'subpath') of viterbi()'s result as one array, as the
    oracle's result holds them."""
    return np.asarray([v for r in results for v in r[key]], np.int32)


def count_ties(results):
    """(predecessor ties, end ties): how many (state, candidate) minima and how many sub-path
    ends are reached by more than one index."""
    return (sum(1 for r in results for idx in r['pred_ties'].values() if len(idx) > 1),
            sum(1 for r in results for idx in r['end_ties'].values() if len(idx) > 1))
