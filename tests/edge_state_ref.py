"""A plain restatement of the edge-state route search's rounds (reporter_amd/csrc/otr_edge1.h),
for coverage only: exact integer arithmetic (mm, 0.1 s), dictionaries instead of tables, no
caps.  The reference for the results is the oracle; tests/test_edge_state_cases_cpu.py checks
this file's labels against Graph.route on every case, and the cases of tests/edge_state_cases.py
use its rounds to assert what they reach (how many states are final in a round, the key count
around a round, which state received an offer beyond the turn-cost cap and in which round).

The search: states are edges, a label is (key, length, time) with key = length + turn costs,
compared in that order.  The root is the source edge with the exit part of the source
candidate.  A round takes every pending state whose label is final by the IN criterion,
key < kmin + in_gap8(mi8_of(len)) + tmin (kmin the smallest pending key, tmin the mode's smallest
turn cost, the root's gap 1 mm), offers its label to the targets that start at its head node and
relaxes its out-edges.  An offer beyond the length or the time bound is dropped; an offer within
them makes the state a key of the table, and only then the turn-cost cap is tested (the order
of e1_relax_sink: a key without a label).  The rounds end when every target is final or out of
reach, or nothing is pending."""
import math

from oracle import pyoracle as po
from reporter_amd.graphfile import GraphFile

TC_CAP = 2097151     # kTcCap, otr_device.h
TB_MAX = 131070      # kTbMax
M_PER_DEG = 20037581.187 / 180.0


def _llround(x):
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def part_mm(frac, whole):
    return _llround(frac * float(whole))


def cos_deg(deg):
    """The oracle's cos_deg (a Taylor polynomial), operation for operation."""
    x = deg * (3.14159265358979323846 / 180.0)
    x2 = x * x
    r = -1.0 / 1124000727777607680000.0
    for c in (1.0 / 2432902008176640000.0, -1.0 / 6402373705728000.0, 1.0 / 20922789888000.0,
              -1.0 / 87178291200.0, 1.0 / 479001600.0, -1.0 / 3628800.0, 1.0 / 40320.0, -1.0 / 720.0,
              1.0 / 24.0, -1.0 / 2.0, 1.0):
        r = r * x2 + c
    return r


def gc_dist(lat1, lon1, lat2, lon2):
    x = (lon1 - lon2) * M_PER_DEG * cos_deg(0.5 * (lat1 + lat2))
    y = (lat1 - lat2) * M_PER_DEG
    return math.sqrt(x * x + y * y)


def mi8_of(length):
    return min(length >> 8, 255)


def in_gap8(mq):
    return mq << 8 if mq else 1


def step_bounds(prm, mode, gcd, dt):
    """(length bound mm, time bound 0.1 s or None) of a step (the oracle's step_ctx)."""
    P = prm[mode]
    bound = P.max_route_distance_factor * max(gcd, P.interpolation_distance)
    bound = min(bound, P.breakage_distance)
    bt = None
    if P.max_route_time_factor > 0.0 and dt > 0:
        b = math.floor(P.max_route_time_factor * float(dt) * 10.0)
        if b <= TB_MAX:
            bt = int(b)
    return int(math.floor(bound * 1000.0)), bt, bound


class RefGraph:
    """The graph as the search sees it under one mode: len_mm, route times, headings, access,
    the out- and in-edges of every node and the mode's turn table."""

    def __init__(self, path, prm=None, mode=0):
        self.gf = gf = GraphFile(path)
        self.og = po.Graph(path)
        self.prm = prm if prm is not None else po.params()
        self.mode = mode
        n = gf.n_edges
        self.src = [int(x) for x in gf.edge_src]
        self.dst = [int(x) for x in gf.edge_dst]
        self.len_mm = [max(1, _llround(float(x) * 1000.0)) for x in gf.edge_len]
        info = [self.og.edge_info(e, self.prm, mode) for e in range(n)]
        self.h_begin = [i[0] for i in info]
        self.h_end = [i[1] for i in info]
        self.time_ds = [i[2] for i in info]
        self.open = [bool((int(a) >> mode) & 1) for a in gf.edge_attr]
        self.row = [int(x) for x in gf.node_row]
        self.rev_row = [int(x) for x in gf.rev_row]
        self.rev_edge = [int(x) for x in gf.rev_edge]
        self.turn = po.turn_table(self.prm, mode)
        self.turn_on = self.prm[mode].turn_penalty_factor > 0.0
        self.tmin = min(self.turn)

    def out_edges(self, v):
        return range(self.row[v], self.row[v + 1])

    def in_edges(self, v):
        return [self.rev_edge[q] for q in range(self.rev_row[v], self.rev_row[v + 1])]

    def turn_degree(self, a, b):
        back = (self.h_end[a] + 180) % 360
        td = (self.h_begin[b] - back + 360) % 360
        return td if td <= 180 else 360 - td

    def turn_cost(self, a, b):
        return self.turn[self.turn_degree(a, b)]


class Search:
    """What one search left: `labels` (state -> final (key, length, time), absolute: the root's
    exit part included), `targets` (per target the best feasible (key, length, time) or None,
    and `via`, the smallest in-edge that gives it), `rounds`, `final_per_round`,
    `keys_after` (key count after each round, keys without a label included), `capped` (state ->
    the first round, from 1, in which an offer to it broke the turn-cost cap), `labelled`
    (state -> the round of its first feasible offer), `final_round` (state -> its round)."""


def search(G, ei, pi, targets, bmm, bt=None, exhaustive=False):
    """The rounds of the search from candidate (ei, pi) for `targets` [(ej, pj)] under the length
    bound bmm (mm) and the time bound bt (0.1 s, None: not applied).  exhaustive: the rounds go
    on until nothing is pending (k_general's search, which no target ends)."""
    assert G.turn_on
    timed = bt is not None
    S = Search()
    d0 = part_mm(1.0 - pi, G.len_mm[ei])
    t0 = part_mm(1.0 - pi, G.time_ds[ei]) if timed else 0
    need = [not (ej == ei and pj >= pi) for ej, pj in targets]
    tpart = [part_mm(pj, G.len_mm[ej]) for ej, pj in targets]
    tpt = [part_mm(pj, G.time_ds[ej]) if timed else 0 for ej, pj in targets]
    tlab = [None] * len(targets)
    via = [None] * len(targets)
    S.labels, S.capped, S.labelled, S.final_round = {}, {}, {}, {}
    S.rounds, S.final_per_round, S.keys_after = 0, [], []
    S.targets, S.via, S.need = tlab, via, need

    def feasible(k, d, t):
        return d <= bmm and (not timed or t <= bt) and k - d <= TC_CAP

    if not any(need) or not feasible(d0, d0, t0):
        return S
    lab = {ei: (d0, d0, t0)}
    gap = {ei: 1}
    keys, pending, final = {ei}, {ei}, set()
    S.labelled[ei] = 0
    while pending:
        kmin = min(lab[s][0] for s in pending)
        dmin = min(lab[s][1] for s in pending)
        tmn = min(lab[s][2] for s in pending)
        done = True
        for q in range(len(targets)):
            if not need[q]:
                continue
            if not ((tlab[q] is not None and tlab[q][0] < kmin + tpart[q] + G.tmin) or dmin + tpart[q] > bmm or
                    (timed and tmn + tpt[q] > bt)):
                done = False
        if done and not exhaustive:
            break
        S.rounds += 1
        take = sorted(s for s in pending if lab[s][0] < kmin + gap[s] + G.tmin)
        assert take
        for s in take:
            pending.discard(s)
            final.add(s)
            S.final_round[s] = S.rounds
        for s in take:  # (labels of this round's states are final: no offer among them improves one)
            k, d, t = lab[s]
            v = G.dst[s]
            for q, (ej, pj) in enumerate(targets):
                if need[q] and G.src[ej] == v:
                    o = (k + G.turn_cost(s, ej) + tpart[q], d + tpart[q], t + tpt[q])
                    if feasible(*o) and (tlab[q] is None or o < tlab[q] or (o == tlab[q] and s < via[q])):
                        tlab[q], via[q] = o, s
            for e in G.out_edges(v):
                if not G.open[e]:
                    continue
                o = (k + G.len_mm[e] + G.turn_cost(s, e), d + G.len_mm[e], t + (G.time_ds[e] if timed else 0))
                if o[1] > bmm or (timed and o[2] > bt):
                    continue
                keys.add(e)
                gap.setdefault(e, in_gap8(mi8_of(G.len_mm[e])))
                if o[0] - o[1] > TC_CAP:
                    S.capped.setdefault(e, S.rounds)
                    continue
                if e not in lab or o < lab[e]:
                    assert e not in final, ('a final label improved', e, lab[e], o)
                    lab[e] = o
                    S.labelled.setdefault(e, S.rounds)
                    pending.add(e)
        S.final_per_round.append(len(take))
        S.keys_after.append(len(keys))
    S.labels = dict(lab)
    S.final = final
    return S


def batch_searches(path, prm, tr, want, exhaustive=False):
    """Every search of batch `tr` (oracle result `want`) in a turn-cost mode, as the engine forms
    them: one per step between two states with candidates (not forced: at most the breakage
    distance apart) and per source candidate with a target that is not ahead on its own edge.
    Yields (trace, step dict, source index, Search)."""
    graphs = {}
    for t in range(tr.n_traces):
        md = int(tr.mode[t])
        if not prm[md].turn_penalty_factor > 0.0:
            continue
        if md not in graphs:
            graphs[md] = RefGraph(path, prm, md)
        G = graphs[md]
        for st in long_steps(G, tr, want, t):
            if st['gcd'] > prm[md].breakage_distance:
                continue
            for i, (ei, pi) in enumerate(st['src']):
                S = search(G, ei, pi, st['dst'], st['bmm'], st['bt'], exhaustive)
                if any(S.need):
                    yield t, st, i, S


def relax_counts(G, S):
    """(relaxations of the search's final states, the same with at most four per state: what the
    adjacency slots alone give, without the CSR-tail pass)."""
    full = capped4 = 0
    for s in getattr(S, 'final', ()):
        n = sum(1 for e in G.out_edges(G.dst[s]) if G.open[e])
        full += n
        capped4 += min(n, 4)
    return full, capped4


def route(G, ei, pi, ej, pj, bmm, bt=None):
    """(length mm, time 0.1 s, turn cost mm) of the transition (ei, pi) -> (ej, pj), or None: the
    same-edge part or the target's label of the search."""
    timed = bt is not None
    if ej == ei and pj >= pi:
        d = part_mm(pj - pi, G.len_mm[ei])
        t = part_mm(pj - pi, G.time_ds[ei]) if timed else 0
        return (d, t, 0) if d <= bmm and (not timed or t <= bt) else None
    S = search(G, ei, pi, [(ej, pj)], bmm, bt)
    if S.targets[0] is None:
        return None
    k, d, t = S.targets[0]
    return (d, t, k - d)


def long_steps(G, tr, want, t, min_gcd=0.0):
    """The steps of trace t of batch `tr` (oracle result `want`) as dicts: the two states, their
    candidates [(edge, fraction)], the great-circle distance, the time difference and the bounds."""
    off = want['trace_state_off']
    a, b = int(off[t]), int(off[t + 1])
    out = []
    act = [s for s in range(a, b) if int(want['cand_count'][s]) > 0]
    for sa, s in zip(act, act[1:]):
        ia, ib = int(want['state_probe'][sa]), int(want['state_probe'][s])
        gcd = gc_dist(float(tr.lat[ia]), float(tr.lon[ia]), float(tr.lat[ib]), float(tr.lon[ib]))
        if gcd < min_gcd:
            continue
        dt = int(tr.time[ib] - tr.time[ia])
        bmm, bt, bound = step_bounds(G.prm, G.mode, gcd, dt)

        def cands(st):
            n = int(want['cand_count'][st])
            return [(int(want['cand_edge'][st][k]), float(want['cand_p'][st][k])) for k in range(n)]
        out.append(dict(state=s, src=cands(sa), dst=cands(s), gcd=gcd, dt=dt, bmm=bmm, bt=bt, bound=bound))
    return out
