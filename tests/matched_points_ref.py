"""Matched points restated in plain Python floats: binary64, one
operation at a time (no FMA), math.sqrt, no numpy arithmetic on decision paths.  A helper
module (no tests, no fixtures): tests/test_matched_points_cpu.py pins what it computes,
tests/test_gpu_matched_points.py holds k_matched_points equal to it bit for bit.

matched_points(res, traces, graph) takes a match result dict (the oracle's or the engine's:
compare() holds them equal), the gen.Traces that were matched and the GraphFile, and returns
the eight per-probe arrays plus, under 'gaps', what each gap looked like (for the tests)."""
import math

import numpy as np

KM = 20037581.187 / 180.0   # metres per degree (otr_device.h kMetersPerDeg)
KMAX = 64
NO_EDGE = 0xFFFFFFFF
FIELDS = ('kind', 'edge', 'frac', 'lat', 'lon', 'dist', 'state', 'pos_mm')


def cos_deg(deg):
    """otr_device.h cos_deg: the Taylor series to x^22 in Horner form."""
    x = deg * (3.14159265358979323846 / 180.0)
    x2 = x * x
    r = -1.0 / 1124000727777607680000.0
    r = r * x2 + 1.0 / 2432902008176640000.0
    r = r * x2 - 1.0 / 6402373705728000.0
    r = r * x2 + 1.0 / 20922789888000.0
    r = r * x2 - 1.0 / 87178291200.0
    r = r * x2 + 1.0 / 479001600.0
    r = r * x2 - 1.0 / 3628800.0
    r = r * x2 + 1.0 / 40320.0
    r = r * x2 - 1.0 / 720.0
    r = r * x2 + 1.0 / 24.0
    r = r * x2 - 1.0 / 2.0
    r = r * x2 + 1.0
    return r


def gc_dist(lat1, lon1, lat2, lon2):
    x = (lon1 - lon2) * KM * cos_deg(0.5 * (lat1 + lat2))
    y = (lat1 - lat2) * KM
    return math.sqrt(x * x + y * y)


def part_mm(frac, len_mm):
    """llround(frac * len_mm): floor, then + 1 if the remainder is >= 0.5."""
    v = frac * float(len_mm)
    f = math.floor(v)
    return int(f) + (1 if v - f >= 0.5 else 0)


class Geometry:
    """An edge's shape as Python floats (e6 of the stored micro-degrees) and len_mm."""

    def __init__(self, graph):
        self.g = graph
        self._shape = {}
        self._len = {}

    def shape(self, e):
        s = self._shape.get(e)
        if s is None:
            k0, k1 = int(self.g.edge_shape[e]), int(self.g.edge_shape[e + 1])
            s = [(float(int(self.g.shape_ll[2 * k])) * 1e-6, float(int(self.g.shape_ll[2 * k + 1])) * 1e-6)
                 for k in range(k0, k1)]
            self._shape[e] = s
        return s

    def len_mm(self, e):
        v = self._len.get(e)
        if v is None:
            x = float(np.float32(self.g.edge_len[e])) * 1000.0   # llround: half away from zero (x >= 0)
            f = math.floor(x)
            v = max(1, int(f) + (1 if x - f >= 0.5 else 0))
            self._len[e] = v
        return v


def _seg(pa, pb, plat, plon, mpl):
    ax = (pa[1] - plon) * mpl
    ay = (pa[0] - plat) * KM
    bx = (pb[1] - plon) * mpl
    by = (pb[0] - plat) * KM
    dx = bx - ax
    dy = by - ay
    return ax, ay, dx, dy, dx * dx + dy * dy


def project(geo, e, plat, plon):
    """(d2, frac) of K1's projection onto the whole polyline of e (oracle.c:203-227, 234)."""
    mpl = KM * cos_deg(plat)
    best, best_along, acc = math.inf, 0.0, 0.0
    sh = geo.shape(e)
    for k in range(len(sh) - 1):
        ax, ay, dx, dy, l2 = _seg(sh[k], sh[k + 1], plat, plon, mpl)
        t = 0.0
        if l2 > 0.0:
            t = -(ax * dx + ay * dy) / l2
            if t < 0.0:
                t = 0.0
            if t > 1.0:
                t = 1.0
        qx = ax + t * dx
        qy = ay + t * dy
        d2 = qx * qx + qy * qy
        sl = math.sqrt(l2)
        if d2 < best:
            best = d2
            best_along = acc + t * sl
        acc = acc + sl
    return best, (best_along / acc if acc > 0.0 else 0.0)


def point_at(geo, e, f, plat, plon):
    mpl = KM * cos_deg(plat)
    sh = geo.shape(e)
    sls = [math.sqrt(_seg(sh[k], sh[k + 1], plat, plon, mpl)[4]) for k in range(len(sh) - 1)]
    acc = 0.0
    for sl in sls:
        acc = acc + sl
    target = f * acc
    cum = 0.0
    k = len(sls) - 1
    for j, sl in enumerate(sls):
        if cum + sl >= target:
            k = j
            break
        if j < len(sls) - 1:
            cum = cum + sl
    sl = sls[k]
    u = (target - cum) / sl if sl > 0.0 else 0.0
    if u < 0.0:
        u = 0.0
    if u > 1.0:
        u = 1.0
    la, lo = sh[k]
    return la + u * (sh[k + 1][0] - la), lo + u * (sh[k + 1][1] - lo)


def matched_points(res, traces, graph):
    geo = Geometry(graph)
    n = int(traces.offsets[-1])
    out = {'kind': np.zeros(n, np.uint8), 'edge': np.full(n, NO_EDGE, np.uint32), 'frac': np.zeros(n, np.float64),
           'lat': np.zeros(n, np.float64), 'lon': np.zeros(n, np.float64), 'dist': np.zeros(n, np.float64),
           'state': np.full(n, -1, np.int64), 'pos_mm': np.full(n, -1, np.int64)}
    gaps = []
    soff = [int(x) for x in res['trace_state_off']]
    roff = [int(x) for x in res['trace_route_off']]
    cand_edge = np.asarray(res['cand_edge']).reshape(-1, KMAX)
    cand_p = np.asarray(res['cand_p']).reshape(-1, KMAX)
    lat_all, lon_all = traces.lat, traces.lon

    def put(i, kind, e, f, state, pos):
        plat, plon = float(lat_all[i]), float(lon_all[i])
        la, lo = point_at(geo, e, f, plat, plon)
        out['kind'][i], out['edge'][i], out['frac'][i] = kind, e, f
        out['lat'][i], out['lon'][i] = la, lo
        out['dist'][i] = gc_dist(plat, plon, la, lo)
        out['state'][i], out['pos_mm'][i] = state, pos

    for t in range(traces.n_traces):
        act = [s for s in range(soff[t], soff[t + 1]) if int(res['cand_count'][s]) > 0]
        win = {}
        for s in act:
            w = int(res['winner'][s])
            assert w >= 0, (t, s)
            win[s] = (int(cand_edge[s, w]), float(cand_p[s, w]))
        # the sub-paths' edge lists of this trace, in order (single-state sub-paths have none)
        route = [int(x) for x in res['route_edge'][roff[t]:roff[t + 1]]]
        lists, cur = [], []
        for x in route:
            if x == NO_EDGE:
                lists.append(cur)
                cur = []
            else:
                cur.append(x)
        if route:
            lists.append(cur)
        sub = [int(res['subpath'][s]) for s in act]
        k, li = 0, 0
        while k < len(act):
            k1 = k + 1
            while k1 < len(act) and sub[k1] == sub[k]:
                k1 += 1
            # sub-path: active ordinals k .. k1 - 1
            pos = 0
            put(int(res['state_probe'][act[k]]), 1, win[act[k]][0], win[act[k]][1], act[k], 0)
            if k1 - k > 1:
                lst = lists[li]
                li += 1
                assert lst and lst[0] == win[act[k]][0], (t, k)
                at = 1
            for q in range(k + 1, k1):
                a, b = act[q - 1], act[q]
                (ea, pa), (eb, pb) = win[a], win[b]
                if eb == ea and pb >= pa:
                    pieces = [(ea, pa, pb)]
                    pos_b = pos + part_mm(pb - pa, geo.len_mm(ea))
                else:
                    end = lst.index(eb, at)    # up to and including the next occurrence of eb
                    path = lst[at:end]
                    at = end + 1
                    pieces = [(ea, pa, 1.0)] + [(e, 0.0, 1.0) for e in path] + [(eb, 0.0, pb)]
                    pos_b = pos + part_mm(1.0 - pa, geo.len_mm(ea))
                    for e in path:
                        pos_b += geo.len_mm(e)
                    pos_b += part_mm(pb, geo.len_mm(eb))
                ia, ib = int(res['state_probe'][a]), int(res['state_probe'][b])
                c, fc = 0, pa
                rec = {'trace': t, 'a': a, 'b': b, 'pieces': pieces, 'probes': list(range(ia + 1, ib)),
                       'pos_a': pos, 'pos_b': pos_b, 'clamped': 0, 'moved': 0}
                for i in range(ia + 1, ib):
                    plat, plon = float(lat_all[i]), float(lon_all[i])
                    bq, bd2, bf = -1, 0.0, 0.0
                    for qq in range(c, len(pieces)):
                        d2, f = project(geo, pieces[qq][0], plat, plon)
                        if bq < 0 or d2 < bd2:
                            bq, bd2, bf = qq, d2, f
                    e, f_lo, f_hi = pieces[bq]
                    f = bf
                    if f < f_lo:
                        f = f_lo
                    if f > f_hi:
                        f = f_hi
                    if bq == c and f < fc:
                        f = fc
                    if f != bf:
                        rec['clamped'] += 1
                    if bq > c:
                        rec['moved'] += 1
                    c, fc = bq, f
                    if bq == 0:
                        pm = pos + part_mm(f - pa, geo.len_mm(ea))
                    else:
                        pm = pos + part_mm(1.0 - pa, geo.len_mm(ea))
                        for pe, _, _ in pieces[1:bq]:
                            pm += geo.len_mm(pe)
                        pm += part_mm(f, geo.len_mm(e))
                    if pm > pos_b:
                        pm = pos_b
                    put(i, 2, e, f, a, pm)
                gaps.append(rec)
                pos = pos_b
                put(ib, 1, eb, pb, b, pos)
            if k1 - k > 1:
                assert at == len(lst), (t, k, at, len(lst))   # the sub-path's list is consumed exactly
            k = k1
        assert li == len(lists), (t, li, len(lists))
    out['gaps'] = gaps
    return out


def same_bits(got, want):
    """The names of the per-probe arrays that differ (bit for bit) between two results."""
    bad = []
    for k in FIELDS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
            bad.append(k)
    return bad


# ---- the batches both test files run ------------------------------------------------------
# name -> (options for every mode, on top of the deployment's); 'deployed' / 'gtt' as in tests/ragged.py
CITY_ARGS = (16, 120, 1, 5.0, 1, 0.3, 0.2)   # 1,920 probes at 1 Hz on the city graph
OPTIONS = {
    'deployed': {},
    'gtt': {'turn_penalty_factor': 0},
    'deployed250': {'interpolation_distance': 250},
    'gtt250': {'turn_penalty_factor': 0, 'interpolation_distance': 250},
    'gtt50': {'turn_penalty_factor': 0, 'interpolation_distance': 50},
}


def city(graph_dir):
    from reporter_amd.tools import gen
    path = gen.graph_path('city', graph_dir)
    return path, gen.make_traces(path, *CITY_ARGS)


def _traces(rows):
    """rows: per trace [(lat, lon)], one probe every 2 s."""
    from reporter_amd.tools.gen import Traces
    lat = np.array([p[0] for r in rows for p in r], np.float64)
    lon = np.array([p[1] for r in rows for p in r], np.float64)
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    tm = np.concatenate([1483228800 + 2 * np.arange(len(r), dtype=np.int64) for r in rows])
    return Traces(lat, lon, tm, off, np.zeros(len(rows), np.uint8))


KAT_NORTH = 0.00002   # degrees: the probes run 2.2 m north of the road


def kat(graph_dir):
    """A straight one-way road on the equator (cos_deg(0) == 1): edge E0 from lon 0 to
    0.001 (111 m), E1 on to 0.002, and four traces beside it (interpolation_distance 50):
    0 collinear: ten probes 22 m apart, states at probes 0, 3, 6, 9;
    1 a step backwards: probe 2 projects behind probe 1;
    2 a later piece: probe 1 is nearest to E1, probe 2 to E0 behind it;
    3 probe 2 follows the last active state (probe 3, a state, is far off the graph)."""
    import os
    from reporter_amd.graphfile import write_graph
    path = os.path.join(graph_dir, 'matched_points_kat.otrg')
    new = write_graph(path, [(0.0, 0.0), (0.0, 0.001), (0.0, 0.002)],
                      [dict(src=0, dst=1, way=1), dict(src=1, dst=2, way=1)])
    y = KAT_NORTH
    rows = [[(y, 0.0001 + 0.0002 * k) for k in range(10)],
            [(y, 0.0001), (y, 0.0004), (y, 0.0003), (y, 0.0007)],
            [(y, 0.0007), (y, 0.00105), (y, 0.00095), (y, 0.0013)],
            [(y, 0.0001), (y, 0.0007), (y, 0.0008), (1.0, 0.0009)]]
    return path, _traces(rows), [int(new[0]), int(new[1])]


ARC_POINTS = 130   # interior shape points of the arc: 131 shape segments


def arc(graph_dir):
    """One edge of ARC_POINTS + 2 shape points, a quarter circle of 445 m radius on the
    equator, then a straight edge; a trace of probes 15 m apart along both, alternately
    3 m inside and outside (interpolation_distance 50): the shape walks of project and
    point_at pass 64 segments."""
    import os
    from reporter_amd.graphfile import write_graph
    path = os.path.join(graph_dir, 'matched_points_arc.otrg')
    R = 0.004

    def on_arc(frac, r):
        th = 0.5 * math.pi * frac
        return (r * math.sin(th), r - r * math.cos(th) + (R - r))
    shape = [on_arc((k + 1) / (ARC_POINTS + 1.0), R) for k in range(ARC_POINTS)]
    write_graph(path, [on_arc(0.0, R), on_arc(1.0, R), (R + 0.002, R)],
                [dict(src=0, dst=1, way=1, shape=shape), dict(src=1, dst=2, way=1)])
    n_arc = 46
    row = [on_arc((k + 0.5) / n_arc, R + (0.000027 if k % 2 else -0.000027)) for k in range(n_arc)]
    row += [(R + 0.000135 * (k + 1), R + (0.00002 if k % 2 else -0.00002)) for k in range(12)]
    return path, _traces([[(round(a, 7), round(b, 7)) for a, b in row]])
