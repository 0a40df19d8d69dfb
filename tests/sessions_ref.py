"""The session store restated as a plain per-point loop: what the
streaming reporter does per key (a session of points, the report gate, the trim by
shape_used, the eviction of quiet sessions), plus the store's cap.  Float steps in numpy
float32, everything else in Python floats and ints, one operation at a time.  A helper
module (no tests, no fixtures): tests/test_sessions_cpu.py pins what it computes,
tests/test_gpu_sessions.py holds the device store equal to it.

match(points, key, trigger) -> (shape_used or None, ok, reports): points is a list of
(lat, lon, time, accuracy) as the matcher sees them (binary64 coordinates after the text round
trip, float accuracy); reports a list of (id, next_id, t0, t1, length, queue_length)."""
import math

import numpy as np

from tests.matched_points_ref import KM, cos_deg

NO_ID = 0xFFFFFFFFFFFFFFFF
MATCH_ERROR = 500
WINDOW_FIELDS = (('key', np.uint64), ('trigger', np.int64), ('n_points', np.int32), ('shape_used', np.int32),
                 ('status', np.int32), ('trimmed', np.int32))
REPORT_FIELDS = (('id', np.uint64), ('next_id', np.uint64), ('t0', np.float64), ('t1', np.float64),
                 ('length', np.int32), ('queue_length', np.int32))
SNAPSHOT_FIELDS = ('key', 'point_off', 'max_sep', 'last_update', 'lat', 'lon', 'accuracy', 'time')
POINT_TYPES = (('key', np.uint64), ('lat', np.float32), ('lon', np.float32), ('accuracy', np.int32),
               ('time', np.int64), ('timestamp', np.int64))


def dist(alat, alon, blat, blon):
    """The reporter's distance between two float32 points: differences and the mid latitude in
    binary32, the rest in binary64."""
    alat, alon, blat, blon = np.float32(alat), np.float32(alon), np.float32(blat), np.float32(blon)
    dlon = np.float32(alon - blon)
    mid = np.float32(np.float32(0.5) * np.float32(alat + blat))
    dlat = np.float32(alat - blat)
    x = (float(dlon) * KM) * cos_deg(float(mid))
    y = float(dlat) * KM
    return math.sqrt(x * x + y * y)


def widen(f):
    """What the six-decimal HALF_EVEN text of a float32 coordinate parses back to."""
    return float(np.rint(float(np.float32(f)) * 1e6)) / 1e6


class Store:
    def __init__(self, match, max_points, report_dist=500.0, report_count=10, report_time=60, session_gap=60000):
        self.match = match
        self.max_points = max_points
        self.report_dist = np.float32(report_dist)
        self.report_count, self.report_time, self.session_gap = report_count, report_time, session_gap
        self.sessions = {}   # key -> {'pts': [(lat f32, lon f32, accuracy, time)], 'max_sep': f32, 'last': ts}
        self.n_forced = self.n_dropped = 0

    # -- one window: match, trim, the window record
    def _report(self, key, s, trigger):
        pts = s['pts']
        n = len(pts)
        shape_used, ok, reports = self.match([(widen(p[0]), widen(p[1]), int(p[3]), float(np.float32(p[2])))
                                              for p in pts], key, trigger)
        if not ok or shape_used is None or shape_used <= 0:
            shape_used = None
        trim = shape_used if shape_used is not None and shape_used < n else n
        del pts[:trim]
        s['max_sep'] = np.float32(0.0)
        for p in pts[1:]:
            s['max_sep'] = np.float32(max(float(s['max_sep']), dist(p[0], p[1], pts[0][0], pts[0][1])))
        return {'key': key, 'trigger': trigger, 'n_points': n, 'shape_used': -1 if shape_used is None else shape_used,
                'status': 0 if ok else MATCH_ERROR, 'trimmed': trim, 'reports': list(reports) if ok else []}

    def process(self, key, lat, lon, accuracy, time, timestamp, trigger):
        """One point in arrival order; returns the window it triggered, or None."""
        p = (np.float32(lat), np.float32(lon), int(accuracy), int(time))
        s = self.sessions.get(key)
        if s is None:
            self.sessions[key] = {'pts': [p], 'max_sep': np.float32(0.0), 'last': int(timestamp)}
            return None
        pts = s['pts']
        s['max_sep'] = np.float32(max(float(s['max_sep']), dist(p[0], p[1], pts[0][0], pts[0][1])))
        pts.append(p)
        s['last'] = int(timestamp)
        n = len(pts)
        elapsed = pts[-1][3] - pts[0][3]
        report = not (s['max_sep'] < self.report_dist or n < self.report_count or elapsed < self.report_time)
        if not report and n == self.max_points:   # the cap: as at eviction, or cleared
            if elapsed >= 0:
                report = True
                self.n_forced += 1
            else:
                self.n_dropped += 1
                del self.sessions[key]
                return None
        if not report:
            return None
        w = self._report(key, s, trigger)
        if not pts:
            del self.sessions[key]
        return w

    def push(self, points):
        """points: dict of arrays (POINT_TYPES); the windows in ascending trigger order."""
        out = []
        for i in range(len(points['key'])):
            w = self.process(int(points['key'][i]), points['lat'][i], points['lon'][i], points['accuracy'][i],
                             points['time'][i], points['timestamp'][i], i)
            if w is not None:
                out.append(w)
        return out

    def punctuate(self, ts):
        """(windows in ascending key order, number of sessions deleted)."""
        out = []
        stale = sorted(k for k, s in self.sessions.items() if ts - s['last'] > self.session_gap)
        for rank, key in enumerate(stale):
            s = self.sessions.pop(key)
            pts = s['pts']
            if len(pts) >= 2 and pts[-1][3] - pts[0][3] >= 0:
                w = self._report(key, {'pts': list(pts), 'max_sep': s['max_sep']}, -1 - rank)
                w['trimmed'] = len(pts)
                out.append(w)
        return out, len(stale)

    def snapshot(self):
        keys = sorted(self.sessions)
        pts = [p for k in keys for p in self.sessions[k]['pts']]
        off = np.zeros(len(keys) + 1, np.int64)
        off[1:] = np.cumsum([len(self.sessions[k]['pts']) for k in keys])
        return {'key': np.array(keys, np.uint64), 'point_off': off,
                'max_sep': np.array([self.sessions[k]['max_sep'] for k in keys], np.float32),
                'last_update': np.array([self.sessions[k]['last'] for k in keys], np.int64),
                'lat': np.array([p[0] for p in pts], np.float32), 'lon': np.array([p[1] for p in pts], np.float32),
                'accuracy': np.array([p[2] for p in pts], np.int32), 'time': np.array([p[3] for p in pts], np.int64)}


def windows_to_arrays(windows):
    """A list of window records in the layout of _lib.session_result_to_numpy."""
    out = {k: np.array([w[k] for w in windows], dt) for k, dt in WINDOW_FIELDS}
    reps = [r for w in windows for r in w['reports']]
    off = np.zeros(len(windows) + 1, np.int64)
    off[1:] = np.cumsum([len(w['reports']) for w in windows])
    out['rep_off'] = off
    for j, (k, dt) in enumerate(REPORT_FIELDS):
        out[k] = np.array([r[j] for r in reps], dt)
    return out


def by_trigger(res):
    """A result's windows and reports reordered by ascending trigger (the forward order)."""
    order = np.argsort(np.asarray(res['trigger']), kind='stable')
    out = {k: np.asarray(res[k])[order] for k, _ in WINDOW_FIELDS}
    off = np.asarray(res['rep_off'])
    sel = np.concatenate([np.arange(off[w], off[w + 1]) for w in order] + [np.zeros(0, np.int64)]).astype(np.int64)
    out['rep_off'] = np.concatenate([[0], np.cumsum((off[1:] - off[:-1])[order])]).astype(np.int64)
    for k, _ in REPORT_FIELDS:
        out[k] = np.asarray(res[k])[sel]
    return out


def concat(results, bases):
    """Several pushes' results as one, triggers shifted by each chunk's first arrival index."""
    out = {k: np.concatenate([np.asarray(r[k]) + (b if k == 'trigger' else 0) for r, b in zip(results, bases)])
           .astype(dt) for k, dt in WINDOW_FIELDS}
    nrep = np.concatenate([np.diff(np.asarray(r['rep_off'])) for r in results] + [np.zeros(0, np.int64)])
    out['rep_off'] = np.concatenate([[0], np.cumsum(nrep)]).astype(np.int64)
    for k, dt in REPORT_FIELDS:
        out[k] = np.concatenate([np.asarray(r[k]) for r in results]).astype(dt)
    return out


def differing(got, want, fields):
    """The names of the arrays that differ bit for bit."""
    bad = []
    for k in fields:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
            bad.append('%s: got %s %s want %s %s' % (k, a.dtype, a.tolist()[:8], b.dtype, b.tolist()[:8]))
    return bad


RESULT_FIELDS = tuple(k for k, _ in WINDOW_FIELDS) + ('rep_off',) + tuple(k for k, _ in REPORT_FIELDS)


def take(points, lo, hi):
    return {k: np.asarray(points[k])[lo:hi] for k, _ in POINT_TYPES}


# ---- the scripted stream (no matcher): GPU job 1 and the CPU pins ---------------------------
SCRIPT = dict(max_sessions=16, max_points=16, report_dist=120.0, report_count=5, report_time=8, session_gap=5000)
SCRIPT_CHUNKS = 6


def scripted_match(points, key, trigger):
    """shape_used from a script that depends on (key, trigger, n) only, so it answers the same
    in the device store's round order as in arrival order: partial, absent, whole or error."""
    n = len(points)
    h = (int(key) * 2654435761 + (int(trigger) + 7) * 40503 + n * 97) & 0xFFFFFFFF
    h = ((h ^ (h >> 15)) * 2246822519) & 0xFFFFFFFF
    h ^= h >> 13
    kind = h % 8
    if kind == 0:
        return None, False, []
    if kind == 1:
        return None, True, []
    if kind == 2:
        return n, True, []
    return 1 + (h >> 4) % (n - 1), True, []


def script_key(i):
    return (i + 1) * 0x9E3779B97F4A7C15 % (1 << 64)


def scripted_chunk(p, seed=5):
    """Chunk p of the scripted stream: the 8 keys of group p (last seen long ago in stream time:
    stale at the punctuate that follows) and the 8 of group p + 1 (fresh: they go on in chunk
    p + 1), so 16 sessions live at a time and 24 keys in the table of 32 after two chunks.  0-40
    points per key interleaved in one chunk, walking north-east at 0-40 m per point; every fifth
    key stands still (it reaches the cap and is reported by force), every fifth has a clock that
    runs backwards (it reaches the cap and is cleared).  Returns (points, punctuate ts)."""
    rng = np.random.RandomState(seed * 1000 + p)
    base = p * 100000
    rows = []
    for g, stale in ((p, 1), (p + 1, 0)):
        for k in range(8):
            i = g * 8 + k
            count = {0: 40, 1: 0 if not stale else 3, 2: 1}.get(k, int(rng.randint(0, 41)))
            lat, lon = np.float32(52.0 + 0.01 * i + 0.001 * stale), np.float32(13.0 + 0.01 * i)
            still, back = i % 5 == 4, i % 5 == 3
            pos = np.sort(rng.uniform(0, 1, count))
            step = rng.uniform(0, 0.5 if still else 40, count) / KM
            for j in range(count):
                lat = np.float32(lat + np.float32(step[j]))
                lon = np.float32(lon + np.float32(step[j] * 1.3))
                tm = 1483228800 + base // 100 + (-3 * j if back else 3 * j + int(rng.randint(0, 3)))
                rows.append((pos[j], script_key(i), lat, lon, int(rng.randint(0, 30)), tm, stale))
    rows.sort(key=lambda r: r[0])
    n = len(rows)
    pts = {'key': np.array([r[1] for r in rows], np.uint64), 'lat': np.array([r[2] for r in rows], np.float32),
           'lon': np.array([r[3] for r in rows], np.float32), 'accuracy': np.array([r[4] for r in rows], np.int32),
           'time': np.array([r[5] for r in rows], np.int64),
           'timestamp': base + np.arange(n, dtype=np.int64) - 10000 * np.array([r[6] for r in rows], np.int64)}
    return pts, base + n + 100


# ---- the city stream (real matching): GPU job 2 and the coverage pin -----------------------
CITY = dict(max_sessions=32, max_points=128, report_dist=150.0, report_count=10, report_time=20, session_gap=60000)


def city_stream(graph_dir):
    """(graph path, points): the city batch narrowed to float32, key 1000 + trace, arrival order
    interleaved by time (stable), stream time in milliseconds; plus one key with a single point
    (its eviction does not report)."""
    from tests import matched_points_ref as mref
    path, tr = mref.city(graph_dir)
    key = np.repeat(np.arange(tr.n_traces, dtype=np.uint64) + 1000, np.diff(tr.offsets))
    tm = np.asarray(tr.time, np.int64)
    order = np.argsort(tm, kind='stable')
    pts = {'key': key[order], 'lat': np.asarray(tr.lat)[order].astype(np.float32),
           'lon': np.asarray(tr.lon)[order].astype(np.float32),
           'accuracy': (5 + np.arange(len(order)) % 7).astype(np.int32), 'time': tm[order]}
    pts['timestamp'] = pts['time'] * 1000
    for k, dt in POINT_TYPES:
        single = {'key': 7}.get(k, pts[k][0])
        pts[k] = np.concatenate([pts[k][:50], np.array([single], dt), pts[k][50:]]).astype(dt)
    return path, pts


def window_traces(points):
    """A window's points as a one-trace gen.Traces (mode auto)."""
    from reporter_amd.tools.gen import Traces
    return Traces(np.array([p[0] for p in points], np.float64), np.array([p[1] for p in points], np.float64),
                  np.array([p[2] for p in points], np.int64), np.array([0, len(points)], np.int64),
                  np.zeros(1, np.uint8), np.array([p[3] for p in points], np.float32))


def result_to_match(res, status=0):
    """(shape_used, ok, reports) of a one-trace match result dict."""
    su = int(res['shape_used'][0])
    reps = [(int(res['rep_id'][k]), int(res['rep_next'][k]), float(res['rep_t0'][k]), float(res['rep_t1'][k]),
             int(res['rep_length'][k]), int(res['rep_queue'][k])) for k in range(len(res['rep_id']))]
    return (su if su > 0 else None), status == 0, reps


def push_rounds(store, points):
    """The chunk consumed in rounds, as the device store does: every key with unconsumed points
    takes them one by one until it reports; yields each round's windows by ascending trigger.
    Keys are independent, so the end state is the one of Store.push."""
    per_key = {}
    for i, k in enumerate(np.asarray(points['key']).tolist()):
        per_key.setdefault(k, []).append(i)
    cursor = dict.fromkeys(per_key, 0)
    while True:
        wins = []
        for k, idx in per_key.items():
            while cursor[k] < len(idx):
                i = idx[cursor[k]]
                cursor[k] += 1
                w = store.process(k, points['lat'][i], points['lon'][i], points['accuracy'][i], points['time'][i],
                                  points['timestamp'][i], i)
                if w is not None:
                    wins.append(w)
                    break
        if not wins:
            return
        yield sorted(wins, key=lambda w: w['trigger'])


# ---- the small streams of GPU jobs 3 and 4 --------------------------------------------------
def _still(rows):
    """rows of (key, time, timestamp): points that all stand on one spot, accuracy 4."""
    n = len(rows)
    return {'key': np.array([r[0] for r in rows], np.uint64), 'lat': np.full(n, 52.5, np.float32),
            'lon': np.full(n, 13.4, np.float32), 'accuracy': np.full(n, 4, np.int32),
            'time': np.array([r[1] for r in rows], np.int64), 'timestamp': np.array([r[2] for r in rows], np.int64)}


# session_gap 60000, no gate ever passes.  At ts 100000: keys 2 (clock backwards), 3 (one point),
# 5 (elapsed 0) and 12 are stale, 5 and 12 report; 11 is exactly at the gap and stays, 9 is fresh.
PUNCTUATE_POINTS = _still([(5, 5, 900), (3, 1, 500), (9, 1, 80000), (11, 1, 30000), (2, 9, 600), (12, 1, 100),
                           (5, 5, 1000), (11, 2, 40000), (2, 4, 700), (12, 2, 200), (9, 2, 90000), (12, 3, 300)])
PUNCTUATE_TS = (100000, 100001, 10 ** 9)


def refusal_points(keys):
    """One point per listed key, in order, all on one spot, times 100, 101, ..."""
    return _still([(k, 100 + i, 1000 + i) for i, k in enumerate(keys)])
