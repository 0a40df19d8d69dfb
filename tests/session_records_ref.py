"""Restore, export and move of the session store restated over
tests/sessions_ref.py's Store: Batch.Serder's value bytes (Batch.java:110-116, Point.java:50-55)
with struct, the refusal rules of otr_sessions_restore, and the shard rule of otr_sessions_take.
A helper module (no tests, no fixtures): tests/test_session_restore_cpu.py pins what it computes,
tests/test_gpu_session_restore.py holds the device store equal to it."""
import struct

import numpy as np

from tests import sessions_ref as R

E_LAYOUT, E_KEY, E_COUNT, E_DUPLICATE, E_LIVE, E_FULL = 1, 2, 3, 4, 5, 6
HEADER, POINT = struct.Struct('>ifq'), struct.Struct('>ffiq')
assert (HEADER.size, POINT.size) == (16, 20)


def _f32(bits_of):
    """A float32 value as the Python float struct packs back to the same bits (NaNs aside: the
    streams here hold none)."""
    return float(np.float32(bits_of))


def encode(snapshot):
    """(key, rec_off, data): one record per session of a snapshot dict."""
    off = np.asarray(snapshot['point_off']).tolist()
    parts = []
    for i in range(len(snapshot['key'])):
        a, b = off[i], off[i + 1]
        rec = [HEADER.pack(b - a, _f32(snapshot['max_sep'][i]), int(snapshot['last_update'][i]))]
        for k in range(a, b):
            rec.append(POINT.pack(_f32(snapshot['lat'][k]), _f32(snapshot['lon'][k]), int(snapshot['accuracy'][k]),
                                  int(snapshot['time'][k])))
        parts.append(b''.join(rec))
    rec_off = np.zeros(len(parts) + 1, np.int64)
    rec_off[1:] = np.cumsum([len(p) for p in parts])
    return np.asarray(snapshot['key'], np.uint64).copy(), rec_off, b''.join(parts)


def record_layout_ok(rec_off, data, i):
    """The record's offsets lie in the data in order, it holds a header and is as long as its
    count says (Python ints: no width to overflow)."""
    a, b = int(rec_off[i]), int(rec_off[i + 1])
    if a < 0 or b < a or b > len(data) or b - a < HEADER.size:
        return False
    return HEADER.size + POINT.size * struct.unpack_from('>i', data, a)[0] == b - a


def decode_record(data, a):
    """(count, max_sep float32, last_update, [(lat float32, lon float32, accuracy, time)])."""
    n, ms, last = HEADER.unpack_from(data, a)
    pts = []
    for k in range(n):
        la, lo, ac, tm = POINT.unpack_from(data, a + HEADER.size + POINT.size * k)
        pts.append((np.float32(la), np.float32(lo), ac, tm))
    return n, np.float32(ms), last, pts


def decode(key, rec_off, data):
    """The snapshot dict of well-formed records (the inverse of encode)."""
    recs = [decode_record(data, int(rec_off[i])) for i in range(len(key))]
    pts = [p for r in recs for p in r[3]]
    off = np.zeros(len(recs) + 1, np.int64)
    off[1:] = np.cumsum([r[0] for r in recs])
    return {'key': np.asarray(key, np.uint64).copy(), 'point_off': off,
            'max_sep': np.array([r[1] for r in recs], np.float32), 'last_update': np.array([r[2] for r in recs], np.int64),
            'lat': np.array([p[0] for p in pts], np.float32), 'lon': np.array([p[1] for p in pts], np.float32),
            'accuracy': np.array([p[2] for p in pts], np.int32), 'time': np.array([p[3] for p in pts], np.int64)}


def _refusal(store, max_sessions, keys, layout_ok, counts):
    """(bad_session, bad_reason) of a restore: the lowest index with any per-session reason and
    the first of its reasons in the order layout, key, count, duplicate, live; full only when no
    session has one."""
    seen = set()
    for i, key in enumerate(keys):
        reasons = []
        if not layout_ok[i]:
            reasons.append(E_LAYOUT)
        if key == R.NO_ID:
            reasons.append(E_KEY)
        if layout_ok[i] and not 1 <= counts[i] <= store.max_points - 1:
            reasons.append(E_COUNT)
        if key in seen:
            reasons.append(E_DUPLICATE)
        if key in store.sessions:
            reasons.append(E_LIVE)
        seen.add(key)
        if reasons:
            return i, min(reasons)
    if max_sessions is not None and len(store.sessions) + len(keys) > max_sessions:
        return -1, E_FULL
    return -1, 0


def _merge(store, keys, sessions):
    for key, (ms, last, pts) in zip(keys, sessions):
        store.sessions[key] = {'pts': list(pts), 'max_sep': np.float32(ms), 'last': int(last)}


def restore(store, snapshot, max_sessions=None):
    """otr_sessions_restore on an R.Store: merges the snapshot's sessions (max_sep and last_update
    as stored) or, refused, leaves the store as it is (max_sessions None: never full).  Returns
    (bad_session, bad_reason)."""
    keys = [int(k) for k in snapshot['key']]
    off = [int(o) for o in snapshot['point_off']]
    n, npt = len(keys), len(snapshot['time'])
    if n == 0:
        return (-1, 0) if npt == 0 else (-1, E_LAYOUT)
    layout_ok = [not (off[i + 1] < off[i] or (i == 0 and off[0] != 0) or (i == n - 1 and off[n] != npt))
                 for i in range(n)]
    counts = [off[i + 1] - off[i] for i in range(n)]
    bad = _refusal(store, max_sessions, keys, layout_ok, counts)
    if bad[1]:
        return bad
    _merge(store, keys, [(snapshot['max_sep'][i], snapshot['last_update'][i],
                          [(np.float32(snapshot['lat'][k]), np.float32(snapshot['lon'][k]), int(snapshot['accuracy'][k]),
                            int(snapshot['time'][k])) for k in range(off[i], off[i + 1])]) for i in range(n)])
    return bad


def restore_records(store, key, rec_off, data, max_sessions=None):
    """otr_sessions_restore_records on an R.Store; returns (bad_session, bad_reason)."""
    keys = [int(k) for k in key]
    layout_ok = [record_layout_ok(rec_off, data, i) for i in range(len(keys))]
    counts = [struct.unpack_from('>i', data, int(rec_off[i]))[0] if layout_ok[i] else 0 for i in range(len(keys))]
    bad = _refusal(store, max_sessions, keys, layout_ok, counts)
    if bad[1]:
        return bad
    recs = [decode_record(data, int(rec_off[i])) for i in range(len(keys))]
    _merge(store, keys, [(r[1], r[2], r[3]) for r in recs])
    return bad


def take(store, n_parts, part, remove):
    """otr_sessions_take: the snapshot of the sessions with key % n_parts == part; remove deletes
    them without a report."""
    keys = [k for k in store.sessions if k % n_parts == part]
    sub = R.Store(store.match, store.max_points)
    sub.sessions = {k: store.sessions[k] for k in keys}
    snap = sub.snapshot()
    if remove:
        for k in keys:
            del store.sessions[k]
    return snap


def scripted_cuts():
    """The restatement run over the scripted stream: for every chunk p the snapshot after its
    push ('push', p) and after its punctuate ('punctuate', p), in stream order."""
    ref = R.Store(R.scripted_match, **{k: v for k, v in R.SCRIPT.items() if k != 'max_sessions'})
    cuts = []
    for p in range(R.SCRIPT_CHUNKS):
        pts, ts = R.scripted_chunk(p)
        ref.push(pts)
        cuts.append((('push', p), ref.snapshot()))
        ref.punctuate(ts)
        cuts.append((('punctuate', p), ref.snapshot()))
    return cuts


# ---- the refusal cases of the CPU pins and of the GPU job --------------------------------------
def small_store(keys=(), max_points=4):
    """A store whose gates never pass, holding one point per listed key."""
    st = R.Store(lambda points, key, trigger: (None, True, []), max_points, 1e9, 99, 0, 60000)
    for k in keys:
        st.sessions[k] = {'pts': [(np.float32(1), np.float32(2), 3, 4)], 'max_sep': np.float32(0), 'last': 5}
    return st


def still_snapshot(keys, counts, off=None):
    """A snapshot dict of sessions standing on one spot (point_off from counts, or as given)."""
    n = sum(counts)
    o = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64) if off is None else np.asarray(off, np.int64)
    return {'key': np.array(keys, np.uint64), 'point_off': o, 'max_sep': np.arange(len(keys), dtype=np.float32),
            'last_update': np.arange(len(keys), dtype=np.int64) + 100, 'lat': np.full(n, 52.5, np.float32),
            'lon': np.full(n, 13.4, np.float32), 'accuracy': np.arange(n, dtype=np.int32),
            'time': np.arange(n, dtype=np.int64) + 1000}


# name -> (live keys, snapshot, max_sessions, (bad_session, bad_reason)); max_points is 4
REFUSALS = {
    'layout_first_offset': ((), still_snapshot([1, 2], [1, 1], off=[1, 1, 2]), 4, (0, E_LAYOUT)),
    'layout_decreasing': ((), still_snapshot([1, 2, 3], [1, 1, 1], off=[0, 2, 1, 3]), 4, (1, E_LAYOUT)),
    'layout_last_offset': ((), still_snapshot([1, 2], [1, 1], off=[0, 1, 3]), 4, (1, E_LAYOUT)),
    'key': ((), still_snapshot([1, R.NO_ID], [1, 1]), 4, (1, E_KEY)),
    'count_zero': ((), still_snapshot([1, 2], [1, 0]), 4, (1, E_COUNT)),
    'count_cap': ((), still_snapshot([1, 2], [4, 3]), 4, (0, E_COUNT)),
    'duplicate': ((), still_snapshot([1, 2, 1], [1, 1, 1]), 4, (2, E_DUPLICATE)),
    'three_of_a_kind': ((), still_snapshot([5, 6, 5, 5], [1, 1, 1, 1]), 4, (2, E_DUPLICATE)),
    'live': ((2,), still_snapshot([1, 2], [1, 1]), 4, (1, E_LIVE)),
    'full': ((8, 9), still_snapshot([1, 2, 3], [1, 1, 1]), 4, (-1, E_FULL)),
    # two reasons on one session: the first in the order wins
    'key_and_count': ((), still_snapshot([R.NO_ID], [0]), 4, (0, E_KEY)),
    'duplicate_and_live': ((1,), still_snapshot([2, 1, 1], [1, 1, 1]), 4, (1, E_LIVE)),
    # two sessions compete: the lowest index wins whatever its reason
    'lowest_index': ((3,), still_snapshot([3, 1, 1, 2], [1, 1, 1, 0]), 4, (0, E_LIVE)),
    'count_before_duplicate': ((), still_snapshot([1, 1], [3, 4]), 4, (1, E_COUNT)),
    # a per-session reason beats full
    'reason_beats_full': ((8, 9, 10), still_snapshot([1, 1], [1, 1]), 4, (1, E_DUPLICATE)),
}


def record_layout_cases():
    """name -> (key, rec_off, data, (bad_session, E_LAYOUT)): three good records (1, 2 and 3 points)
    with one malformed: truncated, count -1, count 2^31 - 1, a count whose 16 + 20 * count is the
    record's real length in 32 bits, an offset past the end."""
    key, rec_off, data = encode(still_snapshot([1, 2, 3], [1, 2, 3]))
    cases = {'truncated': (key, rec_off.copy(), data[:-1], (2, E_LAYOUT))}
    for name, count in (('minus_one', -1), ('int_max', 2 ** 31 - 1), ('wraps', 2 ** 30 + 2)):
        d = bytearray(data)
        d[int(rec_off[1]):int(rec_off[1]) + 4] = struct.pack('>i', count)
        cases[name] = (key, rec_off.copy(), bytes(d), (1, E_LAYOUT))
    assert (16 + 20 * (2 ** 30 + 2)) % 2 ** 32 == 56 == int(rec_off[2] - rec_off[1])
    past = rec_off.copy()
    past[-1] += 20
    cases['offset_past_end'] = (key, past, data, (2, E_LAYOUT))
    return cases


# live + given == max_sessions: restored beside one live key of a 4-session store
BRIM = still_snapshot([3, 1, 2], [3, 1, 2])

# ---- the 4 x 4 store of the GPU jobs (gates that never pass: only the cap reports) --------------
# keys 1 (two points) and 2 go quiet and are evicted at DEAD_TS, key 3 stays; key 1 comes back
# beside the new key 7, and the second chunk takes both to the cap
DEAD_FIRST = R._still([(1, 100, 1000), (2, 101, 1000), (3, 102, 5000), (1, 103, 1001)])
DEAD_TS = 2500
DEAD_RESTORE = still_snapshot([1, 7], [2, 1])
DEAD_SECOND = R._still([(1, 2000, 6000), (7, 2001, 6000), (1, 2002, 6001), (7, 2003, 6002), (7, 2004, 6003)])
DEAD_THIRD = R._still([(3, 3000, 7000), (1, 3001, 7001), (7, 3002, 7002), (2, 3003, 7003), (3, 3004, 7004)])

# a session of max_points - 1 points (times 1000 .. 1002) and the point that takes it to the cap
CAP_SESSION = still_snapshot([5], [3])


def cap_point(time):
    return R._still([(5, time, 7000)])
