"""The session store's uuid directory restated over
tests/sessions_ref.py's Store: one name per live key, the refusal rules of a named chunk (the
lowest arrival index with any reason, there the lowest reason) and of a named restore, evictions
in name order, and the names of a snapshot, take and export.  A helper module (no tests, no
fixtures): tests/test_session_names_cpu.py pins what it computes, tests/test_gpu_session_names.py
holds the device store equal to it.

Names travel as the device takes them: (data, off, len, n_bytes) with name i = data[off[i] ..
off[i] + len[i]); raw(list of bytes) packs a list end to end."""
import functools

import numpy as np

from tests import session_records_ref as S
from tests import sessions_ref as R

E_LONG, E_COLLISION, E_LAYOUT = 1, 2, 3
E_NAME = 7


def raw(names):
    names = [bytes(x) for x in names]
    ln = [len(x) for x in names]
    off = [sum(ln[:i]) for i in range(len(names))]
    data = b''.join(names)
    return {'bytes': np.frombuffer(data, np.uint8).copy(), 'off': np.array(off, np.int64),
            'len': np.array(ln, np.int32), 'n_bytes': len(data)}


def own_reasons(off, ln, n_bytes, uuid_bytes):
    """The reasons a name has by itself (Python ints: nothing wraps)."""
    out = []
    if off < 0 or ln < 0 or off + ln > n_bytes:
        out.append(E_LAYOUT)
    if ln > uuid_bytes:
        out.append(E_LONG)
    return out


def name_at(names, i):
    off, ln = int(names['off'][i]), int(names['len'][i])
    return bytes(np.asarray(names['bytes'], np.uint8)[off:off + ln].tobytes())


def point_reason(names, i, uuid_bytes, stored=None, first=None):
    """The lowest reason of name i, 0 when it has none: its own faults; else, when its key is live,
    a stored name that differs; else, when its key is new in the chunk and point `first` was its
    first arrival, that point's name (if well formed) differing."""
    n_bytes = int(names['n_bytes'])
    reasons = own_reasons(int(names['off'][i]), int(names['len'][i]), n_bytes, uuid_bytes)
    if not reasons:
        if stored is not None:
            if name_at(names, i) != stored:
                reasons.append(E_COLLISION)
        elif first is not None and not own_reasons(int(names['off'][first]), int(names['len'][first]), n_bytes,
                                                   uuid_bytes) and name_at(names, first) != name_at(names, i):
            reasons.append(E_COLLISION)
    return min(reasons) if reasons else 0


def compare(a, b):
    """Unsigned bytes position by position; a proper prefix comes first."""
    for x, y in zip(a, b):
        if x != y:
            return -1 if x < y else 1
    return (len(a) > len(b)) - (len(a) < len(b))


def name_order(items):
    """(name, key) pairs in eviction order: ascending name, ties by key."""
    return sorted(items, key=functools.cmp_to_key(lambda p, q: compare(p[0], q[0]) or (p[1] > q[1]) - (p[1] < q[1])))


def sort_words(name, uuid_bytes):
    """The device's sort words of a name's zero-filled row: big-endian 64-bit words."""
    row = name + b'\0' * (8 * ((uuid_bytes + 7) // 8) - len(name))
    return [int.from_bytes(row[8 * w:8 * w + 8], 'big') for w in range((uuid_bytes + 7) // 8)]


class Store(R.Store):
    def __init__(self, match, max_points, uuid_bytes, **kw):
        super().__init__(match, max_points, **kw)
        self.uuid_bytes = uuid_bytes
        self.names = {}      # key -> bytes, of the live sessions
        self._pending = {}

    def refusal(self, keys, names):
        """(point, reason) of a named chunk against the store as it is, (-1, 0) when accepted.  A
        name with a fault of its own is compared with nothing; a key that is new in the chunk is
        held to the name of its first arrival (when that one is well formed)."""
        first = {}
        for i, key in enumerate(int(k) for k in keys):
            why = point_reason(names, i, self.uuid_bytes, self.names.get(key) if key in self.sessions else None,
                               first.get(key))
            if key not in self.sessions:
                first.setdefault(key, i)
            if why:
                return i, why
        return -1, 0

    def begin(self, keys, names):
        """A named chunk arrives: its refusal, or (-1, 0) with the names of its new keys noted for
        sync() after the chunk's points went through process / push / push_rounds."""
        bad = self.refusal(keys, names)
        if bad[1] == 0:
            for i, key in enumerate(int(k) for k in keys):
                if key not in self.sessions and key not in self._pending:
                    self._pending[key] = name_at(names, i)
        return bad

    def sync(self):
        """After a chunk, a punctuate or a take: a name per live session, none for the others."""
        for k in self.sessions:
            if k not in self.names:
                self.names[k] = self._pending[k]
        for k in list(self.names):
            if k not in self.sessions:
                del self.names[k]
        self._pending = {}

    def push_named(self, points, names):
        bad = self.begin(points['key'], names)
        if bad[1]:
            return bad, []
        wins = self.push(points)
        self.sync()
        return bad, wins

    def punctuate(self, ts):
        """(windows in ascending name order, number of sessions deleted)."""
        out = []
        stale = name_order([(self.names[k], k) for k, s in self.sessions.items() if ts - s['last'] > self.session_gap])
        for rank, (_, key) in enumerate(stale):
            s = self.sessions.pop(key)
            pts = s['pts']
            if len(pts) >= 2 and pts[-1][3] - pts[0][3] >= 0:
                w = self._report(key, {'pts': list(pts), 'max_sep': s['max_sep']}, -1 - rank)
                w['trimmed'] = len(pts)
                out.append(w)
        self.sync()
        return out, len(stale)

    def snapshot_names(self):
        return [self.names[k] for k in sorted(self.sessions)]


def take(store, n_parts, part, remove):
    """(snapshot, names) of otr_sessions_take on a named store."""
    names = [store.names[k] for k in sorted(store.sessions) if k % n_parts == part]
    snap = S.take(store, n_parts, part, remove)
    store.sync()
    return snap, names


def _restore_refusal(store, max_sessions, keys, layout_ok, counts, names):
    """session_records_ref._refusal with the name's reason, last in the order."""
    seen = set()
    n_bytes = int(names['n_bytes'])
    for i, key in enumerate(keys):
        reasons = []
        if not layout_ok[i]:
            reasons.append(S.E_LAYOUT)
        if key == R.NO_ID:
            reasons.append(S.E_KEY)
        if layout_ok[i] and not 1 <= counts[i] <= store.max_points - 1:
            reasons.append(S.E_COUNT)
        if key in seen:
            reasons.append(S.E_DUPLICATE)
        if key in store.sessions:
            reasons.append(S.E_LIVE)
        if own_reasons(int(names['off'][i]), int(names['len'][i]), n_bytes, store.uuid_bytes):
            reasons.append(E_NAME)
        seen.add(key)
        if reasons:
            return i, min(reasons)
    if max_sessions is not None and len(store.sessions) + len(keys) > max_sessions:
        return -1, S.E_FULL
    return -1, 0


def restore_named(store, snapshot, names, max_sessions=None):
    """otr_sessions_restore_named on a Store: (bad_session, bad_reason); names stored as given."""
    keys = [int(k) for k in snapshot['key']]
    off = [int(o) for o in snapshot['point_off']]
    n, npt = len(keys), len(snapshot['time'])
    if n == 0:
        return (-1, 0) if npt == 0 else (-1, S.E_LAYOUT)
    layout_ok = [not (off[i + 1] < off[i] or (i == 0 and off[0] != 0) or (i == n - 1 and off[n] != npt))
                 for i in range(n)]
    counts = [off[i + 1] - off[i] for i in range(n)]
    bad = _restore_refusal(store, max_sessions, keys, layout_ok, counts, names)
    if bad[1]:
        return bad
    assert S.restore(store, snapshot, max_sessions) == (-1, 0)
    for i, k in enumerate(keys):
        store.names[k] = name_at(names, i)
    return bad


# ---- the streams of the CPU pins and of the GPU jobs --------------------------------------------
UUID_BYTES = 24


def script_name(key):
    return b'veh-%d' % int(key)


def names_for(keys, name=script_name):
    return raw([name(k) for k in keys])


def small_store(names_by_key, uuid_bytes=UUID_BYTES, max_points=4):
    """A named store whose gates never pass, holding one point per key."""
    st = Store(lambda points, key, trigger: (None, True, []), max_points, uuid_bytes, report_dist=1e9,
               report_count=99, report_time=0, session_gap=60000)
    for k, nm in names_by_key.items():
        st.sessions[k] = {'pts': [(np.float32(52.5), np.float32(13.4), 4, 100)], 'max_sep': np.float32(0), 'last': 1000}
        st.names[k] = nm
    return st


def _shifted(names, **change):
    out = dict(names)
    for k, (i, v) in change.items():
        a = np.array(out[k]).copy()
        a[i] = v
        out[k] = a
    return out


STORED = {5: b'veh-000000000000000five1', 6: b'veh-6'}   # key 5's name has exactly UUID_BYTES bytes
assert len(STORED[5]) == UUID_BYTES


def refusal_cases():
    """name -> (keys of the chunk, names, (point, reason)) against a store holding STORED (keys 5
    and 6) in 8 sessions; every chunk also brings new keys, so a refusal has entries to roll back."""
    five = STORED[5]
    cases = {
        'last_byte': ([9, 5, 10], raw([b'veh-9', five[:-1] + b'2', b'veh-10']), (1, E_COLLISION)),
        'prefix_of_stored': ([9, 5], raw([b'veh-9', five[:-1]]), (1, E_COLLISION)),
        'longer_than_stored': ([9, 6, 10], raw([b'veh-9', b'veh-6x', b'veh-10']), (1, E_COLLISION)),
        # key 9 is new: its points 0 and 2 agree, point 3 is the first that differs
        'within_chunk': ([9, 10, 9, 9, 9], raw([b'veh-9', b'veh-10', b'veh-9', b'veh-9b', b'veh-9']), (3, E_COLLISION)),
        'two_faults': ([9, 6, 5, 10], raw([b'veh-9', b'veh-7', b'x' * (UUID_BYTES + 1), b'veh-10']), (1, E_COLLISION)),
        'long_and_collision': ([9, 5], raw([b'veh-9', five + b'!']), (1, E_LONG)),
        'one_too_long': ([9, 10], raw([b'veh-9', b'y' * (UUID_BYTES + 1)]), (1, E_LONG)),
    }
    ok = raw([b'veh-9', b'veh-10', b'veh-6'])
    keys = [9, 10, 6]
    cases['layout_negative_off'] = (keys, _shifted(ok, off=(1, -1)), (1, E_LAYOUT))
    cases['layout_negative_len'] = (keys, _shifted(ok, len=(0, -1)), (0, E_LAYOUT))
    cases['layout_past_end'] = (keys, _shifted(ok, len=(2, 6)), (2, E_LAYOUT))
    cases['layout_off_past_end'] = (keys, _shifted(ok, off=(2, 2 ** 40)), (2, E_LAYOUT))
    cases['layout_huge_off'] = (keys, _shifted(ok, off=(1, 2 ** 63 - 1)), (1, E_LAYOUT))
    return cases


# accepted after every refusal: keys 9 and 10 are new (had the refused chunk's claims not been
# rolled back they would be met in the table), 5 comes under its stored name of UUID_BYTES bytes
THEN_KEYS = [10, 5, 9, 10]
THEN_NAMES = raw([b'veh-10', STORED[5], b'veh-9', b'veh-10'])

# eviction order: the key order is the reverse of the name order; a prefix pair, a pair that
# first differs at byte 9 and one at byte UUID_BYTES (the last byte of the third sort word)
EVICT_NAMES = [b'a', b'ab', b'veh-0000A', b'veh-0000B', b'veh-0000B' + b'0' * 14 + b'1', b'veh-0000B' + b'0' * 14 + b'2',
               b'\x80high', b'\xffhigher']
assert max(len(x) for x in EVICT_NAMES) == UUID_BYTES
EVICT_KEYS = [100 - i for i in range(len(EVICT_NAMES))]
