"""The tile store's snapshot, restore and Segment.ListSerder records
restated in plain Python over struct.pack('>...'): what AnonymisingProcessor keeps in its two
state stores (AnonymisingProcessor.java:47-59, 119-152), written out and read back.  A helper
module (no tests, no fixtures) that imports tests/tile_store_ref.py and does not change it:
tests/test_tile_records_cpu.py pins what it computes, tests/test_gpu_tile_records.py holds the
device code equal to it.

A "held" state is (rows, t0, t1): numpy TILE_ROW rows in arrival order with the two times of the
report each row came from.  "records" is the dict of Matcher.tile_store_export_records: start,
tile_id, rec_off, name_off (int64), slice (int32), bytes, names, map_bytes (uint8), n_slices,
n_tiles, n_bytes, n_name_bytes, slice_size."""
import math
import struct

import numpy as np

from oracle import tiles as T
from tests import tile_store_ref as TS

E_LAYOUT, E_KEY, E_COUNT, E_SEGMENT, E_DUPLICATE, E_MAP, E_FULL, E_ROW = range(1, 9)
INVALID = T.INVALID_SEGMENT_ID
SLICE_SIZE = 20000                      # AnonymisingProcessor.java:45
SEGMENT = struct.Struct('>qqddii')      # Segment.Serder.put, Segment.java:82-89
MAP_ENTRY = struct.Struct('>qqi')       # TimeQuantisedTile.Serder's key, Kafka's integer value
RECORD_ARRAYS = ('start', 'tile_id', 'slice', 'rec_off', 'bytes', 'names', 'name_off', 'map_bytes')
RECORD_TYPES = dict(start=np.int64, tile_id=np.int64, slice=np.int32, rec_off=np.int64, bytes=np.uint8,
                    names=np.uint8, name_off=np.int64, map_bytes=np.uint8)


class Refused(ValueError):
    def __init__(self, reason, bad_slice=-1, bad_tile=-1):
        ValueError.__init__(self, 'refused: reason %d slice %d tile %d' % (reason, bad_slice, bad_tile))
        self.reason, self.bad_slice, self.bad_tile = reason, bad_slice, bad_tile


def _i64(u):
    u = int(u)
    return u - (1 << 64) if u >= 1 << 63 else u


def row_of(bucket, sid, nx, t0, t1, ln, qu):
    """The row an add derives for `bucket` from one report (oracle.tiles.stream_rows_from_reports)."""
    nx = INVALID if nx == T.NO_ID else nx
    f = (bucket << 25) | ((sid & 7) << 22) | ((sid >> 3) & 0x3FFFFF)
    return (f, sid, nx, int(math.floor(t0)), int(math.ceil(t1)), T._java_round(t1 - t0), ln, qu,
            T.speed_bin(ln, t0, t1))


def times_of(reports, q):
    """(t0, t1) per row of TS.rows_of(reports, q): a report that spans several buckets gives each
    of its rows the same pair."""
    a, b = [], []
    for k in range(len(reports['id'])):
        t0, t1 = float(reports['t0'][k]), float(reports['t1'][k])
        if TS.valid(t0, t1, int(reports['length'][k]), int(reports['queue_length'][k])):
            nb = int(t1) // q - int(t0) // q + 1
            a += [t0] * nb
            b += [t1] * nb
    return np.array(a, np.float64), np.array(b, np.float64)


def held_of(adds, q):
    """The held state after the given adds of reports."""
    rows = [TS.rows_of(a, q) for a in adds]
    tt = [times_of(a, q) for a in adds]
    held = (np.concatenate(rows + [np.zeros(0, T.TILE_ROW)]), np.concatenate([t[0] for t in tt] + [np.zeros(0)]),
            np.concatenate([t[1] for t in tt] + [np.zeros(0)]))
    assert len(held[0]) == len(held[1]) == len(held[2])
    return held


def empty_held():
    return np.zeros(0, T.TILE_ROW), np.zeros(0, np.float64), np.zeros(0, np.float64)


def concat(a, b):
    return tuple(np.concatenate([x, y]) for x, y in zip(a, b))


def slice_key(start, tile_id, slice_):
    """Long.toString(start) "_" Long.toString(tile_id) "." slice (AnonymisingProcessor.java:131)."""
    return ('%d_%d.%d' % (start, tile_id, slice_)).encode()


def tile_id_of(file):
    return ((file >> 22) & 7) | ((file & 0x3FFFFF) << 3)


def file_of(start, tile_id, q):
    return ((start // q) << 25) | ((tile_id & 7) << 22) | ((tile_id >> 3) & 0x3FFFFF)


def encode_slice(segments):
    """Segment.ListSerder's serialiser (Segment.java:142-150) over (id, next_id, min, max, length,
    queue) tuples; ids as unsigned."""
    return struct.pack('>i', len(segments)) + b''.join(
        SEGMENT.pack(_i64(s[0]), _i64(s[1]), s[2], s[3], s[4], s[5]) for s in segments)


def records_of(slices, slice_size, map_entries=None):
    """A records dict from [(start, tile_id, slice, value bytes)] and [(start, tile_id, value)]."""
    off = np.concatenate([[0], np.cumsum([len(s[3]) for s in slices])]).astype(np.int64)
    names = [slice_key(*s[:3]) for s in slices]
    rec = {'start': np.array([s[0] for s in slices], np.int64), 'tile_id': np.array([s[1] for s in slices], np.int64),
           'slice': np.array([s[2] for s in slices], np.int32), 'rec_off': off,
           'bytes': np.frombuffer(b''.join(s[3] for s in slices), np.uint8),
           'names': np.frombuffer(b''.join(names), np.uint8),
           'name_off': np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.int64),
           'map_bytes': None if map_entries is None else np.frombuffer(
               b''.join(MAP_ENTRY.pack(*e) for e in map_entries), np.uint8),
           'n_slices': len(slices), 'n_tiles': -1 if map_entries is None else len(map_entries),
           'slice_size': slice_size}
    rec['n_bytes'], rec['n_name_bytes'] = len(rec['bytes']), len(rec['names'])
    return rec


def export(held, q, slice_size):
    """otr_tile_store_export_records: per file in `file` order, its rows in arrival order cut
    into slices of slice_size, and one map entry with value n // slice_size."""
    rows, t0, t1 = held
    S = int(slice_size)
    slices, entries = [], []
    files = rows['file'].tolist()
    for f in sorted(set(files)):
        idx = [i for i, x in enumerate(files) if x == f]
        start, tid = (f >> 25) * q, tile_id_of(f)
        for s in range((len(idx) + S - 1) // S):
            segs = [(int(rows['id'][i]), int(rows['next_id'][i]), float(t0[i]), float(t1[i]), int(rows['length'][i]),
                     int(rows['queue_length'][i])) for i in idx[s * S:(s + 1) * S]]
            slices.append((start, tid, s, encode_slice(segs)))
        entries.append((start, tid, len(idx) // S))
    return records_of(slices, S, entries)


def records_differing(got, want):
    bad = []
    for k in RECORD_ARRAYS:
        a, b = np.ascontiguousarray(got[k], RECORD_TYPES[k]), np.ascontiguousarray(want[k], RECORD_TYPES[k])
        if a.shape != b.shape or a.tobytes() != b.tobytes():
            bad.append('%s: got %s %s want %s %s' % (k, a.shape, a.tolist()[:6], b.shape, b.tolist()[:6]))
    for k in ('n_slices', 'n_tiles', 'n_bytes', 'n_name_bytes', 'slice_size'):
        if int(got[k]) != int(want[k]):
            bad.append('%s: got %d want %d' % (k, got[k], want[k]))
    return bad


def key_ok(start, tile_id, slice_, q):
    return start >= 0 and start % q == 0 and start // q < 1 << 39 and 0 <= tile_id <= 0x1FFFFFF and slice_ >= 0


def decode_slice(data, b, e):
    """(count, segments) of record [b, e) of data, or None where its layout is refused; ids unsigned."""
    if b < 0 or e < b or e > len(data) or e - b < 4:
        return None
    count = struct.unpack_from('>i', data, b)[0]
    if 4 + 40 * count != e - b:
        return None
    segs = []
    for k in range(count):
        i, n, t0, t1, ln, qu = SEGMENT.unpack_from(data, b + 4 + 40 * k)
        segs.append((i & 0xFFFFFFFFFFFFFFFF, n & 0xFFFFFFFFFFFFFFFF, t0, t1, ln, qu))
    return count, segs


def segment_ok(seg, tile_id, bucket, q):
    sid, _, t0, t1, ln, qu = seg
    if not TS.valid(t0, t1, ln, qu) or t1 >= 2.0 ** 62 or (sid & 0x1FFFFFF) != tile_id:
        return False
    return int(t0) // q <= bucket <= int(t1) // q


def record_reason(rec, i, q):
    """The lowest per-record reason of record i but E_DUPLICATE, 0 for none, and its segments."""
    data = bytes(np.ascontiguousarray(rec['bytes'], np.uint8))
    d = decode_slice(data, int(rec['rec_off'][i]), int(rec['rec_off'][i + 1]))
    start, tid, sl = int(rec['start'][i]), int(rec['tile_id'][i]), int(rec['slice'][i])
    if d is None:
        return E_LAYOUT, None
    if not key_ok(start, tid, sl, q):
        return E_KEY, None
    if d[0] < 1 or d[0] > rec['slice_size']:
        return E_COUNT, None
    if not all(segment_ok(s, tid, start // q, q) for s in d[1]):
        return E_SEGMENT, None
    return 0, d[1]


def restore_records(held, rec, q, max_rows, use_map=True):
    """otr_tile_store_restore_records: (the new held state, the result's counts), or Refused."""
    n = int(rec['n_slices'])
    segs, seen = {}, set()
    for i in range(n):
        reason, s = record_reason(rec, i, q)
        k = (int(rec['start'][i]), int(rec['tile_id'][i]), int(rec['slice'][i]))
        if reason not in (E_LAYOUT, E_KEY):
            if k in seen:
                reason = min(reason, E_DUPLICATE) if reason else E_DUPLICATE
            seen.add(k)
        if reason:
            raise Refused(reason, bad_slice=i)
        segs[i] = s
    named = None
    if use_map and rec.get('map_bytes') is not None:
        mb = bytes(np.ascontiguousarray(rec['map_bytes'], np.uint8))
        named = {}
        for t in range(len(mb) // 20):
            start, tid, v = MAP_ENTRY.unpack_from(mb, 20 * t)
            if not key_ok(start, tid, 0, q) or v < 0 or (start, tid) in named:
                raise Refused(E_MAP, bad_tile=t)
            named[(start, tid)] = v
    order = sorted(range(n), key=lambda i: (file_of(int(rec['start'][i]), int(rec['tile_id'][i]), q),
                                            int(rec['slice'][i])))
    out = {'n_slices': 0, 'n_rows': 0, 'n_unreferenced_slices': 0, 'n_unreferenced_rows': 0, 'n_missing_slices': 0}
    rows, t0, t1 = [], [], []
    for i in order:
        start, tid, sl = int(rec['start'][i]), int(rec['tile_id'][i]), int(rec['slice'][i])
        if named is not None and not ((start, tid) in named and sl <= named[(start, tid)]):
            out['n_unreferenced_slices'] += 1
            out['n_unreferenced_rows'] += len(segs[i])
            continue
        out['n_slices'] += 1
        for s in segs[i]:
            rows.append(row_of(start // q, *s))
            t0.append(s[2])
            t1.append(s[3])
    out['n_rows'] = len(rows)
    if named is not None:
        out['n_missing_slices'] = sum(v + 1 for v in named.values()) - out['n_slices']
    if len(held[0]) + len(rows) > max_rows:
        raise Refused(E_FULL)
    new = concat(held, (np.array(rows, T.TILE_ROW) if rows else np.zeros(0, T.TILE_ROW), np.array(t0, np.float64),
                        np.array(t1, np.float64)))
    out['n_rows_held'] = len(new[0])
    return new, out


def restore_rows(held, snap, q, max_rows, timed=True):
    """otr_tile_store_restore: the snapshot's rows appended, or Refused(E_ROW, lowest row)."""
    rows, t0, t1 = snap
    if timed:
        for i in range(len(rows)):
            r = rows[i]
            a, b, ln, qu = float(t0[i]), float(t1[i]), int(r['length']), int(r['queue_length'])
            bucket = int(r['file']) >> 25
            ok = TS.valid(a, b, ln, qu) and b < 2.0 ** 62 and int(a) // q <= bucket <= int(b) // q
            if ok:
                w = np.array([row_of(bucket, int(r['id']), int(r['next_id']), a, b, ln, qu)], T.TILE_ROW)
                ok = w.tobytes() == np.array([r], T.TILE_ROW).tobytes()
            if not ok:
                raise Refused(E_ROW, bad_slice=i)
    if len(held[0]) + len(rows) > max_rows:
        raise Refused(E_FULL)
    return concat(held, snap)


def flush_of(held, q, privacy):
    """The flush of a held state through tests/tile_store_ref.py's Store."""
    st = TS.Store(1 << 30, q, privacy)
    st.add_rows(held[0])
    return st.flush()


# ---- the hand-built cases ------------------------------------------------------------------
Q = TS.SCRIPT_Q
T0 = TS.T0


def case_reports(S):
    """One add of reports covering: files whose rows interleave in arrival order; a report that
    spans three buckets (one row in each of three files, the same times); a next_id of none; a
    .5 tie of Math.round; a t0 within an ulp below a bucket boundary; files of 1, S - 1, S, S + 1
    and 2 S rows (tiles 201 .. 205, each report inside one bucket)."""
    A, B = (1, 300), (0, 300)
    w = []
    for k in range(6):                                   # A and B take turns
        tl = A if k % 2 == 0 else B
        w.append((TS.sid(*tl, k), TS.sid(*tl, k + 1), T0 + 1 + k, T0 + 3.25 + k, 50 + k, k % 2))
    w.append((TS.sid(2, 310, 1), TS.sid(2, 310, 2), T0 + 55.0, T0 + 175.5, 900, 0))      # buckets 0, 1, 2
    w.append((TS.sid(2, 311, 1), TS.NO_ID, T0 + 5.0, T0 + 7.5, 30, 1))                   # none; 2.5 rounds up
    w.append((TS.sid(2, 312, 1), TS.sid(2, 312, 2), np.nextafter(T0 + 60.0, 0.0), T0 + 61.0, 20, 0))
    sized = []
    for tile, n in zip(range(201, 206), (1, S - 1, S, S + 1, 2 * S)):
        for k in range(n):
            sized.append((TS.sid(1, tile, k % 3), TS.sid(1, tile, k % 3 + 1), T0 + 2 + 0.001 * k, T0 + 4 + 0.002 * k,
                          10 + k % 90, 0))
    return TS.reports_of([w, [], sized])


def synthetic_file(n, tile=400):
    """One add whose n reports all fall into one file."""
    return TS.reports_of([[(TS.sid(1, tile, k % 11), TS.sid(1, tile, (k + 1) % 11), T0 + 1 + 0.002 * k,
                            T0 + 3 + 0.002 * k, 25 + k % 50, k % 3) for k in range(n)]])


# the known answer of tests/test_tile_records_cpu.py, by hand from the Java layout
KAT_START, KAT_TILE = 1500000000, 8001
KAT_A = (0x4001f41, 0x6001f41, 1500000058.5, 1500000061.0, 44, 0)
KAT_B = (0x8001f41, T.NO_ID, 1500000002.25, 1500000003.75, 7, 2)
KAT_KEY = b'1500000000_8001.0'
KAT_MAP = bytes.fromhex('0000000059682f00' '0000000000001f41' '00000000')
KAT_VALUE = bytes.fromhex(
    '00000002' '0000000004001f41' '0000000006001f41' '41d65a0bcea00000' '41d65a0bcf400000' '0000002c' '00000000'
    '0000000008001f41' '00003fffffffffff' '41d65a0bc0900000' '41d65a0bc0f00000' '00000007' '00000002')


# ---- the refusal and map cases: tests/test_tile_records_cpu.py and the GPU jobs --------------
def _slices(rec):
    data = rec['bytes'].tobytes()
    return [(int(rec['start'][i]), int(rec['tile_id'][i]), int(rec['slice'][i]),
             data[int(rec['rec_off'][i]):int(rec['rec_off'][i + 1])]) for i in range(rec['n_slices'])]


def _entries(rec):
    return [MAP_ENTRY.unpack_from(rec['map_bytes'].tobytes(), 20 * t) for t in range(rec['n_tiles'])]


def refusal_cases():
    """(name, records, max_rows, reason, bad_slice, bad_tile): every reason of the restore, the
    lowest index and the lowest reason where two apply.  Shared with the GPU test."""
    held = held_of([case_reports(3)], Q)
    good = export(held, Q, 3)
    sl, en, n = _slices(good), _entries(good), len(held[0])

    def with_slice(i, s):
        return sl[:i] + [s] + sl[i + 1:]

    def value(*segs):
        return encode_slice(list(segs))

    s2 = sl[2]
    tid, st = s2[1], s2[0]
    ok_seg = (tid | (5 << 25), T.INVALID_SEGMENT_ID, st + 1.0, st + 2.0, 5, 0)
    cases = []
    bad_off = records_of(sl, 3, en)
    bad_off['rec_off'] = bad_off['rec_off'].copy()
    bad_off['rec_off'][3] = bad_off['rec_off'][2] - 4                       # record 2 runs backwards
    cases.append(('offsets backwards', bad_off, n, E_LAYOUT, 2, -1))
    beyond = records_of(sl, 3, en)
    beyond['rec_off'] = beyond['rec_off'].copy()
    beyond['rec_off'][-1] += 40
    cases.append(('beyond n_bytes', beyond, n, E_LAYOUT, len(sl) - 1, -1))
    cases.append(('shorter than a header', records_of(with_slice(1, sl[1][:3] + (b'\0\0',)), 3, en), n, E_LAYOUT, 1, -1))
    cases.append(('length is not 4 + 40 count', records_of(with_slice(1, sl[1][:3] + (sl[1][3] + b'\0' * 4,)), 3, en),
                  n, E_LAYOUT, 1, -1))
    cases.append(('count negative', records_of(with_slice(0, sl[0][:3] + (struct.pack('>i', -1),)), 3, en), n,
                  E_LAYOUT, 0, -1))
    # 40 * 0x06666667 = 2^32 + 24: in 32 bits a 28-byte record would pass
    cases.append(('count times 40 wraps 32 bits',
                  records_of(with_slice(0, sl[0][:3] + (struct.pack('>i', 0x06666667) + b'\0' * 24,)), 3, en), n,
                  E_LAYOUT, 0, -1))
    for name, key in (('start negative', (-60, tid, 0)), ('start off the grid', (st + 1, tid, 0)),
                      ('bucket beyond 39 bits', ((1 << 39) * Q, tid, 0)), ('tile_id negative', (st, -1, 0)),
                      ('tile_id beyond 25 bits', (st, 0x2000000, 0)), ('slice negative', (st, tid, -1))):
        cases.append((name, records_of(with_slice(2, key + (s2[3],)), 3, en), n, E_KEY, 2, -1))
    cases.append(('count zero', records_of(with_slice(2, s2[:3] + (value(),)), 3, en), n, E_COUNT, 2, -1))
    cases.append(('count above slice_size', records_of(with_slice(2, s2[:3] + (value(*[ok_seg] * 4),)), 3, en), n,
                  E_COUNT, 2, -1))
    for name, s in (('segment invalid', ok_seg[:4] + (0, 0)), ('segment min not positive', ok_seg[:2] + (-1.0, st + 2.0, 5, 0)),
                    ('segment max NaN', ok_seg[:3] + (float('nan'), 5, 0)),
                    ('segment max beyond 2^62', ok_seg[:3] + (2.0 ** 62, 5, 0)),
                    ('segment of another tile', ((tid ^ 8) | (5 << 25),) + ok_seg[1:]),
                    ('bucket outside the span', ok_seg[:2] + (st + 61.0, st + 62.0, 5, 0))):
        cases.append((name, records_of(with_slice(2, s2[:3] + (value(ok_seg, s),)), 3, en), n + 2, E_SEGMENT, 2, -1))
    cases.append(('duplicate key', records_of(sl + [sl[1]], 3, en), 2 * n, E_DUPLICATE, len(sl), -1))
    # two bad records, the lower index with the higher reason; and two reasons on one record
    cases.append(('lowest index first', records_of(with_slice(1, sl[1][:3] + (value(),)) + [sl[0][:3] + (b'\0',)], 3, en),
                  n, E_COUNT, 1, -1))
    cases.append(('lowest reason of one record', records_of(sl + [(st, tid, -1, value())], 3, en), n, E_KEY, len(sl), -1))
    cases.append(('duplicate and count', records_of(sl + [sl[1][:3] + (value(),)], 3, en), n, E_COUNT, len(sl), -1))
    cases.append(('map key invalid', records_of(sl, 3, en[:1] + [(en[1][0] + 1, en[1][1], 0)] + en[2:]), n, E_MAP, -1, 1))
    cases.append(('map value negative', records_of(sl, 3, en[:2] + [en[2][:2] + (-1,)] + en[3:]), n, E_MAP, -1, 2))
    cases.append(('map key repeated', records_of(sl, 3, en + [en[0]]), n, E_MAP, -1, len(en)))
    cases.append(('slice reason before map', records_of(with_slice(2, s2[:3] + (value(),)), 3, [en[0][:2] + (-1,)] + en[1:]),
                  n, E_COUNT, 2, -1))
    cases.append(('full', good, n - 1, E_FULL, -1, -1))
    cases.append(('full only alone', records_of(with_slice(2, s2[:3] + (value(),)), 3, en), 1, E_COUNT, 2, -1))
    return cases


def map_cases():
    """(name, records, use_map, counts): unreferenced, missing, no map.  Shared with the GPU test."""
    held = held_of([case_reports(3)], Q)
    good = export(held, Q, 3)
    sl, en = _slices(good), _entries(good)
    per = {}
    for s in sl:
        per.setdefault(s[:2], []).append(s)
    big = [e[:2] for e in en if e[2] == 2]                            # the file of 2 S rows: slices 0, 1; value 2
    assert len(big) == 1 and len(per[big[0]]) == 2
    big = big[0]
    lower = [e if e[:2] != big else big + (0,) for e in en]           # slice 1 unreferenced
    gone = [e for e in en if e[:2] != big]                            # both unreferenced
    higher = [e if e[:2] != big else big + (5,) for e in en]          # slices 2 .. 5 missing
    lost = [s for s in sl if s != per[big][0]]                        # slice 0 of the file is not in the input
    rows_of = lambda s: (len(s[3]) - 4) // 40
    n, ns = len(held[0]), len(sl)
    base = sum(e[2] + 1 - len(per[e[:2]]) for e in en)              # the exact multiples: one named slice each
    assert base >= 2
    return [('unreferenced slice', records_of(sl, 3, lower), True,
             dict(n_slices=ns - 1, n_rows=n - 3, n_unreferenced_slices=1, n_unreferenced_rows=3, n_missing_slices=base - 1)),
            ('unreferenced file', records_of(sl, 3, gone), True,
             dict(n_slices=ns - 2, n_rows=n - 6, n_unreferenced_slices=2, n_unreferenced_rows=6, n_missing_slices=base - 1)),
            ('missing slices', records_of(sl, 3, higher), True,
             dict(n_slices=ns, n_rows=n, n_unreferenced_slices=0, n_unreferenced_rows=0, n_missing_slices=base + 3)),
            ('slice lost', records_of(lost, 3, en), True,
             dict(n_slices=ns - 1, n_rows=n - rows_of(per[big][0]), n_unreferenced_slices=0, n_unreferenced_rows=0,
                  n_missing_slices=base + 1)),
            ('no map', records_of(sl, 3, gone), False,
             dict(n_slices=ns, n_rows=n, n_unreferenced_slices=0, n_unreferenced_rows=0, n_missing_slices=0)),
            ('empty map', records_of(sl, 3, []), True,
             dict(n_slices=0, n_rows=0, n_unreferenced_slices=ns, n_unreferenced_rows=n, n_missing_slices=0))]
