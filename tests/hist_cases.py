"""Hand-built entry sets for otr_hist_reduce (the keyed speed histogram, otr_tiles.hip
Matcher::hist_reduce).  A helper module (no tests, no fixtures): tests/test_hist_cases_cpu.py pins
the branch every family takes and that its reduction is not trivial, tests/test_gpu_hist_keyed.py
runs them on the device against oracle/hist.reduce.

Matcher::hist_reduce sorts by (file, id, next id, speed bin) with LSD radix passes chosen from the
data (k_entry_range: OR of the ids and of the next ids, min / max bucket, whether every file is
the one K9 derives from its id):
  low passes   'combined' one pass over next id << 3 | bin when bit_width(next OR) + 3 <= 64,
               else 'split': the bin (3 bits), then the next id;
  high passes  'packed' one pass over (bucket - min bucket) << 46 | level << 43 | tile << 21 |
               index when the files are K9's, the ids fit 46 bits and bit_width(max - min bucket)
               + 46 <= 64, else 'id_file': the id, then the file.
pass_choice() restates that choice; the families sit on each side of every threshold.  With
privacy > 1, k_pair_file_top2 finds a file's string-last and string-second pair with one
1024-thread block (a strided loop, then a tree in LDS): the big_* families have files of more
than 1024 pairs.  k_entry_range strides a fixed grid of 128 x 1024 threads: the n_* families
keep the entry that alone decides the bucket spread at the last index.

Every set is seeded, shuffled and has keys repeated in all 8 speed bins.  An id of more than
18 decimal digits keys on its leading 18 in the device's string order (otr_tile_kernels.h dec_key):
the wide ids here differ within those (checked by _leading18)."""
import numpy as np

from oracle import hist as oh
from oracle import tiles as ot

BINS = 8
B60 = 1483228800 // 60  # the 60 s bucket of 2017-01-01T00:00:00Z
INV = ot.INVALID_SEGMENT_ID


def seg_id(index, tile, level):
    return (index << 25) | (tile << 3) | level


def k9_file(bucket, sid):
    """The file K9 derives from a segment id (otr_tile_row.file)."""
    return (bucket << 25) | ((sid & 7) << 22) | ((sid >> 3) & 0x3FFFFF)


def edge_file(bucket, sid):
    """A file that is not K9's: tile index 0, as otr_edge_observations writes them."""
    return (bucket << 25) | ((sid & 7) << 22)


def bit_width(v):
    return int(v).bit_length()


def pass_choice(e):
    """(low passes, high passes, [(field, end bit)]) of Matcher::hist_reduce for the entries e."""
    nor = ior = fo = 0
    for v in e['next_id'].tolist():
        nor |= v
    for v in e['id'].tolist():
        ior |= v
    for v in e['file'].tolist():
        fo |= v
    b = e['file'] >> np.uint64(25)
    ws = bit_width(int(b.max()) - int(b.min()))
    foreign = bool(((e['file'] & np.uint64(0x1FFFFFF)) !=
                    (((e['id'] & np.uint64(7)) << np.uint64(22)) |
                     ((e['id'] >> np.uint64(3)) & np.uint64(0x3FFFFF)))).any())
    wn, wi = bit_width(nor), bit_width(ior)
    if wn + 3 <= 64:
        low, passes = 'combined', [(4, wn + 3)]
    else:
        low, passes = 'split', [(3, 3), (2, wn)]
    if not foreign and wi <= 46 and ws + 46 <= 64:
        high = 'packed'
        passes.append((5, max(46 + ws, 1)))
    else:
        high = 'id_file'
        passes += [(1, max(wi, 1)), (0, max(bit_width(fo), 1))]
    return low, high, passes


def _leading18(values):
    """Distinct values keep distinct leading 18 decimal digits (so dec_key orders them as strings)."""
    v = sorted(set(int(x) for x in values))
    assert len(set(str(x)[:18] for x in v)) == len(v), 'two ids share their leading 18 digits'


def _entries(rows):
    return np.array(rows, dtype=oh.HIST_ENTRY) if rows else np.zeros(0, oh.HIST_ENTRY)


# ids whose decimal strings sort differently from their values (2, 3, 30, 298 -> 9 to 11 digits),
# levels 0 to 2, and index 2^21 - 1: bit 45, the widest id K9's packed key holds
IDS = [seg_id(2, 5, 0), seg_id(3, 5, 0), seg_id(30, 5, 1), seg_id(298, 77, 1), seg_id(2980, 77, 2),
       seg_id(29802, 4000000, 0), seg_id((1 << 21) - 1, 5, 0), seg_id(1 << 20, (1 << 22) - 1, 2)]
NEXTS = [INV, seg_id(2, 5, 0), seg_id(30, 5, 1), seg_id(298, 77, 1), seg_id(3, 6, 0), seg_id(29, 5, 2),
         seg_id((1 << 21) - 1, 5, 0), seg_id(7, 9, 1)]
WEIGHTS = [1, 1, 2, 3, 16, 1, 2, 5]  # entries per pair; 16: every bin twice (the keys that pad a set)


def build(seed, n=700, ids=IDS, nexts=NEXTS, buckets=(B60, B60 + 1, B60 + 2), file_of=k9_file, n_pairs=64,
          repeat=None, last=None):
    """n entries over n_pairs (id, next id) pairs, pair k in bucket buckets[k % len(buckets)]:
    WEIGHTS[k % 8] entries of count 1 in random bins (totals of 1, 2, 3, 5: kept or culled at
    privacy 2 and 3), the pairs of weight 16 in every bin twice with counts 1 to 3.  The set is
    padded to n with further entries of the heavy pairs' keys, then shuffled.  repeat: (k, times)
    adds `times` more copies of the first entry of pair k before the shuffle.  last: (bucket,)
    appends one entry of pair 0's id in that bucket AFTER the shuffle (the last index)."""
    rng = np.random.default_rng(seed)
    _leading18(list(ids) + list(nexts))
    rows, heavy, firsts = [], [], {}
    for k in range(n_pairs):
        sid, nx = ids[k % len(ids)], nexts[(k // len(ids) + k) % len(nexts)]
        f = file_of(buckets[k % len(buckets)], sid)
        w = WEIGHTS[k % len(WEIGHTS)]
        firsts[k] = len(rows)
        if w == 16:
            for b in list(range(BINS)) * 2:
                rows.append((f, sid, nx, b, int(rng.integers(1, 4))))
                heavy.append((f, sid, nx, b, 1))
        else:
            for b in rng.integers(0, BINS, w).tolist():
                rows.append((f, sid, nx, b, 1))
    assert len(set(r[:3] for r in rows)) == n_pairs, 'pairs repeat'
    if repeat:
        rows += [rows[firsts[repeat[0]]]] * repeat[1]
    room = n - len(rows) - (1 if last else 0)
    assert room >= 0, (n, len(rows))
    rows += [heavy[i] for i in rng.integers(0, len(heavy), room).tolist()]
    e = _entries(rows)[rng.permutation(len(rows))]
    if last:
        e = np.concatenate([e, _entries([(file_of(last[0], ids[0]), ids[0], nexts[1], 3, 1)])])
    assert len(e) == n
    return e


def _wide(nexts, *wide):
    """NEXTS with its last len(wide) values replaced."""
    return list(nexts[:len(nexts) - len(wide)]) + list(wide)


# next ids of 61 bits (2^61 - 1 the widest: the combined pass ends at bit 64), 19 digits each,
# different within their leading 18
N61 = [(1 << 61) - 1, (1 << 61) - 1 - 1000, (1 << 60) + 12345, (1 << 60) + 12345 + 77000]
FAMILIES = {
    # name: (builder, low passes, high passes, the end bits that matter)
    'baseline': (lambda: build(1), 'combined', 'packed', {4: 49, 5: 48}),
    'next_61_bits': (lambda: build(2, nexts=_wide(NEXTS, *N61)), 'combined', 'packed', {4: 64}),
    'next_62_bits': (lambda: build(3, nexts=_wide(NEXTS, *(N61[1:] + [1 << 61]))), 'split', 'packed', {2: 62}),
    'next_bit_63': (lambda: build(4, nexts=_wide(NEXTS, (1 << 63) + 12345)), 'split', 'packed', {2: 64}),
    'spread_18_bits': (lambda: build(5, buckets=(B60, B60 + 7, B60 + (1 << 18) - 1)), 'combined', 'packed', {5: 64}),
    'spread_19_bits': (lambda: build(6, buckets=(B60, B60 + 7, B60 + (1 << 18))), 'combined', 'id_file', {}),
    # two ids that differ in bit 46 only: the same file, the same packed key
    'id_bit_46': (lambda: build(7, ids=IDS[:6] + [IDS[2] | (1 << 46), IDS[6]]), 'combined', 'id_file', {1: 47}),
    'foreign_files': (lambda: build(8, file_of=edge_file), 'combined', 'id_file', {1: 46}),
    'foreign_wide_next': (lambda: build(9, file_of=edge_file, nexts=_wide(NEXTS, (1 << 63) + 999, 1 << 61)),
                          'split', 'id_file', {2: 64}),
    'one_key_1025': (lambda: build(10, n=1800, repeat=(3, 1024)), 'combined', 'packed', {}),
    # k_entry_range: one block less one thread, one block, one thread of a second block, and one
    # entry beyond the fixed grid; the last entry alone has the largest bucket
    'n_1023': (lambda: build(11, n=1023, buckets=(B60, B60 + 1), last=(B60 + 2,)), 'combined', 'packed', {5: 48}),
    'n_1024': (lambda: build(12, n=1024, buckets=(B60, B60 + 1), last=(B60 + 2,)), 'combined', 'packed', {5: 48}),
    'n_1025': (lambda: build(13, n=1025, buckets=(B60, B60 + 1), last=(B60 + 2,)), 'combined', 'packed', {5: 48}),
    'n_131073': (lambda: build(14, n=131073, n_pairs=128, buckets=(B60, B60 + 1, B60 + 2), last=(B60 + 4,)),
                 'combined', 'packed', {5: 49}),
}
# (131073 = 128 x 1024 + 1: k_entry_range's whole grid and one entry more)


# ---- files of more than 1024 pairs --------------------------------------------------------
X_INDEX = 29802  # seg_id(29802, 5, 0) = 999989182504: its string sorts after every other id below


def big_file_spec(rng, bucket, n_pairs, last_pos, last_total, second_total, level):
    """The (bucket, id, next id, bin, lines) spec (tests/test_hist_cull_cpu._rows) of one file of
    n_pairs pairs with distinct ids.  The string-last pair has `last_total` lines and is number
    last_pos in numeric order (thread last_pos % 1024 of k_pair_file_top2 meets it in stride
    last_pos // 1024); the string-second pair has second_total lines."""
    x = seg_id(X_INDEX, 5, level)
    below = [i for i in range(1, X_INDEX) if str(seg_id(i, 5, level)) < str(x)]
    lo = sorted(rng.choice(below, last_pos, replace=False).tolist())
    hi = list(range(X_INDEX + 1, X_INDEX + n_pairs - last_pos))
    ids = [seg_id(i, 5, level) for i in lo] + [x] + [seg_id(i, 5, level) for i in hi]
    assert ids == sorted(ids) and len(set(ids)) == n_pairs and ids[last_pos] == x
    assert max(ids, key=str) == x
    second = max((i for i in ids if i != x), key=str)
    spec = []
    for sid in ids:
        nx = INV if sid % 3 == 0 else IDS[sid % len(IDS)]
        w = last_total if sid == x else (second_total if sid == second else int(rng.choice([1, 1, 2, 3])))
        spec += [(bucket, sid, nx, int(rng.integers(0, BINS)), 1) for _ in range(w)]
    return spec, ids.index(second)


# name: [(pairs, the string-last pair's numeric position, its lines, the string-second pair's lines)]
# the big file's trailing single line is judged with the pair before it (1 + 1 kept at privacy 2,
# 2 + 1 kept at 3); the sibling's string-last pair has two lines, so every pair is judged alone
BIG = {
    'big_1500': [(1500, 1450, 1, 1), (1100, 1060, 2, 1)],
    'big_2500': [(2500, 2040, 1, 2), (1100, 30, 2, 2)],
}


def big_rows(name):
    """(tile rows, shuffled; [(file, pairs, position of the string-last pair, of the string-second)])."""
    from tests.test_hist_cull_cpu import _rows
    rng = np.random.default_rng(sorted(BIG).index(name) + 40)
    spec, where = [], []
    for level, (n_pairs, pos, t1, t2) in enumerate(BIG[name]):
        s, second_pos = big_file_spec(rng, 412008, n_pairs, pos, t1, t2, level)
        spec += s
        where.append((k9_file(412008, s[0][1]), n_pairs, pos, second_pos))
    # a few small files beside them
    spec += [(412009, IDS[k], NEXTS[k], k, 1 + k % 3) for k in range(6)]
    rows = _rows(spec)
    return rows[rng.permutation(len(rows))], where


def big_entries(name):
    return oh.entries_from_rows(big_rows(name)[0])


for _n in BIG:
    FAMILIES[_n] = ((lambda n=_n: big_entries(n)), 'combined', 'packed', {})

_CACHE = {}


def entries(name):
    """The family's entries, built once per process (callers leave them unchanged)."""
    if name not in _CACHE:
        _CACHE[name] = FAMILIES[name][0]()
    return _CACHE[name]


_WANT = {}


def reduced(name, privacy):
    """oracle/hist.reduce of the family, computed once per process."""
    if (name, privacy) not in _WANT:
        _WANT[(name, privacy)] = oh.reduce(entries(name), privacy)
    return _WANT[(name, privacy)]
