"""The tile file texts restated in Python from the rules of
include/otr.h otr_tiles_text: rows grouped by file -> file table, names, texts.  A helper module
(no tests, no fixtures): tests/test_tile_text_cpu.py pins what it computes to the library's host
formatter otr_tiles_format and to simple_reporter's host payloads, tests/test_gpu_tile_text.py
holds the device writer equal to it byte for byte.

A case is a dict: name, rows (numpy TILE_ROW, the rows of one file adjacent), q (quantisation),
source and mode (bytes)."""
import numpy as np

from oracle import tiles as T

TILE_ROW = T.TILE_ROW
SIMPLE, STREAM = 0, 1
INVALID = 0x3fffffffffff           # OTR_INVALID_SEGMENT_ID
HEADER = (b'segment_id,next_segment_id,duration,count,length,queue_length,minimum_timestamp,maximum_timestamp,'
          b'source,vehicle_type')
M64 = (1 << 64) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def upper_ascii(b):
    return bytes(c - 32 if 97 <= c <= 122 else c for c in b)


def tag_of(source, mode, rules):
    return b',' + source + b',' + upper_ascii(mode) + (b'' if rules == STREAM else b'\n')


def row_bytes(r, rules, tag):
    """One row's bytes: "\\n" first under the stream rules, next_id left out there when invalid."""
    nxt = b'' if rules == STREAM and int(r['next_id']) == INVALID else b'%d' % int(r['next_id'])
    return (b'\n' if rules == STREAM else b'') + b','.join([
        b'%d' % int(r['id']), nxt, b'%d' % int(r['duration']), b'1', b'%d' % int(r['length']),
        b'%d' % int(r['queue_length']), b'%d' % int(r['start']), b'%d' % int(r['end'])]) + tag


def name_of(file, q):
    """"{b*q}_{(b+1)*q-1}/{level}/{tile}", both products modulo 2^64."""
    file = int(file)
    b = file >> 25
    return b'%d_%d/%d/%d' % ((b * q) & M64, ((b + 1) * q - 1) & M64, (file >> 22) & 7, file & 0x3fffff)


def name_wraps(file, q):
    return ((int(file) >> 25) + 1) * q - 1 > M64


def build(rows, q, rules, source, mode):
    """Everything otr_tiles_text returns for rows: file, row_off, text, text_off, names, name_off
    (numpy) and row_len (each row's own bytes).  Runs of equal `file` are the files."""
    tag = tag_of(source, mode, rules)
    head = HEADER + (b'' if rules == STREAM else b'\n')
    files, row_off, texts, names, row_len = [], [], [], [], []
    for i, r in enumerate(rows):
        if i == 0 or int(r['file']) != int(rows[i - 1]['file']):
            files.append(int(r['file']))
            row_off.append(i)
            texts.append([head])
            names.append(name_of(r['file'], q))
        line = row_bytes(r, rules, tag)
        row_len.append(len(line))
        texts[-1].append(line)
    texts = [b''.join(t) for t in texts]
    return {'n_rows': len(rows), 'n_files': len(files), 'file': np.array(files, np.uint64),
            'row_off': np.array(row_off + [len(rows)], np.int64),
            'text': np.frombuffer(b''.join(texts), np.uint8),
            'text_off': np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64),
            'names': np.frombuffer(b''.join(names), np.uint8),
            'name_off': np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.int64),
            'n_text_bytes': sum(len(t) for t in texts), 'n_name_bytes': sum(len(x) for x in names),
            'row_len': row_len}


ARRAYS = ('file', 'row_off', 'text', 'text_off', 'names', 'name_off')
COUNTS = ('n_rows', 'n_files', 'n_text_bytes', 'n_name_bytes')


def differing(got, want):
    """What differs between a result and the restatement: arrays byte for byte, counts by value."""
    bad = []
    for k in ARRAYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
            d = int(np.flatnonzero(a[:min(len(a), len(b))] != b[:min(len(a), len(b))])[:1].sum())
            bad.append('%s: got %s want %s, first difference near %d: %r / %r' % (
                k, a.shape, b.shape, d, a[max(d - 8, 0):d + 24].tobytes(), b[max(d - 8, 0):d + 24].tobytes()))
    for k in COUNTS:
        if int(got[k]) != int(want[k]):
            bad.append('%s: got %d want %d' % (k, got[k], want[k]))
    return bad


def check_lines(case):
    """What tools/tiletextcheck prints for the case (its output split at newlines)."""
    out = []
    for rules in (SIMPLE, STREAM):
        w = build(case['rows'], case['q'], rules, case['source'], case['mode'])
        out.append('rules %d files %d rows %d text %d names %d' % (rules, w['n_files'], w['n_rows'], w['n_text_bytes'],
                                                                   w['n_name_bytes']))
        out.append('lens' + ''.join(' %d' % x for x in w['row_len']))
        text, names = w['text'].tobytes(), w['names'].tobytes()
        for f in range(w['n_files']):
            out.append('file %d %d %d %s' % (w['file'][f], w['row_off'][f], w['text_off'][f],
                                             names[w['name_off'][f]:w['name_off'][f + 1]].decode()))
            out.append('text ' + text[w['text_off'][f]:w['text_off'][f + 1]].hex())
    return out + ['']


def check_file(case):
    """The case as tools/tiletextcheck reads it."""
    rows = np.ascontiguousarray(case['rows'], TILE_ROW)
    return (np.array([len(rows), case['q'], len(case['source']), len(case['mode'])], np.int64).tobytes() +
            rows.tobytes() + case['source'] + case['mode'])


# ---- the hand-built cases -----------------------------------------------------------------
T0 = 1500000000


def file_of(bucket, level, tile):
    return (bucket << 25) | (level << 22) | tile


def plain_rows(n, files, seed=1):
    """n everyday rows (ids of 10 to 13 digits, times of 10, small lengths: 75 to 85 bytes a
    row with the usual tag), row i in file files[i]."""
    rng = np.random.RandomState(seed)
    rows = np.zeros(n, TILE_ROW)
    rows['file'] = np.asarray(files, np.uint64)
    rows['id'] = rng.randint(1 << 33, 1 << 43, n).astype(np.uint64)
    rows['next_id'] = rng.randint(1 << 33, 1 << 43, n).astype(np.uint64)
    rows['next_id'][rng.randint(0, 4, n) == 0] = INVALID
    rows['start'] = T0 + rng.randint(0, 3600, n)
    rows['end'] = rows['start'] + rng.randint(1, 200, n)
    rows['duration'] = rows['end'] - rows['start']
    rows['length'] = rng.randint(1, 2000, n)
    rows['queue_length'] = rng.randint(0, 3, n) * rng.randint(0, 150, n)
    rows['speed_bin'] = rng.randint(0, 8, n)
    return rows


def _edges(bits, signed):
    """The digit-count edges of a width: powers of ten and powers of ten minus one, and the
    range's ends; for signed widths both signs."""
    top = (1 << (bits - 1)) - 1 if signed else (1 << bits) - 1
    v = [0, top]
    k = 10
    while k <= top:
        v += [k, k - 1]
        k *= 10
    if signed:
        v += [-x for x in v if x] + [-top - 1, -1]
    return v


def extreme_rows():
    """Every field at its extremes and digit-count edges, spread over three files."""
    u64, i64, i32 = _edges(64, False), _edges(64, True), _edges(32, True)
    ids = [0, M64] + u64
    nxt = [INVALID, INVALID - 1, 0, M64] + u64
    n = max(len(ids), len(nxt), len(i64), len(i32)) + 3
    rows = np.zeros(n, TILE_ROW)
    for i in range(n):
        rows[i]['id'] = ids[i % len(ids)]
        rows[i]['next_id'] = nxt[i % len(nxt)]
        rows[i]['duration'] = i32[i % len(i32)]
        rows[i]['length'] = i32[(i + 1) % len(i32)]
        rows[i]['queue_length'] = i32[(i + 2) % len(i32)]
        rows[i]['start'] = i64[i % len(i64)]
        rows[i]['end'] = i64[(i + 1) % len(i64)]
    # the named extremes together in single rows
    rows[-3] = (0, 0, INVALID, I64_MIN, I64_MAX, I32_MIN, I32_MAX, -1, 0)
    rows[-2] = (0, M64, INVALID - 1, -1, 0, -1, 0, I32_MIN, 0)
    rows[-1] = (0, M64, M64, I64_MAX, I64_MIN, I32_MAX, I32_MIN, I32_MAX, 0)
    rows['file'] = [file_of(25000000 + i * 3 // n, 1, 1000) for i in range(n)]
    return rows


def longest_rows(n):
    """Rows whose every numeric field prints at its longest (122 bytes before the tag)."""
    rows = np.zeros(n, TILE_ROW)
    rows['file'] = [file_of(25000000, 2, 7 + i // 120) for i in range(n)]
    rows['id'] = M64 - np.arange(n).astype(np.uint64)
    rows['next_id'] = M64
    rows['start'] = I64_MIN
    rows['end'] = I64_MIN + 1
    rows['duration'] = I32_MIN
    rows['length'] = I32_MIN + 1
    rows['queue_length'] = I32_MIN + 2
    return rows


def span_start(rows, i, rules, source, mode):
    """The text offset at which row i's bytes (its file's header first) begin."""
    w = build(rows[:i], 1, rules, source, mode)
    return w['n_text_bytes']


def cases():
    out = []

    def add(name, rows, q=3600, source=b'reporter', mode=b'auto'):
        out.append({'name': name, 'rows': np.ascontiguousarray(rows, TILE_ROW), 'q': q, 'source': source, 'mode': mode})

    one = file_of(25000000, 1, 1000)
    for n in (0, 1, 2, 255, 256, 257, 513):
        add('one_file_%d' % n, plain_rows(n, [one] * n, seed=n))
        add('own_file_%d' % n, plain_rows(n, [file_of(25000000 + i // 200, i % 3, 5 + i) for i in range(n)], seed=n + 1))
    for at in (255, 256, 257):
        add('second_file_at_%d' % at, plain_rows(300, [one] * at + [one + 1] * (300 - at), seed=at), q=60)
    add('extremes', extreme_rows())
    # 300 rows, a source of k bytes.  256 rows shift the second block's span by a multiple of 16
    # whatever k is, so row 0's id is given the digits that put that span's start (and the first
    # block's end) at residue k mod 16 under the stream rules, and k + 4 under the simple ones
    # (four files begin among the first 256 rows, each with one byte more of header)
    for k in range(16):
        rows = plain_rows(300, [one + i // 77 for i in range(300)], seed=40)
        rows[0]['id'] = 1
        rows['next_id'][rows['next_id'] == INVALID] = INVALID - 1   # (printed under both rule sets)
        source = b'sixteen_bytes_src'[:k]
        at = span_start(rows, 256, STREAM, source, b'auto')
        rows[0]['id'] = 10 ** ((k - at) % 16)
        add('source_%d' % k, rows, source=source)
    long_source = bytes(33 + i % 94 for i in range(255))
    add('longest_lower', longest_rows(300), source=long_source, mode=bytes(97 + i % 26 for i in range(255)))
    add('longest_mixed', longest_rows(300), source=long_source,
        mode=bytes((b'aZ{`z@A[/m9 ~')[i % 13] for i in range(255)))
    name_files = [file_of(b, l, t) for b in (0, 1, 416666, (1 << 39) - 1) for l in (0, 7) for t in (0, 9, 0x3fffff)]
    for q in (60, 3600, (1 << 31) - 1):
        add('names_q%d' % q, plain_rows(2 * len(name_files), [f for f in name_files for _ in (0, 1)], seed=q % 97), q=q)
    # every name at its longest, 51 bytes: both products of 20 digits after the wrap, a tile of 7
    q = (1 << 31) - 1
    longest = [b for b in range((1 << 39) - 1, (1 << 39) - 200, -1)
               if (b * q) & M64 >= 10 ** 19 and ((b + 1) * q - 1) & M64 >= 10 ** 19][:5]
    add('names_longest', plain_rows(5, [file_of(b, 7, 0x3fffff) for b in longest], seed=8), q=q)
    add('file_recurs', plain_rows(7, [one, one, one + 1, one, one, one + 1, one + 1], seed=9))
    add('empty_tag', plain_rows(5, [one] * 5, seed=3), source=b'', mode=b'')
    return out
