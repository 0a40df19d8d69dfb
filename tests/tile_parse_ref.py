"""Tile file texts read back into rows restated in Python from the
rules of include/otr.h otr_tiles_parse.  A helper module (no tests, no fixtures):
tests/test_tile_parse_cpu.py holds the header's functions (tools/tileparsecheck, under sanitizers)
equal to it, tests/test_gpu_tile_parse.py the device parser.

The rule is applied literally: a piece is split at its commas, its numeric fields are read as
Python ints from any run of digits behind an optional '-', the row they give is rendered again by
tests/tile_text_ref.py, and the piece is a row if and only if those bytes are the line's bytes.
The reasons of the lines that are not rows are worked out separately, by the table of
include/otr.h, and the two must agree (an AssertionError here means the table and the rule
disagree).  Every line of a file whose name was refused is U_NAME, whatever it holds.

A case is a dict: name, files (a list of (name bytes, text bytes)), q, rules, source, mode."""
import re

import numpy as np

from tests import tile_text_ref as X

TILE_ROW = X.TILE_ROW
SIMPLE, STREAM = X.SIMPLE, X.STREAM
ROW, HEADER, E_FIELDS = 0, 1, 2
U_NAME, U_END, U_HEADER, U_FIELDS, U_NUMBER, U_NEXT, U_COUNT, U_TAG = 32, 33, 34, 35, 36, 37, 38, 39
NO_ID = X.M64
_DIGITS = re.compile(rb'-?[0-9]+\Z')
_UDIGITS = re.compile(rb'[0-9]+\Z')


def parse_name(name, q):
    """The file value of "{a}_{b}/{level}/{tile}", or None."""
    m = re.match(rb'([0-9]+)_([0-9]+)/([0-9]+)/([0-9]+)\Z', name)
    if not m:
        return None
    a, b, level, tile = (int(x) for x in m.groups())
    if any(x != b'%d' % v for x, v in zip(m.groups(), (a, b, level, tile))):
        return None
    if a > X.M64 or b > X.M64 or a % q or b != a + q - 1 or a // q >= 1 << 39 or level > 7 or tile >= 1 << 22:
        return None
    file = (a // q) << 25 | level << 22 | tile
    assert X.name_of(file, q) == name and not X.name_wraps(file, q)
    return file


def pieces_of(text, rules):
    """[(piece, terminated)] of one file's text: the pieces that are lines."""
    if not text:
        return []
    p = text.split(b'\n')
    out = [(x, True) for x in p[:-1]]
    if rules == STREAM or p[-1]:
        out.append((p[-1], False))
    return out


def _row_of(fields, rules, file):
    """The row the ten fields give when every numeric one is digits behind an optional '-' of a
    value its member holds (next_id: empty under the stream rules is the invalid id), else None."""
    num = {}
    for k, i, lo, hi, rx in (('id', 0, 0, X.M64, _UDIGITS), ('next_id', 1, 0, X.M64, _UDIGITS),
                             ('duration', 2, X.I32_MIN, X.I32_MAX, _DIGITS), ('length', 4, X.I32_MIN, X.I32_MAX, _DIGITS),
                             ('queue_length', 5, X.I32_MIN, X.I32_MAX, _DIGITS),
                             ('start', 6, X.I64_MIN, X.I64_MAX, _DIGITS), ('end', 7, X.I64_MIN, X.I64_MAX, _DIGITS)):
        if k == 'next_id' and fields[i] == b'' and rules == STREAM:
            num[k] = X.INVALID
            continue
        if not rx.match(fields[i]):
            return None
        v = int(fields[i])
        if not lo <= v <= hi:
            return None
        num[k] = v
    r = np.zeros(1, TILE_ROW)[0]
    r['file'] = file
    for k, v in num.items():
        r[k] = v
    r['speed_bin'] = -1
    return r


def _canonical(x, lo, hi, signed):
    if not (_DIGITS if signed else _UDIGITS).match(x):
        return False
    v = int(x)
    return lo <= v <= hi and x == b'%d' % v


def _reason(piece, first, terminated, rules, source, mode):
    """The status of a piece by the table of include/otr.h (ROW: no reason applies)."""
    if first and piece == X.HEADER:
        return HEADER
    f = piece.split(b',')
    if len(f) < 2:
        return E_FIELDS
    if rules == SIMPLE and not terminated:
        return U_END
    if piece == X.HEADER or (rules == STREAM and first):
        return U_HEADER
    if len(f) != 10:
        return U_FIELDS
    checks = [(0, 0, X.M64, False), (1, 0, X.M64, False), (2, X.I32_MIN, X.I32_MAX, True), (4, X.I32_MIN, X.I32_MAX, True),
              (5, X.I32_MIN, X.I32_MAX, True), (6, X.I64_MIN, X.I64_MAX, True), (7, X.I64_MIN, X.I64_MAX, True)]
    for i, lo, hi, signed in checks:
        if i == 1 and f[1] == b'':
            continue
        if not _canonical(f[i], lo, hi, signed):
            return U_NUMBER
    if (f[1] == b'' and rules == SIMPLE) or (rules == STREAM and f[1] == b'%d' % X.INVALID):
        return U_NEXT
    if f[3] != b'1':
        return U_COUNT
    if f[8] != source or f[9] != X.upper_ascii(mode):
        return U_TAG
    return ROW


def parse_piece(piece, first, terminated, rules, source, mode, file):
    """(status, row or None) of one piece of a file whose name gave `file`."""
    tag = X.tag_of(source, mode, rules)
    # the line's own bytes: a stream file's first piece has no "\n" before it, and a simple
    # file's unterminated one none behind it, so neither is ever a row's bytes
    if rules == STREAM:
        line = (b'' if first else b'\n') + piece
    else:
        line = piece + (b'\n' if terminated else b'')
    f = piece.split(b',')
    row = _row_of(f, rules, file) if len(f) == 10 else None
    # THE RULE: a row iff writing it back gives the line's bytes
    is_row = row is not None and X.row_bytes(row, rules, tag) == line
    status = _reason(piece, first, terminated, rules, source, mode)
    assert is_row == (status == ROW), (piece, first, terminated, rules, status)
    return status, (row if is_row else None)


def parse(case):
    """Everything otr_tiles_parse returns for the case (numpy arrays and counts)."""
    q, rules, source, mode = case['q'], case['rules'], case['source'], case['mode']
    status, rows, row_off, files, fstat, line_off = [], [], [0], [], [], [0]
    for name, text in case['files']:
        file = parse_name(name, q)
        files.append(NO_ID if file is None else file)
        fstat.append(1 if file is None else 0)
        for j, (piece, terminated) in enumerate(pieces_of(text, rules)):
            if file is None:
                status.append(U_NAME)
                continue
            st, row = parse_piece(piece, j == 0, terminated, rules, source, mode, file)
            status.append(st)
            if row is not None:
                rows.append(row)
        row_off.append(len(rows))
        line_off.append(len(status))
    status = np.array(status, np.uint8)
    bad = np.flatnonzero(status >= E_FIELDS)
    first_bad = int(bad[0]) if len(bad) else -1
    line_off = np.array(line_off, np.int64)
    return {'n_files': len(files), 'n_lines': len(status), 'n_rows': len(rows),
            'n_headers': int((status == HEADER).sum()), 'n_bad': len(bad), 'n_bad_names': int(sum(fstat)),
            'first_bad': first_bad,
            'first_bad_file': int(np.searchsorted(line_off, first_bad, side='right') - 1) if len(bad) else -1,
            'first_bad_reason': int(status[first_bad]) if len(bad) else 0,
            'rows': np.array(rows, TILE_ROW) if rows else np.zeros(0, TILE_ROW),
            'row_off': np.array(row_off, np.int64), 'file': np.array(files, np.uint64),
            'file_status': np.array(fstat, np.uint8), 'file_line_off': line_off, 'line_status': status}


ARRAYS = ('rows', 'row_off', 'file', 'file_status', 'file_line_off', 'line_status')
COUNTS = ('n_files', 'n_lines', 'n_rows', 'n_headers', 'n_bad', 'n_bad_names', 'first_bad', 'first_bad_file',
          'first_bad_reason')


def differing(got, want):
    """What differs between a result and the restatement: arrays byte for byte, counts by value."""
    bad = []
    for k in ARRAYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
            n = min(len(a), len(b))
            d = int(np.flatnonzero(a[:n] != b[:n])[:1].sum()) if n else 0
            bad.append('%s: got %s want %s, first difference near %d: %r / %r' % (
                k, a.shape, b.shape, d, a[d:d + 2].tolist(), b[d:d + 2].tolist()))
    for k in COUNTS:
        if int(got[k]) != int(want[k]):
            bad.append('%s: got %d want %d' % (k, got[k], want[k]))
    return bad


def pack(case):
    """The case's files as the four arrays otr_tiles_parse takes."""
    def cat(parts):
        off = np.zeros(len(parts) + 1, np.int64)
        off[1:] = np.cumsum([len(p) for p in parts])
        return np.frombuffer(b''.join(parts), np.uint8), off
    text, text_off = cat([t for _, t in case['files']])
    names, name_off = cat([n for n, _ in case['files']])
    return text, text_off, names, name_off


def check_file(case):
    """The case as tools/tileparsecheck reads it."""
    text, text_off, names, name_off = pack(case)
    head = np.array([len(case['files']), case['q'], case['rules'], len(case['source']), len(case['mode']), len(text),
                     len(names)], np.int64)
    return (head.tobytes() + text_off.tobytes() + name_off.tobytes() + text.tobytes() + names.tobytes() +
            case['source'] + case['mode'])


def check_lines(case):
    """What tools/tileparsecheck prints for the case (its output split at newlines)."""
    w = parse(case)
    out = ['files %d lines %d rows %d headers %d bad %d bad_names %d first_bad %d %d %d' % tuple(
        w[k] for k in ('n_files', 'n_lines', 'n_rows', 'n_headers', 'n_bad', 'n_bad_names', 'first_bad',
                       'first_bad_file', 'first_bad_reason'))]
    for f in range(w['n_files']):
        out.append('file %d %d %d %d' % (w['file'][f], w['file_status'][f], w['file_line_off'][f], w['row_off'][f]))
    out.append('status' + ''.join(' %d' % s for s in w['line_status']))
    for r in w['rows']:
        out.append('row %d %d %d %d %d %d %d %d %d' % tuple(int(r[k]) for k in (
            'file', 'id', 'next_id', 'start', 'end', 'duration', 'length', 'queue_length', 'speed_bin')))
    return out + ['']
