"""Hand-built cases for the tile file parser (K21, include/otr.h otr_tiles_parse), at the smallest
sizes where its kernels can go wrong.  A helper module (no tests, no fixtures):
tests/test_tile_parse_cpu.py pins what the cases cover and their hand-written statuses to the
restatement tests/tile_parse_ref.py and runs them through tools/tileparsecheck,
tests/test_gpu_tile_parse.py through the device parser.

A case is a dict: name, files [(name, text)], q, rules, source, mode, and where the statuses were
written by hand `expect`, the list of every line's status."""
from tests import tile_parse_ref as P
from tests import tile_text_ref as X

SIMPLE, STREAM = P.SIMPLE, P.STREAM
H = X.HEADER
Q = 3600
BUCKET = 416666
SRC, MODE = b'smpl_rprt', b'auto'
ROW, HEADER, E_FIELDS = P.ROW, P.HEADER, P.E_FIELDS
U_NAME, U_END, U_HEADER, U_FIELDS, U_NUMBER, U_NEXT, U_COUNT, U_TAG = (P.U_NAME, P.U_END, P.U_HEADER, P.U_FIELDS,
                                                                       P.U_NUMBER, P.U_NEXT, P.U_COUNT, P.U_TAG)
INVALID = b'%d' % X.INVALID


def name(bucket=BUCKET, level=1, tile=1000, q=Q):
    return b'%d_%d/%d/%d' % (bucket * q, (bucket + 1) * q - 1, level, tile)


def line(id=b'8589934593', nxt=b'8589934601', dur=b'30', count=b'1', length=b'400', queue=b'0', start=b'1500000000',
         end=b'1500000030', source=SRC, mode=b'AUTO'):
    """One line's fields joined (no newline); every field is bytes and goes in as it is."""
    return b','.join([id, nxt, dur, count, length, queue, start, end, source, mode])


def good(i, source=SRC, mode=b'AUTO', stream_invalid=False):
    """An everyday row's line, different for every i."""
    nxt = b'' if stream_invalid else b'%d' % (8589934601 + 8 * i)
    return line(id=b'%d' % (8589934593 + 8 * (i % 50)), nxt=nxt, dur=b'%d' % (20 + i % 40), length=b'%d' % (100 + i),
                queue=b'%d' % (i % 3), start=b'%d' % (1500000000 + i), end=b'%d' % (1500000030 + i), source=source,
                mode=mode)


def text(lines, rules, header=True):
    """A well-formed file of the lines: what K19 writes (header=False: the reference's match-dir
    form, simple rules only)."""
    if rules == STREAM:
        return H + b''.join(b'\n' + x for x in lines)
    return (H + b'\n' if header else b'') + b''.join(x + b'\n' for x in lines)


def _fit(lines, rules, header, residue):
    """The lines with the first one's id given the digits that make the file's text `residue`
    bytes long modulo 16."""
    for digits in range(1, 20):
        first = line(id=b'1' + b'0' * (digits - 1))
        t = text([first] + lines[1:], rules, header)
        if len(t) % 16 == residue:
            return t
    raise AssertionError('no id length fits')


def cases():
    out = []

    def add(name, files, rules, q=Q, source=SRC, mode=MODE, expect=None):
        out.append({'name': name, 'files': files, 'q': q, 'rules': rules, 'source': source, 'mode': mode,
                    'expect': expect})

    # ---- alignment: 19 files of two rows, each 1 byte long modulo 16, so that the files start
    # at every residue (0, 15, 16 and 17 among the offsets' residues) and a newline sits on every
    # byte of a chunk: the simple rules' closing one at start + 0, the stream rules' first at
    # start + 117; the whole text is 1 byte long modulo 16
    for rules in (SIMPLE, STREAM):
        files = [(name(tile=100 + k), _fit([good(0), good(k + 1)], rules, k % 2 == 0, 1)) for k in range(19)]
        files[0] = (files[0][0], _fit([good(0), good(1)], rules, True, 15))   # the second file starts at 15
        files[1] = (files[1][0], _fit([good(0), good(2)], rules, False, 1))   # the third at 16
        add('align_%d' % rules, files, rules)
    # ---- a line of more than 16 x 4 bytes: the 255-byte source and mode
    long_source = bytes(33 + (i * 7) % 11 for i in range(255)).replace(b',', b'-')
    long_mode = bytes(97 + i % 26 for i in range(255))
    for rules in (SIMPLE, STREAM):
        lines = [good(i, long_source, X.upper_ascii(long_mode)) for i in range(3)]
        add('long_tag_%d' % rules, [(name(), text(lines, rules))], rules, source=long_source, mode=long_mode,
            expect=[HEADER, ROW, ROW, ROW])
    # ---- empty files first, in the middle and last
    for rules in (SIMPLE, STREAM):
        t = text([good(1), good(2)], rules)
        add('empty_files_%d' % rules, [(name(tile=1), b''), (name(tile=2), t), (name(tile=3), b''), (name(tile=4), b''),
                                       (name(tile=5), t), (name(tile=6), b'')], rules, expect=[HEADER, ROW, ROW] * 2)
    add('only_empty_files', [(name(tile=1), b''), (name(tile=2), b'')], SIMPLE, expect=[])
    add('no_files', [], STREAM, expect=[])
    # ---- a file of only H, with and without its newline (a p0 that equals H is the header
    # whatever follows it: the table's order)
    add('only_header_0', [(name(tile=1), H), (name(tile=2), H + b'\n')], SIMPLE, expect=[HEADER, HEADER])
    add('only_header_1', [(name(tile=1), H), (name(tile=2), H + b'\n')], STREAM, expect=[HEADER, HEADER, E_FIELDS])
    # ---- the line structure
    add('stream_no_header', [(name(tile=1), good(1) + b'\n' + good(2)), (name(tile=2), b'\n' + good(3)),
                             (name(tile=3), H[:-1] + b'\n' + good(4))], STREAM,
        expect=[U_HEADER, ROW, E_FIELDS, ROW, U_HEADER, ROW])
    add('stream_trailing_newline', [(name(), text([good(1)], STREAM) + b'\n')], STREAM, expect=[HEADER, ROW, E_FIELDS])
    add('simple_unterminated', [(name(tile=1), text([good(1)], SIMPLE) + good(2)),
                                (name(tile=2), text([good(3)], SIMPLE, False) + b'x')], SIMPLE,
        expect=[HEADER, ROW, U_END, ROW, E_FIELDS])
    add('simple_headerless', [(name(tile=1), text([good(1), good(2)], SIMPLE, False)),
                              (name(tile=2), text([good(3)], SIMPLE, True))], SIMPLE, expect=[ROW, ROW, HEADER, ROW])
    for rules in (SIMPLE, STREAM):
        add('header_in_the_middle_%d' % rules, [(name(), text([good(1), H, good(2), H], rules))], rules,
            expect=[HEADER, ROW, U_HEADER, ROW, U_HEADER])
        add('same_name_twice_%d' % rules, [(name(), text([good(1)], rules)), (name(tile=7), text([good(2)], rules)),
                                           (name(), text([good(3), good(4)], rules))], rules,
            expect=[HEADER, ROW, HEADER, ROW, HEADER, ROW, ROW])
    # ---- the fields: (line, status under the simple rules, under the stream rules)
    fields = [
        (good(1), ROW, ROW),
        # the members' limits and one beyond
        (line(id=b'18446744073709551615', nxt=b'18446744073709551615'), ROW, ROW),
        (line(id=b'18446744073709551616'), U_NUMBER, U_NUMBER),
        (line(nxt=b'18446744073709551616'), U_NUMBER, U_NUMBER),
        (line(dur=b'2147483647', length=b'2147483647', queue=b'2147483647'), ROW, ROW),
        (line(dur=b'-2147483648', length=b'-2147483648', queue=b'-2147483648'), ROW, ROW),
        (line(dur=b'2147483648'), U_NUMBER, U_NUMBER),
        (line(length=b'2147483648'), U_NUMBER, U_NUMBER),
        (line(queue=b'-2147483649'), U_NUMBER, U_NUMBER),
        (line(dur=b'-2147483649'), U_NUMBER, U_NUMBER),
        (line(start=b'-9223372036854775808', end=b'9223372036854775807'), ROW, ROW),
        (line(start=b'9223372036854775807', end=b'-9223372036854775808'), ROW, ROW),
        (line(start=b'-9223372036854775809'), U_NUMBER, U_NUMBER),
        (line(end=b'9223372036854775808'), U_NUMBER, U_NUMBER),
        (line(id=b'0', nxt=b'0', dur=b'0', length=b'0', queue=b'0', start=b'0', end=b'0'), ROW, ROW),
        (line(dur=b'-1', length=b'-1', queue=b'-1', start=b'-1', end=b'-1'), ROW, ROW),
        # 21 digits, and 20 digits that wrap to a small value
        (line(id=b'100000000000000000000'), U_NUMBER, U_NUMBER),
        (line(start=b'100000000000000000000'), U_NUMBER, U_NUMBER),
        (line(id=b'18446744073709551617'), U_NUMBER, U_NUMBER),
        (line(id=b'000000000000000000001'), U_NUMBER, U_NUMBER),
        # numerals Python's int() takes and K19 never writes
        (line(dur=b'-0'), U_NUMBER, U_NUMBER),
        (line(start=b'-0'), U_NUMBER, U_NUMBER),
        (line(dur=b'+1'), U_NUMBER, U_NUMBER),
        (line(id=b'+1'), U_NUMBER, U_NUMBER),
        (line(id=b'-1'), U_NUMBER, U_NUMBER),
        (line(nxt=b'-1'), U_NUMBER, U_NUMBER),
        (line(length=b'01'), U_NUMBER, U_NUMBER),
        (line(id=b'08589934593'), U_NUMBER, U_NUMBER),
        (line(queue=b'1 '), U_NUMBER, U_NUMBER),
        (line(queue=b' 1'), U_NUMBER, U_NUMBER),
        (line(length=b'1.0'), U_NUMBER, U_NUMBER),
        (line(length=b'1e3'), U_NUMBER, U_NUMBER),
        (line(end=b'1_0'), U_NUMBER, U_NUMBER),
        (line(dur=b'-'), U_NUMBER, U_NUMBER),
        (line(dur=b'--1'), U_NUMBER, U_NUMBER),
        # empty numeric fields
        (line(id=b''), U_NUMBER, U_NUMBER),
        (line(dur=b''), U_NUMBER, U_NUMBER),
        (line(length=b''), U_NUMBER, U_NUMBER),
        (line(queue=b''), U_NUMBER, U_NUMBER),
        (line(start=b''), U_NUMBER, U_NUMBER),
        (line(end=b''), U_NUMBER, U_NUMBER),
        # the next id, empty or spelled
        (line(nxt=b''), U_NEXT, ROW),
        (line(nxt=INVALID), ROW, U_NEXT),
        (line(nxt=b'%d' % (X.INVALID - 1)), ROW, ROW),
        (line(nxt=b'%d' % (X.INVALID + 1)), ROW, ROW),
        (line(nxt=b'', dur=b'x'), U_NUMBER, U_NUMBER),         # the number comes before the next id
        (line(nxt=b'', count=b'2'), U_NEXT, U_COUNT),
        # the count
        (line(count=b'2'), U_COUNT, U_COUNT),
        (line(count=b''), U_COUNT, U_COUNT),
        (line(count=b'01'), U_COUNT, U_COUNT),
        (line(count=b'2', mode=b'auto'), U_COUNT, U_COUNT),    # the count comes before the tag
        # the field count
        (b','.join(line().split(b',')[:9]), U_FIELDS, U_FIELDS),
        (line() + b',x', U_FIELDS, U_FIELDS),
        (line() + b',', U_FIELDS, U_FIELDS),
        (b'1,2', U_FIELDS, U_FIELDS),
        (b',', U_FIELDS, U_FIELDS),
        (b'8589934593', E_FIELDS, E_FIELDS),
        (b'', E_FIELDS, E_FIELDS),
        (H + b' ', U_NUMBER, U_NUMBER),                        # ten fields, the first no number
        # the tag
        (line(mode=b'auto'), U_TAG, U_TAG),
        (line(mode=b'AUTO\r'), U_TAG, U_TAG),
        (line(source=b'smpl_rprs'), U_TAG, U_TAG),
        (line(source=b'smpl_rpr'), U_TAG, U_TAG),
        (line(source=b'smpl_rprt '), U_TAG, U_TAG),
        (line(source=b'', mode=b''), U_TAG, U_TAG),
        (line(mode=b'AUT'), U_TAG, U_TAG),
        (line(mode=b'AUTOO'), U_TAG, U_TAG),
        (good(2), ROW, ROW),
    ]
    for rules in (SIMPLE, STREAM):
        add('fields_%d' % rules, [(name(), text([f[0] for f in fields], rules))], rules,
            expect=[HEADER] + [f[1 + rules] for f in fields])
    add('empty_tag', [(name(), text([line(source=b'', mode=b''), line()], SIMPLE))], SIMPLE, source=b'', mode=b'',
        expect=[HEADER, ROW, U_TAG])
    add('comma_in_source', [(name(), text([line(source=b'a,b')], SIMPLE))], SIMPLE, source=b'a,b', expect=[HEADER, U_FIELDS])
    # ---- names: (name, accepted) at q = 3600
    a = BUCKET * Q
    names = [
        (name(), True),
        (name(bucket=0, level=0, tile=0), True),
        (name(bucket=(1 << 39) - 1, level=7, tile=(1 << 22) - 1), True),
        (b'0%d_%d/1/1000' % (a, a + Q - 1), False),                 # digits that are not canonical
        (b'%d_0%d/1/1000' % (a, a + Q - 1), False),
        (b'%d_%d/01/1000' % (a, a + Q - 1), False),
        (b'%d_%d/1/01000' % (a, a + Q - 1), False),
        (b'+%d_%d/1/1000' % (a, a + Q - 1), False),
        (b'%d_%d/1/1000' % (a + 1, a + Q), False),                  # a is no multiple of q
        (b'%d_%d/1/1000' % (a, a + Q), False),                      # b off by one
        (b'%d_%d/1/1000' % (a, a + Q - 2), False),
        (name(level=8), False),
        (name(tile=4194304), False),
        (name(bucket=1 << 39), False),
        (b'dir/' + name(), False),                                  # a leading directory
        (b'/' + name(), False),
        (b'', False),
        (name() + b'/', False),
        (name() + b'.gz', False),
        (name()[:-5], False),                                       # "{a}_{b}/1": a part short
        (name().replace(b'_', b'-'), False),
        (b'18446744073709551616_18446744073709555215/1/1000', False),
    ]
    body = text([good(1), good(2)], SIMPLE)
    files = [(n, body) for n, _ in names] + [(b'dir/x', b''), (b'bad', b'\n\n')]
    expect = []
    for _, ok in names:
        expect += [HEADER, ROW, ROW] if ok else [U_NAME] * 3
    add('names', files, SIMPLE, expect=expect + [U_NAME, U_NAME])
    # the same bytes are another bucket, or no name, at another quantisation
    # (the last bucket whose name does not wrap modulo 2^64, and the first that does: refused)
    for q in (60, (1 << 31) - 1):
        top = min((1 << 39) - 1, (1 << 64) // q - 1)
        files = [(name(bucket=b, level=l, tile=t, q=q), body) for b, l, t in
                 ((0, 0, 0), (25000000, 2, 9), (top, 7, 0x3fffff), (top + 1, 7, 0x3fffff))] + [(name(), body)]
        add('names_q%d' % q, files, SIMPLE, q=q, expect=[HEADER, ROW, ROW] * 3 + [U_NAME] * 6)
    # ---- more files than one block of the per-file kernels: 3,000 files of one row
    for rules in (SIMPLE, STREAM):
        files = [(name(bucket=BUCKET + k // 1000, tile=k % 1000), text([good(k)], rules, k % 3 != 0)) for k in range(3000)]
        add('many_files_%d' % rules, files, rules)
    # ---- more lines than one block of the line kernel and more than one tile of the scans:
    # one file of 70,000 short rows, every 7th line bad, so the compaction's offsets are not the
    # identity
    for rules in (SIMPLE, STREAM):
        lines = [line(id=b'%d' % (i % 97), nxt=b'%d' % (i % 89) if i % 7 != 3 else b'x', dur=b'1', length=b'%d' % (i % 10),
                      queue=b'0', start=b'%d' % i, end=b'%d' % (i + 1), source=b's', mode=b'M') for i in range(70000)]
        add('many_lines_%d' % rules, [(name(tile=1), b''), (name(tile=2), text(lines, rules)), (name(tile=3), text(lines[:5], rules))],
            rules, source=b's', mode=b'm')
    return out
