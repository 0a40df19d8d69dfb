"""Tile file texts read back into rows (K21) without a GPU: what the hand-built cases of
tests/tile_parse_cases.py cover, their hand-written statuses against the restatement
tests/tile_parse_ref.py, the per-line and per-name functions and the line table of
reporter_amd/csrc/otr_tileparse.h run on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer (tools/tileparsecheck) against the restatement, the struct layouts, the
refusals that need no device, simple_reporter.read_tile_files, and a pin to the reference's
report() loop through the goldens."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from reporter_amd import _lib, build
from reporter_amd import simple_reporter as sr
from tests import tile_parse_cases as C
from tests import tile_parse_ref as P
from tests import tile_text_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = C.cases()
IDS = [c['name'] for c in CASES]
BY = {c['name']: c for c in CASES}
_WANT = {}


def want_of(case):
    """The restatement's result of a case, computed once and left unchanged."""
    if case['name'] not in _WANT:
        _WANT[case['name']] = P.parse(case)
    return _WANT[case['name']]


def test_cases_cover_what_they_claim():
    for rules in (P.SIMPLE, P.STREAM):
        text, text_off, _, _ = P.pack(BY['align_%d' % rules])
        starts = text_off[:-1].tolist()
        assert [s % 16 for s in starts[:4]] == [0, 15, 0, 1]         # offsets 0, 15, 16 and 17 modulo 16
        assert {s % 16 for s in starts} == set(range(16))
        nl = {int(p) % 16 for p in np.flatnonzero(text == 10)}
        assert nl == set(range(16))                      # a newline on every byte of a chunk, 15 and 0 among them
        assert len(text) % 16 != 0
        w = want_of(BY['align_%d' % rules])
        assert w['n_bad'] == 0 and w['n_rows'] == 38
        long = BY['long_tag_%d' % rules]
        assert min(len(x) for x in long['files'][0][1].split(b'\n') if x and x != X.HEADER) > 255 + 255 > 16 * 4
        assert [len(t) for _, t in BY['empty_files_%d' % rules]['files']] .count(0) == 4
        many = BY['many_files_%d' % rules]
        assert len(many['files']) == 3000 > 256 and want_of(many)['n_rows'] == 3000 and want_of(many)['n_bad'] == 0
        lines = want_of(BY['many_lines_%d' % rules])
        assert lines['n_lines'] > 70000 > 256 and lines['n_bad'] == 10001
        st = lines['line_status'][1:70001]
        assert (np.flatnonzero(st != P.ROW) % 7 == 3).all() and (st != P.ROW).sum() == 10000
        assert lines['row_off'].tolist() == [0, 0, 60000, 60004] and lines['first_bad'] == 4
        same = BY['same_name_twice_%d' % rules]
        assert same['files'][0][0] == same['files'][2][0] != same['files'][1][0]
    seen = set()
    for c in CASES:
        seen |= set(want_of(c)['line_status'].tolist())
    assert seen == {P.ROW, P.HEADER, P.E_FIELDS, P.U_NAME, P.U_END, P.U_HEADER, P.U_FIELDS, P.U_NUMBER, P.U_NEXT,
                    P.U_COUNT, P.U_TAG}
    text = BY['fields_0']['files'][0][1]
    for numeral in (b'18446744073709551615', b'18446744073709551616', b'2147483647', b'2147483648', b'-2147483648',
                    b'-2147483649', b'-9223372036854775808', b'-9223372036854775809', b'100000000000000000000', b'-0',
                    b'+1', b'01', b'1 ', b'1.0', b'\r\n'):
        assert numeral in text, numeral
    names = want_of(BY['names'])
    assert names['n_bad_names'] == len(BY['names']['files']) - 3 and names['file'][3] == P.NO_ID
    assert names['file'][2] == ((1 << 39) - 1) << 25 | 7 << 22 | ((1 << 22) - 1)


@pytest.mark.parametrize('case', [c for c in CASES if c['expect'] is not None],
                         ids=[c['name'] for c in CASES if c['expect'] is not None])
def test_hand_written_statuses(case):
    """The restatement gives every hand-built line the status written beside it by hand, and its
    counts, offsets and first_bad follow from those statuses."""
    w = want_of(case)
    assert w['line_status'].tolist() == case['expect']
    e = np.array(case['expect'], np.int64)
    assert w['n_rows'] == int((e == P.ROW).sum()) == len(w['rows']) and w['n_headers'] == int((e == P.HEADER).sum())
    bad = np.flatnonzero(e >= P.E_FIELDS)
    assert w['n_bad'] == len(bad) and w['first_bad'] == (int(bad[0]) if len(bad) else -1)
    assert w['first_bad_reason'] == (int(e[bad[0]]) if len(bad) else 0)
    assert w['file_line_off'][-1] == len(e) and w['row_off'][-1] == w['n_rows']
    assert (w['rows']['speed_bin'] == -1).all()
    for f in range(w['n_files']):
        assert (w['rows']['file'][w['row_off'][f]:w['row_off'][f + 1]] == w['file'][f]).all()


@pytest.fixture(scope='module')
def tileparsecheck(tmp_path_factory):
    if not shutil.which('g++'):
        pytest.skip('no C++ compiler')
    return build.build_tileparsecheck(force=True, sanitize=True,
                                      out=str(tmp_path_factory.mktemp('tileparsecheck') / 'tileparsecheck_san'))


_LINES = {}


@pytest.mark.parametrize('shift', [0, 1, 3])
def test_tileparsecheck_on_the_cases(tileparsecheck, tmp_path, shift):
    """The header's functions on the CPU under the sanitizers give the restatement's statuses,
    rows, file table and counts for every case; with shift 1 and 3 the text, the names and the
    tag are read from a misaligned address in an exactly sized allocation."""
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1:verify_asan_link_order=0',
               UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    for case in CASES:
        path = tmp_path / 'case.bin'
        path.write_bytes(P.check_file(case))
        p = subprocess.run([tileparsecheck, str(path), str(shift)], capture_output=True, text=True, env=env,
                           timeout=120)
        assert p.returncode == 0 and not p.stderr.strip(), (case['name'], p.stdout[-400:], p.stderr[-4000:])
        if case['name'] not in _LINES:
            _LINES[case['name']] = P.check_lines(case)
        got, want = p.stdout.split('\n'), _LINES[case['name']]
        assert len(got) == len(want), case['name']
        for i, (a, b) in enumerate(zip(got, want)):
            assert a == b, (case['name'], i, a[:200], b[:200])


def test_struct_layouts(tmp_path):
    """_lib.TileTexts and _lib.TileParseResult have the C compiler's sizes and offsets, and the
    status values are the header's."""
    if not shutil.which('gcc'):
        pytest.skip('no C compiler')
    structs = {'otr_tile_texts': _lib.TileTexts, 'otr_tile_parse_result': _lib.TileParseResult}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "otr.h"', 'int main(void) {']
    for cname, cls in structs.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    for k in _lib.TILE_LINE:
        prog.append('printf("%s %%d\\n", OTR_TILE_LINE_%s);' % (k, k))
    prog.append('printf("UNSUPPORTED %d\\nNO_HOST %d\\n", OTR_TILE_LINE_UNSUPPORTED, OTR_TILE_PARSE_NO_HOST);')
    prog.append('return 0; }')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(prog))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert ctypes.sizeof(_lib.TileTexts) == 4 * 8 + 2 * 4 and ctypes.sizeof(_lib.TileParseResult) == 6 * 8 + 4 * 4 + 12 * 8
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got['%s.%s' % (cname, f[0])]) == getattr(cls, f[0]).offset, (cname, f[0])
    for k, v in _lib.TILE_LINE.items():
        assert int(got[k]) == v == getattr(P, k), k
    assert int(got['UNSUPPORTED']) == _lib.OTR_TILE_LINE_UNSUPPORTED and int(got['NO_HOST']) == _lib.OTR_TILE_PARSE_NO_HOST


def test_symbol_and_refusals_before_any_device_call():
    """otr_tiles_parse is exported, and its arguments are checked before the device is touched:
    quantisation 0, unknown rules, a source or mode of 256 bytes, n_files below 0 and null arguments
    are OTR_BAD_REQUEST on a matcher without a graph."""
    from reporter_amd import matcher as M
    L = _lib.lib()
    assert hasattr(L, 'otr_tiles_parse') and 'otr_tiles_parse' in _lib.EXPORTS
    m = M.Matcher()
    text, text_off, names, name_off = P.pack(BY['simple_headerless'])
    args = dict(text=text, text_off=text_off, names=names, name_off=name_off)
    with pytest.raises(ValueError, match='quantisation'):
        m.tiles_parse(quantisation=0, **args)
    for rules in (-1, 2):
        with pytest.raises(ValueError, match='unknown rules'):
            m.tiles_parse(rules=rules, **args)
    for kw in ({'source': b'x' * 256}, {'mode': b'm' * 256}):
        with pytest.raises(ValueError, match='255 bytes'):
            m.tiles_parse(**args, **kw)
    with pytest.raises(ValueError, match='n_files'):
        m.tiles_parse(text=1, text_off=1, names=1, name_off=1, device=True, n_files=-1)
    with pytest.raises(ValueError, match='offsets'):
        m.tiles_parse(text=text, text_off=text_off, names=names, name_off=name_off[:-1])
    c, r = _lib.TileTexts(), _lib.TileParseResult()
    assert L.otr_tiles_parse(m._h, None, 60, 0, b'', b'', 0, ctypes.byref(r)) == _lib.OTR_BAD_REQUEST
    assert L.otr_tiles_parse(m._h, ctypes.byref(c), 60, 0, b'', b'', 0, None) == _lib.OTR_BAD_REQUEST
    c.n_files = 1
    assert L.otr_tiles_parse(m._h, ctypes.byref(c), 60, 0, b'', b'', 0, ctypes.byref(r)) == _lib.OTR_BAD_REQUEST


def _tiles_of_rows(rows, q=3600):
    """{name: [lines]} of rows in any order, each line written by the host formatter."""
    order = np.argsort(rows['file'], kind='stable')
    return sr.rows_to_tiles(rows[order], q, 'auto', 'smpl_rprt')


def test_read_tile_files(tmp_path):
    """report_match_dir's host half: a tree written by write_tiles, and one in the reference's
    header-less form, come back as the four arrays in sorted order with the directory stripped,
    and the restatement reads every line of them as the row that wrote it."""
    rows = np.concatenate([X.plain_rows(40, [X.file_of(416666 + i % 3, i % 2, 7 + i % 5) for i in range(40)], seed=3)])
    tiles = _tiles_of_rows(rows)
    assert len(tiles) > 5
    with_header, without = tmp_path / 'with', tmp_path / 'without'
    sr.write_tiles(tiles, str(with_header))
    for key, lines in tiles.items():                      # simple_reporter.py:199-206: appended lines, no column line
        os.makedirs(os.path.dirname(str(without / key)), exist_ok=True)
        with open(str(without / key), 'a') as f:
            f.write(''.join(lines))
    for root, header in ((with_header, True), (without, False)):
        text, text_off, names, name_off = sr.read_tile_files(str(root))
        got_names = [names[a:b].tobytes().decode() for a, b in zip(name_off[:-1], name_off[1:])]
        assert got_names == sorted(tiles, key=lambda k: k.split('/')) and text_off[0] == 0 == name_off[0]
        files = []
        for f, key in enumerate(got_names):
            body = text[text_off[f]:text_off[f + 1]].tobytes()
            assert body == ((sr.COLUMNS + '\n') if header else '').encode() + ''.join(tiles[key]).encode()
            files.append((key.encode(), body))
        w = P.parse({'files': files, 'q': 3600, 'rules': P.SIMPLE, 'source': b'smpl_rprt', 'mode': b'auto'})
        assert w['n_bad'] == 0 and w['n_bad_names'] == 0 and w['n_rows'] == len(rows)
        assert w['n_headers'] == (len(tiles) if header else 0)
        assert _tiles_of_rows(w['rows']) == tiles
    # an empty directory, and names the parser will refuse, pass through as they are
    empty = tmp_path / 'empty'
    empty.mkdir()
    text, text_off, names, name_off = sr.read_tile_files(str(empty))
    assert len(text) == len(names) == 0 and text_off.tolist() == [0] == name_off.tolist()


def test_pinned_to_the_reference_loop():
    """The pin to the reference, through the goldens.  tests/golden/cull_cases.json holds lines of
    three and four fields, which no row can express (every one is U_FIELDS: checked here), so the
    files are built by bucket() from the reports of tests/golden/report_cases.json, whose lines
    are canonical.  ''.join(cull(sorted(lines), p)) is what the reference's report() loop writes
    for a file (tests/test_golden_report.py pins cull to it); it must equal the re-rendered rows
    the restatement parsed from the file, sorted and culled the same way."""
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, 'golden', 'cull_cases.json')) as f:
        plain = [l for c in json.load(f)['cases'] for l in c['lines']]
    w = P.parse({'files': [(C.name(), ''.join(plain).encode())], 'q': 3600, 'rules': P.SIMPLE, 'source': b's',
                 'mode': b'm'})
    assert len(plain) > 1000 and set(w['line_status'].tolist()) == {P.U_FIELDS}
    with open(os.path.join(here, 'golden', 'report_cases.json')) as f:
        cases = json.load(f)['cases']
    tiles = {}
    for c in cases:
        times = [p['time'] for p in c['trace']]
        reports = (c['expected'].get('datastore') or {}).get('reports') or []
        for key, lines in sr.bucket(int(min(times)), int(max(times)), reports, 3600, 'auto', 'smpl_rprt').items():
            tiles.setdefault(key, []).extend(lines)
    assert len(tiles) > 50 and sum(len(v) for v in tiles.values()) > 90
    # (most of these files hold one line: every line once more in one file of its own, where the
    # cull meets runs of all lengths; a row's file comes from the name alone)
    tiles[C.name().decode()] = [l for v in tiles.values() for l in v]
    files = [(k.encode(), ''.join(v).encode()) for k, v in sorted(tiles.items())]
    w = P.parse({'files': files, 'q': 3600, 'rules': P.SIMPLE, 'source': b'smpl_rprt', 'mode': b'auto'})
    assert w['n_bad'] == 0 and w['n_bad_names'] == 0 and w['n_headers'] == 0
    assert w['n_rows'] == sum(len(v) for v in tiles.values())
    tag = X.tag_of(b'smpl_rprt', b'auto', P.SIMPLE)
    differs = 0
    for f, (key, _) in enumerate(files):
        again = [X.row_bytes(r, P.SIMPLE, tag).decode() for r in w['rows'][w['row_off'][f]:w['row_off'][f + 1]]]
        for privacy in (1, 2, 3):
            want = ''.join(sr.cull(sorted(tiles[key.decode()]), privacy))
            assert ''.join(sr.cull(sorted(again), privacy)) == want, (key, privacy)
            differs += want != ''.join(sorted(again))
    assert differs > 0          # the cull deleted something somewhere: the pin is not vacuous
