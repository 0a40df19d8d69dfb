"""The tile file texts (K19) without a GPU: the restatement tests/tile_text_ref.py against the
library's host formatter otr_tiles_format and simple_reporter's host payloads, the per-row and
per-file functions of reporter_amd/csrc/otr_tiletext.h run on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer (tools/tiletextcheck), the struct layout, the exported symbols and the
refusals that need no device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from reporter_amd import _lib, build
from reporter_amd import simple_reporter as sr
from tests import tile_text_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = X.cases()
IDS = [c['name'] for c in CASES]


def _tiles_format(rows, source, mode, rules):
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    L = _lib.lib()
    rc = L.otr_tiles_format(rows.ctypes.data if len(rows) else None, len(rows), source, mode, rules,
                            ctypes.byref(out), ctypes.byref(n))
    assert rc == 0, _lib.last_error()
    got = ctypes.string_at(out.value, n.value) if out.value else b''
    if out.value:
        L.otr_free(out.value)
    return got


def test_cases_cover_what_they_claim():
    by = {c['name']: c for c in CASES}
    assert [len(by['one_file_%d' % n]['rows']) for n in (0, 1, 2, 255, 256, 257, 513)] == [0, 1, 2, 255, 256, 257, 513]
    assert X.build(by['own_file_513']['rows'], 3600, X.STREAM, b's', b'm')['n_files'] == 513
    for at in (255, 256, 257):
        assert X.build(by['second_file_at_%d' % at]['rows'], 60, 0, b'', b'')['row_off'].tolist() == [0, at, 300]
    e = by['extremes']['rows']
    for k, lo, hi in (('duration', X.I32_MIN, X.I32_MAX), ('length', X.I32_MIN, X.I32_MAX),
                      ('queue_length', X.I32_MIN, X.I32_MAX), ('start', X.I64_MIN, X.I64_MAX),
                      ('end', X.I64_MIN, X.I64_MAX)):
        assert {lo, -1, 0, hi} <= set(e[k].tolist()), k
    assert {0, X.M64} <= set(e['id'].tolist()) and {X.INVALID, X.INVALID - 1} <= set(e['next_id'].tolist())
    for k, top in (('id', 19), ('next_id', 19), ('start', 18), ('end', 18), ('duration', 9), ('length', 9),
                   ('queue_length', 9)):
        have = set(e[k].tolist())
        assert all(10 ** p in have and 10 ** p - 1 in have for p in range(1, top + 1)), k
    # the span starts of the second block (row 256) of the alignment sweep hit every residue
    for rules, shift in ((X.STREAM, 0), (X.SIMPLE, 4)):
        for k in range(16):
            c = by['source_%d' % k]
            assert len(c['source']) == k and len(c['rows']) == 300
            assert X.span_start(c['rows'], 256, rules, c['source'], c['mode']) % 16 == (k + shift) % 16
    # a block's span of the longest rows (158 KB) is more than six of the emit kernel's staging
    # windows (256 * 96 bytes) and within a header of all the LDS a CU has
    lo = by['longest_lower']
    w = X.build(lo['rows'], 3600, X.STREAM, lo['source'], lo['mode'])
    assert min(w['row_len']) == max(w['row_len']) == 1 + 121 + 512 and sum(w['row_len'][:256]) > 6 * 256 * 96
    assert X.build(by['file_recurs']['rows'], 3600, 0, b'', b'')['n_files'] == 4
    assert any(X.name_wraps(f, c['q']) for c in CASES for f in c['rows']['file'])
    lg = by['names_longest']
    w = X.build(lg['rows'], lg['q'], 0, b'', b'')
    assert w['n_files'] == 5 and np.diff(w['name_off']).tolist() == [51] * 5


@pytest.mark.parametrize('case', CASES, ids=IDS)
@pytest.mark.parametrize('rules', [X.SIMPLE, X.STREAM])
def test_rows_equal_tiles_format(case, rules):
    """The restatement's per-row bytes are otr_tiles_format's for the same rows."""
    tag = X.tag_of(case['source'], case['mode'], rules)
    want = b''.join(X.row_bytes(r, rules, tag) for r in case['rows'])
    assert _tiles_format(case['rows'], case['source'], case['mode'], rules) == want
    w = X.build(case['rows'], case['q'], rules, case['source'], case['mode'])
    assert sum(w['row_len']) == len(want)
    assert w['n_text_bytes'] == len(want) + w['n_files'] * (len(X.HEADER) + (0 if rules == X.STREAM else 1))


def _host_comparable(case, w):
    """The host paths key their dicts by name and compute names in Python integers."""
    names = [w['names'].tobytes()[a:b] for a, b in zip(w['name_off'][:-1], w['name_off'][1:])]
    return len(set(names)) == len(names) and not any(X.name_wraps(f, case['q']) for f in w['file'])


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_texts_equal_host_payloads(case):
    """File texts and names equal what the host builds from the same rows: stream_tile_payloads
    (stream rules) and rows_to_tiles under the column line as write_tiles writes it (simple)."""
    source, mode = case['source'].decode('latin-1'), case['mode'].decode('latin-1')
    for rules in (X.SIMPLE, X.STREAM):
        w = X.build(case['rows'], case['q'], rules, case['source'], case['mode'])
        if not _host_comparable(case, w):
            assert case['name'] in ('file_recurs',) or case['name'].startswith('names_')
            continue
        got = sr.text_payloads(w)
        if rules == X.STREAM:
            flush = {'rows': case['rows'], 'n_files': w['n_files'], 'file': w['file'], 'row_off': w['row_off'],
                     'quantisation': case['q']}
            want = sr.stream_tile_payloads(flush, mode, source)
        else:
            tiles = sr.rows_to_tiles(case['rows'], case['q'], mode, source, rules=rules)
            want = {k: sr.COLUMNS + '\n' + ''.join(v) for k, v in tiles.items()}
        assert got == want


def test_names_equal_file_key():
    n = 0
    for case in CASES:
        for f in set(case['rows']['file'].tolist()):
            if not X.name_wraps(f, case['q']):
                assert X.name_of(f, case['q']).decode() == sr.file_key(f, case['q'])
                n += 1
    assert n > 500
    # the wrap rule on the largest bucket: 2^39 * q - 1 modulo 2^64
    f, q = X.file_of((1 << 39) - 1, 7, 0x3fffff), (1 << 31) - 1
    assert X.name_of(f, q) == b'%d_%d/7/4194303' % ((((1 << 39) - 1) * q) % (1 << 64), ((1 << 39) * q - 1) % (1 << 64))


@pytest.fixture(scope='module')
def tiletextcheck(tmp_path_factory):
    if not shutil.which('g++'):
        pytest.skip('no C++ compiler')
    return build.build_tiletextcheck(force=True, sanitize=True,
                                     out=str(tmp_path_factory.mktemp('tiletextcheck') / 'tiletextcheck_san'))


@pytest.mark.parametrize('shift', [0, 1])
def test_tiletextcheck_on_the_cases(tiletextcheck, tmp_path, shift):
    """The header's functions on the CPU under the sanitizers give the restatement's lengths,
    offsets, names and bytes for both rule sets; with shift 1 the rows are read from, and every
    text and name is written to, an odd address in an exactly sized allocation."""
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1:verify_asan_link_order=0',
               UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    for case in CASES:
        path = tmp_path / 'case.bin'
        path.write_bytes(X.check_file(case))
        p = subprocess.run([tiletextcheck, str(path), str(shift)], capture_output=True, text=True, env=env,
                           timeout=120)
        assert p.returncode == 0 and not p.stderr.strip(), (case['name'], p.stdout[-400:], p.stderr[-4000:])
        got, want = p.stdout.split('\n'), X.check_lines(case)
        assert len(got) == len(want), case['name']
        for i, (a, b) in enumerate(zip(got, want)):
            assert a == b, (case['name'], i, a[:200], b[:200])


def test_text_result_layout(tmp_path):
    """_lib.TileTextResult has the C compiler's size and offsets of otr_tile_text_result."""
    if not shutil.which('gcc'):
        pytest.skip('no C compiler')
    cname, cls = 'otr_tile_text_result', _lib.TileTextResult
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "otr.h"', 'int main(void) {',
            'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for f in cls._fields_:
        prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    prog.append('printf("no_host %d\\n", OTR_TILE_TEXT_NO_HOST);')
    prog.append('return 0; }')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(prog))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls) == 3 * 8 + 4 * 4 + 12 * 8
    for f in cls._fields_:
        assert int(got['%s.%s' % (cname, f[0])]) == getattr(cls, f[0]).offset, f[0]
    assert int(got['no_host']) == _lib.OTR_TILE_TEXT_NO_HOST


def test_symbols_exported():
    L = _lib.lib()
    assert hasattr(L, 'otr_tile_store_flush_text')
    assert hasattr(L, 'otr_tiles_text')
    assert {'otr_tile_store_flush_text', 'otr_tiles_text'} <= set(_lib.EXPORTS)


def test_refusals_before_any_device_call():
    """Arguments are checked before the device is touched: a source or mode of 256 bytes,
    quantisation 0 and unknown rules are OTR_BAD_REQUEST on a matcher without a graph."""
    from reporter_amd import matcher as M
    m = M.Matcher()
    rows = X.plain_rows(3, [5, 5, 6])
    for kw in ({'source': b'x' * 256}, {'mode': b'm' * 256}):
        with pytest.raises(ValueError, match='255 bytes'):
            m.tiles_text(rows, **kw)
        with pytest.raises(ValueError, match='255 bytes'):
            m.tile_store_flush_text(**kw)
    with pytest.raises(ValueError, match='quantisation'):
        m.tiles_text(rows, quantisation=0)
    for rules in (-1, 2, 7):
        with pytest.raises(ValueError, match='unknown rules'):
            m.tiles_text(rows, rules=rules)
    with pytest.raises(ValueError, match='otr_tile_store_open'):
        m.tile_store_flush_text()                         # 255 bytes pass; there is no store
    L = _lib.lib()
    r = _lib.TileTextResult()
    assert L.otr_tiles_text(m._h, None, 1, 0, 60, 0, b'', b'', 0, ctypes.byref(r)) == _lib.OTR_BAD_REQUEST
    assert L.otr_tiles_text(m._h, None, 0, 0, 60, 0, b'', b'', 0, None) == _lib.OTR_BAD_REQUEST
