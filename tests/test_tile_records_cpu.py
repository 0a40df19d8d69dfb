"""The tile store's records without a GPU: a known answer by hand
from the Java layout, the restatement tests/tile_records_ref.py (slices, round trips, every
refusal, the map rules), the header's per-record rules on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer (tools/tilerecordcheck), the key helpers through ctypes, the struct
layouts and the exported symbols."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from oracle import tiles as T
from reporter_amd import _lib, build
from tests import tile_records_ref as X
from tests import tile_store_ref as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = X.Q


def _kat_held():
    return X.held_of([TS.reports_of([[X.KAT_A, X.KAT_B]])], Q)


def test_known_answer():
    """q = 60, one slice of two segments under start 1500000000, tile_id 8001: the key, the map
    entry and the 84 value bytes written out by hand, and A's restored row."""
    held = _kat_held()
    rec = X.export(held, Q, X.SLICE_SIZE)
    # (A ends at second 61: it also has a row in the next bucket, a second slice of one segment)
    assert rec['n_slices'] == 2 and rec['n_tiles'] == 2
    assert (int(rec['start'][0]), int(rec['tile_id'][0]), int(rec['slice'][0])) == (X.KAT_START, X.KAT_TILE, 0)
    assert (int(rec['start'][1]), int(rec['tile_id'][1]), int(rec['slice'][1])) == (X.KAT_START + 60, X.KAT_TILE, 0)
    n0 = int(rec['name_off'][1])
    assert rec['names'].tobytes()[:n0] == X.KAT_KEY and n0 == len(X.KAT_KEY)
    assert rec['map_bytes'].tobytes()[:20] == X.KAT_MAP
    assert len(X.KAT_VALUE) == 84 and rec['rec_off'].tolist() == [0, 84, 128]
    assert rec['bytes'].tobytes()[:84] == X.KAT_VALUE
    assert rec['bytes'].tobytes()[84:] == b'\0\0\0\1' + X.KAT_VALUE[4:44]
    new, out = X.restore_records(X.empty_held(), rec, Q, 16)
    a = new[0][0]
    assert (int(a['file']), int(a['duration']), int(a['start']), int(a['end'])) == (838860804195304, 3, 1500000058,
                                                                                    1500000061)
    assert int(new[0][1]['next_id']) == T.INVALID_SEGMENT_ID
    # (file, slice, position) order is the arrival order here but for A's second row, which arrived second
    assert sorted(new[0].tolist()) == sorted(held[0].tolist()) and out['n_rows'] == 3 and out['n_missing_slices'] == 0
    assert not X.records_differing(X.export(new, Q, X.SLICE_SIZE), rec)


@pytest.mark.parametrize('S', [1, 3, 64, 65])
def test_slices_and_round_trip(S):
    """Record and map counts of every file, the exact-multiple case, and restore(export(store)):
    the same flush at privacy 1 and 2 and the same export again."""
    held = X.held_of([X.case_reports(S)], Q)
    rec = X.export(held, Q, S)
    files = sorted(set(held[0]['file'].tolist()))
    per_file = {f: int((held[0]['file'] == f).sum()) for f in files}
    assert {1, max(S - 1, 1), S, S + 1, 2 * S} <= set(per_file.values())
    assert rec['n_tiles'] == len(files) and rec['n_slices'] == sum(-(-n // S) for n in per_file.values())
    entries = [X.MAP_ENTRY.unpack_from(rec['map_bytes'].tobytes(), 20 * t) for t in range(rec['n_tiles'])]
    assert [X.file_of(s, t, Q) for s, t, _ in entries] == files
    assert [v for _, _, v in entries] == [per_file[f] // S for f in files]
    counts = [struct.unpack_from('>i', rec['bytes'].tobytes(), int(o))[0] for o in rec['rec_off'][:-1]]
    assert all(1 <= c <= S for c in counts) and sum(counts) == len(held[0])
    assert np.diff(rec['rec_off']).tolist() == [4 + 40 * c for c in counts]
    # a file of exactly S (or 2 S) rows: the slice the map names has no record yet
    exact = [f for f in files if per_file[f] % S == 0]
    assert exact
    new, out = X.restore_records(X.empty_held(), rec, Q, len(held[0]))
    assert out['n_missing_slices'] == len(exact) and out['n_unreferenced_slices'] == 0
    assert out['n_rows'] == len(held[0]) and out['n_slices'] == rec['n_slices']
    assert not X.records_differing(X.export(new, Q, S), rec)
    for privacy in (1, 2):
        assert not TS.differing(X.flush_of(new, Q, privacy), X.flush_of(held, Q, privacy))
    # the three rows of the report spanning three buckets carry the same times
    three = [i for i in range(len(held[0])) if int(held[0]['id'][i]) == TS.sid(2, 310, 1)]
    assert len(three) == 3 and len({(held[1][i], held[2][i]) for i in three}) == 1
    assert len({int(held[0]['file'][i]) >> 25 for i in three}) == 3


def test_empty_store():
    rec = X.export(X.empty_held(), Q, 7)
    assert rec['n_slices'] == 0 and rec['n_tiles'] == 0 and rec['rec_off'].tolist() == [0] and rec['n_bytes'] == 0
    new, out = X.restore_records(X.empty_held(), rec, Q, 1)
    assert len(new[0]) == 0 and out['n_rows'] == 0


def test_arrival_order_within_a_file():
    """Two files whose rows interleave: each slice holds its file's rows in arrival order, which
    the flush's (id, next_id) order would break."""
    held = X.held_of([X.case_reports(3)], Q)
    rec = X.export(held, Q, 3)
    fa = X.file_of(X.T0, TS.sid(1, 300, 0) & 0x1FFFFFF, Q)
    ids = [int(r['id']) for r in held[0] if int(r['file']) == fa]
    assert ids == [TS.sid(1, 300, k) for k in (0, 2, 4)] and ids != sorted(ids, reverse=True)
    i = [k for k in range(rec['n_slices']) if X.file_of(int(rec['start'][k]), int(rec['tile_id'][k]), Q) == fa]
    segs = X.decode_slice(rec['bytes'].tobytes(), int(rec['rec_off'][i[0]]), int(rec['rec_off'][i[0] + 1]))[1]
    assert [s[0] for s in segs] == ids


CASES = X.refusal_cases()


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_refusals(case):
    name, rec, max_rows, reason, bad_slice, bad_tile = case
    with pytest.raises(X.Refused) as e:
        X.restore_records(X.empty_held(), rec, Q, max_rows)
    assert (e.value.reason, e.value.bad_slice, e.value.bad_tile) == (reason, bad_slice, bad_tile), name


def test_refusal_cases_cover_every_reason():
    assert {c[3] for c in CASES} == {X.E_LAYOUT, X.E_KEY, X.E_COUNT, X.E_SEGMENT, X.E_DUPLICATE, X.E_MAP, X.E_FULL}
    held = X.held_of([X.case_reports(3)], Q)
    snap = tuple(a.copy() for a in held)
    snap[0]['duration'][4] += 1
    snap[1][2] = -1.0
    with pytest.raises(X.Refused) as e:
        X.restore_rows(X.empty_held(), snap, Q, 1 << 20)
    assert (e.value.reason, e.value.bad_slice) == (X.E_ROW, 2)
    assert len(X.restore_rows(held, held, Q, 1 << 20)[0]) == 2 * len(held[0])
    with pytest.raises(X.Refused) as e:
        X.restore_rows(held, held, Q, 2 * len(held[0]) - 1)
    assert e.value.reason == X.E_FULL


MAPS = X.map_cases()


@pytest.mark.parametrize('case', MAPS, ids=[c[0] for c in MAPS])
def test_map_rules(case):
    name, rec, use_map, want = case
    new, out = X.restore_records(X.empty_held(), rec, Q, 1 << 20, use_map=use_map)
    assert {k: out[k] for k in want} == want, name
    assert len(new[0]) == want['n_rows']
    # what is restored is the referenced records' rows in (file, slice, position) order
    files = new[0]['file'].tolist()
    assert files == sorted(files)


# ---- the library's host helpers and ABI (no GPU call) ----------------------------------------
def test_slice_key_helpers():
    from reporter_amd import matcher as M
    for key in ((0, 0, 0), (1500000000, 8001, 0), (X.KAT_START, 0x1FFFFFF, 2147483647), (-60, -1, -2147483648),
                ((1 << 63) - 1, -(1 << 63), 7)):
        text = M.tile_slice_key(*key)
        assert text == X.slice_key(*key) and M.tile_slice_key_parse(text) == key
    assert M.tile_slice_key(1500000000, 8001, 0) == X.KAT_KEY
    for bad in (b'+1_2.0', b'01_2.0', b'1_2.', b'1_2.0 ', b' 1_2.0', b'1_02.0', b'1_2.00', b'-0_2.0', b'1_2', b'1.2_0',
                b'', b'_2.0', b'1__2.0', b'9223372036854775808_2.0', b'1_2.2147483648', b'1_2.0\0', b'1_2.0.1', b'1_-_2.0'):
        with pytest.raises(ValueError):
            M.tile_slice_key_parse(bad)
    L = _lib.lib()
    buf = ctypes.create_string_buffer(8)
    assert L.otr_tile_slice_key(1500000000, 8001, 0, buf, 8) == -1     # too small: nothing written
    assert L.otr_tile_slice_key(1, 2, 3, buf, 5) == 5 and buf.raw[:5] == b'1_2.3'


def test_struct_layouts(tmp_path):
    """ctypes mirrors of the three new structs have the C compiler's sizes and offsets."""
    if not shutil.which('gcc'):
        pytest.skip('no C compiler')
    structs = {'otr_tile_snapshot': _lib.TileSnapshot, 'otr_tile_restore_result': _lib.TileRestoreResult,
               'otr_tile_records': _lib.TileRecords}
    names = ('LAYOUT', 'KEY', 'COUNT', 'SEGMENT', 'DUPLICATE', 'MAP', 'FULL', 'ROW')
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "otr.h"', 'int main(void) {']
    for cname, cls in structs.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    for k in names:
        prog.append('printf("E_%s %%d\\n", OTR_TILE_RESTORE_E_%s);' % (k, k))
    prog.append('printf("TIMES %d\\n", OTR_TILE_STORE_TIMES); printf("NO_HOST %d\\n", OTR_TILE_SNAPSHOT_NO_HOST);')
    prog.append('return 0; }')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(prog))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got['%s.%s' % (cname, f[0])]) == getattr(cls, f[0]).offset, (cname, f[0])
    for k in names:
        assert int(got['E_' + k]) == getattr(_lib, 'OTR_TILE_RESTORE_E_' + k) == getattr(X, 'E_' + k)
    assert int(got['TIMES']) == _lib.OTR_TILE_STORE_TIMES and int(got['NO_HOST']) == _lib.OTR_TILE_SNAPSHOT_NO_HOST
    assert sorted(_lib.TILE_RESTORE_REASONS) == list(range(1, 9))


def test_new_symbols_exported():
    L = _lib.lib()
    for s in ('otr_tile_store_open_ex', 'otr_tile_store_snapshot', 'otr_tile_store_restore',
              'otr_tile_store_export_records', 'otr_tile_store_restore_records', 'otr_tile_slice_key',
              'otr_tile_slice_key_parse'):
        assert s in _lib.EXPORTS and hasattr(L, s), s


def test_no_store_refusals_without_gpu():
    """On a matcher without a tile store every new call is refused before any device call."""
    from reporter_amd import matcher as M
    m = M.Matcher()
    held = _kat_held()
    for f, a in ((m.tile_store_snapshot, ()), (m.tile_store_export_records, (3,)),
                 (m.tile_store_restore, ({'rows': held[0], 't0': held[1], 't1': held[2]},)),
                 (m.tile_store_restore_records, (X.export(held, Q, 3),))):
        with pytest.raises(ValueError, match='otr_tile_store_open'):
            f(*a)


# ---- the per-record rules on the CPU, under the sanitizers ----------------------------------
@pytest.fixture(scope='module')
def tilerecordcheck(tmp_path_factory):
    if not shutil.which('g++'):
        pytest.skip('no C++ compiler')
    return build.build_tilerecordcheck(force=True, sanitize=True,
                                       out=str(tmp_path_factory.mktemp('tilerecordcheck') / 'tilerecordcheck_san'))


def check_file(rec, q):
    n = int(rec['n_slices'])
    data = np.ascontiguousarray(rec['bytes'], np.uint8).tobytes()
    return (np.array([n, len(data), q, rec['slice_size']], np.int64).tobytes() +
            np.ascontiguousarray(rec['start'], np.int64).tobytes() + np.ascontiguousarray(rec['tile_id'], np.int64).tobytes() +
            np.ascontiguousarray(rec['slice'], np.int64).tobytes() + np.ascontiguousarray(rec['rec_off'], np.int64).tobytes() +
            data)


def check_lines(rec, q):
    """tilerecordcheck's output from the restatement."""
    out = []
    for i in range(int(rec['n_slices'])):
        reason, segs = X.record_reason(rec, i, q)
        if reason:
            out.append('%d refused %d' % (i, reason))
            continue
        out.append('%d ok %d %s' % (i, len(segs), X.slice_key(int(rec['start'][i]), int(rec['tile_id'][i]),
                                                                int(rec['slice'][i])).decode()))
        for s in segs:
            out.append('%d %d %d %d %d %d' % (s[0], s[1], struct.unpack('<Q', struct.pack('<d', s[2]))[0],
                                              struct.unpack('<Q', struct.pack('<d', s[3]))[0], s[4], s[5]))
    return out + ['']


@pytest.mark.parametrize('shift', range(8))
def test_tilerecordcheck_under_sanitizers(tilerecordcheck, tmp_path, shift):
    """The header's functions on the CPU under ASan + UBSan: the known answer, the hand-built
    cases at S = 3 and 64 and every malformed input of the refusal cases (truncated, count
    negative, count times 40 overflowing 32 bits, offsets running backwards), with the bytes at
    byte shifts 0 .. 7 in an exactly sized allocation.  The output equals the restatement's lines."""
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    inputs = [('kat', X.export(_kat_held(), Q, X.SLICE_SIZE))]
    inputs += [('cases S=%d' % S, X.export(X.held_of([X.case_reports(S)], Q), Q, S)) for S in (3, 64)]
    inputs += [(c[0], c[1]) for c in CASES if c[3] not in (X.E_MAP, X.E_FULL, X.E_DUPLICATE)]
    for name, rec in inputs:
        path = tmp_path / 'case.bin'
        path.write_bytes(check_file(rec, Q))
        p = subprocess.run([tilerecordcheck, str(path), str(shift)], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0 and not p.stderr.strip(), (name, p.stdout[-400:], p.stderr[-4000:])
        got, want = p.stdout.split('\n'), check_lines(rec, Q)
        assert len(got) == len(want), name
        for i, (a, b) in enumerate(zip(got, want)):
            assert a == b, (name, i, a[:200], b[:200])
