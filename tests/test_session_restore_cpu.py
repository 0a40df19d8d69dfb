"""Restore, export and move of the session store (K17) without a GPU: the record layout against
a known answer from the Java layout, the restatement's round trip at every cut of the scripted
stream and what those cuts cover, its refusal rules, the per-record rules of
reporter_amd/csrc/otr_session_records.h run on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer (tools/recordcheck, a stand-alone program), the new structs' layouts
and otr_uuid_key."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from reporter_amd import _lib, build
from tests import formatter_ref
from tests import session_records_ref as S
from tests import sessions_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def cuts():
    return S.scripted_cuts()


def test_known_answer_from_the_java_layout():
    """DataOutputStream order and widths: writeInt, writeFloat, writeLong, then per point
    writeFloat, writeFloat, writeInt, writeLong, all big-endian."""
    snap = {'key': [77], 'point_off': [0, 1], 'max_sep': [0.0], 'last_update': [1], 'lat': [1.0], 'lon': [2.0],
            'accuracy': [3], 'time': [4]}
    key, rec_off, data = S.encode(snap)
    want = '00000001 00000000 0000000000000001 3f800000 40000000 00000003 0000000000000004'
    assert data.hex() == want.replace(' ', '')
    assert key.tolist() == [77] and rec_off.tolist() == [0, 36]


def test_round_trip_at_every_cut(cuts):
    assert len(cuts) == 2 * R.SCRIPT_CHUNKS
    for name, snap in cuts:
        key, rec_off, data = S.encode(snap)
        assert len(data) == 16 * len(snap['key']) + 20 * len(snap['time']), name
        bad = R.differing(S.decode(key, rec_off, data), snap, R.SNAPSHOT_FIELDS)
        assert not bad, (name, bad)


def test_what_the_cuts_cover(cuts):
    """Sessions of 1 and of max_points - 1 points, max_sep zero and positive; 14-15 sessions
    after a push, 6-7 after a punctuate; a 15-point session at both cuts of chunks 4 and 5."""
    cap = R.SCRIPT['max_points'] - 1
    sizes = [np.diff(snap['point_off']) for _, snap in cuts]
    assert min(s.min() for s in sizes) == 1 and max(s.max() for s in sizes) == cap
    assert any((snap['max_sep'] > 0).any() for _, snap in cuts) and any((snap['max_sep'] == 0).any() for _, snap in cuts)
    for (kind, p), snap in cuts:
        n = len(snap['key'])
        assert (14 <= n <= 15) if kind == 'push' else (6 <= n <= 7), (kind, p, n)
        assert n <= R.SCRIPT['max_sessions']
        if p in (4, 5):
            assert cap in np.diff(snap['point_off']), (kind, p)
    assert {int(x) for s in sizes for x in s} >= {1, cap}


@pytest.mark.parametrize('name', sorted(S.REFUSALS))
def test_refusals_in_the_restatement(name):
    live, snap, ms, want = S.REFUSALS[name]
    st = S.small_store(live)
    before = st.snapshot()
    assert S.restore(st, snap, ms) == want
    assert not R.differing(st.snapshot(), before, R.SNAPSHOT_FIELDS)
    if 'layout' not in name:   # the same sessions as records are refused the same way
        key, rec_off, data = S.encode(snap)
        assert S.restore_records(S.small_store(live), key, rec_off, data, ms) == want


@pytest.mark.parametrize('name', sorted(S.record_layout_cases()))
def test_record_layout_refusals_in_the_restatement(name):
    key, rec_off, data, want = S.record_layout_cases()[name]
    st = S.small_store()
    assert S.restore_records(st, key, rec_off, data, 4) == want and not st.sessions


def test_restore_merges_and_fills_to_the_brim():
    st = S.small_store((8,))
    snap = S.still_snapshot([3, 1, 2], [3, 1, 2])
    assert S.restore(st, snap, 4) == (-1, 0)          # live + given == max_sessions is accepted
    got = st.snapshot()
    assert got['key'].tolist() == [1, 2, 3, 8] and np.diff(got['point_off']).tolist() == [1, 2, 3, 1]
    assert got['max_sep'].tolist() == [1.0, 2.0, 0.0, 0.0] and got['last_update'].tolist() == [101, 102, 100, 5]
    assert S.take(st, 2, 0, False)['key'].tolist() == [2, 8] and len(st.sessions) == 4
    assert S.take(st, 2, 1, True)['key'].tolist() == [1, 3] and sorted(st.sessions) == [2, 8]
    assert not R.differing(S.take(st, 1, 0, False), st.snapshot(), R.SNAPSHOT_FIELDS)


# ---- tools/recordcheck under ASan + UBSan -------------------------------------------------------
@pytest.fixture(scope='module')
def recordcheck(tmp_path_factory):
    if not shutil.which('g++'):
        pytest.skip('no C++ compiler')
    return build.build_recordcheck(force=True, sanitize=True,
                                   out=str(tmp_path_factory.mktemp('recordcheck') / 'recordcheck_san'))


def _run_recordcheck(exe, tmp_path, rec_off, data, shift):
    path = tmp_path / 'records.bin'
    rec_off = np.asarray(rec_off, np.int64)
    with open(path, 'wb') as f:
        f.write(struct.pack('<qq', len(rec_off) - 1, len(data)))
        f.write(rec_off.astype('<i8').tobytes())
        f.write(data)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1:verify_asan_link_order=0',
               UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    p = subprocess.run([exe, str(path), str(shift)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), p.stderr[-4000:]
    return p.stdout.split('\n')


def _expected_lines(rec_off, data):
    """What recordcheck prints, from the restatement: verdicts and decoded values (floats by bits)."""
    bits = lambda f: int(np.float32(f).view(np.uint32))   # noqa: E731
    out = []
    for i in range(len(rec_off) - 1):
        if not S.record_layout_ok(rec_off, data, i):
            out.append('%d bad' % i)
            continue
        n, ms, last, pts = S.decode_record(data, int(rec_off[i]))
        out.append('%d ok %d %d %d' % (i, n, bits(ms), last))
        out += ['%d %d %d %d' % (bits(p[0]), bits(p[1]), p[2], p[3]) for p in pts]
    return out + ['']


@pytest.mark.parametrize('shift', [0, 1])
def test_recordcheck_on_the_cuts(recordcheck, cuts, tmp_path, shift):
    """Every cut's records decode to the restatement's values and encode back to their bytes; with
    shift 1 the byte buffer starts at an odd address."""
    for name, snap in cuts:
        _, rec_off, data = S.encode(snap)
        assert _run_recordcheck(recordcheck, tmp_path, rec_off, data, shift) == _expected_lines(rec_off, data), name


def test_recordcheck_on_malformed_records(recordcheck, cuts, tmp_path):
    """A truncated record, count -1, count 2^31 - 1 (16 + 20 * count overflows 32 bits to a small
    positive length), an offset past the end: each refused alone, its neighbours still decoded."""
    snap = cuts[8][1]   # after chunk 4's push: sizes 1 .. 15
    _, rec_off, data = S.encode(snap)
    n = len(rec_off) - 1
    assert n >= 4
    cases = {}
    cases['truncated'] = (rec_off.copy(), data[:-1], [n - 1])             # the last record lacks a byte
    short = rec_off.copy()
    short[-1] = short[-2] + 15                                                # shorter than a header
    cases['short'] = (short, data, [n - 1])
    for label, count in (('minus_one', -1), ('int_max', 2 ** 31 - 1), ('zero', 0)):
        d = bytearray(data)
        d[int(rec_off[1]):int(rec_off[1]) + 4] = struct.pack('>i', count)
        cases[label] = (rec_off.copy(), bytes(d), [1])
    # a count whose 16 + 20 * count is 36 in 32 bits, on a real one-point record's 36 bytes
    wrap = 2 ** 30 + 1
    assert (16 + 20 * wrap) % 2 ** 32 == 36
    one = (struct.pack('>ifq', wrap, 0.0, 7) + struct.pack('>ffiq', 1.0, 2.0, 3, 4))
    cases['wraps_to_36'] = (np.array([0, 36], np.int64), one, [0])
    past = rec_off.copy()
    past[-1] = len(data) + 20
    cases['offset_past_end'] = (past, data, [n - 1])
    back = rec_off.copy()
    back[2] = back[1] - 4
    cases['offsets_decrease'] = (back, data, [1, 2])
    for label, (off, d, bad) in cases.items():
        want = _expected_lines(off, d)
        assert [int(x.split()[0]) for x in want if x.endswith(' bad')] == bad, label
        for shift in (0, 1):
            assert _run_recordcheck(recordcheck, tmp_path, off, d, shift) == want, (label, shift)


def test_restore_struct_layouts(tmp_path):
    """ctypes mirrors of the two new structs have the C compiler's sizes and offsets."""
    if not shutil.which('gcc'):
        pytest.skip('no C compiler')
    structs = {'otr_session_records': _lib.SessionRecords, 'otr_session_restore_result': _lib.SessionRestoreResult}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "otr.h"', 'int main(void) {']
    for cname, cls in structs.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    for k in ('LAYOUT', 'KEY', 'COUNT', 'DUPLICATE', 'LIVE', 'FULL'):
        prog.append('printf("E_%s %%d\\n", OTR_RESTORE_E_%s);' % (k, k))
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
    for k in ('LAYOUT', 'KEY', 'COUNT', 'DUPLICATE', 'LIVE', 'FULL'):
        assert int(got['E_' + k]) == getattr(_lib, 'OTR_RESTORE_E_' + k) == getattr(S, 'E_' + k)
    assert sorted(_lib.RESTORE_REASONS) == [1, 2, 3, 4, 5, 6]


def test_uuid_key_is_the_formatter_hash():
    from reporter_amd import matcher as M
    for u in (b'', b'a', b'veh-000017', b'0123456789abcdef0123456789abcdef', 'zürich-車'.encode(), bytes(range(256))):
        assert M.session_key(u) == formatter_ref.uuid_hash(u), u
    assert M.session_key('zürich') == formatter_ref.uuid_hash('zürich'.encode())
