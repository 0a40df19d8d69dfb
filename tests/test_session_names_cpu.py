"""The session store's uuid directory (K18) without a GPU: the per-name rules of
reporter_amd/csrc/otr_session_names.h run on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer (tools/namecheck, a stand-alone program) against the restatement
tests/session_names_ref.py, the restatement's refusal cases and name order, and the new structs'
layouts."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from reporter_amd import _lib, build
from tests import session_names_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UB = N.UUID_BYTES


# ---- tools/namecheck under ASan + UBSan -----------------------------------------------------------
@pytest.fixture(scope='module')
def namecheck(tmp_path_factory):
    if not shutil.which('g++'):
        pytest.skip('no C++ compiler')
    return build.build_namecheck(force=True, sanitize=True,
                                 out=str(tmp_path_factory.mktemp('namecheck') / 'namecheck_san'))


def _run_namecheck(exe, tmp_path, uuid_bytes, rows, names, data, shift):
    """rows: (off, len); names: (off, len, row or -1, first or -1)."""
    path = tmp_path / 'names.bin'
    with open(path, 'wb') as f:
        f.write(struct.pack('<qqqq', uuid_bytes, len(rows), len(names), len(data)))
        for r in rows:
            f.write(struct.pack('<qq', *r))
        for n in names:
            f.write(struct.pack('<qqqq', *n))
        f.write(data)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1:verify_asan_link_order=0',
               UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    p = subprocess.run([exe, str(path), str(shift)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), p.stderr[-4000:]
    return p.stdout.split('\n')


def _expected(uuid_bytes, rows, names, data):
    """What namecheck prints, from the restatement."""
    raw = {'bytes': np.frombuffer(data, np.uint8), 'off': [n[0] for n in names], 'len': [n[1] for n in names],
           'n_bytes': len(data)}
    stored = [data[o:o + l] for o, l in rows]
    out = ['row %d %d 1 %s' % (r, len(s), ' '.join('%016x' % w for w in N.sort_words(s, uuid_bytes)))
           for r, s in enumerate(stored)]
    for i, (_, _, row, first) in enumerate(names):
        out.append('%d %d' % (i, N.point_reason(raw, i, uuid_bytes, stored[row] if row >= 0 else None,
                                                first if first >= 0 else None)))
    return out + ['']


def _cases(uuid_bytes):
    """(rows, names, data): names of every length of interest against rows that hold the same
    name, a name differing in the last byte only, one differing in length only; bytes >= 0x80,
    an embedded NUL; offsets that are negative or past the end; and the same compares against a
    first arrival instead of a row.  The last name ends at the last byte of the buffer."""
    lens = sorted({0, 1, 15, 16, 17, uuid_bytes} - {n for n in (15, 16, 17) if n > uuid_bytes})
    body = bytes((0x80 + 7 * i) % 256 or 1 for i in range(uuid_bytes + 1))
    parts, rows, names = [], [], []

    def put(b):
        off = sum(len(p) for p in parts)
        parts.append(b)
        return off, len(b)

    for ln in lens:
        a = body[:ln]
        same = put(a)
        rows.append(same)
        r = len(rows) - 1
        names.append(put(a) + (r, -1))                         # equal
        if ln:
            names.append(put(a[:-1] + bytes([a[-1] ^ 1])) + (r, -1))   # the last byte differs
            names.append(put(a[:-1]) + (r, -1))                # shorter: a proper prefix
        if ln < uuid_bytes:
            names.append(put(a + b'\0') + (r, -1))             # longer by a NUL: the zero padding must not match
        names.append(put(a) + (-1, -1))                        # a new key's first arrival
        f = len(names) - 1
        names.append(put(a) + (-1, f))                         # equal to it
        if ln:
            names.append(put(a[:-1] + bytes([a[-1] ^ 0x80])) + (-1, f))
    if uuid_bytes >= 5:
        rows.append(put(b'ab\0cd'))
        names.append(put(b'ab\0cd') + (len(rows) - 1, -1))
        names.append(put(b'ab\0ce') + (len(rows) - 1, -1))
        names.append(put(b'ab') + (len(rows) - 1, -1))
    long_one = put(body[:uuid_bytes + 1])                      # uuid_bytes + 1
    names.append(long_one + (0, -1))
    names.append(long_one + (-1, -1))
    f = len(names) - 1
    names.append(put(b'x') + (-1, f))                          # its first arrival is too long: not compared
    total = sum(len(p) for p in parts)
    names.append((-1, 1, 0, -1))                               # negative offset
    names.append((0, -1, 0, -1))                               # negative length
    names.append((total, 1, 0, -1))                            # starts at the end
    names.append((total - 1, 2, 0, -1))                        # runs past the end
    names.append((2 ** 62, 2 ** 31 - 1, 0, -1))                # a sum that must not wrap
    names.append((total + 5, uuid_bytes + 1, -1, -1))          # layout and length: the lower reason
    last = put(body[:3])
    names.append(last + (-1, -1))                              # ends at the buffer's last byte
    return rows, names, b''.join(parts)


@pytest.mark.parametrize('shift', [0, 1])
@pytest.mark.parametrize('uuid_bytes', [UB, 17, 1, 255])
def test_namecheck_agrees_with_the_restatement(namecheck, tmp_path, uuid_bytes, shift):
    rows, names, data = _cases(uuid_bytes)
    got = _run_namecheck(namecheck, tmp_path, uuid_bytes, rows, names, data, shift)
    want = _expected(uuid_bytes, rows, names, data)
    assert got == want
    reasons = {int(line.split()[1]) for line in want[len(rows):-1]}
    assert reasons == {0, N.E_LONG, N.E_COLLISION, N.E_LAYOUT}


# ---- the restatement --------------------------------------------------------------------------------
def test_name_order_is_byte_order():
    names = [b'', b'a', b'a\0', b'ab', b'abcdefgh1', b'abcdefgh2', b'abcdefghijklmnop1', b'abcdefghijklmnop2',
             b'abcdefgh', b'\x7f', b'\x80', b'\xff', b'b']
    items = [(nm, 1000 - i) for i, nm in enumerate(names)]
    got = N.name_order(items[::-1])
    assert [g[0] for g in got] == sorted(names)
    assert got.index((b'a', 999)) + 1 == got.index((b'a\0', 998))                  # a prefix pair
    assert got.index((b'abcdefgh1', 996)) + 1 == got.index((b'abcdefgh2', 995))    # first difference past byte 8
    assert got.index((b'abcdefghijklmnop1', 994)) + 1 == got.index((b'abcdefghijklmnop2', 993))   # past byte 16
    assert N.name_order([(b'x', 2), (b'x', 1)]) == [(b'x', 1), (b'x', 2)]            # ties by key
    # the device's (words, length, key) order is this order
    dev = sorted(items, key=lambda p: (N.sort_words(p[0], 24), len(p[0]), p[1]))
    assert dev == got
    got = N.name_order(list(zip(N.EVICT_NAMES, N.EVICT_KEYS)))
    assert [g[0] for g in got] == N.EVICT_NAMES == sorted(N.EVICT_NAMES)
    assert [g[1] for g in got] == sorted(N.EVICT_KEYS, reverse=True)


@pytest.mark.parametrize('name', sorted(N.refusal_cases()))
def test_refusals_in_the_restatement(name):
    keys, names, want = N.refusal_cases()[name]
    st = N.small_store(dict(N.STORED))
    assert st.refusal(keys, names) == want
    assert st.begin(keys, names) == want and st.names == N.STORED and not st._pending
    pts = _points(N.THEN_KEYS)
    bad, _ = st.push_named(pts, N.THEN_NAMES)
    assert bad == (-1, 0)
    assert st.names == {**N.STORED, 9: b'veh-9', 10: b'veh-10'} and len(st.sessions[10]['pts']) == 2


def _points(keys):
    from tests import sessions_ref as R
    return R.refusal_points(keys)


def test_a_name_lives_as_long_as_its_session():
    st = N.small_store({})
    st.session_gap = 10
    assert st.push_named(_points([3]), N.raw([b'first'])) == ((-1, 0), [])
    assert st.push_named(_points([3]), N.raw([b'second']))[0] == (0, N.E_COLLISION)
    st.punctuate(10 ** 6)
    assert not st.names and not st.sessions
    assert st.push_named(_points([3]), N.raw([b'second']))[0] == (-1, 0) and st.names == {3: b'second'}


def test_restore_refusals_in_the_restatement():
    from tests import session_records_ref as S
    st = N.small_store({2: b'two'})
    snap = S.still_snapshot([1, 3], [1, 1])
    assert N.restore_named(st, snap, N.raw([b'one', b'x' * (UB + 1)]), 8) == (1, N.E_NAME)
    bad_layout = N.raw([b'one', b'three'])
    bad_layout['off'][1] = 5
    assert N.restore_named(st, snap, bad_layout, 8) == (1, N.E_NAME)
    assert N.restore_named(st, S.still_snapshot([2, 3], [1, 1]), N.raw([b'x' * (UB + 1), b'three']), 8) == (0, S.E_LIVE)
    assert N.restore_named(st, snap, N.raw([b'one', b'x' * (UB + 1)]), 2) == (1, N.E_NAME)   # before full
    assert sorted(st.sessions) == [2] and st.names == {2: b'two'}
    assert N.restore_named(st, snap, N.raw([b'one', b'x' * UB]), 8) == (-1, 0)
    assert st.snapshot_names() == [b'one', b'two', b'x' * UB]
    snap0, names0 = N.take(st, 2, 0, True)
    assert snap0['key'].tolist() == [2] and names0 == [b'two'] and st.names == {1: b'one', 3: b'x' * UB}


# ---- layouts ----------------------------------------------------------------------------------------
def test_struct_layouts_against_c_header(tmp_path):
    if not shutil.which('gcc'):
        pytest.skip('no C compiler')
    structs = {'otr_session_names': _lib.SessionNames, 'otr_session_name_refusal': _lib.SessionNameRefusal,
               'otr_session_name_list': _lib.SessionNameList}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "otr.h"', 'int main(void) {']
    for cname, cls in structs.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    prog.append('printf("reasons %d %d %d %d\\n", OTR_NAME_E_LONG, OTR_NAME_E_COLLISION, OTR_NAME_E_LAYOUT, '
                'OTR_RESTORE_E_NAME);')
    prog.append('return 0; }')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(prog))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    got = dict(line.split() for line in lines[:-1])
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got['%s.%s' % (cname, f[0])]) == getattr(cls, f[0]).offset, (cname, f[0])
    assert lines[-1].split()[1:] == [str(x) for x in (_lib.OTR_NAME_E_LONG, _lib.OTR_NAME_E_COLLISION,
                                                      _lib.OTR_NAME_E_LAYOUT, _lib.OTR_RESTORE_E_NAME)]
    assert (N.E_LONG, N.E_COLLISION, N.E_LAYOUT, N.E_NAME) == (1, 2, 3, 7)


def test_pack_names_round_trip():
    names = [b'', b'abc', b'\xff\0x']
    data, off, ln = _lib.pack_names(names)
    assert data.tobytes() == b'abc\xff\0x' and off.tolist() == [0, 0, 3] and ln.tolist() == [0, 3, 3]
    r = N.raw(names)
    assert [N.name_at(r, i) for i in range(3)] == names
