"""The stream formatter (K16) on the CPU: the restatement tests/formatter_ref.py against known
answers, against Python's own JSON grammar and against the host build of the device code's
per-message functions (tools/libformatcheck.so) on the corpus and on seeded mutations of it; the
renderers' round trip; the --formatter spec parser.  No GPU call."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import formatter_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W00T = (F.KEPT, 0, b'w00t', np.float32(0.0), np.float32(0.0), 7, 1483250740)


def _fmt(name):
    return F.FORMATS[name]


def _same_result(a, b):
    return a[:3] == b[:3] and a[5:] == b[5:] and all(
        (x is None and y is None) or (x is not None and y is not None and
                                      np.float32(x).tobytes() == np.float32(y).tobytes())
        for x, y in zip(a[3:5], b[3:5]))


def test_formatter_test_java_known_answers():
    """FormatterTest.java:34 and :38."""
    assert _same_result(F.format_sv(b'2017-01-01 06:05:40|w00t||||6.5||||0.0|0.0', _fmt('psv')), W00T)
    assert _same_result(F.format_json(b'{"t":"2017-01-01 06:05:40","id":"w00t","la":0.0,"lo":0.0,"a":6.5}',
                                      _fmt('json_ymd')), W00T)


def _ymd(la='52.5', lo='13.4', t='"2017-01-01 06:05:40"', a='6.5', uid='"w00t"', more=''):
    return ('{"t":%s,"id":%s,"la":%s,"lo":%s,"a":%s%s}' % (t, uid, la, lo, a, more)).encode()


def _psv(acc='6.5', lat='52.5', lon='13.4', tm='2017-01-01 06:05:40', uid='w00t'):
    return ('%s|%s||||%s||||%s|%s' % (tm, uid, acc, lat, lon)).encode()


def test_hand_derived_rows():
    j, s = (lambda m: F.format_json(m, _fmt('json_ymd'))), (lambda m: F.format_sv(m, _fmt('psv')))
    # the last duplicate wins, a string coordinate follows the SV rule
    r = j(b'{"t":"2017-01-01 06:05:40","id":"first","la":1,"lo":2,"a":6.5,"id":"last","la":"3.5","a":7}')
    assert r[:3] == (F.KEPT, 0, b'last') and (float(r[3]), float(r[4]), r[5], r[6]) == (3.5, 2.0, 7, 1483250740)
    # Double.toString's E-notation class is unsupported, its neighbour inside [1e-3, 1e7) kept
    assert j(_ymd(la='5.0E-4'))[:2] == (F.UNSUPPORTED, F.U_NUMBER)
    assert j(_ymd(la='0.0005'))[:2] == (F.UNSUPPORTED, F.U_NUMBER)
    assert j(_ymd(la='0.001', lo='9999999.5'))[:2] == (F.KEPT, 0)
    assert j(_ymd(lo='10000000'))[:2] == (F.UNSUPPORTED, F.U_NUMBER)
    assert j(_ymd(la='1e1'))[:2] == (F.UNSUPPORTED, F.U_NUMBER)
    assert float(j(_ymd(la='"1e1"'))[3]) == 10.0
    # JSON accuracy goes through the double, SV accuracy through float
    assert j(_ymd(a='16777216.5'))[:2] == (F.UNSUPPORTED, F.U_ACCURACY)       # ceil(16777216.5) = 16777217
    assert s(_psv(acc='16777216.5'))[5] == 16777216                            # (float)16777216.5 = 16777216
    assert j(_ymd(a='16777215.5'))[5] == 16777216 and j(_ymd(a='-0.5'))[5] == 0
    assert s(_psv(acc='16777217.5'))[:2] == (F.UNSUPPORTED, F.U_ACCURACY)
    assert s(_psv(acc='x'))[:2] == (F.DROPPED, F.D_ACCURACY)
    assert j(_ymd(a='"6.5"'))[:2] == (F.UNSUPPORTED, F.U_KIND)
    # uuid: an integer token gives its text, -0 does not
    assert j(_ymd(uid='12345'))[2] == b'12345' and j(_ymd(uid='-7'))[2] == b'-7'
    assert j(_ymd(uid='-0'))[:2] == (F.UNSUPPORTED, F.U_NUMBER)
    assert j(_ymd(uid='1.5'))[:2] == (F.UNSUPPORTED, F.U_NUMBER)
    assert j(_ymd(uid='"w\\"t"'))[:2] == (F.UNSUPPORTED, F.U_ESCAPE)
    # depth 64 against 65, trailing bytes, an escaped top-level key
    assert F.format_json(F._deep(64), _fmt('json_ymd'))[:2] == (F.KEPT, 0)
    assert F.format_json(F._deep(65), _fmt('json_ymd'))[:2] == (F.UNSUPPORTED, F.U_DEPTH)
    assert j(_ymd() + b' x')[:2] == (F.UNSUPPORTED, F.U_TRAILING) and j(_ymd() + b' \n')[:2] == (F.KEPT, 0)
    assert j(_ymd(more=',"k\\u0061":1'))[:2] == (F.UNSUPPORTED, F.U_ESCAPE)
    assert j(_ymd(more=',"z":{"k\\n":1}'))[:2] == (F.KEPT, 0)
    # time: a number under a pattern is dropped, the epoch reading takes integers within int64 only
    assert j(_ymd(t='1483250740'))[:2] == (F.DROPPED, F.D_TIME)
    assert j(_ymd(t='true'))[:2] == (F.UNSUPPORTED, F.U_KIND)
    e = lambda t: F.format_json(('{"id":"u","latitude":1,"longitude":2,"timestamp":%s,"accuracy":1}' % t).encode(),
                                _fmt('json'))
    assert e('9223372036854775807')[6] == (1 << 63) - 1
    assert e('9223372036854775808')[:2] == e('1.0')[:2] == e('1e9')[:2] == (F.UNSUPPORTED, F.U_NUMBER)
    assert e('"5"')[:2] == (F.UNSUPPORTED, F.U_KIND)
    # not JSON, not an object, a missing key; a certain drop beats an unsupported reading
    assert j(b'{"a":1,}')[:2] == (F.DROPPED, F.D_JSON) and j(b'[1,2]')[:2] == (F.DROPPED, F.D_ROOT)
    assert j(b'{}')[:2] == (F.DROPPED, F.D_MISSING)
    assert j(_ymd(la='1e1', t='"2017-13-01 06:05:40"'))[:2] == (F.DROPPED, F.D_TIME)
    assert j(b'{"id":"w00t"} x')[:2] == (F.DROPPED, F.D_MISSING)
    # SV: String.split drops trailing empty fields
    assert s(b'2017-01-01 06:05:40|w00t||||6.5||||52.5|13.4|||')[:2] == (F.KEPT, 0)
    assert s(b'2017-01-01 06:05:40|w00t||||6.5||||52.5|')[:2] == (F.DROPPED, F.D_FIELDS)
    assert s(_psv(tm='2017-13-01 06:05:40'))[:2] == (F.DROPPED, F.D_TIME)
    assert s(_psv(tm='2017-01-01 06:0x:40'))[:2] == (F.DROPPED, F.D_INT)
    assert s(_psv(lat='52.123456789012345678901'))[:2] == (F.KEPT, 0)
    assert s(_psv(lat='9007199254740993.00000000000000000001'))[:2] == (F.UNSUPPORTED, F.U_PRECISION)


def test_grammar_equals_python_json():
    """On the whole corpus (and its mutations) "valid JSON" in the restatement is what
    json.loads accepts strictly, NaN and the infinities refused; with bytes after the root
    value, what raw_decode accepts up to the same end."""
    def constant(name):
        raise ValueError(name)

    dec = json.JSONDecoder(strict=True, parse_constant=constant)
    msgs = [m for name, m in F.corpus() if name.startswith('json')]
    msgs += [m for _, m in _mutations(2000, json_only=True)]
    n_valid = n_trailing = 0
    for m in msgs:
        text = m.decode('latin-1')
        valid, end = F.json_valid(m)
        start = len(text) - len(text.lstrip(' \t\n\r'))
        try:
            _, py_end = dec.raw_decode(text, start)
        except (ValueError, RecursionError):
            py_end = None
        assert valid == (py_end is not None), m
        if valid:
            assert end == py_end, m
            n_valid += 1
            n_trailing += bool(text[end:].strip(' \t\n\r'))
    assert n_valid > 100 and n_trailing > 10 and n_valid < len(msgs) - 100


def test_corpus_covers_every_reason():
    """Every status and every reason occurs, U_NO_ID excepted: the key is a bijection of the
    FNV-1a state, and no input that hashes to OTR_NO_ID is known."""
    seen = {}
    for name, m in F.corpus():
        r = F.format_message(m, _fmt(name))
        assert (r[0] == F.KEPT) == (r[1] == 0) and (r[0] == F.DROPPED) == (0 < r[1] < 32)
        seen.setdefault((name.startswith('json'), r[1]), m)
    reasons = {r for _, r in seen}
    assert reasons == {0} | (set(F.REASONS) - {F.U_NO_ID})
    sv_only, json_only = {F.D_FIELDS, F.D_ACCURACY}, {F.D_JSON, F.D_ROOT, F.D_MISSING, F.U_DEPTH, F.U_TRAILING,
                                                      F.U_ESCAPE, F.U_NUMBER, F.U_KIND}
    assert {r for is_json, r in seen if not is_json} == reasons - json_only
    assert {r for is_json, r in seen if is_json} == reasons - sv_only


def _streams(graph_dir):
    from tests import sessions_ref as R
    yield R.city_stream(graph_dir)[1]
    for p in range(R.SCRIPT_CHUNKS):
        yield R.scripted_chunk(p)[0]


def test_renderers_round_trip(graph_dir):
    """Rendered as SV and as JSON, under a pattern and as epoch seconds, the streams' points come
    back by bits."""
    n = 0
    for pts in _streams(graph_dir):
        want = F.rendered_keys(pts)
        for name in F.FORMATS:
            fmt = _fmt(name)
            msgs = (F.render_json if fmt['type'] == 'json' else F.render_sv)(pts, fmt)
            got = F.to_points([F.format_message(m, fmt) for m in msgs], pts['timestamp'])
            assert got['n_dropped'] == got['n_unsupported'] == 0, name
            for k in ('key', 'lat', 'lon', 'accuracy', 'time', 'timestamp'):
                assert got[k].dtype == want[k].dtype and got[k].tobytes() == np.asarray(want[k]).tobytes(), (name, k)
            assert got['uuid'] == [F.uuid_of_key(k) for k in pts['key']]
            n += len(msgs)
    assert n > 4000


# ---- the host build of the device code ----------------------------------------------------------
@pytest.fixture(scope='module')
def check():
    from reporter_amd import build
    lib = ctypes.CDLL(build.build_formatcheck())
    i32p, i64p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_float)
    lib.fc_format_sv.argtypes = [ctypes.c_int, ctypes.c_int, i32p, ctypes.c_char_p, ctypes.c_int64, i64p, i32p, f32p]
    lib.fc_format_json.argtypes = [ctypes.c_int, ctypes.c_char_p, i32p, ctypes.c_char_p, ctypes.c_int64, i64p, i32p,
                                   f32p]
    order = ('uuid', 'time', 'lat', 'lon', 'accuracy')   # K11's order

    def run(msg, fmt):
        o64, o32, of = (ctypes.c_int64 * 3)(), (ctypes.c_int32 * 2)(), (ctypes.c_float * 2)()
        if fmt['type'] == 'sv':
            idx = (ctypes.c_int32 * 5)(*[fmt[k + '_index'] for k in order])
            r = lib.fc_format_sv(ord(fmt['separator']), fmt['time_format'], idx, msg, len(msg), o64, o32, of)
        else:
            keys = [fmt[k + '_key'].encode() for k in order]
            klen = (ctypes.c_int32 * 5)(*[len(k) for k in keys])
            r = lib.fc_format_json(fmt['time_format'], b''.join(k.ljust(64, b'\0') for k in keys), klen, msg, len(msg),
                                   o64, o32, of)
        if r:
            return (F.DROPPED if r < 32 else F.UNSUPPORTED), r, None, None, None, None, None
        assert o64[0] % (1 << 64) == F.uuid_hash(msg[o64[1]:o64[1] + o32[0]])
        return F.KEPT, 0, msg[o64[1]:o64[1] + o32[0]], np.float32(of[0]), np.float32(of[1]), o32[1], o64[2]
    return run


def _mutations(n, json_only=False, seed=16):
    """Seeded mutations of corpus messages: byte flips, truncations, inserted quotes, braces and
    backslashes, a few of them at a time."""
    rng = np.random.RandomState(seed)
    base = [(name, m) for name, m in F.corpus() if m and (not json_only or name.startswith('json'))]
    pool = [b'"', b'{', b'}', b'[', b']', b'\\', b',', b':', b'|', b'0', b'e', b'.', b'-', b' ', b'\\u00', b'1e5']
    out = []
    for _ in range(n):
        name, m = base[rng.randint(len(base))]
        m = bytearray(m)
        for _ in range(1 + rng.randint(3)):
            kind, at = rng.randint(4), rng.randint(len(m) + 1)
            if kind == 0 and m:
                m[min(at, len(m) - 1)] = rng.randint(256) if rng.randint(2) else rng.randint(32, 127)
            elif kind == 1:
                del m[at:]
            elif kind == 2:
                m[at:at] = pool[rng.randint(len(pool))]
            elif m:
                del m[min(at, len(m) - 1)]
        out.append((name, bytes(m)))
    return out


def test_host_build_equals_restatement(check):
    """Classification, reason and kept fields identical on the corpus and on 6000 mutations."""
    cases = F.corpus() + _mutations(6000)
    counts = {}
    for name, m in cases:
        want, got = F.format_message(m, _fmt(name)), check(m, _fmt(name))
        assert _same_result(got, want), (name, m, got, want)
        counts[want[1]] = counts.get(want[1], 0) + 1
    assert counts[0] > 100 and len(counts) >= len(F.REASONS) - 1


def test_formatter_from_spec():
    from reporter_amd import matcher as M
    for name, spec in F.SPECS.items():
        assert M.formatter_from_spec(spec) == F.FORMATS[name], name
    # FormatterTest.java:18-25
    for bogus in ('%sv%,%a', '%json%a%b%c%d', 'bogus_formatter'):
        with pytest.raises(ValueError):
            M.formatter_from_spec(bogus)
    for bad, named in ((',sv,\\s+,1,9,10,0,5', '\\\\s+'), (',sv,|,1,9,10,0,5', "'|'"), (',sv,ab,1,9,10,0,5', 'ab'),
                       (',sv,;,1,9,10,0,5,HH:mm', 'HH:mm'), ('@json@id@la@lo@t@a@yyyy', 'yyyy'),
                       (',sv,;,1,9,x,0,5', 'index'), ('@json@i"d@la@lo@t@a', 'i"d')):
        with pytest.raises(ValueError) as e:
            M.formatter_from_spec(bad)
        assert named in str(e.value), (bad, str(e.value))


def test_struct_layouts(tmp_path):
    """The ctypes mirrors of the formatter's structs have the C compiler's sizes and offsets."""
    import shutil
    import subprocess
    from reporter_amd import _lib
    if not shutil.which('gcc'):
        pytest.skip('no C compiler')
    structs = {'otr_message_format': _lib.MessageFormat, 'otr_messages': _lib.Messages,
               'otr_format_result': _lib.FormatResult}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "otr.h"', 'int main(void) {']
    for cname, cls in structs.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
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
    # the reason table of the header is the restatement's and the Python names'
    hdr = open(os.path.join(ROOT, 'include', 'otr.h')).read()
    import re
    codes = {int(v) for v in re.findall(r'#define OTR_FORMAT_[DU]_[A-Z_]+ (\d+)', hdr)}
    assert codes == set(F.REASONS) == set(_lib.FORMAT_REASONS)
