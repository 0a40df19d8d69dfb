"""The numerals and texts of tests/ingest_cases.py reach what they are named for (CPU only).
Requirements on the inputs of tests/test_gpu_ingest_edges.py: when a numeral or a text changes,
this file says which branch or edge the GPU tests lost.  The numerals: every tag is met as often
as ingest_cases.REQUIRED says, the main corpus holds nothing that is predicted refused, and for
every numeral the restatement, Python (float(), oracle.ingest.py2_str_float) and the host build of
the device parsers (reporter_amd/tools/libparsecheck.so) agree bit for bit.  The texts: the
oracle's output has the property each case is named for."""
import ctypes
import math
import struct

import numpy as np
import pytest

from oracle import ingest as oi
from tests import ingest_cases as ic


@pytest.fixture(scope='module')
def pc():
    from reporter_amd import build
    lib = ctypes.CDLL(build.build_parsecheck())
    lib.pc_float.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)]
    lib.pc_py2_str.argtypes = lib.pc_float.argtypes
    return lib


def _bits(x):
    return struct.unpack('<Q', struct.pack('<d', x))[0]


def _host(f, s):
    out = ctypes.c_double()
    b = s.encode('latin-1')
    rc = f(b, len(b), ctypes.byref(out))
    return rc, _bits(out.value)


# ---- numerals ----------------------------------------------------------------------------------------
def test_tag_counts():
    got = ic.tag_counts()
    print({t: got.get(t, 0) for t in sorted(set(got) | set(ic.REQUIRED))})
    short = {t: (got.get(t, 0), n) for t, n in ic.REQUIRED.items() if got.get(t, 0) < n}
    assert not short, short
    # branches no decimal is known to reach (the module's docstring says why): pinned at zero, so
    # that a numeral that does reach one is noticed
    assert {t: got.get(t, 0) for t in ic.UNREACHED} == {t: 0 for t in ic.UNREACHED}


def test_lists_and_their_sizes():
    n = ic.numerals()
    assert 1000 < len(n['main']) <= ic.MAX_CORPUS and len(set(n['main'])) == len(n['main'])
    assert n['main'] == ic.numerals.__wrapped__()['main']      # deterministic from its seeds
    assert len(n['refused']) >= 8 and len(n['py2_refused']) >= 2 and len(n['non_finite']) + len(n['in_texts']) >= 4
    assert len(n['refused']) + len(n['py2_refused']) + len(n['rejected']) + len(n['non_finite']) <= 26
    assert set(n['rejected']) == {'1e', '.', 'e5', '1e+', '0x10', '', '--1', '1.2.3', '1_0', 'inf', 'nan', '1e5x'}
    for s in ('+.5', '1.', '00000.000001', '1E5', '\t12\x0b', '1e0000000005', '1e-9999999', '9007199254740993',
              '5e-324', '4e-320', '2.4703282292062328e-324', '2.47e-324', '2.2250738585072011e-308', '1e-342', '0e999',
              '-0.0', '9007199254740991.5', '%de22' % (1 << 53), '%de-22' % (1 << 53), '%de0' % ((1 << 53) - 1)):
        assert s in n['main'], s
    for s in ('1e309', '1.7976931348623159e308'):
        assert s in n['non_finite']
    assert '9007199254740993.00000000000000000001' in n['refused']
    assert '1.' + '0' * 15 + '1110223024625156540423631668090820312' + '5' in n['refused']   # 1 + 2^-53
    for s in n['tie_outside']:
        d = ic.parse_dec(s.encode())
        assert d[1].bit_length() == 54 and d[1] & 1 and d[2] in (-6, -5, 24, 25) and not d[3]
        assert not ic.classify(s)[1] & {'tie_even', 'tie_odd', 'clinger_mul', 'clinger_div'}
    # the signs of zero, and both directions under the smallest subnormal
    assert _bits(float('-0.0')) == ic.classify('-0.0')[0] == 1 << 63 and ic.classify('0e999')[0] == 0
    assert ic.classify('2.4703282292062328e-324')[0] == 1 and ic.classify('2.47e-324')[0] == 0


def test_main_corpus_has_no_predicted_refusal():
    for s in ic.numerals()['main']:
        b, tags = ic.classify(s)
        b2, tags2 = ic.classify_py2(s)
        assert b is not None and b2 is not None and math.isfinite(float(s)), (s, tags, tags2)
        assert not (tags | tags2) & {'reject', 'inexact_refuse', 'py2_refuse', 'giveup', 'inf'}, s


def test_restatement_python_and_host_build_agree(pc):
    n = ic.numerals()
    for name in ('main', 'refused', 'py2_refused', 'non_finite', 'in_texts'):
        for s in n[name]:
            want = _bits(float(s))
            b, tags = ic.classify(s)
            rc, got = _host(pc.pc_float, s)
            assert rc == (2 if b is None else 0), (s, tags)
            if b is None:
                assert ic.digits(s) > 19 and name == 'refused' and 'inexact_refuse' in tags, s
                continue
            assert b == want == got, (s, tags, hex(b), hex(want), hex(got))
            if not math.isfinite(float(s)):
                assert name in ('non_finite', 'in_texts') and 'inf' in tags
                continue
            want2 = _bits(float(oi.py2_str_float(float(s))))
            b2, tags2 = ic.classify_py2(s)
            rc, got2 = _host(pc.pc_py2_str, s)
            assert rc == (2 if b2 is None else 0), (s, tags2)
            if b2 is None:
                assert name == 'py2_refused' and 'py2_refuse' in tags2 and ic.digits(s) <= 19, s
                continue
            assert b2 == want2 == got2, (s, tags2, hex(b2), hex(want2), hex(got2))
    for s in n['refused'] + n['py2_refused']:
        assert ic.classify_py2(s)[0] is None
    for s in n['py2_refused']:
        assert ic.classify(s)[0] is not None      # refused under the RAW rules alone


def test_grammar(pc):
    n = ic.numerals()
    for s in n['rejected']:
        assert ic.classify(s) == (None, {'reject'}) and _host(pc.pc_float, s)[0] == 1, s
        with pytest.raises(ValueError):
            oi._py2_float(s)
    for s in ic.GRAMMAR_ACCEPTED + ic._exp_long():
        assert s in n['main'] and _host(pc.pc_float, s) == (0, _bits(float(s))), s
    assert [float(s) for s in ic._exp_long()] == [1.0, -100.0, 0.01]
    assert sum('exp_long' in ic.classify(s)[1] for s in ic._exp_long()) == 3


# ---- texts -------------------------------------------------------------------------------------------
def _exp(name):
    return ic.cases()[name].expected()


def _counts(name):
    e = _exp(name)
    return e['n_lines'], e['n_kept'], e['n_uuids'], e['n_traces'], e['n_probes']


def test_chunk_and_line_edges():
    text = ic.cases()['newline_lanes'].text
    nl = ic.nl_positions(text)
    assert {p % 16 for p in nl} == set(range(16))
    assert any(p % 16 == 15 and p + 1 < len(text) for p in nl)      # a line that starts on byte 0
    per_chunk = np.bincount(np.array(nl) // 16, minlength=(len(text) + 15) // 16)
    assert set(per_chunk.tolist()) == {0, 1, 2}
    assert _exp('newline_lanes')['n_probes'] == len(nl) == 22
    for r in (0, 1, 15):
        a, b = ic.cases()['len_%d_nl' % r].text, ic.cases()['len_%d_open' % r].text
        assert len(a) % 16 == len(b) % 16 == r and a.endswith(b'\n') and not b.endswith(b'\n')
        assert _counts('len_%d_nl' % r) == _counts('len_%d_open' % r) == (3, 3, 2, 1, 2)
    assert ic.cases()['crlf'].text.count(b'\r\n') == 4 and _counts('crlf') == (4, 4, 2, 2, 4)
    assert _counts('crlf_raw') == (4, 4, 1, 1, 4)
    assert len(ic.UUID300) == 300 and sorted(map(len, _exp('uuid_300')['soa'][0])) == [299, 300]
    for n in (1, 2, 255, 256, 257, 513):
        e = _exp('lines_%d' % n)
        assert e['n_lines'] == n and ic.cases()['lines_%d' % n].text.endswith(b'\n') == (n % 2 == 0)
        assert e['n_probes'] == (n if n > 2 else 0)
    assert _exp('newline_only') == {'error': 'line 0: fields', 'line': 0, 'reason': 'fields'}


def test_reuse_sequence_has_newlines_in_the_padding():
    long1, short1, long2, short2 = ic.reuse_sequence()
    for lng, sht in ((long1, short1), (long2, short2)):
        n = len(sht.text)
        assert n % 16 and len(lng.text) > 16 * ((n + 15) // 16)
        assert lng.text[n:16 * ((n + 15) // 16)] == b'\n' * (16 - n % 16)
        assert 'error' not in sht.expected() and sht.expected()['n_lines'] == 3
    assert 'error' not in long1.expected() and long2.expected()['error'] == 'line 3: fields'
    assert len(short1.text) % 16 == 15 and len(short2.text) % 16 == 3


def test_groups_and_order():
    c = ic.cases()['groups']
    e = c.expected()
    uuids = e['soa'][0]
    first = []
    for u in uuids:
        if u not in first:
            first.append(u)
    assert first == ['aa', 'A', 'a', '', 'a ', ic.UUID300, 'neg', 'z']     # first appearance, byte-exact names
    win = dict((u, p) for u, p in e['windows'] if u == 'a')['a']
    same = [p for p in win if p[2] == 100]
    assert len(same) == 4 and [p[0] for p in same] == [40.25, 43.25, 46.25, 49.25]   # file order under equal times
    times = [int(x.split(b',')[1]) for x in c.text.split(b'\n')[:30]]
    assert times == sorted(times, reverse=True)
    neg = [[p[2] for p in pts] for u, pts in e['windows'] if u == 'neg']
    assert neg == [[-301, -300], [-7, -5, 3]]
    z = [[p[2] for p in pts] for u, pts in e['windows'] if u == 'z']
    assert z == [[-2 ** 63, -2 ** 63 + 1], [2 ** 63 - 2, 2 ** 63 - 1]]
    # an int64 gap between them wraps to -3: no split, one window of four
    assert ((2 ** 63 - 2) - (-2 ** 63 + 1) + 2 ** 63) % 2 ** 64 - 2 ** 63 < 0


def test_windows():
    e = _exp('gap_at_limit')
    assert [(u, [p[2] for p in pts]) for u, pts in e['windows']] == [('a', [10, 130, 250]), ('b', [10, 11]),
                                                                     ('b', [132, 133])]
    assert ic.cases()['gap_at_limit'].inactivity == 120
    e = _exp('gap_at_limit_0')
    assert [[p[2] for p in pts] for _, pts in e['windows']] == [[5, 5, 5], [6, 6], [9, 9]]
    e = _exp('lone_windows')
    assert [(u, [p[2] for p in pts]) for u, pts in e['windows']] == [
        ('s', [1000, 1001]), ('m', [0, 1]), ('m', [1000, 1001]), ('e', [0, 1]), ('k', [7, 8])]
    assert e['n_uuids'] == 5 and e['n_kept'] - e['n_probes'] == 6
    assert _counts('all_dropped') == (6, 6, 3, 0, 0)
    assert [u for u, _ in _exp('last_kept')['windows']] == ['b'] and _counts('last_kept')[1] == 4
    assert [(u, len(p)) for u, p in _exp('last_dropped')['windows']] == [('a', 2), ('b', 2)]
    assert _counts('last_dropped')[1] == 5


def test_fields():
    assert _exp('shard_4_fields')['error'] == _exp('shard_6_fields')['error'] == 'line 1: fields'
    e = _exp('shard_blanks')
    assert e['soa'][0] == ['a', 'b '] and e['soa'][4].tolist() == [1, 2, 3, 4]
    assert e['soa'][2].tolist() == [1.5, 1.75, 1.0, 1.0] and e['soa'][3].tolist() == [2.5, -2.5, 2.0, 2.0]
    for rules in (ic.RAW, ic.JAVA):
        for sep in (59, 9):
            c = ic.cases()['%s_idx_sep_%d' % (rules, sep)]
            assert c.idx == (3, 4, 0, 2, 1) and c.text.count(bytes([sep])) >= 16 and b'|' not in c.text
            assert c.expected()['soa'][0] == ['u', 'v'] and c.expected()['soa'][4].tolist() == [5, 7, 6, 8]
        assert ic.cases()['%s_uuid_index_40' % rules].idx[0] == 40
        assert _exp('%s_uuid_index_40' % rules)['soa'][0] == ['u', 'w']
        assert _exp('%s_index_at_count' % rules)['error'] == 'line 1: fields'
    assert _exp('raw_trailing_uuid')['soa'][0] == [''] and _exp('java_trailing_uuid')['error'] == 'line 0: fields'
    assert _exp('raw_trailing_accuracy')['error'] == 'line 1: accuracy'
    assert _exp('java_trailing_accuracy')['error'] == 'line 1: fields'


def test_bbox():
    c = ic.cases()['bbox_edges']
    e = c.expected()
    assert (e['n_lines'], e['n_kept']) == (8, 3)
    assert e['soa'][2].tolist() == [10.5, 30.75, 20.0] and e['soa'][3].tolist()[:2] == [20.25, 40.125]
    assert e['soa'][3][2] == 30.1234567890 and e['soa'][2][2] != float('20.000000000000004')   # the str() round trip
    lines = c.text.split(b'\n')
    assert math.nextafter(float(lines[2].split(b'|')[9]), 11.0) == ic.BBOX[0]
    assert math.nextafter(float(lines[3].split(b'|')[10]), 0.0) == ic.BBOX[3]
    # the skipped lines are wrong beyond their coordinates: without the bbox the first of them ends the ingest
    with pytest.raises(oi.IngestError) as err:
        oi.raw_to_shard_text(c.text)
    assert (err.value.line, err.value.reason) == (4, 'int')
    assert _exp('bbox_bad_latitude')['error'] == 'line 4: float'
    assert _exp('bbox_none_overflow')['error'] == 'line 2: float' and ic.cases()['bbox_none_overflow'].bbox is None
    assert b'1e400' in lines[5] and b'1e400' in ic.cases()['bbox_none_overflow'].text


def test_accuracy():
    assert _exp('shard_acc_kept')['soa'][5].tolist() == [16777216, -16777216, 0, 0, 7, 12]
    assert _exp('shard_acc_over')['error'] == _exp('shard_acc_under')['error'] == 'line 1: accuracy'
    assert _exp('shard_acc_2_63')['error'] == 'line 1: int'
    acc = _exp('raw_acc_kept')['soa'][5]
    assert acc.tolist() == [0, 1000, 1000, 1000, -16777216, 999, 1000, 1, 0, 1000, 1000]
    assert not np.signbit(acc).any() or acc.tolist()[4] < 0
    for name, line in (('raw_acc_under', 1), ('raw_acc_inf', 2), ('raw_acc_overflow', 1), ('java_acc_over', 1),
                       ('java_acc_3e9', 1), ('java_acc_minus_3e9', 0)):
        assert _exp(name)['error'] == 'line %d: accuracy' % line
    assert _exp('java_acc_kept')['soa'][5].tolist() == [16777216, -16777216, 0, 7, 16777216, 0]


def test_time():
    e = _exp('ymdhms_accepted')
    t0 = 1483250740      # 2017-01-01 06:05:40
    want = [t0, t0 + 1, t0 - 86400, t0 + 44 * 86400, t0 + 93 * 3600, t0 - 6 * 86400, t0 + 4 * 86400, t0 - 36,
            t0 - 36]
    got = dict(zip(e['soa'][2].tolist(), e['soa'][4].tolist()))      # by latitude: the line's number + .5
    assert [got[i + .5] for i in range(9)] == want
    assert got[9.5] < 0 and got[10.5] == 253402300799 and got[11.5] == -62135596800
    # the largest inactivity the C-ABI carries (68 years): year 1 with year 17, 2017, year 9999
    assert ic.cases()['ymdhms_accepted'].inactivity == 2 ** 31 - 1 and [len(p) for _, p in e['windows']] == [2, 9, 2]
    assert _exp('ymdhms_accepted_java')['soa'][4].tolist() == e['soa'][4].tolist()
    for name, why in (('ymdhms_17_bytes', 'int'), ('ymdhms_10_bytes', 'int'), ('ymdhms_empty', 'int'),
                      ('ymdhms_year_0', 'time'), ('ymdhms_month_13', 'time')):
        assert _exp(name)['error'] == 'line 1: ' + why
    assert _exp('epoch_raw_blanks')['soa'][4].tolist() == [-3, 5, 12, 12]
    assert _exp('epoch_java_blanks')['error'] == 'line 3: int'
    assert _exp('epoch_java_plus')['soa'][4].tolist() == [-3, 5, 12]
    assert _exp('epoch_raw_2_63')['error'] == _exp('epoch_java_2_63')['error'] == 'line 1: int'


def test_which_error_wins():
    want = {'reason_fields': (1, 'fields'), 'reason_float': (1, 'float'), 'reason_int': (1, 'int'),
            'reason_time': (0, 'time'), 'reason_accuracy': (0, 'accuracy'), 'reason_uuid': (1, 'uuid'),
            'reason_precision': (2, 'precision'), 'reason_precision_py2': (1, 'precision'),
            'lowest_bad_line': (3, 'int'), 'lowest_bad_line_not_reason': (511, 'accuracy'),
            'first_reason_float': (0, 'float'), 'first_reason_float_raw': (0, 'float'),
            'first_reason_float_java': (0, 'float'), 'accuracy_before_uuid': (0, 'accuracy'),
            'time_before_accuracy': (0, 'int'), 'raw_newline_only': (0, 'fields'), 'java_newline_only': (0, 'fields')}
    for name, (line, why) in want.items():
        assert _exp(name)['error'] == 'line %d: %s' % (line, why), name
    # every reason the device can give but the collision (reporter_amd/_lib.py INGEST_REASONS)
    assert {w for _, w in want.values()} == {'fields', 'float', 'int', 'time', 'uuid', 'precision', 'accuracy'}
    # the two device-only refusals: the oracle accepts the text, the restatement refuses the numeral
    for name, py2 in (('reason_precision', False), ('reason_precision_py2', True)):
        c = ic.cases()[name]
        assert len(c.records()) == len(oi._lines(c.text))
        line = oi._lines(c.text)[c.refusal[0]]
        nums = line.split(',')[2:4] if c.rules == ic.SHARD else line.split('|')[9:11]
        assert [(ic.classify_py2 if py2 else ic.classify)(s)[0] is None for s in nums].count(True) == 1
    # the second bad line of each two-line text is bad on its own, and in another block of 256 lines
    c = ic.cases()['lowest_bad_line']
    lines = c.text.split(b'\n')
    with pytest.raises(oi.IngestError) as err:
        oi.shard_records(b'\n'.join(lines[4:]))
    assert (err.value.line + 4, err.value.reason) == (700, 'float')
    lines = ic.cases()['lowest_bad_line_not_reason'].text.split(b'\n')
    with pytest.raises(oi.IngestError) as err:
        oi.shard_records(b'\n'.join(lines[512:]))
    assert (err.value.line + 512, err.value.reason) == (512, 'fields')


def test_corpus_texts():
    """The numeral texts of the GPU test give every numeral back, in order, under every rule set."""
    main = ic.numerals()['main']
    for rules in (ic.SHARD, ic.RAW, ic.JAVA):
        e = ic.corpus_case(rules, main).expected()
        assert (e['n_lines'], e['n_traces'], e['n_probes']) == (len(main), 1, len(main))
        want = [float(s) for s in main]
        if rules == ic.RAW:
            want = [float(oi.py2_str_float(v)) for v in want]
        if rules == ic.JAVA:
            with np.errstate(over='ignore'):
                want = np.asarray(want).astype(np.float32).astype(np.float64).tolist()
        assert e['soa'][2].tobytes() == np.asarray(want).tobytes()
        assert e['soa'][3].tobytes() == np.asarray(want[-1:] + want[:-1]).tobytes()
    e = ic.corpus_case(ic.SHARD, main, uuids=5, seed=7).expected()
    assert (e['n_uuids'], e['n_traces'], e['n_probes']) == (5, 5, len(main))
    for rules in (ic.RAW, ic.JAVA):
        acc = ic.accuracy_numerals(rules)
        e = ic.corpus_case(rules, acc, field='accuracy').expected()
        assert e['n_probes'] == len(acc) > len(main) // 2
        assert len(set(e['soa'][5].tolist())) > (3 if rules == ic.RAW else 100)
    # every numeral with a text of its own ends it at line 2, under the reason the list stands for
    n = ic.numerals()
    for s in n['rejected'] + n['non_finite']:
        for rules in (ic.SHARD, ic.RAW, ic.JAVA):
            assert ic.single_numeral_case(s, rules).expected()['error'] == 'line 2: float', s
    for s in n['refused'] + n['py2_refused']:
        for rules in (ic.SHARD, ic.RAW, ic.JAVA):
            assert 'error' not in ic.single_numeral_case(s, rules).expected(), s
