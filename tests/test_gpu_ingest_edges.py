"""K11 ingest on the GPU at its edges (tests/ingest_cases.py) against oracle/ingest.py, bit for bit:
the numeral corpus as coordinates under the three rule sets, shuffled over five uuids, and as the
accuracy; every refused, rejected and non-finite numeral in a text of its own; every hand-built
text with its counts or its exact error; one matcher used again after a longer and after a
rejected text; and one text taken from device memory.  What the numerals and texts reach is
pinned by tests/test_ingest_cases_cpu.py; the same numerals meet the formatter's compile of the
parsers in tests/test_gpu_formatter.py.

Each of these edits to the OTR_HD functions of otr_ingest.h was applied to a copy of the tree, the
host build rebuilt and tests/test_ingest_cases_cpu.py run (stopping at the first failure); each
failed test_restatement_python_and_host_build_agree at the numeral shown, with its tags, and
nothing failed without an edit:
  the second product never taken                      6079454753933113.5 (second, carry, tie_odd)
  the carry `if (hi2 > lo) ++hi` dropped              6079454753933113.5 (second, carry, tie_odd)
  the round-to-even line dropped                      9007199254740993e0 (tie_even, clinger_miss)
  `m += m & 1` removed in the subnormal branch        2.4703282292062328e-324 (subnormal)
  Clinger `<= (1ull << 53)` -> `<= (1ull << 54)`      9007199254740993e22 (clinger_miss)
  Clinger `q <= 22` -> `q <= 23` (table one longer)   8211237901815073e19 (py2_side: 10^23 in the round trip)
  an inexact w accepted without the w + 1 check       9007199254740993.00000000000000000001 (inexact_refuse:
                                                      return code 0 for 2)
  `nd <= 12` -> `nd <= 13`                            11.44462452565 (py2_exact_lt)
  an exact py2 tie resolved upwards                   123456789012.5 (py2_exact_eq)
  exponent clamp `x < 1000000` -> `x < 1000`          0.<9999 zeros>1e10000 (exp_long)
Kernel-only edits and the case written for each.  The three that change a comparison were each
built once into a scratch library and this file run against it once on an MI355X (marked "run":
exactly the tests named failed, the rest passed); the others change a size, an index or the order
of the code and were not run:
  `gap >` -> `gap >=` in k_win_heads         run     gap_at_limit, gap_at_limit_0,
                                                     test_inactivity_beyond_the_abi_is_refused
  bbox `<` / `>` -> `<=` / `>=`              run     bbox_edges (from host and from device memory)
  atomicMin -> atomicMax in ingest_reject    run     every rejected text, lowest_bad_line and
                                                     lowest_bad_line_not_reason among them (46 tests:
                                                     over a word that starts at ~0 the maximum
                                                     reports no line at all)
  an int64_t gap                             not run groups (uuid z: the gap wraps to -3)
  `len >= 2` -> `len >= 1` in k_win_len      not run lone_windows, all_dropped, lines_1
  the last-chunk memset removed              not run test_matcher_used_again (n_lines of the short texts)
  `last != '\\n'` ignored                     not run len_*_open, lines_1, lines_255
  the bbox test moved after the time parse   not run bbox_edges (line 4: 'no time')"""
import pytest

from reporter_amd import matcher as M
from reporter_amd.tools import gen
from tests import ingest_cases as ic
from tests.test_gpu_ingest import _got, _same

pytestmark = pytest.mark.gpu

COUNTS = ('n_lines', 'n_kept', 'n_uuids', 'n_traces', 'n_probes')


@pytest.fixture(scope='module')
def matcher(graph_dir):
    M.configure(M.default_config(gen.graph_path('tiny', graph_dir)))
    return M.Matcher()


def _check(m, case, **where):
    """One ingest against the oracle: the exact error, or the counts and every array."""
    want = case.expected()
    kw = dict(case.ingest_kw(), **where)
    text = None if where else case.text
    if 'error' in want:
        with pytest.raises(ValueError) as e:
            m.ingest(text, **kw)
        assert str(e.value) == want['error'], case.name
        return None
    r, b = m.ingest(text, **kw)
    assert [int(getattr(r, k)) for k in COUNTS] == [want[k] for k in COUNTS], case.name
    if want['n_traces']:     # (no trace: no arrays to read)
        _same(_got(case.text, r, b), want['soa'])
    return r


@pytest.mark.parametrize('rules', [ic.SHARD, ic.RAW, ic.JAVA])
def test_corpus_as_coordinates(matcher, rules):
    main = ic.numerals()['main']
    case = ic.corpus_case(rules, main)
    r = _check(matcher, case)
    assert r.n_traces == 1 and r.n_probes == len(main)


def test_corpus_through_the_sorts(matcher):
    r = _check(matcher, ic.corpus_case(ic.SHARD, ic.numerals()['main'], uuids=5, seed=7))
    assert r.n_uuids == 5 and r.n_traces == 5


@pytest.mark.parametrize('rules', [ic.RAW, ic.JAVA])
def test_corpus_as_accuracy(matcher, rules):
    acc = ic.accuracy_numerals(rules)
    r = _check(matcher, ic.corpus_case(rules, acc, field='accuracy'))
    assert r.n_probes == len(acc)


def test_numerals_with_a_text_of_their_own(matcher):
    """Rejected and non-finite numerals end the ingest where the oracle does; a numeral that only
    the device code refuses ends it with 'precision' at its line, under the rules the restatement
    says (more than 19 digits: all three; the str() round trip: RAW alone)."""
    n = ic.numerals()
    assert len(n['rejected']) + len(n['non_finite']) + len(n['refused']) + len(n['py2_refused']) <= 26
    for k, s in enumerate(n['rejected'] + n['non_finite']):
        _check(matcher, ic.single_numeral_case(s, (ic.SHARD, ic.RAW, ic.JAVA)[k % 3]))
    for k, s in enumerate(n['refused']):
        case = ic.single_numeral_case(s, (ic.SHARD, ic.RAW, ic.JAVA)[k % 3])
        case.refusal = (2, 'precision')
        _check(matcher, case)
    for s in n['py2_refused']:
        case = ic.single_numeral_case(s, ic.RAW)
        case.refusal = (2, 'precision')
        _check(matcher, case)


def test_py2_refused_numerals_pass_the_other_rules(matcher):
    """No numeral of at most 19 digits is refused by dec_to_double: one text holds the three."""
    nums = ic.numerals()['py2_refused']
    for rules in (ic.SHARD, ic.JAVA):
        r = _check(matcher, ic.corpus_case(rules, nums))
        assert r.n_probes == len(nums)


@pytest.mark.parametrize('name', list(ic.cases()))
def test_hand_built_text(matcher, name):
    _check(matcher, ic.cases()[name])


def test_matcher_used_again(matcher):
    """The short texts after a longer accepted and after a longer rejected text, whose bytes hold
    '\\n' where the short text's last chunk is padding: the same result as on a fresh matcher."""
    fresh = M.Matcher()
    for case in ic.reuse_sequence():
        r = _check(matcher, case)
        if case.name.startswith('reuse_short'):
            f = _check(fresh, case)
            assert [int(getattr(r, k)) for k in COUNTS] == [int(getattr(f, k)) for k in COUNTS]
            assert r.n_lines == 3
    fresh.close()


def test_inactivity_beyond_the_abi_is_refused(matcher):
    """otr_ingest_format.inactivity is an int32: a larger value is refused by the wrapper (it used
    to wrap: 1 << 40 became 0 and split every window)."""
    for bad in (1 << 31, 1 << 40, -1):
        with pytest.raises(ValueError) as e:
            matcher.ingest(b'a,1,1.5,2.5,5\na,2,1.5,2.5,5\n', inactivity=bad)
        assert 'inactivity' in str(e.value)
    r, _ = matcher.ingest(b'a,1,1.5,2.5,5\na,2147483648,1.5,2.5,5\nb,1,1.5,2.5,5\nb,2147483649,1.5,2.5,5\n',
                          inactivity=(1 << 31) - 1)
    assert (r.n_traces, r.n_probes) == (1, 2)


@pytest.mark.parametrize('name', ['groups', 'bbox_edges', 'len_15_open'])
def test_text_in_device_memory(matcher, name):
    import torch
    case = ic.cases()[name]
    d_text = torch.frombuffer(bytearray(case.text), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert d_text.numel() == len(case.text)
    _check(matcher, case, device_ptr=d_text.data_ptr(), nbytes=len(case.text))
