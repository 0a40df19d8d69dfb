"""The entry sets of tests/hist_cases.py take the branches of Matcher::hist_reduce they are named for,
and their reductions are not trivial (CPU only).  Requirements on the inputs of the family tests
in tests/test_gpu_hist_keyed.py: when a set or the pass choice changes, this file says which
branch the GPU tests lost."""
import numpy as np
import pytest

from tests import hist_cases as hc


def test_pass_choice_thresholds():
    """The restated choice at its boundaries: end bit 64 exactly, 61 against 62 bits of next id,
    18 against 19 bits of bucket spread, 46 against 47 bits of id, one foreign file."""
    def one(next_id=5, sid=hc.IDS[0], spread=0, file_of=hc.k9_file):
        return hc._entries([(file_of(hc.B60, sid), sid, next_id, 0, 1), (file_of(hc.B60 + spread, sid), sid, 1, 1, 1)])
    assert hc.pass_choice(one((1 << 61) - 1)) == ('combined', 'packed', [(4, 64), (5, 46)])
    assert hc.pass_choice(one(1 << 61)) == ('split', 'packed', [(3, 3), (2, 62), (5, 46)])
    assert hc.pass_choice(one(1 << 63))[2][:2] == [(3, 3), (2, 64)]
    assert hc.pass_choice(one(spread=(1 << 18) - 1))[1:] == ('packed', [(4, 6), (5, 64)])
    assert hc.pass_choice(one(spread=1 << 18))[1] == 'id_file'
    assert hc.pass_choice(one(sid=hc.IDS[6]))[1] == 'packed' and hc.bit_width(hc.IDS[6]) == 46
    assert hc.pass_choice(one(sid=hc.IDS[6] | (1 << 46)))[1] == 'id_file'
    assert hc.pass_choice(one(file_of=hc.edge_file))[1] == 'id_file'
    assert hc.k9_file(hc.B60, hc.IDS[0] | (1 << 46)) == hc.k9_file(hc.B60, hc.IDS[0])


@pytest.mark.parametrize('name', list(hc.FAMILIES))
def test_family_takes_its_branch_and_reduces(name):
    e = hc.entries(name)
    _, low, high, ends = hc.FAMILIES[name]
    got_low, got_high, passes = hc.pass_choice(e)
    r1, r2, r3 = (hc.reduced(name, p) for p in (1, 2, 3))
    pairs = len(set(zip(r1['file'].tolist(), r1['id'].tolist(), r1['next_id'].tolist())))
    print('%s: %d entries, %s + %s passes %s, %d keys in %d pairs and %d files, kept at privacy 2 / 3: %d / %d' % (
        name, len(e), got_low, got_high, passes, len(r1), pairs, len(set(r1['file'].tolist())), len(r2), len(r3)))
    assert (got_low, got_high) == (low, high)
    for field, end in ends.items():
        assert (field, end) in passes, (field, end, passes)
    # several runs, keys met more than once in every bin, something kept and something culled
    assert len(e) > len(r1) > 20 and set(r1['speed_bin'].tolist()) == set(range(hc.BINS))
    dup = {}
    for f, i, n, b in zip(e['file'].tolist(), e['id'].tolist(), e['next_id'].tolist(), e['speed_bin'].tolist()):
        dup[(f, i, n, b)] = dup.get((f, i, n, b), 0) + 1
    assert {k[3] for k, c in dup.items() if c > 1} == set(range(hc.BINS))
    assert len(r1) > len(r2) > len(r3) > 0
    assert int(r1['count'].sum()) == int(e['count'].sum())
    # (shuffled: the input is not in key order)
    key = list(zip(e['file'].tolist(), e['id'].tolist(), e['next_id'].tolist(), e['speed_bin'].tolist()))
    assert key != sorted(key)


def test_sizes_and_the_entry_that_decides_the_spread():
    for name, n in (('n_1023', 1023), ('n_1024', 1024), ('n_1025', 1025), ('n_131073', 131073)):
        e = hc.entries(name)
        b = e['file'] >> np.uint64(25)
        assert len(e) == n and int(b[-1]) == int(b.max()) and int((b == b.max()).sum()) == 1
        # without the last entry the spread has one bit less: the packed pass would end below its bucket
        end = hc.pass_choice(e)[2][-1]
        assert end == (5, hc.FAMILIES[name][3][5]) and hc.pass_choice(e[:-1])[2][-1] == (5, end[1] - 1)
    assert 200 <= len(hc.reduced('n_131073', 1)) <= 999  # a few hundred keys


def test_one_key_1025_times():
    e = hc.entries('one_key_1025')
    _, counts = np.unique(e[['file', 'id', 'next_id', 'speed_bin']], return_counts=True)
    assert counts.max() >= 1025 and (counts >= 1025).sum() == 1


def test_wide_ids_are_in_the_sets():
    nx = set(hc.entries('next_61_bits')['next_id'].tolist())
    assert max(nx) == (1 << 61) - 1
    assert max(hc.entries('next_62_bits')['next_id'].tolist()) == 1 << 61
    assert sum(1 for v in set(hc.entries('next_bit_63')['next_id'].tolist()) if v >> 63) == 1
    ids = set(hc.entries('id_bit_46')['id'].tolist())
    assert any(v >> 46 and (v ^ (1 << 46)) in ids for v in ids)
    for name in ('next_61_bits', 'next_62_bits', 'next_bit_63', 'foreign_wide_next'):
        e = hc.entries(name)
        hc._leading18(e['id'].tolist() + e['next_id'].tolist())
    b = hc.entries('spread_18_bits')['file'] >> np.uint64(25)
    assert int(b.max()) - int(b.min()) == (1 << 18) - 1
    b = hc.entries('spread_19_bits')['file'] >> np.uint64(25)
    assert int(b.max()) - int(b.min()) == 1 << 18


@pytest.mark.parametrize('name', list(hc.BIG))
def test_big_files(name):
    """Files of more than 1024 pairs: where the string-last pair sits, and that the reference
    loop's trailing-run quirk decides something in the big file and nothing in its sibling."""
    from tests.test_hist_cull_cpu import _pairs_from_entries, _pairs_from_lines
    rows, where = hc.big_rows(name)
    e = hc.entries(name)
    tot = _pairs_from_entries(hc.reduced(name, 1))
    for (f, n_pairs, pos, second), (want_pairs, want_pos, t1, t2) in zip(where, hc.BIG[name]):
        prs = sorted(k for k in tot if k[0] == f)  # numeric order, as the device sorts them
        assert len(prs) == n_pairs == want_pairs > 1024
        by_str = sorted(prs, key=lambda k: (str(k[1]) + ',', str(k[2]) + ','))
        assert prs.index(by_str[-1]) == pos == want_pos and prs.index(by_str[-2]) == second
        assert tot[by_str[-1]] == t1 and tot[by_str[-2]] == t2
        print('%s file %d: %d pairs, string-last at %d (thread %d, stride %d, %d line), string-second at %d (%d)' % (
            name, f, n_pairs, pos, pos % 1024, pos // 1024, t1, second, t2))
        assert pos < n_pairs - 1  # numerically in the middle
    big, sib = hc.BIG[name]
    assert big[1] >= 1024 and big[1] % 1024 >= 400  # a later stride, a high thread index
    assert big[2] == 1 and sib[2] == 2
    for p in (2, 3):
        got = _pairs_from_entries(hc.reduced(name, p))
        assert got == _pairs_from_lines(rows, p)
        alone = {k: v for k, v in tot.items() if v >= p}  # every pair judged by its own total
        diff = set(got) ^ set(alone)
        print('%s privacy %d: %d pairs kept, the quirk decides %d' % (name, p, len(got), len(diff)))
        assert where[1][0] not in {k[0] for k in diff}  # never in the sibling
    assert any(set(_pairs_from_entries(hc.reduced(name, p))) != {k for k, v in tot.items() if v >= p} for p in (2, 3))
    assert len(e) == len(rows)
