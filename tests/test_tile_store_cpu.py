"""The tile store's restatement (tests/tile_store_ref.py) against oracle.tiles, what its script
covers, and the parts of the feature that need no device: the ctypes mirrors, the refusals on a
matcher without a store and the payload text.  (No GPU.)"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import tiles as T
from reporter_amd import _lib
from tests import tile_store_ref as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = TS.SCRIPT_Q


def _lines_by_file(flush, source='reporter', mode='auto'):
    out = {}
    for f in range(flush['n_files']):
        a, b = int(flush['row_off'][f]), int(flush['row_off'][f + 1])
        out[T.file_name(flush['file'][f], flush['quantisation'])] = [T.java_line(r, source, mode)
                                                                    for r in flush['rows'][a:b]]
    return out


@pytest.mark.parametrize('privacy', [1, 2, 3])
def test_flush_equals_stream_tiles_of_everything_added(privacy):
    """Every flush of the script equals oracle.tiles.stream_tiles over the concatenation of the
    rows added since the last flush, files ascending, and the counts add up."""
    ref = TS.Store(1 << 20, Q, privacy)
    since = []
    n_flushes = 0
    for i, a in enumerate(TS.script_adds()):
        r = ref.add_reports(a)
        since.append(TS.rows_of(a, Q))
        assert r['n_rows_added'] == len(since[-1]) and r['n_rows'] == sum(len(s) for s in since)
        assert r['n_reports'] == len(a['id']) >= r['n_valid']
        if i not in TS.SCRIPT_FLUSH_AFTER:
            continue
        rows = np.concatenate(since)
        want = T.stream_tiles(rows, privacy, Q)
        fl = ref.flush()
        assert _lines_by_file(fl) == want
        assert list(_lines_by_file(fl)) == [T.file_name(f, Q) for f in sorted(set(fl['file'].tolist()))]
        assert np.all(np.diff(fl['file'].astype(np.int64)) > 0)
        assert fl['n_rows_in'] == len(rows) and fl['n_rows'] == len(fl['rows']) == fl['row_off'][-1]
        assert fl['n_files'] + fl['n_files_empty'] == len(set(rows['file'].tolist()))
        for f, n in zip(fl['file'], fl['n_unclean']):
            assert n == np.count_nonzero(rows['file'] == f)
        assert ref.n_rows == 0
        since = []
        n_flushes += 1
    assert n_flushes == 3 and ref.flush()['n_files'] == 0


def test_restatement_refuses_past_max_rows():
    adds = TS.script_adds()
    n0 = len(TS.rows_of(adds[0], Q))
    ref = TS.Store(n0, Q, 1)
    assert ref.add_reports(adds[0])['n_rows'] == n0
    with pytest.raises(ValueError, match='max_rows'):
        ref.add_reports(adds[1])
    assert ref.n_rows == n0
    assert ref.flush()['n_rows_in'] == n0
    assert ref.add_reports(adds[1])['n_rows'] == len(TS.rows_of(adds[1], Q))


def test_script_coverage():
    """What the script must hold at q = 60, so that a later edit cannot hollow it out."""
    adds = TS.script_adds()
    sizes = [int(n) for a in adds for n in np.diff(a['rep_off'])]
    assert 65 in sizes and 129 in sizes

    def buckets(a, k):
        return int(a['t1'][k]) // Q - int(a['t0'][k]) // Q + 1

    def is_valid(a, k):
        return TS.valid(float(a['t0'][k]), float(a['t1'][k]), int(a['length'][k]), int(a['queue_length'][k]))

    # a report of 3 buckets at position 63 of its window and one at position 64
    at = {63: False, 64: False}
    for a in adds:
        for w in range(len(a['rep_off']) - 1):
            lo, hi = int(a['rep_off'][w]), int(a['rep_off'][w + 1])
            for p in at:
                if hi - lo > p and is_valid(a, lo + p) and buckets(a, lo + p) == 3:
                    at[p] = True
    assert at == {63: True, 64: True}
    # a window without reports between two with reports
    assert any(s[i] > 0 and s[i + 1] == 0 and s[i + 2] > 0 for a in adds for s in [np.diff(a['rep_off'])]
               for i in range(len(s) - 2))
    # one report failing each of Segment.valid's five terms alone or first (t1 == t0 included)
    fails = set()
    for a in adds:
        for k in range(len(a['id'])):
            t0, t1, ln, qu = float(a['t0'][k]), float(a['t1'][k]), int(a['length'][k]), int(a['queue_length'][k])
            terms = (t0 > 0, t1 > 0, t1 > t0, ln > 0, qu >= 0)
            if not all(terms):
                fails.add(terms.index(False))
            if t1 == t0:
                fails.add('equal')
    assert fails == {0, 1, 2, 3, 4, 'equal'}
    assert any(int(x) == TS.NO_ID for a in adds for x in a['next_id'])
    # a pair whose rows arrive in three different adds (of one flush interval) with different durations
    first = [TS.rows_of(a, Q) for a in adds[:TS.SCRIPT_FLUSH_AFTER[0] + 1]]
    pairs = [set(zip(r['file'].tolist(), r['id'].tolist(), r['next_id'].tolist())) for r in first]
    shared = pairs[0] & pairs[1] & pairs[2]
    assert shared
    for f, i, n in shared:
        durs = [int(r['duration'][(r['file'] == f) & (r['id'] == i) & (r['next_id'] == n)][0]) for r in first]
        assert len(set(durs)) == 3
    # Math.round's tie goes up
    assert any(float(a['t1'][k]) - float(a['t0'][k]) == 2.5 for a in adds for k in range(len(a['id'])))
    _, fl1 = TS.script_flushes(1)
    _, fl2 = TS.script_flushes(2)
    # a file cleaned to nothing at privacy 2, and partial cleans too
    assert fl2[0]['n_files_empty'] > 0 and fl1[0]['n_files_empty'] == 0
    assert 0 < fl2[0]['n_rows'] < fl1[0]['n_rows'] and 0 < fl2[1]['n_rows'] < fl1[1]['n_rows']
    # the last-range case of clean: a file of two rows of different pairs, both kept at privacy 2
    last_range = False
    for f in range(fl2[0]['n_files']):
        a, b = int(fl2[0]['row_off'][f]), int(fl2[0]['row_off'][f + 1])
        r = fl2[0]['rows'][a:b]
        if b - a == 2 and fl2[0]['n_unclean'][f] == 2 and (r['id'][0], r['next_id'][0]) != (r['id'][1], r['next_id'][1]):
            last_range = True
    assert last_range
    # two files that differ only in level, two that differ only in bucket
    files = [int(f) for f in fl1[0]['file']]
    split = [(f >> 25, (f >> 22) & 7, f & 0x3FFFFF) for f in files]
    assert any(a[0] == b[0] and a[2] == b[2] and a[1] != b[1] for a in split for b in split)
    assert any(a[1:] == b[1:] and a[0] != b[0] for a in split for b in split)
    # arrival order is not pair order, and pairs repeat (the stable sort has work to do)
    r0 = first[0]
    key = list(zip(r0['file'].tolist(), r0['id'].tolist(), r0['next_id'].tolist()))
    assert key != sorted(key) and len(set(key)) < len(key)


def test_ctypes_mirrors_against_c_header(tmp_path):
    """The new structs' ctypes mirrors have the C compiler's sizes and offsets."""
    if not shutil.which('gcc'):
        pytest.skip('no C compiler')
    structs = {'otr_tile_store_config': _lib.TileStoreConfig, 'otr_tile_add_result': _lib.TileAddResult,
               'otr_tile_flush_result': _lib.TileFlushResult}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "otr.h"', 'int main(void) {']
    for cname, cls in structs.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    prog.append('printf("otr_tile_row %zu\\n", sizeof(otr_tile_row));')
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
    assert int(got['otr_tile_row']) == _lib.TILE_ROW.itemsize == T.TILE_ROW.itemsize


def test_every_call_without_a_store_names_open():
    """On a matcher without a store every tile-store call is refused before any device call."""
    from reporter_amd import matcher as M
    m = M.Matcher()
    empty = TS.reports_of([])
    calls = [m.tile_store_close, m.tile_store_add_session, lambda: m.tile_store_add_reports(empty),
             lambda: m.tile_store_add_reports(TS.script_adds()[1]),
             lambda: m.tile_store_add_rows(np.zeros(1, _lib.TILE_ROW)), m.tile_store_flush]
    for f in calls:
        with pytest.raises(ValueError, match='otr_tile_store_open'):
            f()
    # and a config out of range is refused before the device is touched
    for bad in (dict(max_rows=0), dict(max_rows=(1 << 27) + 1), dict(max_rows=8, quantisation=59),
                dict(max_rows=8, privacy=0)):
        with pytest.raises(ValueError, match='out of range'):
            m.tile_store_open(**bad)


def test_stream_tile_payloads_text():
    """The header plus oracle.tiles.java_line lines, for a three-row flush of two files."""
    from reporter_amd import simple_reporter as sr
    ref = TS.Store(16, Q, 1)
    ref.add_reports(TS.reports_of([[(TS.sid(1, 9, 2), TS.sid(1, 9, 3), TS.T0 + 1.0, TS.T0 + 3.5, 30, 1),
                                    (TS.sid(1, 9, 1), TS.NO_ID, TS.T0 + 2.0, TS.T0 + 4.0, 31, 0)],
                                   [(TS.sid(0, 9, 1), TS.sid(0, 9, 2), TS.T0 + 61.0, TS.T0 + 65.0, 32, 0)]]))
    fl = ref.flush()
    assert fl['n_rows'] == 3 and fl['n_files'] == 2
    got = sr.stream_tile_payloads(fl, 'auto', 'src')
    header = ('segment_id,next_segment_id,duration,count,length,queue_length,minimum_timestamp,maximum_timestamp,'
              'source,vehicle_type')
    want = {k: header + ''.join(v) for k, v in _lines_by_file(fl, 'src', 'auto').items()}
    assert got == want and len(got) == 2
    assert set(got) == {'%d_%d/0/9' % (TS.T0 + 60, TS.T0 + 119), '%d_%d/1/9' % (TS.T0, TS.T0 + 59)}
    one = got['%d_%d/1/9' % (TS.T0, TS.T0 + 59)].split('\n')
    assert one[0] == header and one[1].startswith('%d,,2,1,31,0,' % TS.sid(1, 9, 1)) and one[2].endswith(',src,AUTO')
