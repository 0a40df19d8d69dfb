"""Stages that share workspace slots, alternating on ONE matcher while the slots grow and shrink.

The tile cull and the keyed histogram share the permutation, key, head, keep and scan slots and
the sort workspace; probe ingest and the stream formatter share the text, newline and uuid slots.
Every other test runs a stage on a matcher of its own or repeats one stage.  Here 3 -> 40 items
crosses the pool's quarter of headroom, so a shared slot is freed and allocated again between two
stages that use it, and 40 -> 3 runs a stage in a buffer larger than it needs, with the other
stage's contents in it.  Every result must equal the same call on a fresh matcher and the
restatement the stages' own tests compare against."""
import numpy as np
import pytest

from oracle import hist as oh
from oracle import tiles as ot
from reporter_amd import matcher as M
from reporter_amd import simple_reporter as sr
from reporter_amd.tools import gen
from tests import formatter_ref as F
from tests import ingest_cases as ic
from tests.test_gpu_formatter import _check_format
from tests.test_gpu_ingest import _got, _same
from tests.test_gpu_tile_stages import _want_rows

pytestmark = pytest.mark.gpu

COUNTS = ('n_lines', 'n_kept', 'n_uuids', 'n_traces', 'n_probes')
# the layout of tests/ingest_cases.py shard_line as a message format
SHARD_FMT = {'type': 'sv', 'separator': ',', 'uuid_index': 0, 'time_index': 1, 'lat_index': 2, 'lon_index': 3,
             'accuracy_index': 4, 'time_format': F.TIME_EPOCH}
FORMAT_KEYS = ('n_messages', 'n_points', 'n_dropped', 'n_unsupported', 'first_bad', 'first_bad_reason')
FORMAT_ARRAYS = ('status', 'key', 'lat', 'lon', 'accuracy', 'time', 'timestamp', 'message', 'uuid_off', 'uuid_len')


def _inputs(graph_dir):
    """3 and 40 rows (each row twice over, so that privacy 2 keeps some), their entries, texts of 2
    and 30 lines."""
    rows = _want_rows('ragged_city', 'gtt', 60, 'simple', graph_dir)
    rows3, rows40 = np.concatenate([rows[:2], rows[:1]]), np.concatenate([rows[:20], rows[:20]])
    text2 = ic._join([ic.shard_line('u', 5), ic.shard_line('u', 7, '1.75')])  # (one trace of two probes)
    return {3: rows3, 40: rows40}, {3: oh.entries_from_rows(rows3), 40: oh.entries_from_rows(rows40)}, \
        {2: text2, 30: ic._n_lines(30)}


def _cull(m, rows, privacy):
    kept = sr.cull_rows(m, rows, privacy)
    assert sr.rows_to_tiles(kept, 60) == ot.tiles(rows, privacy, q=60)
    return kept


def _hist(m, entries, privacy):
    got = sr.hist_reduce(m, entries, len(entries), privacy=privacy, memory='host')
    assert np.array_equal(got, oh.reduce(entries, privacy))
    return got


def _format(m, text):
    got = {k: v for k, v in m.format_messages(text, SHARD_FMT, timestamp=77).items() if k != 'device'}
    _check_format(got, text, F.split_lines(text), SHARD_FMT, 77, '%d bytes' % len(text))
    return got


def _ingest(m, text):
    case = ic.Case('shared', text)
    want = case.expected()
    r, b = m.ingest(text, **case.ingest_kw())
    counts = [int(getattr(r, k)) for k in COUNTS]
    assert counts == [want[k] for k in COUNTS] and want['n_traces'] > 0
    got = _got(text, r, b)
    _same(got, want['soa'])
    return counts, got


@pytest.mark.parametrize('privacy', [1, 2])
def test_stages_alternate_on_shared_slots(privacy, graph_dir):
    rows, entries, texts = _inputs(graph_dir)
    M.configure(M.default_config(gen.graph_path('tiny', graph_dir)))
    m = M.Matcher()
    steps = [(_cull, rows[3]), (_hist, entries[40]), (_cull, rows[40]), (_hist, entries[3]),
             (_format, texts[2]), (_ingest, texts[30]), (_format, texts[30]), (_ingest, texts[2])]
    kept = 0
    for k, (stage, data) in enumerate(steps):
        args = (data, privacy) if stage in (_cull, _hist) else (data,)
        got = stage(m, *args)
        fresh = M.Matcher()
        want = stage(fresh, *args)
        fresh.close()
        if stage in (_cull, _hist):
            assert np.array_equal(got, want), k
            kept += len(got)
        elif stage is _format:
            assert [got[f] for f in FORMAT_KEYS] == [want[f] for f in FORMAT_KEYS], k
            for f in FORMAT_ARRAYS:
                assert np.array_equal(got[f], want[f]), (k, f)
            assert got['n_points'] > 0 and got['n_messages'] == len(F.split_lines(data))
        else:
            assert got[0] == want[0], k
            _same(got[1], want[1])
    assert kept > 0
    m.close()
