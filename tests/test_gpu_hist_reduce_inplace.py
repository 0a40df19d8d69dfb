"""otr_hist_reduce on tile rows that are already in device memory reads them where they are.

The reduce used to copy device rows into a staging buffer before converting them; now the
conversion kernel reads the caller's buffer, which therefore must come back byte for byte, and a
second call on the same matcher must not see anything of the first (the key ranges are started
on the device by the conversion kernel, the counts come through the matcher's pinned mailbox).
One matcher reduces n = 1 row, then n = 3,000 rows (tests/hist_cases.py big_2500: two files of
more than 1024 pairs, duplicates, small files beside them), at privacy 1 and 2: the entries are
oracle/hist.reduce's, as in tests/test_gpu_hist_keyed.py."""
import numpy as np
import pytest

from oracle import hist as oh
from reporter_amd import _lib
from reporter_amd import matcher as M
from reporter_amd import simple_reporter as sr
from reporter_amd.tools import gen
from tests import hist_cases as hc

pytestmark = pytest.mark.gpu

N_ROWS = 3000


@pytest.fixture(scope='module')
def rows(graph_dir):
    M.configure(M.default_config(gen.graph_path('city', graph_dir)))
    r, _ = hc.big_rows('big_2500')
    assert len(r) > N_ROWS
    r = np.ascontiguousarray(r[:N_ROWS])
    e = oh.entries_from_rows(r)
    assert len(np.unique(e['file'])) >= 2 and len(oh.reduce(e, 1)) < N_ROWS  # a second file, duplicates
    return r


@pytest.mark.parametrize('privacy', [1, 2])
def test_device_rows_are_reduced_in_place_and_left_alone(rows, privacy):
    import torch
    m = M.Matcher()
    for n in (1, N_ROWS):
        host = rows[:n].view(np.uint8).reshape(-1).copy()
        dev = torch.from_numpy(host.copy()).cuda()
        got = sr.hist_reduce(m, dev.data_ptr(), n, privacy=privacy, rows_in=True)
        want = oh.reduce(oh.entries_from_rows(rows[:n]), privacy)
        assert np.array_equal(got, want), (n, privacy)
        if privacy == 1:
            assert len(got) > 0 and int(got['count'].sum()) == n
        assert np.array_equal(dev.cpu().numpy(), host), 'the input rows were modified'
    assert len(oh.reduce(oh.entries_from_rows(rows), 2)) > 0
