"""The winner-path buffer that proves too small: the path stage grows it and runs again.

The stage's cap flag no longer has a host wait of its own: k_capacity and its scan are queued
behind every attempt, and the flag, the cursors and the capacity layout's total come back in one
mailbox record.  A set flag must still lead to exactly the old loop: grow to 1.5 x the largest
cursor, clear the path stage's words, run the path kernels, k_capacity and the scan again.  The
test-only knob OTR_PATH_CAP0 (first attempt's capacity in entries, read once per process) makes
the first attempt of a 3-trace city batch overflow: 64 entries, one per shard.  The result must
equal the default run's field for field, and the regrow must have happened (the attempt count
is reported on stderr with OTR_DEBUG_FAIL set).  Both in node mode and with the deployed turn
penalties (the edge-state path tiers).  A child process per run: the knob is read once."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys
sys.path.insert(0, %r)
import numpy as np
from reporter_amd import _lib
from reporter_amd import matcher as M
from reporter_amd.tools import gen
path = gen.graph_path('city', %r)
M.configure(M.default_config(path, **%r))
tr = gen.make_traces(path, 3, 100, 15, 10.0, 2)
m = M.Matcher()
for rep in range(2):  # (the second batch starts from the grown buffer and the first one's words)
    r = m.match_batch(tr, copy_out=True)
    assert r.status == 0, r.status
    d = _lib.result_to_numpy(r)
    d.pop('counters')
    # a state's candidate slots beyond its count are never written: not part of the result
    unused = np.arange(d['cand_edge'].shape[1])[None, :] >= d['cand_count'][:, None]
    for k in ('cand_edge', 'cand_p', 'cand_sqd'):
        d[k][unused] = 0
    np.savez(%r + str(rep) + '.npz', **d)
print('done')
'''


def run(graph_dir, out, options, cap0):
    env = dict(os.environ)
    for k in ('OTR_LIB', 'OTR_TIERS', 'OTR_EST_K', 'OTR_FORCE_EDGE', 'OTR_PATH_CAP0'):
        env.pop(k, None)
    env['OTR_DEBUG_FAIL'] = '1'
    if cap0:
        env['OTR_PATH_CAP0'] = str(cap0)
    p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, options, out)], env=env, capture_output=True,
                       text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    regrown = [int(x) for x in re.findall(r'winner paths regrown: (\d+) attempts', p.stderr)]
    return [dict(np.load(out + str(rep) + '.npz')) for rep in range(2)], regrown


@pytest.mark.parametrize('options', [{'turn_penalty_factor': 0}, {}], ids=['node', 'deployed'])
def test_small_path_buffer_regrows_to_the_same_result(graph_dir, tmp_path, options):
    want, none = run(graph_dir, str(tmp_path / 'want'), options, 0)
    got, regrown = run(graph_dir, str(tmp_path / 'got'), options, 64)
    print('attempts:', regrown)
    assert none == []  # the default capacity fits at the first attempt
    assert regrown and all(2 <= a <= 8 for a in regrown), regrown
    assert len(want[0]['route_edge']) > 64  # (the paths cannot fit 64 entries)
    for rep in range(2):
        assert sorted(got[rep]) == sorted(want[rep])
        for k in want[rep]:
            assert np.array_equal(got[rep][k], want[rep][k]), (rep, k)
