"""One Matcher, many batches: what a batch leaves behind must not reach the next one.

A batch's control block (work counters, list counters, path cursors, work queues) is zeroed by
one fill at batch start, the task flags are written by k_tasks instead of being filled, the turn
cost tables are uploaded only when the parameters or their buffer changed, and the host reads
its scalars from one pinned mailbox per matcher.  Each of these goes wrong in the same way: a
word or a table of a larger or different earlier batch is still there.  So one Matcher on the
city graph runs, in this order,

  1. 3 traces with the deployed turn penalties (every task flag 5: the edge-state tiers and dumps),
  2. the same traces in node mode (turn_penalty_factor 0: other tables, the node tiers),
  3. 1 trace of 2 probes,
  4. 1 trace of 1 probe (one state, no task),
  5. no trace at all,
  6. batch 1 again (the deployed tables come back),
  7. a node-mode batch of exactly 4097 states (several scan blocks and one state more),

and every result (copy_out=True, route_work=True) must equal, field for field, the result of a
fresh Matcher for that batch, and the oracle's (oracle.compare.compare).  The work counters that
the route tier fixture (tests/golden/route_tier_slots.json) found stable between runs (5, 6, 7)
and the route tier codes are compared too.  Runs in a child process: it reconfigures the library.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S_TARGET = 4097
CHILD = r'''
import sys
sys.path.insert(0, %r)
import numpy as np
from oracle import pyoracle as po
from oracle.compare import compare
from reporter_amd import _lib
from reporter_amd import matcher as M
from reporter_amd.tools import gen

path = gen.graph_path('city', %r)
S_TARGET = %d
graph = po.Graph(path)


def cut(tr, lens):
    """The first lens[i] probes of trace i, for the first len(lens) traces."""
    sel = np.concatenate([np.arange(tr.offsets[i], tr.offsets[i] + n) for i, n in enumerate(lens)]) \
        if lens else np.zeros(0, np.int64)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return gen.Traces(tr.lat[sel].copy(), tr.lon[sel].copy(), tr.time[sel].copy(), off,
                      tr.mode[:len(lens)].copy())


def states(tr, prm):
    return int(po.match_batch(graph, tr, prm)['trace_state_off'][-1])


def exact_states(tr, prm, target):
    """A prefix of tr (whole traces, then a shortened last one) with exactly `target` states."""
    per = po.match_batch(graph, tr, prm)['trace_state_off']
    k = int(np.searchsorted(per, target, side='left'))  # the first k traces hold >= target states
    assert 0 < k <= tr.n_traces, (k, int(per[-1]))
    full = [int(tr.offsets[i + 1] - tr.offsets[i]) for i in range(k)]
    last = tr.slice(k - 1, k)  # (traces are matched independently: only the last one is cut and run again)
    for n in range(full[-1], 0, -1):
        if int(per[k - 1]) + states(cut(last, [n]), prm) == target:
            return cut(tr, full[:-1] + [n])
    raise AssertionError('no prefix with %%d states' %% target)


def run(m, tr):
    r = m.match_batch(tr, copy_out=True, route_work=True)
    assert r.status == 0, r.status
    d = _lib.result_to_numpy(r)  # (copies)
    d.pop('counters')
    # a state's candidate slots beyond its count are never written: not part of the result
    unused = np.arange(d['cand_edge'].shape[1])[None, :] >= d['cand_count'][:, None]
    for k in ('cand_edge', 'cand_p', 'cand_sqd'):
        d[k][unused] = 0
    d['n_states'] = int(r.n_states)
    d['n_probes'] = int(r.n_probes)
    d['stable_counters'] = [int(r.counters[k]) for k in (5, 6, 7)]
    d['route_tier_code'] = [int(r.route_tier_code[t]) for t in range(16)]
    return d


def same(a, b):
    bad = [k for k in a if not (np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k])]
    return bad + [k for k in b if k not in a]


three = gen.make_traces(path, 3, 100, 15, 10.0, 2)
many = gen.make_traces(path, 60, 100, 15, 10.0, 5)
node = po.params(turn_penalty_factor=0.0)
batches = [('deployed', three, None), ('node', three, node), ('two probes', cut(three, [2]), node),
           ('one probe', cut(three, [1]), node), ('no trace', cut(three, []), node), ('deployed again', three, None),
           ('%%d states' %% S_TARGET, exact_states(many, node, S_TARGET), node)]

deployed = M.default_config(path)
node_cfg = M.default_config(path, turn_penalty_factor=0)
M.configure(deployed)
kept = M.Matcher()
now = None
for name, tr, prm in batches:
    if prm is not now:
        M.configure(node_cfg if prm is not None else deployed)
        now = prm
    got = run(kept, tr)
    fresh = run(M.Matcher(), tr)
    bad = same(got, fresh)
    assert not bad, (name, 'differs from a fresh matcher in', bad)
    if tr.n_traces == 0:
        assert got['n_states'] == 0 and got['n_probes'] == 0 and len(got['route_edge']) == 0, name
    else:
        errors, stats = compare(got, po.match_batch(graph, tr, prm or po.params()))
        assert not errors, (name, errors[:5])
    if name == 'one probe':
        assert got['n_states'] == 1 and got['stable_counters'][0] == 0, got  # S = 1, NT = 0
    if name.endswith('states'):
        assert got['n_states'] == S_TARGET, got['n_states']
    if name.startswith('deployed'):
        assert got['stable_counters'][0] > 0 and got['route_tier_code'][10] != 0, got  # the edge-state tiers ran
    print('batch ok:', name, got['n_states'], got['stable_counters'])
print('reuse ok')
'''


def test_one_matcher_many_batches(graph_dir):
    env = dict(os.environ)
    for k in ('OTR_LIB', 'OTR_TIERS', 'OTR_EST_K', 'OTR_FORCE_EDGE', 'OTR_PATH_CAP0'):
        env.pop(k, None)
    env['OTR_DEBUG_TASKS'] = '1'  # the host check that k_tasks wrote every task's flag
    p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, S_TARGET)], env=env, capture_output=True,
                       text=True, timeout=240)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert 'reuse ok' in p.stdout
