"""The rounds of the node search on hand-built graphs (the search keeps no
pending bit in its keys — a relaxation appends a node exactly when it finds the empty label —
and runs its per-round predicates in 32 bits), field by field against the oracle:

  (a) `diamond`: from S the nodes A and B settle in one round and both offer to H (A 320 m,
      B 315 m; the second diamond H -> A2 / B2 -> H2 has the lengths the other way round, so
      one of the two has the better offer second); a chain of ten 10 m edges S .. H (and
      H .. H2) then improves H, still pending, rounds later;
  (b) a step onto the island road of the same graph: no target is reachable and the search
      ends with an empty pending list;
  (c) the traces run as batches of 1, 2, 3, ... of them, so the task count and the pairing
      of the searches in a wave change from batch to batch.  Asserted: the searches of a
      batch do not all take the same number of rounds (the round total is no multiple of the
      search count), so lane groups of one wave finish in different rounds.  Not asserted,
      only made likely by the varying counts: a last unit with a lane group that has no task
      (the task count is not among the work counters);
  (d) `hub`: a node with eight out-edges (the CSR-tail path), a trace into every spoke.

A bound beyond 2^31 mm (sh = 0 and labels past 2 147 km) cannot be built: the configuration
limits breakage_distance, which caps every step's bound, to 30 km (otr_configure rejects
more), so no search sees such lengths; tests/test_route_pred32.py covers that range on the
host.

Each batch runs with route_work on and off (both compilations of the kernels).  Once with
the product library, and once with libotr_tiercheck.so and OTR_FORCE_EDGE=128: every search
goes down the retry tiers, is stopped after 2 (3) rounds, dumped and resumed, so the pending
marks come from the dump (a labelled key that is not settled).  Runs in child processes
(one library per process)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_diamond(path):
    from reporter_amd.graphfile import write_graph
    from tests import kat_graphs as K
    nodes, names, edges = [], {}, []

    def node(name, x, y):
        names[name] = len(nodes)
        nodes.append(K.ll(x, y))

    def one(a, b, **kw):
        edges.append(dict(src=names[a], dst=names[b], way=100 + len(edges), level=1, speed=50, **kw))
    node('W', -100, 0)
    for k in range(21):  # S = X0, H = X10, H2 = X20, ten 10 m edges between them
        node('X%d' % k, 10 * k, 0)
    node('Z', 300, 0)
    node('Z2', 400, 0)
    node('A', 30, 40)
    node('B', 30, -40)
    node('A2', 130, 40)
    node('B2', 130, -40)
    for k in range(3):
        node('I%d' % k, 100 * k, 200)  # the island road (disconnected)
    one('W', 'X0')
    for k in range(20):
        one('X%d' % k, 'X%d' % (k + 1), length=10.0)
    one('X20', 'Z')
    one('Z', 'Z2')
    # the diamonds' stored lengths: both heads settle one round after their tail
    one('X0', 'A', length=20.0)
    one('X0', 'B', length=25.0)
    one('A', 'X10', length=300.0)
    one('B', 'X10', length=290.0)
    one('X10', 'A2', length=20.0)
    one('X10', 'B2', length=25.0)
    one('A2', 'X20', length=290.0)
    one('B2', 'X20', length=300.0)
    for k in range(2):
        one('I%d' % k, 'I%d' % (k + 1))
    write_graph(path, nodes, edges, [dict(id=K.osmlr(1, 410, 1), edges=[21, 22])])  # X20 -> Z -> Z2
    traces = [[(-60, 2), (-5, 2), (230, 2), (270, 2)],     # W-S, then beyond H2
              [(-60, 2), (-5, 2), (120, 2), (160, 2)],     # targets on the chain H .. H2
              [(-60, 2), (-5, 2), (20, 202), (60, 202)],   # onto the island: nothing reachable
              [(30, 2), (70, 2), (150, 2), (250, 2)],      # along the chains
              [(-60, -2), (-5, -2), (330, -2), (370, -2)]]
    return [K.trace(p, dt=20) for p in traces]


def build_hub(path):
    import math
    from reporter_amd.graphfile import write_graph
    from tests import kat_graphs as K
    nodes = [K.ll(-200, 0), K.ll(0, 0)]
    edges = []
    K.two_way(edges, 0, 1, 200, level=1, speed=50)
    angles = [-75 + 25 * k for k in range(7)]
    for k, a in enumerate(angles):  # seven two-way spokes east of the hub, each with an extension
        c, s = math.cos(math.radians(a)), math.sin(math.radians(a))
        nodes.append(K.ll(150 * c, 150 * s))
        nodes.append(K.ll(300 * c, 300 * s))
        K.two_way(edges, 1, len(nodes) - 2, 201 + k, level=1, speed=50)
        K.two_way(edges, len(nodes) - 2, len(nodes) - 1, 201 + k, level=1, speed=50)
    write_graph(path, nodes, edges, [dict(id=K.osmlr(1, 411, 1), edges=[0])])
    traces = []
    for a in angles:
        c, s = math.cos(math.radians(a)), math.sin(math.radians(a))
        traces.append([(-120, 2), (-60, 2), (70 * c, 70 * s), (180 * c, 180 * s)])
    return [K.trace(p, dt=20) for p in traces]


CHILD = r'''
import os
import sys
sys.path.insert(0, %r)
from oracle import pyoracle as po
from oracle.compare import compare
from reporter_amd import _lib
from reporter_amd import matcher as M
from tests import kat_graphs as K
from tests import test_gpu_route_rounds as T
gdir, retry = %r, %r
cases = [('rounds_diamond', T.build_diamond, {'turn_penalty_factor': 0}, True),
         ('rounds_hub', T.build_hub, {'turn_penalty_factor': 0}, False),
         # (the same graphs without a time bound: sh = 0, the label word is the length)
         ('rounds_diamond', T.build_diamond, {'turn_penalty_factor': 0, 'max_route_time_factor': 0}, False),
         ('rounds_hub', T.build_hub, {'turn_penalty_factor': 0, 'max_route_time_factor': 0}, False)]
for name, build, opts, prefixes in cases:
    path = os.path.join(gdir, name + '.otrg')
    trs = build(path)
    M.configure(M.default_config(path, **opts))
    g = po.Graph(path)
    searched = retried = 0
    for n in (range(1, len(trs) + 1) if prefixes else [len(trs)]):
        b = K.batch(trs[:n])
        want = po.match_batch(g, b, po.params(**{k: float(v) for k, v in opts.items()}))
        r = M.Matcher().match_batch(b, copy_out=True, route_work=True)
        assert r.status == 0, r.status
        c = [int(r.counters[k]) for k in range(24)]
        searched += c[6]
        retried += c[9]
        got = _lib.result_to_numpy(r)
        errors, stats = compare(got, want)
        assert not errors, (name, n, errors)
        r2 = M.Matcher().match_batch(b, copy_out=True, route_work=False)
        assert r2.status == 0, r2.status
        errors, stats = compare(_lib.result_to_numpy(r2), got)
        exact = [v for k, v in stats.items() if k.endswith('_bitexact')]  # (floats bit-exact too)
        assert not errors and exact and all(exact), (name, n, errors, stats)
        print(name, n, 'searches', c[6], 'settled', c[3], 'rounds', c[13], 'resumed', c[11], 'dumped', c[12])
        if prefixes:  # (c): searches of unequal round counts share the waves
            assert c[6] > 0 and c[13] %% c[6] != 0, (name, n, c[6], c[13])
        if retry:
            # forced stops after 2 (3) rounds: searches were dumped in one tier and resumed in
            # the next from the dump's synthesised pending marks (as tests/test_gpu_tiers.py)
            assert c[12] > 0 and c[11] > 0 and c[12] >= c[11], (name, n, c)
    assert searched > 0, name
    if retry:  # the retry tiers settled nodes: every first-tier search went down to them
        assert retried > 0, name
print('rounds ok')
'''


@pytest.mark.parametrize('retry', [False, True])
def test_route_rounds_equal_oracle(graph_dir, retry):
    env = dict(os.environ)
    for k in ('OTR_LIB', 'OTR_TIERS', 'OTR_EST_K', 'OTR_FORCE_EDGE', 'OTR_NDUMP_GB', 'OTR_OPT_RESERVE_GB'):
        env.pop(k, None)
    if retry:
        lib = os.path.join(ROOT, 'reporter_amd', 'libotr_tiercheck.so')
        assert os.path.exists(lib), 'build first: python -m reporter_amd.build'
        env.update(OTR_LIB=lib, OTR_FORCE_EDGE='128')
    p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, retry)], env=env, capture_output=True,
                       text=True, timeout=240)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and 'rounds ok' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
