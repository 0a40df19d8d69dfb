"""The node search does the same work as before its instruction stream was trimmed (DESIGN.md
§6s): the work counters of a route_work=True batch (settled nodes, relaxations, transition
entries, searches, search rounds, table keys) of the two small node-search cases equal
those recorded on the commit named in tests/golden/route_work_counts.json.  Same rounds and
same settled counts mean the same algorithm.  Runs in a child process (one library per
process)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'route_work_counts.json')
CHILD = r'''
import json
import sys
sys.path.insert(0, %r)
from reporter_amd import matcher as M
from reporter_amd.tools import gen
c = json.loads(%r)
path = gen.graph_path(c['graph'], %r)
M.configure(M.default_config(path, **c['config']))
tr = gen.make_traces(path, c['traces'], c['points'], c['sample_rate'], c['sigma'], c['seed'], 0.0, 0.0, c['accuracy'])
r = M.Matcher().match_batch(tr, copy_out=True, route_work=True)
assert r.status == 0, r.status
print('counters ' + json.dumps({k: int(r.counters[int(k)]) for k in c['counters']}))
'''


@pytest.mark.parametrize('case', ['city', 'metro'])
def test_route_work_counters_unchanged(graph_dir, case):
    with open(GOLDEN) as f:
        c = json.load(f)['cases'][case]
    env = dict(os.environ)
    for k in ('OTR_LIB', 'OTR_TIERS', 'OTR_EST_K', 'OTR_FORCE_EDGE'):
        env.pop(k, None)
    p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, json.dumps(c), graph_dir)], env=env, capture_output=True,
                       text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('counters ')][-1]
    got = json.loads(line[len('counters '):])
    print(case, got)
    assert got == c['counters'], (got, c['counters'])
