"""Every route tier still counts into, and reports from, the slot it had before its numbering
moved into reporter_amd/csrc/otr_tiers.h: route_tier_code[0..15], route_tier_work[t][0..3] of
every slot and counters[0..15, 22, 23] of a copy_out=True, route_work=True batch equal those
recorded on the commit named in tests/golden/route_tier_slots.json (the node-search cases of
tests/golden/route_work_counts.json, the city case with the deployed per-mode turn penalties,
which runs the edge-state tiers, and the city case on the tiercheck library, which sends every
search down the retry tiers).  Fields that differed between two recordings on that commit are
null / absent in the fixture and not compared.  Runs in a child process (one library per
process)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'route_tier_slots.json')
COUNTERS = list(range(16)) + [22, 23]
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
print('slots ' + json.dumps({
    'route_tier_code': [int(r.route_tier_code[t]) for t in range(16)],
    'route_tier_work': [[int(r.route_tier_work[t][k]) for k in range(4)] for t in range(16)],
    'counters': {str(k): int(r.counters[k]) for k in %r}}))
'''


def run_case(c, graph_dir):
    """The batch of fixture case c in a child process: its slots as a dict."""
    env = dict(os.environ)
    for k in ('OTR_LIB', 'OTR_TIERS', 'OTR_EST_K', 'OTR_FORCE_EDGE'):
        env.pop(k, None)
    if c['lib'] != 'libotr.so':
        env['OTR_LIB'] = os.path.join(ROOT, 'reporter_amd', c['lib'])
    p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, json.dumps(c), graph_dir, COUNTERS)], env=env,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('slots ')][-1]
    return json.loads(line[len('slots '):])


@pytest.mark.parametrize('case', ['city', 'metro', 'city_turns', 'city_tiercheck'])
def test_route_tier_slots_unchanged(graph_dir, case):
    with open(GOLDEN) as f:
        c = json.load(f)['cases'][case]
    got, want = run_case(c, graph_dir), c['slots']
    print(case, got)
    assert got['route_tier_code'] == want['route_tier_code']
    for t in range(16):
        for k in range(4):
            if want['route_tier_work'][t][k] is not None:
                assert got['route_tier_work'][t][k] == want['route_tier_work'][t][k], (t, k)
    assert set(want['counters']) >= {'5', '6', '7'}
    for k, v in want['counters'].items():
        assert got['counters'][k] == v, k
