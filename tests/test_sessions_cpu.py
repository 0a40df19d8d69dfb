"""The session store's restatement (tests/sessions_ref.py) pinned without a GPU: known answers
for the gate, the float narrowing, the trims, eviction and the cap; the coordinate identity the
gather kernel relies on; what the streams of tests/test_gpu_sessions.py cover; and the layouts
of the new C structs."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from reporter_amd import _lib
from tests import sessions_ref as R
from tests.matched_points_ref import KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAT0, LON0 = np.float32(52.5), np.float32(13.4)


def north(metres):
    """A float32 latitude about `metres` north of LAT0."""
    return np.float32(float(LAT0) + metres / KM)


class Script:
    """A match callback that answers from a list and records what it was asked."""

    def __init__(self, *answers):
        self.answers, self.calls = list(answers), []

    def __call__(self, points, key, trigger):
        self.calls.append((key, trigger, points))
        su, ok = self.answers.pop(0)
        return su, ok, [(1, 2, 0.5, 1.5, 10, 0)] if ok else []


def feed(store, rows, key=1):
    """rows: (lat, lon, time[, timestamp]); returns the windows."""
    out = []
    for i, r in enumerate(rows):
        w = store.process(key, r[0], r[1], 3, r[2], r[3] if len(r) > 3 else 1000 * i, i)
        if w:
            out.append(w)
    return out


def walk(n, step_m=100.0, dt=10):
    return [(north(step_m * i), LON0, 1000 + dt * i) for i in range(n)]


def test_gate_fails_on_each_term_alone():
    # distance short (5 x 90 m = 450 m), count and time fine
    s = R.Store(Script(), 64, 500.0, 4, 30)
    assert not feed(s, walk(6, 90.0)) and len(s.sessions[1]['pts']) == 6
    # count short
    s = R.Store(Script(), 64, 500.0, 10, 30)
    assert not feed(s, walk(8, 100.0))
    # time short (7 x 4 s = 28 s)
    s = R.Store(Script(), 64, 500.0, 4, 30)
    assert not feed(s, walk(8, 100.0, 4))
    # all three pass at the sixth point: 505 m, 6 points, 50 s
    m = Script((None, True))
    s = R.Store(m, 64, 500.0, 6, 50)
    w = feed(s, walk(8, 101.0))
    assert [x['trigger'] for x in w] == [5] and w[0]['n_points'] == 6 and len(m.calls) == 1
    # the first point never reports, whatever the gates
    s = R.Store(Script(), 64, 0.0, 0, 0)
    assert s.process(1, LAT0, LON0, 3, 0, 0, 0) is None and float(s.sessions[1]['max_sep']) == 0.0


def test_max_sep_is_narrowed_to_float():
    """A distance whose binary64 value is below report_dist but whose float value is not: the
    gate compares the float."""
    lim = np.float32(500.0)
    found = None
    lat = north(500.0)
    for _ in range(4000):   # walk the float32 latitudes around 500 m
        d = R.dist(lat, LON0, LAT0, LON0)
        if d < float(lim) and np.float32(d) == lim:
            found = (lat, d)
            break
        lat = np.nextafter(lat, np.float32(0 if d > float(lim) else 90), dtype=np.float32)
    if found is None:
        # no latitude lands in the half-ulp below 500: take the limit from a distance instead
        lat = north(500.0)
        d = R.dist(lat, LON0, LAT0, LON0)
        lim = np.nextafter(np.float32(d), np.float32(1e9)) if np.float32(d) < d else np.float32(d)
        found = (lat, d)
    lat, d = found
    assert abs(float(np.float32(d)) - d) <= float(np.spacing(np.float32(d)))   # within one float ulp
    s = R.Store(Script((None, True)), 64, float(lim), 2, 0)
    w = feed(s, [(LAT0, LON0, 0), (lat, LON0, 1)])
    assert (len(w) == 1) == (not np.float32(d) < lim)
    assert s.sessions.get(1) is None or s.sessions[1]['max_sep'].dtype == np.float32
    # and the stored value is the float, not the double
    s = R.Store(Script(), 64, 1e9, 2, 0)
    feed(s, [(LAT0, LON0, 0), (lat, LON0, 1)])
    assert s.sessions[1]['max_sep'] == np.float32(d) and s.sessions[1]['max_sep'].dtype == np.float32


def test_partial_trim_recomputes_max_sep():
    m = Script((4, True), (None, True))
    s = R.Store(m, 64, 500.0, 6, 50)
    w = feed(s, walk(6, 101.0))
    assert w[0]['trimmed'] == 4 and w[0]['shape_used'] == 4 and len(w[0]['reports']) == 1
    pts = s.sessions[1]['pts']
    assert [p[3] for p in pts] == [1040, 1050]
    assert s.sessions[1]['max_sep'] == np.float32(R.dist(pts[1][0], pts[1][1], pts[0][0], pts[0][1]))
    # what the matcher saw: six-decimal coordinates, float accuracy, in order
    key, trig, seen = m.calls[0]
    assert (key, trig, len(seen)) == (1, 5, 6) and seen[0][3] == 3.0
    assert all(abs(p[0] * 1e6 - round(p[0] * 1e6)) < 1e-6 for p in seen)


def test_absent_shape_used_and_error_clear_the_session():
    for answer in ((None, True), (0, True), (3, False)):
        s = R.Store(Script(answer), 64, 500.0, 6, 50)
        w = feed(s, walk(6, 101.0))
        assert w[0]['trimmed'] == 6 and w[0]['shape_used'] == -1 and 1 not in s.sessions, answer
        assert w[0]['status'] == (0 if answer[1] else R.MATCH_ERROR)
        assert bool(w[0]['reports']) == answer[1]


def test_out_of_order_times():
    # at the gate: the last point's clock is behind the first's, so elapsed is negative
    rows = walk(8, 101.0)
    rows = [(r[0], r[1], 2000 - r[2]) for r in rows]
    s = R.Store(Script(), 64, 500.0, 6, 0)
    assert not feed(s, rows)
    # at eviction: negative elapsed does not report, zero does
    ev, n = s.punctuate(10 ** 9)
    assert (ev, n) == ([], 1) and not s.sessions
    s = R.Store(Script((None, True)), 64, 1e9, 99, 0)
    feed(s, [(LAT0, LON0, 5), (LAT0, LON0, 5)])
    ev, n = s.punctuate(10 ** 9)
    assert n == 1 and ev[0]['trigger'] == -1 and ev[0]['n_points'] == ev[0]['trimmed'] == 2


def test_eviction_exactly_at_the_gap_stays():
    s = R.Store(Script((None, True)), 64, 1e9, 99, 0, session_gap=60000)
    feed(s, [(LAT0, LON0, 1, 500), (LAT0, LON0, 2, 1000)])
    assert s.punctuate(61000) == ([], 0) and 1 in s.sessions
    ev, n = s.punctuate(61001)
    assert n == 1 and len(ev) == 1 and not s.sessions
    # a single point is deleted without a report; keys go in ascending order
    s = R.Store(Script((None, True), (None, True)), 64, 1e9, 99, 0)
    for key in (9, 3, 5):
        feed(s, [(LAT0, LON0, 1, 0)] * (1 if key == 3 else 2), key=key)
    ev, n = s.punctuate(10 ** 6)
    assert n == 3 and [(w['key'], w['trigger']) for w in ev] == [(5, -2), (9, -3)]


def test_cap():
    # standing still: the gate never passes, the 8th point forces a report
    s = R.Store(Script((3, True)), 8, 500.0, 4, 0)
    w = feed(s, [(LAT0, LON0, i) for i in range(8)])
    assert [x['trigger'] for x in w] == [7] and s.n_forced == 1 and len(s.sessions[1]['pts']) == 5
    # a clock running backwards: cleared and counted, the next point starts a session
    s = R.Store(Script(), 8, 500.0, 4, 0)
    assert not feed(s, [(LAT0, LON0, -i) for i in range(9)])
    assert (s.n_forced, s.n_dropped) == (0, 1) and len(s.sessions[1]['pts']) == 1


def test_coordinate_identity():
    """rint(f * 1e6) / 1e6 is what the six-decimal HALF_EVEN text of a float32 parses to: checked
    against Python's own '%.6f' (round-half-even on the exact binary value, and f * 1e6 is exact)
    on 2.3M values, every k/128 tie of the coordinate range included."""
    rng = np.random.RandomState(11)
    ties = (np.arange(-180 * 128, 180 * 128 + 1) / 128.0).astype(np.float32)
    vals = np.concatenate([ties, rng.uniform(-180, 180, 1200000).astype(np.float32),
                           rng.uniform(-1, 1, 600000).astype(np.float32),
                           (rng.randint(-180 * 10 ** 6, 180 * 10 ** 6, 455000) / 1e6).astype(np.float32)])
    assert len(vals) >= 2300000
    x = vals.astype(np.float64)
    from fractions import Fraction
    for v in x[::1151].tolist():   # the product is exact: 24 bits times 15625 * 2^6
        assert Fraction(v) * 10 ** 6 == Fraction(v * 1e6)
    got = np.rint(x * 1e6) / 1e6
    want = np.array(('\n'.join('%.6f' % v for v in x)).split('\n'), np.float64)
    assert np.array_equal(got, want)
    odd = ties[(np.arange(len(ties)) % 2) == 1].astype(np.float64) * 1e6
    assert np.all(odd - np.floor(odd) == 0.5)   # the ties are ties
    assert R.widen(np.float32(0.0078125)) == 0.007812 and R.widen(np.float32(0.0234375)) == 0.023438


def _kind(w):
    if w['status']:
        return 'error'
    if w['shape_used'] < 0:
        return 'absent'
    return 'partial' if w['trimmed'] < w['n_points'] else 'whole'


def test_scripted_stream_coverage():
    """What GPU job 1's stream reaches: every trim kind, probe chains, the cap both ways,
    sessions that continue over chunks, evictions that report and that do not."""
    s = R.Store(R.scripted_match, **{k: v for k, v in R.SCRIPT.items() if k != 'max_sessions'})
    kinds, seen, most_live = [], set(), 0
    reporting = silent = multi_lane = 0
    for p in range(R.SCRIPT_CHUNKS):
        pts, ts = R.scripted_chunk(p)
        assert len(set(pts['key'].tolist()) | set(s.sessions)) <= R.SCRIPT['max_sessions']
        multi_lane += int(np.max(np.unique(pts['key'], return_counts=True)[1]) > 1)
        seen |= set(pts['key'].tolist())
        kinds += [_kind(w) for w in s.push(pts)]
        most_live = max(most_live, len(s.sessions))
        ev, n = s.punctuate(ts)
        reporting += len(ev)
        silent += n - len(ev)
        assert s.sessions   # fresh sessions stay
    assert {'partial', 'absent', 'whole', 'error'} <= set(kinds)
    assert len(seen) >= 3 * R.SCRIPT['max_sessions'] and most_live >= 12 and multi_lane == R.SCRIPT_CHUNKS
    assert s.n_forced > 0 and s.n_dropped > 0 and reporting > 0 and silent > 0
    # keys whose home entries collide in the table of 32 (probe chains)
    from collections import Counter
    assert max(Counter(int(k) % 32 for k in seen).values()) >= 2


def test_city_stream_coverage(graph_dir):
    """What GPU job 2's stream reaches with the oracle as the matcher: partial and absent trims,
    a key that reports at consecutive points, an eviction that reports and one that does not."""
    from oracle import pyoracle as po
    path, pts = R.city_stream(graph_dir)
    G, prm = po.Graph(path), po.params(turn_penalty_factor=0)

    def match(points, key, trigger):
        return R.result_to_match(po.match_batch(G, R.window_traces(points), prm))

    cfg = {k: v for k, v in R.CITY.items() if k != 'max_sessions'}
    s = R.Store(match, **cfg)
    w = s.push(pts)
    kinds = [_kind(x) for x in w]
    print('city: %d windows %s, %d reports' % (len(w), {k: kinds.count(k) for k in set(kinds)},
                                               sum(len(x['reports']) for x in w)))
    assert kinds.count('partial') > 0 and kinds.count('absent') > 0
    assert sum(len(x['reports']) for x in w) > 0
    assert len(s.sessions) <= R.CITY['max_sessions'] and s.n_forced == 0 == s.n_dropped
    last = {}
    consecutive = 0
    arrival = {}
    for i, k in enumerate(pts['key'].tolist()):
        arrival.setdefault(k, []).append(i)
    for x in w:
        idx = arrival[x['key']].index(x['trigger'])
        consecutive += int(last.get(x['key']) == idx - 1)
        last[x['key']] = idx
    assert consecutive > 0
    ev, n = s.punctuate(int(pts['timestamp'].max()) + R.CITY['session_gap'] + 1)
    assert 0 < len(ev) < n and not s.sessions


def test_session_struct_layouts(tmp_path):
    """ctypes mirrors of the session structs have the C compiler's sizes and offsets."""
    if not shutil.which('gcc'):
        pytest.skip('no C compiler')
    structs = {'otr_session_config': _lib.SessionConfig, 'otr_session_points': _lib.SessionPoints,
               'otr_session_result': _lib.SessionResult, 'otr_session_snapshot': _lib.SessionSnapshot}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "otr.h"', 'int main(void) {']
    for cname, cls in structs.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
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
    assert len(got) == sum(1 + len(c._fields_) for c in structs.values())
