"""Ragged trace batches for the per-trace stages (k_link, k_viterbi, k_segments, k_histogram):
traces of 0 to 200 probes in one batch, forced steps and states without candidates at chosen
places, cut from gen.make_traces output with pure numpy.  A helper module (no tests, no
fixtures): tests/test_trace_stage_cases_cpu.py pins what the oracle makes of every case
(coverage), tests/test_gpu_trace_stages.py runs them through the three Viterbi variants.
many_reports, for the output stages (k_histogram, k_tile_rows, the sort + cull): traces of up to
236 reports, pinned by tests/test_tile_stage_cases_cpu.py and run by tests/test_gpu_tile_stages.py.

The boundaries the cases sit on (otr_kernels.h): k_link and k_segments walk a trace in
chunks of 64 states / 64 active states and carry values across chunks; k_viterbi backtracks
in LDS up to VitLds<G>::N states (128 one trace per wave, 104 two per wave) and K <= 32.
"""
import numpy as np

from reporter_amd import matcher as M
from reporter_amd.tools import gen

CHUNK = 64           # states per k_link chunk, active states per k_segments chunk
LDS_STATES = (104, 128)  # VitLds<2>::N, VitLds<1>::N


# ---- builders -----------------------------------------------------------------------------
def _copy(tr):
    return gen.Traces(tr.lat.copy(), tr.lon.copy(), tr.time.copy(), tr.offsets.copy(), tr.mode.copy(),
                      None if tr.accuracy is None else tr.accuracy.copy(),
                      None if tr.truth is None else tr.truth.copy(), None if tr.uuids is None else list(tr.uuids))


def prefixes(full, lens):
    """The first lens[t] probes of every trace of `full` (0 allowed)."""
    lens = np.asarray(lens, np.int64)
    have = np.diff(full.offsets)
    assert len(lens) == full.n_traces and (lens >= 0).all() and (lens <= have).all(), (lens, have)
    parts = [np.arange(full.offsets[t], full.offsets[t] + lens[t]) for t in range(full.n_traces)]
    sel = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    off = np.zeros(full.n_traces + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return gen.Traces(full.lat[sel].copy(), full.lon[sel].copy(), full.time[sel].copy(), off, full.mode.copy(),
                      None if full.accuracy is None else full.accuracy[sel].copy(),
                      None if full.truth is None else full.truth[sel].copy(),
                      None if full.uuids is None else list(full.uuids))


def jump(tr, t, probe, dlat):
    """Shift trace t by dlat degrees of latitude from `probe` on (in place): with more than
    the breakage distance between probe - 1 and probe the step is forced."""
    a, b = int(tr.offsets[t]), int(tr.offsets[t + 1])
    assert 0 < probe < b - a, (t, probe, b - a)
    tr.lat[a + probe:b] += dlat
    return tr


def off_graph(tr, t, probes):
    """Move single probes of trace t one degree north (in place): far from every edge, so
    their states keep no candidates."""
    a, b = int(tr.offsets[t]), int(tr.offsets[t + 1])
    p = np.asarray(list(probes), np.int64)
    assert len(p) == 0 or (p.min() >= 0 and p.max() < b - a), (t, p, b - a)
    tr.lat[a + p] += 1.0
    return tr


def pin_lat(tr, t, probes, lat):
    """Put single probes of trace t on the latitude `lat` (in place), keeping their
    longitudes: just outside the graph's last row they reach few edges."""
    a, b = int(tr.offsets[t]), int(tr.offsets[t + 1])
    p = np.asarray(list(probes), np.int64)
    assert len(p) == 0 or (p.min() >= 0 and p.max() < b - a), (t, p, b - a)
    tr.lat[a + p] = lat
    return tr


def reorder(tr, perm):
    """The traces in the order perm (trace i of the result is trace perm[i] of tr)."""
    perm = np.asarray(perm, np.int64)
    assert sorted(perm.tolist()) == list(range(tr.n_traces))
    return tr.subset(perm)


# ---- configurations -----------------------------------------------------------------------
# name: (options for every mode, per-mode sections).  deployed / gtt as in test_gpu_parity;
# mixed: auto keeps the deployment's turn_penalty_factor 200, bicycle and pedestrian get 0,
# so a two-trace Viterbi wave holds one trace with turn costs and one without.
CONFIGS = {
    'deployed': ({}, {}),
    'gtt': ({'turn_penalty_factor': 0}, {}),
    'mixed': ({}, {'bicycle': {'turn_penalty_factor': 0}, 'pedestrian': {'turn_penalty_factor': 0}}),
    # the options of test_more_than_32_candidates (wide_K's own)
    'wide': ({'search_radius': 200, 'max_search_radius': 200, 'max_candidates': 64, 'turn_penalty_factor': 0}, {}),
}


def engine_config(path, cfg):
    over, modes = CONFIGS[cfg]
    d = M.default_config(path, **over)
    for m, sec in modes.items():
        d['meili'][m].update(sec)
    return d


def oracle_params(cfg):
    from oracle import pyoracle as po
    over, modes = CONFIGS[cfg]
    return po.params(modes={m: {k: float(v) for k, v in sec.items()} for m, sec in modes.items()},
                     **{k: float(v) for k, v in over.items()})


# ---- the case batches ---------------------------------------------------------------------
# ragged_city: probe counts on both sides of 64, 104 and 128 (every probe of these traces
# becomes a state: 15 s apart), then eight more boundary lengths ordered for the pairs
# (2i, 2i + 1) a two-trace wave holds: (22, 23) long before empty, (24, 25) short before long
# and <= 104 next to > 104, (26, 27) > 104 before <= 104, (28, 29) one probe before 128, and
# trace 30 alone in the last wave.
CITY_LENS = [0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 66, 103, 104, 105, 106, 127, 128, 129, 130, 191, 192, 193, 200,
             0, 64, 129, 105, 104, 1, 128, 65]
CITY_SEED = 31
JUMP = 0.025   # degrees of latitude, 2.8 km: beyond breakage_distance (2 km), within the 10 km graph
CITY_LAT = gen.GRAPHS['city'][3]


def _toward_centre(tr, t, probe):
    """The jump of JUMP degrees at `probe` of trace t that points to the graph's centre."""
    lat = tr.lat[int(tr.offsets[t]) + probe]
    return -JUMP if lat > CITY_LAT else JUMP


def _zigzag(tr, t, first, every, n):
    """n jumps from `first` on, one every `every` probes, there and back: n forced steps."""
    d = _toward_centre(tr, t, first)
    for i in range(n):
        jump(tr, t, first + i * every, d if i % 2 == 0 else -d)


def ragged_city(graph_dir):
    path = gen.graph_path('city', graph_dir)
    full = gen.make_traces(path, len(CITY_LENS), 200, 15, 10.0, CITY_SEED, 0.3, 0.2, t_begin=gen.T_BEGIN,
                           t_spread=1800)
    tr = prefixes(full, CITY_LENS)
    # trace 3 (3 probes): states, none of them active
    off_graph(tr, 3, range(3))
    # trace 9 (65): a forced step into state 64: a sub-path ends at ordinal 63 and the next
    # starts at 64, the first state of the second chunk
    jump(tr, 9, 64, _toward_centre(tr, 9, 64))
    # trace 15 (127): no candidates at state 63 (the last of a chunk); trace 18 (130): at 64
    off_graph(tr, 15, [63])
    off_graph(tr, 18, [64])
    # trace 19 (191): states 40..109 without candidates: the k_link chunk 64..127 starts with
    # 46 inactive states; trace 20 (192): probes 60..131 off the graph, so all of the chunk
    # 64..127 is inactive and `last` reaches the states after it from before it
    off_graph(tr, 19, range(40, 110))
    off_graph(tr, 20, range(60, 132))
    # trace 21 (193): ends in 20 states without candidates
    off_graph(tr, 21, range(173, 193))
    # trace 22 (200): a forced step every 3 probes: more than 60 sub-paths, many of them one
    # or two states long, over four chunks
    _zigzag(tr, 22, 3, 3, 64)
    # trace 25 (129, beside a 64-probe trace in its wave): one forced step at state 100
    jump(tr, 25, 100, _toward_centre(tr, 25, 100))
    return path, tr


# many_reports: traces with many more reports than ragged_city's (at most 51), for the stages
# that walk a trace's reports 64 at a time (k_histogram, k_tile_rows): prefixes of six long city
# traces (700 probes, 15 s apart), the prefix lengths found by a search on the oracle so that
# the report counts per trace under 'gtt' are MANY_REPORTS (pinned by
# tests/test_tile_stage_cases_cpu.py; each length sits inside the range of lengths that give its
# count).  (source trace, probes, reports), four traces per 256-thread block of K8 / K9: an
# empty trace and one with probes and no report beside the longest, 64 | 65 and 128 | 129 beside
# each other, three whole chunks (192) and the last block with three traces only.
MANY_SEED = 77
MANY = [(0, 0, 0), (1, 692, 236), (1, 8, 0), (2, 228, 64),
        (0, 247, 65), (0, 6, 1), (1, 375, 128), (2, 533, 129),
        (2, 222, 63), (1, 366, 127), (4, 680, 192), (4, 688, 194),
        (5, 657, 200), (3, 8, 2), (3, 0, 0)]
MANY_SRC = [m[0] for m in MANY]
MANY_LENS = [m[1] for m in MANY]
MANY_REPORTS = [m[2] for m in MANY]


def many_reports(graph_dir):
    path = gen.graph_path('city', graph_dir)
    full = gen.make_traces(path, 6, 700, 15, 10.0, MANY_SEED, t_begin=gen.T_BEGIN, t_spread=1800)
    return path, prefixes(full.subset(MANY_SRC), MANY_LENS)


# The dense histogram's windows for tests/test_gpu_tile_stages.py, per (batch, quantisation):
# (name, base - T_BEGIN, buckets).  aligned: the base every caller passes; inside: an aligned
# base after the first reports with an end before the last ones, so rows fall outside on both
# sides (ragged_city ends within its first hour: no such window at 3600); unaligned: a base
# that is no multiple of the quantisation, where the bucket that starts less than one bucket
# before the base has the floor index -1 (left out: include/otr.h "covers [base, ...)") and
# the truncated index 0.  One bucket is n_segments x 8 counters (1.7 MB for the city graph).
HIST_WINDOWS = {
    ('ragged_city', 3600): [('aligned', 0, 3), ('unaligned', 1800, 2)],
    ('ragged_city', 60): [('aligned', 0, 20), ('inside', 1200, 20), ('unaligned', 630, 20)],
    ('many_reports', 3600): [('aligned', 0, 4), ('inside', 3600, 1), ('unaligned', 1800, 2)],
    ('many_reports', 60): [('aligned', 0, 20), ('inside', 3600, 20), ('unaligned', 630, 20),
                             ('unaligned_busy', 3630, 20)],
}


def trace_times(tr):
    """(first, last) probe time of every trace, 0 for a trace without probes."""
    n = np.diff(tr.offsets)
    first = np.where(n > 0, tr.time[np.minimum(tr.offsets[:-1], len(tr.time) - 1)], 0)
    last = np.where(n > 0, tr.time[np.maximum(tr.offsets[1:] - 1, 0)], 0)
    return first, last


def tiny_T(graph_dir, T):
    """ragged_city's 129-, 104- and 1-probe traces, the first T of them."""
    assert 1 <= T <= 3
    path, tr = ragged_city(graph_dir)
    return path, tr.subset([17, 12, 1][:T])


WIDE_LENS = [60, 127, 128, 129, 130, 140, 100, 135]


def _north_of(graph, metres):
    """The latitude `metres` north of the last row of nodes of a generated graph (otrgen.cpp:
    row r lies (r - rows / 2) * spacing north of the centre)."""
    rows, _, spacing, lat = gen.GRAPHS[graph][:4]
    return lat + ((rows - 1 - rows // 2) * spacing + metres) / (20037581.187 / 180.0)


def wide_K(graph_dir):
    path = gen.graph_path('metro', graph_dir)
    full = gen.make_traces(path, len(WIDE_LENS), 140, 30, 30.0, 9, 0.0, 0.0, 50.0)
    tr = prefixes(full, WIDE_LENS)
    # trace 5 (140): its first 20 probes on a line 170 m outside the graph, where the 200 m
    # radius reaches a few edges of the last row only (K <= 32), then back onto its track
    # (K > 32): the trace stops fitting k_viterbi<1>'s LDS table part-way
    pin_lat(tr, 5, range(20), _north_of('metro', 170.0))
    return path, tr


# case name -> (builder(graph_dir) -> (graph path, traces), configurations)
CASES = {
    'ragged_city': (ragged_city, ('deployed', 'gtt', 'mixed')),
    'tiny_T1': (lambda d: tiny_T(d, 1), ('gtt',)),
    'tiny_T2': (lambda d: tiny_T(d, 2), ('gtt',)),
    'tiny_T3': (lambda d: tiny_T(d, 3), ('gtt',)),
    'wide_K': (wide_K, ('wide',)),
}

# batches of other test files (tests/test_gpu_tile_stages.py), kept out of CASES so that
# tests/test_gpu_trace_stages.py keeps its jobs; oracle_result() knows them too
OTHER_BATCHES = {'many_reports': many_reports}

# the two fixed permutations of ragged_city for the neighbour test: the reversal, and a
# shuffle that moves every trace to the other half of a wave or to another partner
PERMS = {
    'reversed': list(range(len(CITY_LENS) - 1, -1, -1)),
    'shuffled': [int(x) for x in np.random.default_rng(5).permutation(len(CITY_LENS))],
}


_ORACLE = {}


def oracle_result(case, cfg, graph_dir):
    """(graph path, traces, the oracle's result, its seconds) of a case under a
    configuration, computed once per process; callers leave the result unchanged."""
    import time
    from oracle import pyoracle as po
    key = (case, cfg)
    if key not in _ORACLE:
        build = CASES[case][0] if case in CASES else OTHER_BATCHES[case]
        path, tr = build(graph_dir)
        t0 = time.perf_counter()
        want = po.match_batch(po.Graph(path), tr, oracle_params(cfg), threads=8)
        _ORACLE[key] = (path, tr, want, time.perf_counter() - t0)
    return _ORACLE[key]


# ---- what a case covers -------------------------------------------------------------------
def coverage(want, tr):
    """From the oracle's result `want` of batch `tr`: per trace the numbers of states and of
    active states (K > 0), the active ordinals that start a sub-path, the indices (within
    the trace) of the states without candidates; and the largest K of the batch."""
    off = np.asarray(want['trace_state_off'], np.int64)
    K = np.asarray(want['cand_count'])
    sub = np.asarray(want['subpath'])
    assert len(off) == tr.n_traces + 1
    states, active, breaks, empty = [], [], [], []
    for t in range(tr.n_traces):
        k = K[off[t]:off[t + 1]]
        on = np.flatnonzero(k > 0)
        sp = sub[off[t]:off[t + 1]][on]
        states.append(int(len(k)))
        active.append(int(len(on)))
        breaks.append([int(i) for i in range(len(sp)) if i == 0 or sp[i] != sp[i - 1]])
        empty.append([int(i) for i in np.flatnonzero(k <= 0)])
    return {'states': states, 'active': active, 'breaks': breaks, 'empty': empty,
            'max_k': int(K.max()) if len(K) else 0}
