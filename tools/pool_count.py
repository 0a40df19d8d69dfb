#!/usr/bin/env python3
"""Relax iterations of the two-search route tier with its lanes pooled against per group
(DESIGN.md 6s): the CPU simulation of the node searches' exact rounds (tools/edge_stats.c
nr_run) over a C2 sample, consecutive searches paired as a wave pairs its two tasks.
Analysis tool, not a test.

  python tools/pool_count.py [--traces 200]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po  # noqa: E402
from reporter_amd.tools import gen  # noqa: E402


class NrStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ('searches', 'settled_base', 'rounds_base', 'settled_a', 'rounds_a',
                                              'stalls_a')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--traces', type=int, default=200)
    args = ap.parse_args()
    so = os.path.join(ROOT, 'tools', 'libedgestats.so')
    src = os.path.join(ROOT, 'tools', 'edge_stats.c')
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(['gcc', '-O2', '-std=gnu11', '-shared', '-fPIC', '-ffp-contract=off', '-o', so, src,
                               '-lm', '-lpthread'])
    L = ctypes.CDLL(so)
    gpath = gen.graph_path('metro', os.path.join(ROOT, 'build', 'graphs'))
    # the C2 traces: 100 points, 15 s, sigma 10 m, no turn costs (node searches)
    tr = gen.make_traces(gpath, args.traces, 100, 15, 10.0, 2, 0.0, 0.0, None)
    g = po.Graph(gpath)
    prm = po.params(turn_penalty_factor=0.0)
    S = NrStats()
    P = ctypes.POINTER
    L.nr_run.argtypes = [ctypes.c_void_p, P(po.Params), ctypes.c_int32, P(ctypes.c_int64), P(ctypes.c_double),
                         P(ctypes.c_double), P(ctypes.c_int64), ctypes.c_void_p, ctypes.c_double, P(NrStats)]
    L.nr_run(g.h, prm, tr.n_traces, tr.offsets.ctypes.data_as(P(ctypes.c_int64)),
             tr.lat.ctypes.data_as(P(ctypes.c_double)), tr.lon.ctypes.data_as(P(ctypes.c_double)),
             tr.time.ctypes.data_as(P(ctypes.c_int64)), None, 0.5, ctypes.byref(S))
    out = (ctypes.c_int64 * 4)()
    L.nr_pool_get(out)
    per_group, pooled, rounds, searches = (int(x) for x in out)
    # two adjacency slots per lane, and the probe chains of the 160-slot table
    ch = (ctypes.c_int64 * 7)()
    L.nr_chain_get(ch)
    two_slot, inserts, off_home, iters, past_home, past_home4, outgrown = (int(x) for x in ch)
    print(json.dumps({'traces': args.traces, 'searches': searches, 'settled_per_search': S.settled_base / max(searches, 1),
                      'rounds_per_search': S.rounds_base / max(searches, 1), 'pair_rounds': rounds,
                      'relax_iterations_per_group_rule': per_group, 'relax_iterations_pooled': pooled,
                      'pooled_fewer': round(1.0 - pooled / max(per_group, 1), 4),
                      'relax_iterations_per_pair_round': round(per_group / max(rounds, 1), 3),
                      'relax_iterations_two_slots': two_slot,
                      'two_slots_fewer': round(1.0 - two_slot / max(per_group, 1), 4),
                      'table160_inserts': inserts, 'inserts_off_home': round(off_home / max(inserts, 1), 4),
                      'table160_relax_iterations': iters,
                      'slowest_lane_slots_past_home': round(past_home / max(iters, 1), 4),
                      'slowest_lane_with_4_slot_reads': round(past_home4 / max(iters, 1), 4),
                      'searches_outgrowing_160': round(outgrown / max(searches, 1), 4)}))


if __name__ == '__main__':
    main()
