"""How good is the match?  For a named workload (gen.CONFIGS: C1, C2) the matched points
(K12, include/otr.h otr_matched_points) against the generator's truth: the share of state
and of interpolated probes whose matched edge is the edge the generator drove, and the
mean and 95th percentile of the distance between a probe and its matched point.  Also the
device time of K12 beside the wall time of the batch with and without it.

    python -m reporter_amd.tools.match_quality C1 [--traces N] [--steps K]

Prints one JSON line.  The match options are bench.py's for the workload (the
generate_test_trace.py request: turn_penalty_factor 0, gps_accuracy = the noise's 95th
percentile).  Needs a GPU; no threshold is applied: the figures are what they are."""
import argparse
import json
import sys
import time

import numpy as np


def options(name):
    from . import gen
    sigma, radius = gen.CONFIGS[name][4], gen.CONFIGS[name][8]
    return {'turn_penalty_factor': 0, 'beta': 3, 'sigma_z': 4.07, 'breakage_distance': 2000,
            'search_radius': radius, 'gps_accuracy': round(min(100.0, 1.645 * max(1.0, sigma)), 2)}


def quality(points, truth):
    """The figures from the per-probe arrays and the generator's true edges."""
    kind, edge, dist = points['kind'], points['edge'], points['dist']
    out = {'probes': int(len(kind))}
    for k, name in ((1, 'state'), (2, 'interpolated'), (0, 'unmatched')):
        out[name + '_probes'] = int((kind == k).sum())
    for k, name in ((1, 'state'), (2, 'interpolated')):
        sel = kind == k
        out[name + '_true_edge_share'] = round(float((edge[sel] == truth[sel]).mean()), 6) if sel.any() else None
    on = kind > 0
    out['matched_true_edge_share'] = round(float((edge[on] == truth[on]).mean()), 6) if on.any() else None
    out['dist_mean_m'] = round(float(dist[on].mean()), 4) if on.any() else None
    out['dist_p95_m'] = round(float(np.percentile(dist[on], 95)), 4) if on.any() else None
    return out


def main(argv=None):
    from . import gen
    from .. import matcher as M
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('workload', choices=sorted(k for k in gen.CONFIGS if k in ('C1', 'C2')))
    ap.add_argument('--traces', type=int, default=None, help='fewer traces than the workload has')
    ap.add_argument('--steps', type=int, default=3, help='timed repetitions (the median is reported)')
    args = ap.parse_args(argv)
    path, tr = gen.config_traces(args.workload, args.traces)
    M.configure(M.default_config(path, **options(args.workload)))
    m = M.Matcher()
    m.match_batch(tr, copy_out=False)   # warm-up: buffers, code objects

    def timed(**kw):
        ms, r = [], None
        for _ in range(max(1, args.steps)):
            t0 = time.perf_counter()
            r = m.match_batch(tr, **kw)
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms)), r
    plain_ms, _ = timed(copy_out=False, timing=True)
    with_ms, _ = timed(copy_out=False, timing=True, matched_points=True)
    k12_ms = float(m.matched_points_result().kernel_ms)
    m.match_batch(tr, copy_out=True, matched_points=True)
    out = {'workload': args.workload, 'traces': int(tr.n_traces)}
    out.update(quality(m.matched_points(), np.asarray(tr.truth)))
    out.update(k12_ms=round(k12_ms, 4), batch_ms=round(plain_ms, 3), batch_with_points_ms=round(with_ms, 3))
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
