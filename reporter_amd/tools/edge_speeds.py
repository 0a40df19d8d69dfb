"""Per-edge traversals and speeds of a named workload (gen.CONFIGS: C1, C2): the edge
traversals (K13, include/otr.h otr_edge_traversals) and the speed entries made of the complete
ones (otr_edge_observations), counted; the share of each trace's true edges (the generator's,
consecutive-distinct) that occur among its traversal edges; the device time of K13 beside the
wall time of the batch with and without it.

    python -m reporter_amd.tools.edge_speeds C1 [--traces N] [--steps K] [--out FILE]

Prints one JSON line and stores it (default profiles/edge_traversals_<workload>.json; --out -
stores nothing).  The match options are bench.py's for the workload (match_quality.options).
Needs a GPU; no threshold is applied: the figures are what they are."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def figures(trav, truth, probe_off):
    """The counts from the traversal arrays, and how many of the true edges they hold: truth is
    the generator's edge per probe, probe_off the traces' probe offsets."""
    n = int(len(trav['edge']))
    complete = (trav['f0'] == 0.0) & (trav['f1'] == 1.0)
    out = {'traversals': n, 'complete': int(complete.sum()),
           'complete_share': round(float(complete.mean()), 6) if n else None,
           'zero_length': int((trav['s0_mm'] == trav['s1_mm']).sum())}
    shares, found, total = [], 0, 0
    toff = trav['trace_off']
    for t in range(len(toff) - 1):
        tr = np.asarray(truth[int(probe_off[t]):int(probe_off[t + 1])])
        if len(tr) == 0:
            continue
        true = tr[np.concatenate([[True], tr[1:] != tr[:-1]])]
        hit = int(np.isin(true, trav['edge'][int(toff[t]):int(toff[t + 1])]).sum())
        shares.append(hit / len(true))
        found += hit
        total += len(true)
    out['true_edges'] = total
    out['true_edge_share'] = round(found / total, 6) if total else None
    out['true_edge_share_trace_mean'] = round(float(np.mean(shares)), 6) if shares else None
    return out


def main(argv=None):
    from . import gen
    from .match_quality import options
    from .. import matcher as M
    from .. import simple_reporter as sr
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('workload', choices=sorted(k for k in gen.CONFIGS if k in ('C1', 'C2')))
    ap.add_argument('--traces', type=int, default=None, help='fewer traces than the workload has')
    ap.add_argument('--steps', type=int, default=3, help='timed repetitions (the median is reported)')
    ap.add_argument('--out', default=None, help='where the line is stored (- : nowhere)')
    args = ap.parse_args(argv)
    path, tr = gen.config_traces(args.workload, args.traces)
    M.configure(M.default_config(path, **options(args.workload)))
    m = M.Matcher()
    m.match_batch(tr, copy_out=False)   # warm-up: buffers, code objects
    m.match_batch(tr, copy_out=False, edge_traversals=True)

    def timed(**kw):
        ms = []
        for _ in range(max(1, args.steps)):
            t0 = time.perf_counter()
            m.match_batch(tr, **kw)
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms))
    plain_ms = timed(copy_out=False)
    with_ms = timed(copy_out=False, edge_traversals=True)
    m.match_batch(tr, copy_out=False, timing=True, edge_traversals=True)
    k13_ms = float(m.edge_traversals_result().kernel_ms)
    m.match_batch(tr, copy_out=True, edge_traversals=True)
    out = {'workload': args.workload, 'traces': int(tr.n_traces), 'probes': int(tr.n_probes)}
    out.update(figures(m.edge_traversals(), np.asarray(tr.truth), np.asarray(tr.offsets)))
    t0 = time.perf_counter()
    ptr, n = m.edge_observations(3600)
    obs_ms = (time.perf_counter() - t0) * 1e3
    red = sr.hist_reduce(m, ptr, n, privacy=1)
    bins = np.bincount(red['speed_bin'], weights=red['count'], minlength=8).astype(np.int64)
    out.update(entries=int(n), entries_per_bin=[int(x) for x in bins], reduced_entries=int(len(red)),
               k13_ms=round(k13_ms, 4), observations_wall_ms=round(obs_ms, 3), batch_ms=round(plain_ms, 3),
               batch_with_traversals_ms=round(with_ms, 3))
    line = json.dumps(out)
    print(line)
    dst = args.out or os.path.join(ROOT, 'profiles', 'edge_traversals_%s.json' % args.workload.lower())
    if dst != '-':
        with open(dst, 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
