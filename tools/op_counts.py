#!/usr/bin/env python3
"""GPU operations per bench step from one rocprofv3 run in CSV form (--kernel-trace
--memory-copy-trace --hip-trace --output-format csv; no counters):
    python tools/op_counts.py <rocprofv3 output dir> [out.csv]
A step is the span between two consecutive k_link launches (one per device batch): the tail of
one batch, the owner's histogram reduce and the head of the next, i.e. one whole step of the
pipeline.  The last `--steps` batches of the run are the timed ones; their N - 1 whole spans
are averaged.  Classes: kernel dispatches (all, fills and device copy kernels included), fills
(__amd_rocclr_fillBuffer*), copies (the memory-copy trace plus __amd_rocclr_copyBuffer*
kernels), hipStreamSynchronize calls (spans on the host clock, joined to the k_link launches by
correlation id), and the hipcub / rocprim kernels among the dispatches."""
import csv
import glob
import os
import sys


def rows(d, suffix):
    out = []
    for f in sorted(glob.glob(os.path.join(d, '**', '*' + suffix), recursive=True)):
        with open(f, newline='') as fh:
            out += list(csv.DictReader(fh))
    return out


def per_span(stamps, bounds):
    """Mean number of stamps per span [bounds[i], bounds[i + 1])."""
    if len(bounds) < 2:
        return None
    n = sum(1 for t in stamps if bounds[0] <= t < bounds[-1])
    return n / (len(bounds) - 1)


def main(d, out, steps=5):
    kern = rows(d, 'kernel_trace.csv')
    copies = rows(d, 'memory_copy_trace.csv')
    api = rows(d, 'hip_api_trace.csv')
    link = sorted((int(k['Start_Timestamp']), k.get('Correlation_Id')) for k in kern if 'k_link' in k['Kernel_Name'])
    assert len(link) >= steps, 'fewer k_link launches (%d) than timed steps' % len(link)
    dev_bounds = [t for t, _ in link[-steps:]]
    by_corr = {a.get('Correlation_Id'): int(a['Start_Timestamp']) for a in api if 'Launch' in a['Function']}
    host_bounds = [by_corr[c] for _, c in link[-steps:] if c in by_corr]
    name = lambda k: k['Kernel_Name']
    start = lambda rs: [int(r['Start_Timestamp']) for r in rs]
    classes = [
        ('kernel dispatches', start(kern), dev_bounds),
        ('fills', start([k for k in kern if 'fillBuffer' in name(k)]), dev_bounds),
        ('copies (copy trace)', start(copies), dev_bounds),
        ('copies (copyBuffer kernels)', start([k for k in kern if 'copyBuffer' in name(k)]), dev_bounds),
        ('hipcub / rocprim kernels', start([k for k in kern if 'rocprim' in name(k) or 'hipcub' in name(k)]), dev_bounds),
        ('k_post', start([k for k in kern if 'k_post' in name(k)]), dev_bounds),
        ('hipStreamSynchronize', start([a for a in api if a['Function'] == 'hipStreamSynchronize']),
         host_bounds if len(host_bounds) == steps else []),
        ('hipMemcpyAsync', start([a for a in api if a['Function'] == 'hipMemcpyAsync']),
         host_bounds if len(host_bounds) == steps else []),
        ('hipMemsetAsync', start([a for a in api if a['Function'] == 'hipMemsetAsync']),
         host_bounds if len(host_bounds) == steps else []),
    ]
    w = csv.writer(out)
    w.writerow(['class', 'per_step', 'whole_run', 'spans'])
    for label, stamps, bounds in classes:
        p = per_span(stamps, bounds)
        w.writerow([label, '' if p is None else round(p, 2), len(stamps), max(len(bounds) - 1, 0)])


if __name__ == '__main__':
    main(sys.argv[1], open(sys.argv[2], 'w', newline='') if len(sys.argv) > 2 else sys.stdout)
