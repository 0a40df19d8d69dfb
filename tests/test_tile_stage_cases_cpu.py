"""What tests/test_gpu_tile_stages.py relies on (CPU only: the oracle's result of ragged_city
and many_reports of tests/ragged.py, and the restatements oracle/tiles.py, oracle/hist.py).
These are requirements on the inputs, not measurements: when the generator, the graphs or the
defaults change, this file says which edge the GPU tests lost.

Boundaries (otr_kernels.h): k_tile_rows (K9) walks a trace's reports 64 at a time, places a
chunk's rows with a wave prefix sum over the reports' bucket counts and carries `base` across
chunks; k_histogram (K8) strides a trace's reports by 64 and indexes its window by
(bucket start - base) / quantisation; both run four traces per 256-thread block.

Three branches cannot be reached through matching, because real reports never take them (0 such
reports in both batches, pinned below): K9's and K8's filter (t1 - t0 <= .5, length 0, negative
queue), the simple rules' span limit (max bucket - min bucket > the trace's bucket count), and so
a lane without rows between lanes with rows.  They stay covered by tests/golden/bucket_cases.json
on the CPU and by the tile store's report adds (K15, tests/test_gpu_tile_store.py)."""
import numpy as np
import pytest

from oracle import hist as oh
from oracle import tiles as ot
from reporter_amd.tools import gen
from tests import ragged

BATCHES = ['ragged_city', 'many_reports']
BLOCK = 4  # traces per block of K8 / K9 (kTraceWaves)


def _batch(batch, graph_dir):
    path, tr, want, sec = ragged.oracle_result(batch, 'gtt', graph_dir)
    nrep = np.diff(want['trace_rep_off'])
    print('%s gtt: oracle %.2f s, reports per trace %s' % (batch, sec, nrep.tolist()))
    return path, tr, want, nrep


def _buckets(want, first, last, q):
    """Per report: (kept by the filter, buckets under the simple rules, within the span limit,
    buckets under the stream rules), restated from oracle/tiles.py."""
    off = want['trace_rep_off']
    out = []
    for t in range(len(off) - 1):
        lim = (int(last[t]) - int(first[t])) // q + 1
        for k in range(off[t], off[t + 1]):
            t0, t1 = float(want['rep_t0'][k]), float(want['rep_t1'][k])
            keep = t0 > 0 and t1 > 0 and t1 - t0 > .5 and int(want['rep_length'][k]) > 0 and \
                int(want['rep_queue'][k]) >= 0
            simple = int(np.ceil(t1)) // q - int(np.floor(t0)) // q + 1
            out.append((keep, simple, simple - 1 <= lim, int(t1) // q - int(t0) // q + 1, k - off[t]))
    return out


def test_many_reports_counts(graph_dir):
    _, tr, want, nrep = _batch('many_reports', graph_dir)
    T = tr.n_traces
    probes = np.diff(tr.offsets)
    assert probes.tolist() == ragged.MANY_LENS and nrep.tolist() == ragged.MANY_REPORTS
    # every chunk boundary of K8 / K9: one lane, a chunk less one, a whole chunk, one lane of the next
    assert {1, 63, 64, 65, 127, 128, 129, 192} <= set(nrep.tolist()) and nrep.max() >= 193
    assert any(probes[t] > 0 and nrep[t] == 0 for t in range(T)) and any(probes[t] == 0 for t in range(T))
    blocks = [range(b, min(b + BLOCK, T)) for b in range(0, T, BLOCK)]
    # a trace without reports (and one without probes) beside a long one in the same block
    assert any(any(nrep[t] == 0 and probes[t] > 0 for t in b) and any(probes[t] == 0 for t in b) and
               any(nrep[t] >= 193 for t in b) for b in blocks)
    assert T % BLOCK != 0 and probes[T - 1] == 0  # (the last block is not full and ends in an empty trace)
    # ragged_city has no second chunk (the batch the other suites feed to K8)
    assert np.diff(ragged.oracle_result('ragged_city', 'gtt', graph_dir)[2]['trace_rep_off']).max() < 64


def test_many_reports_deployed_has_other_counts(graph_dir):
    """The one run under 'deployed' is another input, still with second and later chunks."""
    want = ragged.oracle_result('many_reports', 'deployed', graph_dir)[2]
    nrep = np.diff(want['trace_rep_off'])
    print('many_reports deployed: reports per trace %s' % nrep.tolist())
    assert nrep.tolist() != ragged.MANY_REPORTS and (nrep > 128).sum() >= 4 and (nrep == 0).sum() >= 2


@pytest.mark.parametrize('batch', BATCHES)
def test_rows_per_report(batch, graph_dir):
    _, tr, want, nrep = _batch(batch, graph_dir)
    first, last = ragged.trace_times(tr)
    for q in (3600, 60):
        b = _buckets(want, first, last, q)
        # the three branches matching never takes (module docstring)
        assert all(keep and ok for keep, _, ok, _, _ in b)
        simple = ot.rows_from_reports(want, first, last, q)
        stream = ot.stream_rows_from_reports(want, q)
        assert len(simple) == sum(x[1] for x in b) and len(stream) == sum(x[3] for x in b)
        files, per_file = np.unique(simple['file'], return_counts=True)
        multi = [x for x in b if x[1] >= 2]
        print('%s q %d: %d reports, %d simple rows, %d stream rows, %d reports of 2+ buckets, %d files, %d of '
              'one row' % (batch, q, len(b), len(simple), len(stream), len(multi), len(files),
                           int((per_file == 1).sum())))
        if q == 60:
            # a lane places more than one row, in the first chunk and (many_reports) in a later one
            assert len(multi) >= 30 and any(x[4] < 64 for x in multi)
            assert batch != 'many_reports' or any(x[4] >= 64 for x in multi)
            assert len(simple) != len(stream)  # the two rule sets differ
            assert len(files) > 50 and (per_file == 1).sum() >= 10  # K10's per-file runs: many small files
        elif batch == 'ragged_city':
            assert not multi and len(simple) == len(b) == len(stream)  # the prefix sum only adds ones
        else:
            # many_reports' traces last up to three hours: a report can lie across an hour boundary,
            # but at most two per trace and boundary (the one that ends in the new hour, and the one
            # whose ceil'd end touches it); all the others have one bucket
            crossings = sum(int(last[t]) // q - int(first[t]) // q for t in range(tr.n_traces) if nrep[t])
            assert len(multi) <= 2 * crossings and len(multi) * 100 < len(b)


def _indices(rows, q, base):
    """Per simple row: the floor index of its bucket in the window (the contract, oracle/hist.py)
    and the index that rounds toward zero (C++ `/`)."""
    d = (rows['file'] >> np.uint64(25)).astype(np.int64) * q - base
    return d // q, np.where(d < 0, -((-d) // q), d // q)


@pytest.mark.parametrize('batch,q', list(ragged.HIST_WINDOWS))
def test_histogram_windows(batch, q, graph_dir):
    from reporter_amd.graphfile import GraphFile
    path, tr, want, _ = _batch(batch, graph_dir)
    first, last = ragged.trace_times(tr)
    rows = ot.rows_from_reports(want, first, last, q)
    G = GraphFile(path)
    idx = {int(s): i for i, s in enumerate(G.seg_id)}
    names = [w[0] for w in ragged.HIST_WINDOWS[(batch, q)]]
    assert 'aligned' in names and 'unaligned' in names and (('inside' in names) or (batch, q) == ('ragged_city', 3600))
    bites = []
    for name, rel, hours in ragged.HIST_WINDOWS[(batch, q)]:
        base = gen.T_BEGIN + rel
        assert hours <= 20
        fl, tz = _indices(rows, q, base)
        inside = (fl >= 0) & (fl < hours)
        h, n = oh.histogram(want, first, last, idx, len(G.seg_id), base, hours, q)
        print('%s q %d %s: %d rows, floor keeps %d, truncation keeps %d, %d before, %d after' % (
            batch, q, name, len(rows), int(inside.sum()), int(((tz >= 0) & (tz < hours)).sum()), int((fl < 0).sum()),
            int((fl >= hours).sum())))
        assert n == len(rows) and int(h.sum()) == int(inside.sum())
        if name == 'aligned':
            assert rel == 0 and (fl == tz).all() and inside.any() and not (fl < 0).any()
        elif name == 'inside':
            assert rel % q == 0 and (fl == tz).all() and inside.any() and (fl < 0).any() and (fl >= hours).any()
        else:
            assert name.startswith('unaligned') and rel % q != 0
            # the rows of the bucket that starts less than one bucket before the base: left out by
            # the restatement, counted in hour 0 by a truncating index
            edge = (fl == -1)
            assert (tz[edge] == 0).all() and (fl[~edge] == tz[~edge])[fl[~edge] >= 0].all()
            assert int(h.sum()) + int(edge.sum()) == int(((tz >= 0) & (tz < hours)).sum())
            bites.append(bool(edge.any()))
    # (T_BEGIN + 630 at 60 s finds no row of many_reports in the bucket before it: that batch has a
    # second unaligned window, where its traces are busy)
    assert any(bites), (batch, q)
