"""The plain bench run (no --full): warm-up, --steps timed steps, the headline line with
ms_per_step and nothing of the --full legs, and --dump-outputs: the last timed step's tile
rows and owned histogram entries as float64 .npy files, equal to what the same batch gives
through the library in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GTT = {'turn_penalty_factor': 0, 'beta': 3, 'sigma_z': 4.07, 'breakage_distance': 2000}


def _columns(a):
    """bench.dump_outputs' layout of a record array: 64-bit ids as (low, high) 32-bit columns."""
    cols = []
    for f in a.dtype.names:
        if a.dtype[f] == np.dtype('<u8'):
            cols += [(a[f] & 0xFFFFFFFF).astype(np.float64), (a[f] >> 32).astype(np.float64)]
        else:
            cols.append(a[f].astype(np.float64))
    return np.stack(cols, axis=1)


def test_plain_run_line_and_dump(graph_dir, tmp_path):
    from reporter_amd import _lib
    from reporter_amd import matcher as M
    from reporter_amd import simple_reporter as sr
    from reporter_amd.tools import gen
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--workload', 'c1',
                          '--traces-per-gpu', '200', '--steps', '3', '--warmup', '1', '--dump-outputs',
                          str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{')][-1])
    assert line['metric'] == 'GPS probes matched/sec (whole node)' and line['unit'] == 'probes/s'
    assert line['higher_is_better'] is True and line['dtype'] == 'f64'
    assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0
    probes = line['config']['probes_per_step']
    assert probes == 200 * 300
    # value and ms_per_step are the same measurement (both rounded in the line)
    assert abs(line['value'] * line['ms_per_step'] * 1e-3 / probes - 1) < 1e-3
    for leg in ('cpu_baseline', 'parity', 'end_to_end', 'json_dropin', 'roofline'):
        assert leg not in line

    dumped = {f[:-4]: np.load(str(tmp_path / f)) for f in os.listdir(str(tmp_path)) if f.endswith('.npy')}
    assert set(dumped) == {'batch_counts', 'hist_entries', 'tile_rows'}
    assert all(a.dtype == np.float64 for a in dumped.values())
    assert sum(a.nbytes for a in dumped.values()) <= 64 << 20

    # the same batch through the library here
    gp = gen.graph_path('city', graph_dir)
    M.configure(M.default_config(gp, **dict(GTT, search_radius=50, gps_accuracy=8.22)))
    tr = gen.make_traces(gp, 200, 300, 1, 5.0, 1, 0.0, 0.0, None, t_begin=gen.T_BEGIN, t_spread=1800)
    m = M.Matcher()
    r = m.match_batch(tr, copy_out=False, tile_rows=True)
    assert r.status == 0 and int(r.n_rows) > 0
    rows = sr.cull_rows(m, None, 1, device_ptr=r.d_rows, n=r.n_rows)  # privacy 1: every row, sorted per file
    want = sr.hist_reduce(m, r.d_rows, r.n_rows, privacy=2, rows_in=True)
    assert len(want) > 0
    assert np.array_equal(dumped['hist_entries'], _columns(want))
    assert dumped['tile_rows'].shape == (int(r.n_rows), 12)
    got_rows, want_rows = dumped['tile_rows'], _columns(rows)  # (the bench's in trace order: compare sorted)
    assert np.array_equal(got_rows[np.lexsort(got_rows.T[::-1])], want_rows[np.lexsort(want_rows.T[::-1])])
    assert dumped['batch_counts'].tolist() == [[200.0, 60000.0, float(r.n_states), float(r.n_rows), 0.0]]
    assert json.load(open(str(tmp_path / 'hist_entries.columns.json'))) == [
        'file_lo32', 'file_hi32', 'id_lo32', 'id_hi32', 'next_id_lo32', 'next_id_hi32', 'speed_bin', 'count']
