"""The case batches of tests/ragged.py still sit on the boundaries the per-trace kernels have
(CPU only: the oracle's result of every case and configuration).  These are requirements on
the inputs of tests/test_gpu_trace_stages.py, not measurements: when the generator, the
graphs or the defaults change, this file says which edge the GPU tests lost.

Boundaries (otr_kernels.h): k_link walks a trace's states in chunks of 64 and carries `last`;
k_segments walks its active states (K > 0) in chunks of 64 and carries c_pos, c_ent, c_sa and
emitted_any; k_viterbi backtracks in LDS up to 104 (two traces per wave) or 128 states and
while K <= 32."""
import numpy as np
import pytest

from tests import ragged

CITY_CFGS = ragged.CASES['ragged_city'][1]


def _cov(case, cfg, graph_dir):
    path, tr, want, sec = ragged.oracle_result(case, cfg, graph_dir)
    print('%s %s: oracle %.2f s, %d states, %d segments, %d reports' % (
        case, cfg, sec, len(want['state_probe']), len(want['seg_id']), len(want['rep_id'])))
    return tr, want, ragged.coverage(want, tr)


def _runs(idx):
    """Maximal runs of consecutive integers in a sorted list: [(first, last)]."""
    out = []
    for i in idx:
        if out and i == out[-1][1] + 1:
            out[-1][1] = i
        else:
            out.append([i, i])
    return [tuple(r) for r in out]


def test_builders():
    from reporter_amd.tools import gen
    n = 4
    full = gen.Traces(np.arange(20.0), np.arange(20.0) + 100, np.arange(20, dtype=np.int64),
                      np.arange(n + 1, dtype=np.int64) * 5, np.array([0, 1, 2, 0], np.uint8), None, None,
                      ['a', 'b', 'c', 'd'])
    tr = ragged.prefixes(full, [0, 5, 2, 1])
    assert tr.offsets.tolist() == [0, 0, 5, 7, 8] and tr.lat.tolist() == [5, 6, 7, 8, 9, 10, 11, 15]
    assert tr.mode.tolist() == [0, 1, 2, 0] and tr.uuids == ['a', 'b', 'c', 'd']
    ragged.jump(tr, 1, 3, 0.5)
    assert tr.lat.tolist() == [5, 6, 7, 8.5, 9.5, 10, 11, 15]
    ragged.off_graph(tr, 2, [1])
    assert tr.lat.tolist() == [5, 6, 7, 8.5, 9.5, 10, 12, 15] and tr.lon[6] == 111
    ragged.pin_lat(tr, 1, [0, 4], 3.0)
    assert tr.lat.tolist() == [3, 6, 7, 8.5, 3, 10, 12, 15]
    assert full.lat.tolist() == np.arange(20.0).tolist()  # (the source batch is left alone)
    r = ragged.reorder(tr, [3, 2, 1, 0])
    assert r.offsets.tolist() == [0, 1, 3, 8, 8] and r.lat.tolist() == [15, 10, 12, 3, 6, 7, 8.5, 3]
    assert r.mode.tolist() == [0, 2, 1, 0] and r.uuids == ['d', 'c', 'b', 'a']
    for p in ragged.PERMS.values():  # every trace gets another wave partner or another half of its wave
        assert sorted(p) == list(range(len(ragged.CITY_LENS)))
        pos = {t: i for i, t in enumerate(p)}

        def wave(order, i):  # (the other trace of position i's wave, the half of the wave i is in)
            return (order[i ^ 1] if i ^ 1 < len(order) else None, i & 1)
        for t in range(len(p)):
            assert wave(p, pos[t]) != wave(list(range(len(p))), t), (p, t)


@pytest.mark.parametrize('cfg', CITY_CFGS)
def test_ragged_city_covers_the_chunk_and_lds_boundaries(cfg, graph_dir):
    tr, want, c = _cov('ragged_city', cfg, graph_dir)
    T = tr.n_traces
    assert T == 31 and np.diff(tr.offsets).tolist() == ragged.CITY_LENS
    assert {0, 1, 2, 63, 64, 65, 104, 105, 128, 129} <= set(c['active']), sorted(set(c['active']))
    assert {104, 105, 128, 129} <= set(c['states']), sorted(set(c['states']))
    brk, emp, st, ac = c['breaks'], c['empty'], c['states'], c['active']
    # a sub-path ends at active ordinal 63 and the next starts at 64 (k_segments' second chunk)
    assert any(64 in brk[t] for t in range(T))
    assert any(64 in brk[t] and ac[t] > 64 for t in range(T))
    # more than 64 active states in one sub-path: c_pos, c_ent, c_sa cross a chunk
    assert any(ac[t] > 64 and brk[t] == [0] for t in range(T))
    # a sub-path that starts in one chunk and ends in a later one, after earlier sub-paths (emitted_any)
    assert any(len(brk[t]) > 1 and any(a < 64 <= b - 1 for a, b in zip(brk[t], brk[t][1:] + [ac[t]]) if a > 0)
               for t in range(T))
    assert any(63 in emp[t] for t in range(T)) and any(64 in emp[t] for t in range(T))
    # a whole k_link chunk without candidates and an active state after it
    assert any(a <= 64 * q and 64 * q + 63 <= b and b + 1 < st[t]
               for t in range(T) for a, b in _runs(emp[t]) for q in range(1, 3))
    assert any(b - a + 1 >= 64 for t in range(T) for a, b in _runs(emp[t]))
    assert any(emp[t] and emp[t][-1] == st[t] - 1 and ac[t] > 0 for t in range(T))  # ends without candidates
    assert any(st[t] > 0 and ac[t] == 0 for t in range(T))
    assert max(len(b) for b in brk) >= 30
    assert any(b - a == 1 for t in range(T) for a, b in zip(brk[t], brk[t][1:]))  # one-state sub-paths
    assert 0 < c['max_k'] <= 32
    # the pairs (2i, 2i + 1) of a two-trace Viterbi wave
    pairs = [(2 * i, 2 * i + 1) for i in range(T // 2)]
    assert any(st[a] > st[b] > 0 for a, b in pairs) and any(0 < st[a] < st[b] for a, b in pairs)
    assert any(0 < st[a] <= 104 < st[b] for a, b in pairs) and any(st[a] > 104 >= st[b] > 0 for a, b in pairs)
    assert any(min(st[a], st[b]) == 0 and max(st[a], st[b]) > 104 for a, b in pairs)
    modes = tr.mode.tolist()
    assert any({modes[a], modes[b]} == {0, 1} and min(st[a], st[b]) > 1 for a, b in pairs)
    assert any(modes[a] == 0 and modes[b] != 0 and min(st[a], st[b]) > 1 for a, b in pairs)  # turn costs first
    assert any(modes[a] != 0 and modes[b] == 0 and min(st[a], st[b]) > 1 for a, b in pairs)  # ... and second
    assert T % 2 == 1 and ac[T - 1] > 1  # the last wave is half empty
    assert len(want['seg_id']) > 0 and len(want['rep_id']) > 0
    # k_histogram: a trace without reports next to one with many
    nrep = np.diff(want['trace_rep_off'])
    assert any(min(nrep[a], nrep[b]) == 0 and max(nrep[a], nrep[b]) > 10 for a, b in zip(range(T), range(1, T)))


@pytest.mark.parametrize('T', [1, 2, 3])
def test_tiny_T(T, graph_dir):
    tr, want, c = _cov('tiny_T%d' % T, 'gtt', graph_dir)
    assert tr.n_traces == T and c['states'][0] >= 129 and c['max_k'] <= 32
    assert len(want['seg_id']) > 0 and len(want['rep_id']) > 0


def test_wide_K(graph_dir):
    tr, want, c = _cov('wide_K', 'wide', graph_dir)
    assert tr.n_traces == 8 and all(60 <= n <= 140 for n in np.diff(tr.offsets))
    assert c['max_k'] > 32
    st = c['states']
    assert max(st) > 128 and min(st) <= 128 and {128, 129} & set(st)  # both sides of the LDS table
    off, K = want['trace_state_off'], want['cand_count']
    late = []  # traces whose first K > 32 state follows >= 10 states of 0 < K <= 32: lds_ok drops part-way
    for t in range(tr.n_traces):
        k = K[off[t]:off[t + 1]]
        w = np.flatnonzero(k > 32)
        if len(w) and w[0] >= 10 and (k[:w[0]] > 0).all():
            late.append(t)
    assert late, 'no trace reaches K > 32 after ten narrower states'
    assert len(want['seg_id']) > 0 and len(want['rep_id']) > 0
