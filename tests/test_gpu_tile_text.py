"""The tile file texts written on the device (K19, include/otr.h otr_tiles_text and
otr_tile_store_flush_text) against the restatement tests/tile_text_ref.py, byte for byte on the
host copy and on the device buffers copied back: the hand-built cases (tests/test_tile_text_cpu.py
pins what they cover) from host and from device rows under both rule sets, the flush with texts
against the plain flush on the tile store's script, a refused flush that leaves the store as it
was, device-only results, and the text -> tile files chain ending on the device.  One child
process per job."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

from reporter_amd import simple_reporter as sr
from tests import tile_store_ref as TS
from tests import tile_text_ref as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = TS.SCRIPT_Q
CASES = X.cases()
CHILD = r'''
import sys, pickle
sys.path.insert(0, %r)
graph_dir, dst, job = %r, %r, %r
import numpy as np
import torch
from reporter_amd import matcher as M
from reporter_amd import _lib
from reporter_amd import simple_reporter as sr
from reporter_amd.tools import gen
from tests import tile_store_ref as TS
from tests import tile_text_ref as X

Q = TS.SCRIPT_Q


def refused(f, *a, **kw):
    try:
        f(*a, **kw)
    except ValueError as e:
        return str(e)
    return None


def device_copies(r):
    """The device buffers of a text result, copied back."""
    d, nf = _lib.device_to_numpy, r['n_files']
    return {'text': d(r['d_text'], r['n_text_bytes'], np.uint8), 'names': d(r['d_names'], r['n_name_bytes'], np.uint8),
            'text_off': d(r['d_text_off'], nf + 1, np.int64), 'name_off': d(r['d_name_off'], nf + 1, np.int64),
            'row_off': d(r['d_row_off'], nf + 1, np.int64), 'file': d(r['d_file'], nf, np.uint64),
            'n_rows': r['n_rows'], 'n_files': nf, 'n_text_bytes': r['n_text_bytes'], 'n_name_bytes': r['n_name_bytes']}


def tiny():
    M.configure(M.default_config(gen.graph_path('tiny', graph_dir), device=0))
    return M.Matcher()


def script(m, privacy, flush):
    """The tile store's script (five adds, a flush after adds 2, 3 and 4) through `flush`."""
    m.tile_store_open(1 << 16, Q, privacy)
    got = []
    for i, a in enumerate(TS.script_adds()):
        m.tile_store_add_reports(a)
        if i in TS.SCRIPT_FLUSH_AFTER:
            got.append(flush())
    return got


out = {}
if job == 'cases':
    m = tiny()
    for c in X.cases():
        for rules in (X.SIMPLE, X.STREAM):
            kw = dict(quantisation=c['q'], rules=rules, source=c['source'], mode=c['mode'])
            host = m.tiles_text(c['rows'], **kw)
            got = {'host': host, 'device': device_copies(host)}
            keep = torch.from_numpy(c['rows'].view(np.uint8).copy()).cuda()
            torch.cuda.synchronize()
            got['from_device'] = m.tiles_text(device_ptr=keep.data_ptr() if len(c['rows']) else 0, n=len(c['rows']), **kw)
            only = m.tiles_text(c['rows'], host=False, **kw)
            got['no_host_keys'] = sorted(only)
            got['no_host'] = device_copies(only)
            out[(c['name'], rules)] = got
elif job == 'flush':
    m = tiny()
    for privacy in (1, 2):
        got = {'plain': script(m, privacy, m.tile_store_flush)}
        got['payloads'] = [sr.stream_tile_payloads(f, 'auto', 'reporter') for f in got['plain']]
        m.tile_store_close()
        got['text'] = script(m, privacy, lambda: m.tile_store_flush_text('reporter', 'auto'))
        got['again'] = m.tile_store_flush_text('reporter', 'auto')
        got['again_plain'] = m.tile_store_flush()
        m.tile_store_close()
        # device copies of the first flush, and a flush that leaves nothing on the host
        m.tile_store_open(1 << 16, Q, privacy)
        for a in TS.script_adds()[:3]:
            m.tile_store_add_reports(a)
        only = m.tile_store_flush_text('reporter', 'auto', host=False)
        got['no_host_keys'] = sorted(only)
        got['no_host'] = device_copies(only)
        got['no_host_rows'] = _lib.device_to_numpy(only['d_rows'], only['n_rows'], _lib.TILE_ROW)
        # a refused flush leaves the store as it was
        for a in TS.script_adds()[:3]:
            m.tile_store_add_reports(a)
        got['refused'] = [refused(m.tile_store_flush_text, 'x' * 256, 'auto'),
                          refused(m.tile_store_flush_text, 'reporter', 'm' * 256)]
        got['after_refused'] = m.tile_store_flush()
        m.tile_store_close()
        out[privacy] = got
else:
    from tests import formatter_ref as F
    from tests import sessions_ref as R
    from tests import test_gpu_formatter as T
    fmt = F.FORMATS['json']
    path, msgs, ts = T.push_stream(graph_dir, 'json')
    M.configure(M.default_config(path))
    m = M.Matcher()
    c = T.cuts_of(ts)['second']
    end_ts = int(ts.max()) + R.CITY['session_gap'] + 1
    chunks = [T.case_text(msgs[c[i]:c[i + 1]], True)[:2] + (ts[c[i]:c[i + 1]],) for i in range(len(c) - 1)]
    for device_text in (False, True):
        m.sessions_open(**R.CITY)
        m.tile_store_open(1 << 16, Q, 1)
        got = sr.stream_text_tiles(m, chunks, fmt, end_ts, mode='bicycle', source='rprtr', device_text=device_text)
        out[device_text] = {'payloads': got['payloads'], 'counts': got['counts'], 'keys': sorted(got['flush']),
                            'flush': {k: got['flush'][k] for k in ('file', 'row_off', 'n_unclean') + TS.FLUSH_COUNTS}}
        m.tile_store_close()
        m.sessions_close()
pickle.dump(out, open(dst, 'wb'))
print('tile text ok')
'''

_RUNS = {}


@pytest.fixture(scope='module')
def run_job(graph_dir, tmp_path_factory):
    def get(job):
        if job not in _RUNS:
            env = dict(os.environ)
            for k in ('OTR_VIT_SPLIT', 'OTR_TIERS', 'OTR_EST_K', 'OTR_LIB', 'OTR_SMALL_KEYS', 'OTR_SMALL_PATH_KEYS',
                      'OTR_TINY_KEYS'):
                env.pop(k, None)
            dst = str(tmp_path_factory.mktemp('tile_text') / (job + '.pkl'))
            t0 = time.perf_counter()
            p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, dst, job)], env=env,
                               capture_output=True, text=True, timeout=240)
            assert p.returncode == 0 and 'tile text ok' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
            print('child %s: %.1f s' % (job, time.perf_counter() - t0))
            with open(dst, 'rb') as f:
                _RUNS[job] = pickle.load(f)
        return _RUNS[job]
    return get


def _same(got, want, what):
    bad = X.differing(got, want)
    assert not bad, (what, bad)


GROUPS = {'row_counts': lambda n: n.startswith(('one_file_', 'own_file_')),
          'file_at_block_edge': lambda n: n.startswith('second_file_at_'),
          'extremes': lambda n: n in ('extremes', 'empty_tag'),
          'alignment': lambda n: n.startswith('source_'),
          'staging_overflow': lambda n: n.startswith('longest_'),
          'names': lambda n: n.startswith('names_'),
          'file_recurs': lambda n: n == 'file_recurs'}


def test_groups_cover_every_case():
    for c in CASES:
        assert sum(1 for g in GROUPS.values() if g(c['name'])) == 1, c['name']


@pytest.mark.parametrize('group', sorted(GROUPS))
def test_cases(group, run_job):
    """Every case of the group under both rule sets: the host copy, the device buffers copied
    back, the same from rows in HBM, and with OTR_TILE_TEXT_NO_HOST (device copies only, no host
    array in the result) all equal the restatement byte for byte."""
    r = run_job('cases')
    n = 0
    for c in CASES:
        if not GROUPS[group](c['name']):
            continue
        for rules in (X.SIMPLE, X.STREAM):
            want = X.build(c['rows'], c['q'], rules, c['source'], c['mode'])
            got = r[(c['name'], rules)]
            for k in ('host', 'device', 'from_device', 'no_host'):
                _same(got[k], want, (c['name'], rules, k))
            assert not set(got['no_host_keys']) & set(X.ARRAYS), got['no_host_keys']
            n += 1
    assert n >= 2
    if group == 'row_counts':
        empty = r[('one_file_0', X.STREAM)]['host']
        assert empty['n_files'] == 0 and empty['text_off'].tolist() == [0] and empty['n_text_bytes'] == 0
    if group == 'file_recurs':
        assert r[('file_recurs', X.SIMPLE)]['host']['n_files'] == 4
    print('%s: %d results, device ms %s' % (group, n, [round(r[(c['name'], X.STREAM)]['host']['device_ms'], 3)
                                                      for c in CASES if GROUPS[group](c['name'])]))


@pytest.mark.parametrize('privacy', [1, 2])
def test_flush_text_against_flush(privacy, run_job):
    """Two stores fed the tile store's script: flush_text gives the plain flush's counts, file
    table and n_unclean, no rows, and the texts stream_tile_payloads builds from the plain flush's
    rows; the store is empty afterwards (a second flush_text and a plain flush give zero files)."""
    r = run_job('flush')[privacy]
    _, want = TS.script_flushes(privacy)
    assert len(r['plain']) == len(r['text']) == len(want) == 3
    for plain, text, payloads, w in zip(r['plain'], r['text'], r['payloads'], want):
        assert not TS.differing(plain, w)
        assert 'rows' not in text and text['d_rows']
        for k in ('file', 'row_off', 'n_unclean'):
            assert text[k].tobytes() == plain[k].tobytes() and text[k].dtype == plain[k].dtype, k
        for k in TS.FLUSH_COUNTS:
            assert text[k] == plain[k], k
        assert text['quantisation'] == Q
        assert sr.text_payloads(text) == payloads and len(payloads) == plain['n_files'] > 0
        _same(dict(text, n_rows=plain['n_rows']), X.build(plain['rows'], Q, X.STREAM, b'reporter', b'auto'), 'flush')
    for k in ('again', 'again_plain'):
        assert r[k]['n_files'] == 0 and r[k]['n_rows'] == 0 and r[k]['n_rows_in'] == 0, k
    again = r['again']
    assert again['n_text_bytes'] == 0 and len(again['text']) == 0 and again['text_off'].tolist() == [0]
    assert again['name_off'].tolist() == [0] and 'rows' not in again


@pytest.mark.parametrize('privacy', [1, 2])
def test_flush_text_device_only_and_refused(privacy, run_job):
    """With OTR_TILE_TEXT_NO_HOST the result has no text or names on the host and the device
    copies (texts, names, offsets, the kept rows) are right; a flush_text refused for a source or
    mode of 256 bytes leaves the store as it was: a plain flush afterwards returns everything."""
    r = run_job('flush')[privacy]
    _, want = TS.script_flushes(privacy)
    first = want[0]
    assert not {'text', 'names', 'text_off', 'name_off', 'rows'} & set(r['no_host_keys'])
    assert r['no_host_rows'].tobytes() == first['rows'].tobytes()
    _same(r['no_host'], X.build(first['rows'], Q, X.STREAM, b'reporter', b'auto'), 'no host')
    assert all(x and '255 bytes' in x for x in r['refused']), r['refused']
    assert not TS.differing(r['after_refused'], first)


def test_stream_text_tiles_device_text(run_job):
    """The text -> tile files chain on the city stream ending in tile_store_flush_text equals the
    chain ending on the host: payloads, counts and file table; the device flush has no rows."""
    r = run_job('city')
    host, dev = r[False], r[True]
    assert dev['payloads'] == host['payloads'] and len(host['payloads']) > 1
    assert all(v.startswith(sr.STREAM_COLUMN_LAYOUT + '\n') and v.endswith(',rprtr,BICYCLE')
               for v in dev['payloads'].values())
    assert dev['counts'] == host['counts']
    for k, v in host['flush'].items():
        assert np.asarray(v).tobytes() == np.asarray(dev['flush'][k]).tobytes(), k
    assert 'rows' in host['keys'] and 'rows' not in dev['keys'] and 'text' in dev['keys']
