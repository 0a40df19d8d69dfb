"""The stream formatter on the device (K16, include/otr.h otr_format_messages and
otr_sessions_push_text) against its restatement tests/formatter_ref.py: the corpus and the
smallest shapes bit for bit, in host and device memory, with offsets and with newlines; the city
stream pushed as SV and as JSON text against sessions_push of the restated points; the whole
text → tile files chain; refusals; and otr_ingest / match_batch unmoved by formatter calls.  What
the corpus covers is pinned by tests/test_formatter_cpu.py.  The numerals of tests/ingest_cases.py
(pinned by tests/test_ingest_cases_cpu.py) go through as psv coordinates: the only place where
k_format_parse's compile of the number parsers meets them.  One child process per job."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import formatter_ref as F
from tests import sessions_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINT_KEYS = ('key', 'lat', 'lon', 'accuracy', 'time', 'timestamp', 'message')
CHUNKINGS = ('one', 'second', 'seven')
Q = 3600


# ---- inputs shared by the children and the checks -------------------------------------------------
def corpus_cases():
    """(name, format name, messages, by offsets, in device memory, a timestamp array)."""
    out = []
    for name in F.FORMATS:
        msgs = [m for n, m in F.corpus() if n == name]
        lines = [m for m in msgs if b'\n' not in m]
        out += [(name + '/off/host/ts', name, msgs, True, False, True),
                (name + '/off/device/all', name, msgs, True, True, False),
                (name + '/nl/host/all', name, lines, False, False, False),
                (name + '/nl/device/ts', name, lines[:-1] + [b'{"last":"no newline"}'], False, True, True)]
    return out


def case_text(msgs, by_offsets, last_newline=True):
    """(text, offsets or None, the messages the call must see)."""
    if by_offsets:
        off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.int64)
        return b''.join(msgs), off, list(msgs)
    text = b'\n'.join(msgs) + (b'\n' if last_newline else b'')
    return text, None, F.split_lines(text)


LINE = b'u1,52.5,13.4,7,5\n'   # 17 bytes


def edge_cases():
    """(name, format name, text, offsets or None): the smallest shapes that can go wrong."""
    def lines(n, fmt):
        rows = []
        for i in range(n):
            if fmt == 'csv':
                rows.append((b'u%d,%d.5,13.25,%d,%d' % (i % 7, i % 90, 1483250740 + i, i % 9)) if i % 5 != 3 else
                            (b'u%d,north,13.25,1,1' % i if i % 2 else b'u,1,2,3,1e99'))
            else:
                rows.append((b'{"id":"u%d","latitude":%d.5,"longitude":13.25,"timestamp":%d,"accuracy":%d}'
                             % (i % 7, i % 90, 1483250740 + i, i % 9)) if i % 5 != 3 else
                            (b'{"id":"u%d"}' % i if i % 2 else b'{"id":"u","latitude":1e1}'))
        return rows

    out = [('bytes%d' % n, 'csv', (LINE * 2)[:n], None) for n in (0, 1, 15, 16, 17)]
    out += [('empty_message', 'csv', b'\n' + LINE + b'\n\n' + LINE[:-1], None),
            ('only_newlines', 'csv', b'\n\n\n', None),
            ('no_messages_off', 'csv', b'', np.zeros(1, np.int64)),
            ('empty_messages_off', 'json', b'{}', np.array([0, 0, 0, 2, 2], np.int64)),
            ('gap_off', 'csv', LINE * 3, np.array([0, 16, 17, 33], np.int64)),
            ('all_dropped', 'csv', b'bad line\n' * 65, None)]
    for n in (1, 64, 65, 256, 257):
        for fmt in ('csv', 'json'):
            text, off, _ = case_text(lines(n, fmt), False, last_newline=n % 2 == 0)
            out.append(('%s%d' % (fmt, n), fmt, text, None))
        text, off, _ = case_text(lines(n, 'json'), True)
        out.append(('json_off%d' % n, 'json', text, off))
    return out


BAD = {'psv': (b'not a message', b'2017-01-01 00:00:00|veh-1000||||1e30||||1|2', b'',
               b'2017-01-01 00:00:00|veh-1000||||1||||9007199254740993.00000000000000000001|2',
               b'2017-13-01 00:00:00|veh-1000||||1||||1|2'),
       'json': (b'not a message', b'{"id":"veh-1000","latitude":1e1,"longitude":2,"timestamp":5,"accuracy":1}', b'',
                b'{"id":"veh-1000","latitude":1,"longitude":2,"timestamp":5,"accuracy":1} x', b'{"id":"veh-1000"}')}


def numeral_messages():
    """The numerals of tests/ingest_cases.py as psv messages, each the latitude of one message and
    the longitude of the next; those that end in a drop or a refusal stand between plain ones."""
    from tests import ingest_cases as ic
    n = ic.numerals()
    nums = list(n['main'])
    for s in n['refused'] + n['py2_refused'] + n['rejected'] + n['non_finite'] + n['in_texts']:
        nums += [s, '1.5']
    return [('2017-01-01 06:05:40|veh-%d||||5||||%s|%s' % (i % 3, s, nums[i - 1])).encode('latin-1')
            for i, s in enumerate(nums)]


def push_stream(graph_dir, fmt_name):
    """(graph path, messages, per-message timestamps): the city stream rendered as messages, with
    undecodable messages and the messages of a uuid that never reports mixed in."""
    path, pts = R.city_stream(graph_dir)
    fmt = F.FORMATS[fmt_name]
    msgs = (F.render_json if fmt['type'] == 'json' else F.render_sv)(pts, fmt)
    ghost = {k: np.asarray(pts[k])[:1] for k, _ in R.POINT_TYPES}
    ghost['key'] = np.array([5], np.uint64)
    ghost_msg = (F.render_json if fmt['type'] == 'json' else F.render_sv)(ghost, fmt)[0]
    out, ts = [], []
    for i, m in enumerate(msgs):
        if i % 37 == 5:
            out.append(BAD[fmt_name][(i // 37) % len(BAD[fmt_name])])
            ts.append(int(pts['timestamp'][i]))
        if i % 211 == 100:
            out.append(ghost_msg)
            ts.append(int(pts['timestamp'][i]))
        out.append(m)
        ts.append(int(pts['timestamp'][i]))
    return path, out, np.array(ts, np.int64)


def cuts_of(ts):
    n = len(ts)
    return {'one': [0, n], 'second': [0] + [i for i in range(1, n) if ts[i] // 1000 != ts[i - 1] // 1000] + [n],
            'seven': list(range(0, n, 7)) + [n]}


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
from tests import formatter_ref as F
from tests import sessions_ref as R
from tests import test_gpu_formatter as T


def refused(f, *a, **kw):
    try:
        f(*a, **kw)
    except ValueError as e:
        return str(e)
    return None


def plain(d):
    return {k: v for k, v in d.items() if k != 'device'}


def fmt_call(m, text, fmt, off, ts, device):
    """format_messages with everything in host or in device memory."""
    if not device:
        return plain(m.format_messages(text, fmt, msg_off=off, timestamp=ts))
    keep = [torch.frombuffer(bytearray(text or b'\0'), dtype=torch.uint8).cuda()]
    d_off = d_ts = None
    if off is not None:
        keep.append(torch.from_numpy(np.ascontiguousarray(off)).cuda())
        d_off = (keep[-1].data_ptr(), len(off) - 1)
    if not isinstance(ts, int):
        keep.append(torch.from_numpy(np.ascontiguousarray(ts)).cuda())
        d_ts = (keep[-1].data_ptr(), len(ts))
    torch.cuda.synchronize()
    return plain(m.format_messages(None, fmt, msg_off=d_off, timestamp=ts if d_ts is None else d_ts,
                                   device_ptr=keep[0].data_ptr(), nbytes=len(text)))


out = {}
if job == 'corpus':
    M.configure(M.default_config(gen.graph_path('tiny', graph_dir)))
    m = M.Matcher()
    for name, fname, msgs, by_off, device, ts_array in T.corpus_cases():
        text, off, seen = T.case_text(msgs, by_off, last_newline=not name.endswith('/ts'))
        ts = 1000 + 3 * np.arange(len(seen), dtype=np.int64) if ts_array else 77
        out[name] = fmt_call(m, text, F.FORMATS[fname], off, ts, device)
elif job == 'edges':
    M.configure(M.default_config(gen.graph_path('tiny', graph_dir)))
    m = M.Matcher()
    for i, (name, fname, text, off) in enumerate(T.edge_cases()):
        out[name] = fmt_call(m, text, F.FORMATS[fname], off, 5, device=i %% 2 == 1)
elif job == 'numerals':
    M.configure(M.default_config(gen.graph_path('tiny', graph_dir)))
    m = M.Matcher()
    text, off, seen = T.case_text(T.numeral_messages(), True)
    out['numerals'] = fmt_call(m, text, F.FORMATS['psv'], off, 5, device=False)
elif job.startswith('push'):
    fname = {'push_sv': 'psv', 'push_json': 'json'}[job]
    fmt = F.FORMATS[fname]
    path, msgs, ts = T.push_stream(graph_dir, fname)
    M.configure(M.default_config(path))
    m = M.Matcher()
    restated = F.to_points([F.format_message(x, fmt) for x in msgs], ts)
    end_ts = int(ts.max()) + R.CITY['session_gap'] + 1
    m.sessions_open(**R.CITY)
    out['want'] = {'result': R.by_trigger(m.sessions_push(restated)), 'snapshot': m.sessions_snapshot(),
                   'punctuate': m.sessions_punctuate(end_ts)}
    m.sessions_close()
    for name, c in T.cuts_of(ts).items():
        m.sessions_open(**R.CITY)
        res, bases, trig_msg, counts = [], [], [], np.zeros(4, np.int64)
        for i in range(len(c) - 1):
            text, off, _ = T.case_text(msgs[c[i]:c[i + 1]], True)
            f, s = m.sessions_push_text(text, fmt, msg_off=off, timestamp=ts[c[i]:c[i + 1]])
            bases.append(int(counts[1]))
            counts += [f['n_messages'], f['n_points'], f['n_dropped'], f['n_unsupported']]
            trig_msg.append(f['message'][s['trigger']] + c[i])
            res.append(s)
        whole = R.concat(res, bases)
        order = np.argsort(whole['trigger'], kind='stable')
        out[name] = {'result': R.by_trigger(whole), 'trigger_message': np.concatenate(trig_msg)[order],
                     'counts': counts, 'snapshot': m.sessions_snapshot(), 'punctuate': m.sessions_punctuate(end_ts),
                     'parse_ms': f['parse_ms'], 'total_ms': f['total_ms']}
        m.sessions_close()
elif job == 'chain':
    fmt = F.FORMATS['json']
    path, msgs, ts = T.push_stream(graph_dir, 'json')
    M.configure(M.default_config(path))
    m = M.Matcher()
    c = T.cuts_of(ts)['second']
    end_ts = int(ts.max()) + R.CITY['session_gap'] + 1
    m.sessions_open(**R.CITY)
    m.tile_store_open(1 << 16, T.Q, 1)
    chunks = [T.case_text(msgs[c[i]:c[i + 1]], True)[:2] + (ts[c[i]:c[i + 1]],) for i in range(len(c) - 1)]
    got = sr.stream_text_tiles(m, chunks, fmt, end_ts)
    out['got'] = {'payloads': got['payloads'], 'rows': got['flush']['rows'], 'file': got['flush']['file'],
                  'row_off': got['flush']['row_off'], 'counts': got['counts']}
    m.tile_store_close()
    m.sessions_close()
    m.sessions_open(**R.CITY)
    m.tile_store_open(1 << 16, T.Q, 1)
    for i in range(len(c) - 1):
        chunk = msgs[c[i]:c[i + 1]]
        m.sessions_push(F.to_points([F.format_message(x, fmt) for x in chunk], ts[c[i]:c[i + 1]]))
        m.tile_store_add_session()
    m.sessions_punctuate(end_ts)
    m.tile_store_add_session()
    fl = m.tile_store_flush()
    out['want'] = {'payloads': sr.stream_tile_payloads(fl), 'rows': fl['rows'], 'file': fl['file'],
                   'row_off': fl['row_off']}
elif job == 'refusals':
    M.configure(M.default_config(gen.graph_path('tiny', graph_dir)))
    m = M.Matcher()
    csv, js = F.FORMATS['csv'], F.FORMATS['json']
    line = lambda u, i: b'%%s,52.5,13.4,%%d,4' %% (u, 100 + i)
    out['no_store'] = refused(m.sessions_push_text, T.LINE, csv)
    out['bad_format'] = [refused(m.format_messages, T.LINE, dict(csv, separator=0)),
                         refused(m.format_messages, T.LINE, dict(csv, lat_index=-1)),
                         refused(m.format_messages, T.LINE, dict(csv, time_format=2)),
                         refused(m.format_messages, b'{}', dict(js, lat_key='a"b')),
                         refused(m.format_messages, b'{}', dict(js, lon_key='x' * 65)),
                         refused(m.format_messages, b'{}', dict(js, uuid_key='')),
                         refused(m.format_messages, b'{}', dict(js, time_key=None))]
    out['key64'] = plain(m.format_messages(b'{}', dict(js, lon_key='x' * 64)))
    out['bad_off'] = [refused(m.format_messages, T.LINE, csv, msg_off=np.array(o, np.int64))
                      for o in ([0, 9, 8, 17], [-1, 17], [0, 18], [3, 2])]
    m.sessions_open(4, 4, report_dist=500.0, report_count=3, report_time=0, session_gap=60000)
    first = [line(u, i) for i, u in enumerate((b'a', b'b', b'c', b'a', b'b'))]
    out['first'] = m.sessions_push_text(b'\n'.join(first), csv, timestamp=1000)[1]
    out['before'] = m.sessions_snapshot()
    many = [line(u, i) for i, u in enumerate((b'a', b'd', b'e', b'b'))]
    out['too_many'] = refused(m.sessions_push_text, b'\n'.join(many), csv, timestamp=1001)
    out['after_too_many'] = m.sessions_snapshot()
    out['push_bad_off'] = refused(m.sessions_push_text, b'\n'.join(many), csv, msg_off=np.array([0, 5, 4], np.int64))
    out['push_bad_format'] = refused(m.sessions_push_text, b'\n'.join(many), dict(csv, separator=256))
    out['after_bad'] = m.sessions_snapshot()
    f, s = m.sessions_push_text(b'\n'.join([line(b'd', 7), b'junk', line(b'a', 8)]), csv, timestamp=1002)
    out['fits'] = (plain(f), s)
    out['after_fits'] = m.sessions_snapshot()
else:
    from tests import ragged
    path, tr = ragged.ragged_city(graph_dir)
    M.configure(ragged.engine_config(path, 'gtt'))
    m = M.Matcher()
    traces = gen.make_traces(path, 40, 60, 10, 8.0, 41, t_begin=gen.T_BEGIN, t_spread=3 * 3600)
    text = gen.probe_text(traces, 'raw', seed=3, shuffle=0.1)

    def ingest():
        r, b = m.ingest(text, rules=_lib.OTR_INGEST_JAVA_SV, inactivity=120)
        nt, npr = int(r.n_traces), int(r.n_probes)
        d = _lib.device_to_numpy
        return {'n': np.array([r.n_lines, r.n_kept, npr, nt, r.n_uuids]),
                'off': d(b.arrays['trace_offsets'], nt + 1, np.int64), 'lat': d(b.arrays['lat'], npr, np.float64),
                'lon': d(b.arrays['lon'], npr, np.float64), 'time': d(b.arrays['time'], npr, np.int64),
                'acc': d(b.arrays['accuracy'], npr, np.float32), 'uoff': d(b.uuid_off, nt, np.int64),
                'ulen': d(b.uuid_len, nt, np.int32)}

    out['ingest_before'] = ingest()
    out['match_before'] = {k: np.asarray(v) for k, v in m.match_batch_numpy(tr).items()}
    psv = F.FORMATS['psv']
    out['formatted'] = plain(m.format_messages(text, psv, timestamp=9))
    held = m.format_messages(b'\n'.join(x for _, x in F.corpus() if b'\n' not in x), F.FORMATS['json_ymd'])
    out['match_after'] = {k: np.asarray(v) for k, v in m.match_batch_numpy(tr).items()}
    out['ingest_after'] = ingest()
    # the formatter's result outlives the ingest and the batch that followed it
    out['held'] = {k: _lib.device_to_numpy(getattr(held['device'].points, k), held['n_points'], dt)
                   for k, dt in _lib.SESSION_POINT_FIELDS}
    out['held_want'] = {k: held[k] for k, _ in _lib.SESSION_POINT_FIELDS}
    out['text'] = text
pickle.dump(out, open(dst, 'wb'))
print('formatter ok')
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
            dst = str(tmp_path_factory.mktemp('formatter') / (job + '.pkl'))
            t0 = time.perf_counter()
            p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, dst, job)], env=env,
                               capture_output=True, text=True, timeout=240)
            assert p.returncode == 0 and 'formatter ok' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
            print('child %s: %.1f s' % (job, time.perf_counter() - t0))
            with open(dst, 'rb') as f:
                _RUNS[job] = pickle.load(f)
        return _RUNS[job]
    return get


def _same(got, want, fields):
    bad = R.differing(got, want, fields)
    assert not bad, bad


def _check_format(got, text, seen, fmt, ts, name):
    """A format result against the restatement of the messages the call must have seen."""
    want = F.to_points([F.format_message(m, fmt) for m in seen], ts)
    bad = [i for i, s in enumerate(want['status']) if s]
    assert got['n_messages'] == len(seen), name
    _same(got, want, ('status',) + POINT_KEYS)
    assert (got['n_points'], got['n_dropped'], got['n_unsupported']) == (
        len(want['key']), want['n_dropped'], want['n_unsupported']), name
    assert (got['first_bad'], got['first_bad_reason']) == ((bad[0], int(want['status'][bad[0]])) if bad else (-1, 0)), name
    uuids = [text[int(o):int(o) + int(n)] for o, n in zip(got['uuid_off'], got['uuid_len'])]
    assert uuids == want['uuid'], name
    return want


def test_corpus(run_job):
    r = run_job('corpus')
    reasons = set()
    for name, fname, msgs, by_off, device, ts_array in corpus_cases():
        text, off, seen = case_text(msgs, by_off, last_newline=not name.endswith('/ts'))
        ts = 1000 + 3 * np.arange(len(seen), dtype=np.int64) if ts_array else 77
        want = _check_format(r[name], text, seen, F.FORMATS[fname], ts, name)
        reasons |= set(want['status'].tolist())
    assert reasons == {0} | (set(F.REASONS) - {F.U_NO_ID})


def test_edges(run_job):
    r = run_job('edges')
    kept = 0
    for name, fname, text, off in edge_cases():
        seen = F.split_lines(text) if off is None else [text[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        want = _check_format(r[name], text, seen, F.FORMATS[fname], 5, name)
        kept += len(want['key'])
    assert r['bytes0']['n_messages'] == 0 and r['bytes1']['n_messages'] == 1 and r['bytes17']['n_points'] == 1
    assert r['bytes16']['n_points'] == 1 and r['bytes15']['n_dropped'] == 1
    assert r['all_dropped']['n_dropped'] == 65 and r['all_dropped']['n_points'] == 0
    assert r['json257']['n_messages'] == 257 and kept > 1000


def test_ingest_numerals(run_job):
    """Every numeral of tests/ingest_cases.py as a psv latitude and longitude: kept with the float
    of Python's own float(), refused where w and w + 1 disagree, dropped where the grammar fails
    or the value is not finite."""
    from tests import ingest_cases as ic
    r = run_job('numerals')
    text, off, seen = case_text(numeral_messages(), True)
    want = _check_format(r['numerals'], text, seen, F.FORMATS['psv'], 5, 'numerals')
    n = ic.numerals()
    status = want['status'].tolist()
    bad = len(n['rejected']) + len(n['non_finite']) + len(n['in_texts'])
    # (the empty numeral as the last field is a trailing empty string: String.split drops it)
    assert (status.count(F.U_PRECISION), status.count(F.D_FLOAT), status.count(F.D_FIELDS)) == (
        2 * len(n['refused']), 2 * bad - 1, 1)
    assert status.count(0) == len(seen) - 2 * len(n['refused']) - 2 * bad
    with np.errstate(over='ignore'):
        main = np.array([float(s) for s in n['main']]).astype(np.float32)
    got = r['numerals']
    assert not any(status[:len(main)]) and got['lat'][:len(main)].tobytes() == main.tobytes()
    assert got['lon'][1:len(main)].tobytes() == main[:-1].tobytes()


@pytest.mark.parametrize('job', ['push_sv', 'push_json'])
def test_push_text_equals_push_of_restated_points(job, run_job, graph_dir):
    r = run_job(job)
    fname = {'push_sv': 'psv', 'push_json': 'json'}[job]
    _, msgs, ts = push_stream(graph_dir, fname)
    restated = F.to_points([F.format_message(m, F.FORMATS[fname]) for m in msgs], ts)
    want = r['want']
    assert len(want['result']['key']) > 100 and len(want['result']['id']) > 0
    assert restated['n_dropped'] > 0 and restated['n_unsupported'] > 0
    ghost = F.uuid_hash(F.uuid_of_key(5))
    assert ghost in restated['key'] and ghost not in want['result']['key']
    print('%s: %d messages, %d points, %d windows; last chunk parse_ms %s' % (
        job, len(msgs), len(restated['key']), len(want['result']['key']),
        {k: round(r[k]['parse_ms'], 3) for k in CHUNKINGS}))
    for name in CHUNKINGS:
        g = r[name]
        assert g['counts'].tolist() == [len(msgs), len(restated['key']), restated['n_dropped'],
                                        restated['n_unsupported']], name
        _same(g['result'], want['result'], R.RESULT_FIELDS)
        _same(g['snapshot'], want['snapshot'], R.SNAPSHOT_FIELDS)
        _same(g['punctuate'], want['punctuate'], R.RESULT_FIELDS)
        # every window's trigger maps through d_message to the message that tripped it
        trig = g['result']['trigger']
        assert g['trigger_message'].tolist() == restated['message'][trig].tolist(), name
        assert [F.uuid_hash(restated['uuid'][t]) for t in trig] == g['result']['key'].tolist(), name


def test_chain_text_to_tile_files(run_job):
    r = run_job('chain')
    got, want = r['got'], r['want']
    _same(got, want, ('rows', 'file', 'row_off'))
    assert got['payloads'] == want['payloads'] and len(got['payloads']) > 0 and len(got['rows']) > 0
    c = got['counts']
    assert c['messages'] == c['points'] + c['dropped'] + c['unsupported'] and c['dropped'] > 0 < c['unsupported']
    assert c['reports'] > 0


def test_refusals(run_job):
    """The collision refusal (two uuids of one chunk under one 64-bit hash) has no constructible
    input: it stays covered through the stage shared with K11 (tests/test_gpu_ingest.py)."""
    r = run_job('refusals')
    assert r['no_store'] and 'otr_sessions_open' in r['no_store']
    assert all(r['bad_format']), r['bad_format']
    assert r['key64']['n_messages'] == 1 and r['key64']['status'].tolist() == [F.D_MISSING]
    assert all(e and 'offsets' in e for e in r['bad_off']), r['bad_off']
    assert r['first']['n_live'] == 3
    assert r['too_many'] and 'max_sessions' in r['too_many']
    _same(r['after_too_many'], r['before'], R.SNAPSHOT_FIELDS)
    assert r['push_bad_off'] and 'offsets' in r['push_bad_off'] and r['push_bad_format']
    _same(r['after_bad'], r['before'], R.SNAPSHOT_FIELDS)
    f, s = r['fits']
    assert (f['n_messages'], f['n_points'], f['n_dropped'], f['first_bad'], f['first_bad_reason']) == (
        3, 2, 1, 1, F.D_FIELDS)
    assert s['n_live'] == 4
    keys = sorted(F.uuid_hash(u) for u in (b'a', b'b', b'c', b'd'))
    assert r['after_fits']['key'].tolist() == keys
    assert sorted(np.diff(r['after_fits']['point_off']).tolist()) == [1, 1, 2, 3]


def test_ingest_and_match_batch_unmoved(run_job):
    r = run_job('unmoved')
    for k, a in r['ingest_before'].items():
        b = r['ingest_after'][k]
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    assert r['ingest_before']['n'][3] > 0 and r['formatted']['n_points'] == r['ingest_before']['n'][0] > 0

    def defined(res):
        out = dict(res)
        live = np.arange(res['cand_edge'].shape[1])[None, :] < res['cand_count'][:, None]
        for k in ('cand_edge', 'cand_p', 'cand_sqd'):
            out[k] = np.where(live, res[k], 0)
        return out

    before, after = defined(r['match_before']), defined(r['match_after'])
    for k, a in before.items():
        assert a.dtype == after[k].dtype and a.shape == after[k].shape and a.tobytes() == after[k].tobytes(), k
    _same(r['held'], r['held_want'], [k for k, _ in R.POINT_TYPES])
    assert len(r['held']['key']) > 10
