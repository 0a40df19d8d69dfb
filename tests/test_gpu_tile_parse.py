"""Tile file texts read back on the device (K21, include/otr.h otr_tiles_parse) against the
restatement tests/tile_parse_ref.py, exactly: the round trip rows -> cull -> texts -> rows of
many_reports under both rule sets, every hand-built case of tests/tile_parse_cases.py from host
text and from device text, the merge of two batches' files that the stage is for, and the
refusals, after which the previous result still stands.  One child process per job."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

from reporter_amd import simple_reporter as sr
from tests import tile_parse_cases as C
from tests import tile_parse_ref as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
from tests import ragged
from tests import tile_parse_cases as C
from tests import tile_parse_ref as P

D = _lib.device_to_numpy


def device_copies(r):
    """The device buffers of a parse result, copied back, with its counts."""
    nf = r['n_files']
    out = {k: r[k] for k in P.COUNTS}
    out.update(rows=D(r['d_rows'], r['n_rows'], _lib.TILE_ROW), row_off=D(r['d_row_off'], nf + 1, np.int64),
               file=D(r['d_file'], nf, np.uint64), file_status=D(r['d_file_status'], nf, np.uint8),
               file_line_off=D(r['d_file_line_off'], nf + 1, np.int64),
               line_status=D(r['d_line_status'], r['n_lines'], np.uint8))
    return out


def on_device(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


def parse_device(m, text, text_off, names, name_off, **kw):
    """tiles_parse of the four arrays uploaded first: device pointers in, device copies only out."""
    keep = [on_device(x) for x in (text, text_off, names, name_off)]
    ptr = [k.data_ptr() if k.numel() else 0 for k in keep]
    r = m.tiles_parse(text=ptr[0], text_off=ptr[1], names=ptr[2], name_off=ptr[3], device=True,
                      n_files=len(text_off) - 1, host=False, **kw)
    return r, device_copies(r)


def text_copies(r):
    nf = r['n_files']
    return {'text': D(r['d_text'], r['n_text_bytes'], np.uint8), 'names': D(r['d_names'], r['n_name_bytes'], np.uint8),
            'text_off': D(r['d_text_off'], nf + 1, np.int64), 'name_off': D(r['d_name_off'], nf + 1, np.int64),
            'row_off': D(r['d_row_off'], nf + 1, np.int64), 'file': D(r['d_file'], nf, np.uint64), 'n_files': nf}


def refused(f, *a, **kw):
    try:
        f(*a, **kw)
    except ValueError as e:
        return str(e)
    return None


def match_dir_tiles():
    """{name: [lines]} of 300 rows over few pairs and files, so that privacy 2 keeps some."""
    from tests import tile_text_ref as X
    rows = X.plain_rows(300, [X.file_of(416666 + i %% 2, i %% 2, 7 + i %% 5) for i in range(300)], seed=5)
    rows['id'] = (1 << 33) + 8 * (rows['id'] %% 9)
    rows['next_id'] = (1 << 33) + 8 * (rows['next_id'] %% 3)
    order = np.argsort(rows['file'], kind='stable')
    return sr.rows_to_tiles(rows[order], 3600, 'auto', 'smpl_rprt')


out = {}
if job == 'cases':
    M.configure(M.default_config(gen.graph_path('tiny', graph_dir), device=0))
    m = M.Matcher()
    for c in C.cases():
        kw = dict(quantisation=c['q'], rules=c['rules'], source=c['source'], mode=c['mode'])
        text, text_off, names, name_off = P.pack(c)
        host = m.tiles_parse(text=text, text_off=text_off, names=names, name_off=name_off, **kw)
        got = {'host': host, 'host_device': device_copies(host), 'ms': host['device_ms']}
        only, got['device'] = parse_device(m, text, text_off, names, name_off, **kw)
        got['no_host_keys'] = sorted(only)
        out[c['name']] = got
elif job == 'round_trip':
    path, tr = ragged.many_reports(graph_dir)
    M.configure(ragged.engine_config(path, 'gtt'))
    m = M.Matcher()
    for rules in (0, 1):
        kw = dict(quantisation=3600, rules=rules, source='smpl_rprt', mode='auto')
        r = m.match_batch(tr, copy_out=False, tile_rows=True, tile_rules=rules, quantisation=3600)
        kept = sr.cull_rows(m, None, 1, device_ptr=r.d_rows, n=r.n_rows, rules=rules)
        t = m.tiles_text(kept, host=False, **kw)
        texts = text_copies(t)
        p = m.tiles_parse(text=t['d_text'], text_off=t['d_text_off'], names=t['d_names'], name_off=t['d_name_off'],
                          device=True, n_files=t['n_files'], host=False, **kw)
        got = {'kept': kept, 'texts': texts, 'parse': device_copies(p)}
        # the parsed rows, still in HBM, through the cull and the texts again
        again = m.tiles_text(device_ptr=p['d_rows'], n=p['n_rows'], host=False, **kw)
        got['texts_again'] = text_copies(again)
        got['parse_after'] = device_copies(p)          # the result outlives the text call
        sr.cull_rows(m, None, 1, device_ptr=p['d_rows'], n=p['n_rows'], rules=rules)
        got['parse_after_cull'] = device_copies(p)
        if rules == 0:  # the reference's match-dir form: no column lines
            body = texts['text'].tobytes()
            parts = [body[a:b] for a, b in zip(texts['text_off'][:-1], texts['text_off'][1:])]
            head = P.X.HEADER + b'\n'
            assert all(x.startswith(head) for x in parts)
            parts = [x[len(head):] for x in parts]
            off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
            got['headerless'] = m.tiles_parse(text=b''.join(parts), text_off=off, names=texts['names'],
                                              name_off=texts['name_off'], **kw)
        out[rules] = got
elif job == 'merge':
    path, tr = ragged.ragged_city(graph_dir)
    M.configure(ragged.engine_config(path, 'gtt'))
    m = M.Matcher()
    kw = dict(quantisation=3600, rules=0, source='smpl_rprt', mode='auto')
    halves = []
    for idx in (np.arange(0, tr.n_traces, 2), np.arange(1, tr.n_traces, 2)):
        r = m.match_batch(tr.subset(idx), copy_out=False, tile_rows=True, quantisation=3600)
        rows = sr.cull_rows(m, None, 1, device_ptr=r.d_rows, n=r.n_rows)      # grouped by file, nothing deleted
        halves.append({'rows': rows, 'lines': sr.rows_to_tiles(rows, 3600, 'auto', 'smpl_rprt'),
                       'text': m.tiles_text(rows, **kw)})
    a, b = halves[0]['text'], halves[1]['text']
    p = m.tiles_parse(text=np.concatenate([a['text'], b['text']]),
                      text_off=np.concatenate([a['text_off'], b['text_off'][1:] + a['text_off'][-1]]),
                      names=np.concatenate([a['names'], b['names']]),
                      name_off=np.concatenate([a['name_off'], b['name_off'][1:] + a['name_off'][-1]]), host=False, **kw)
    kept = sr.cull_rows(m, None, 2, device_ptr=p['d_rows'], n=p['n_rows'])
    out = {'halves': [{k: h[k] for k in ('rows', 'lines')} for h in halves], 'parse': {k: p[k] for k in P.COUNTS},
           'payloads': sr.text_payloads(m.tiles_text(kept, **kw))}
elif job == 'match_dir':
    import os
    M.configure(M.default_config(gen.graph_path('tiny', graph_dir), device=0))
    m = M.Matcher()
    tiles = match_dir_tiles()
    base = os.path.dirname(dst)
    dirs = {k: os.path.join(base, k) for k in ('with', 'without', 'bad_line', 'bad_name')}
    sr.write_tiles(tiles, dirs['with'])
    for d in ('without', 'bad_line', 'bad_name'):      # simple_reporter.py:199-206: appended lines, no column line
        for key, lines in tiles.items():
            os.makedirs(os.path.dirname(os.path.join(dirs[d], key)), exist_ok=True)
            with open(os.path.join(dirs[d], key), 'a') as f:
                f.write(''.join(lines))
    last = sorted(tiles, key=lambda k: k.split('/'))[-1]
    with open(os.path.join(dirs['bad_line'], last), 'a') as f:
        fields = tiles[last][0].split(',')
        f.write(','.join(fields[:3] + ['2'] + fields[4:]))
    with open(os.path.join(dirs['bad_name'], 'notes.txt'), 'w') as f:
        f.write('x\n')
    for privacy in (1, 2):
        out[privacy] = {'with': sr.report_match_dir(m, dirs['with'], privacy),
                        'without': sr.report_match_dir(m, dirs['without'], privacy),
                        'both': sr.report_match_dir(m, [dirs['with'], dirs['without']], privacy)}
    out['bad_line'] = refused(sr.report_match_dir, m, dirs['bad_line'], 1)
    out['bad_name'] = refused(sr.report_match_dir, m, dirs['bad_name'], 1)
    out['tiles'] = tiles
    out['last'] = (last, len(tiles[last]))
    out['none'] = sr.report_match_dir(m, [], 1)
else:
    M.configure(M.default_config(gen.graph_path('tiny', graph_dir), device=0))
    m = M.Matcher()
    c = [x for x in C.cases() if x['name'] == 'fields_0'][0]
    text, text_off, names, name_off = P.pack(c)
    kw = dict(quantisation=c['q'], rules=c['rules'], source=c['source'], mode=c['mode'])
    first = m.tiles_parse(text=text, text_off=text_off, names=names, name_off=name_off, **kw)
    args = dict(text=text, text_off=text_off, names=names, name_off=name_off)
    bad_off = text_off.copy()
    bad_off[0] = 1
    desc = np.array([0, len(text), len(text) - 1], np.int64)
    tries = {'quantisation': dict(args, **dict(kw, quantisation=0)),
             'rules': dict(args, **dict(kw, rules=2)),
             'source': dict(args, **dict(kw, source=b'x' * 256)),
             'mode': dict(args, **dict(kw, mode=b'm' * 256)),
             'text_off_start': dict(args, text_off=bad_off, **kw),
             'name_off_start': dict(args, name_off=name_off + 1, names=np.concatenate([names, names[:1]]), **kw),
             'text_off_descends': dict(kw, text=text, text_off=desc, names=b'ab', name_off=np.array([0, 1, 2], np.int64)),
             'name_off_descends': dict(kw, text=text, text_off=np.array([0, 1, 2], np.int64), names=b'ab',
                                       name_off=np.array([0, 2, 1], np.int64))}
    out['refused'] = {k: refused(m.tiles_parse, **v) for k, v in tries.items()}
    # the same offsets from device memory
    keep = [on_device(x) for x in (text, bad_off, names, name_off)]
    out['refused']['device_text_off_start'] = refused(
        m.tiles_parse, text=keep[0].data_ptr(), text_off=keep[1].data_ptr(), names=keep[2].data_ptr(),
        name_off=keep[3].data_ptr(), device=True, n_files=len(text_off) - 1, **kw)
    # a text of 2^40 bytes is refused by its offsets alone, before a byte of it is touched
    import ctypes
    huge = np.array([0, 1 << 40], np.int64)
    c_in, c_out = _lib.TileTexts(), _lib.TileParseResult()
    c_in.text, c_in.text_off, c_in.names, c_in.name_off = text.ctypes.data, huge.ctypes.data, names.ctypes.data, name_off.ctypes.data
    c_in.n_files, c_in.memory = 1, _lib.OTR_MEM_HOST
    rc = _lib.lib().otr_tiles_parse(m._h, ctypes.byref(c_in), 3600, 0, b's', b'm', 0, ctypes.byref(c_out))
    out['refused']['text_too_large'] = _lib.last_error() if rc == _lib.OTR_BAD_REQUEST else None
    out['first'] = first
    out['after'] = device_copies(first)        # the previous result's device pointers still hold it
    out['rows_again'] = m.tiles_parse(**args, **kw)
pickle.dump(out, open(dst, 'wb'))
print('tile parse ok')
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
            dst = str(tmp_path_factory.mktemp('tile_parse') / (job + '.pkl'))
            t0 = time.perf_counter()
            p = subprocess.run([sys.executable, '-c', CHILD % (ROOT, graph_dir, dst, job)], env=env,
                               capture_output=True, text=True, timeout=240)
            assert p.returncode == 0 and 'tile parse ok' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
            print('child %s: %.1f s' % (job, time.perf_counter() - t0))
            with open(dst, 'rb') as f:
                _RUNS[job] = pickle.load(f)
        return _RUNS[job]
    return get


_WANT = {}


def want_of(case):
    """The restatement's result of a case, computed once."""
    if case['name'] not in _WANT:
        _WANT[case['name']] = P.parse(case)
    return _WANT[case['name']]


def _same(got, want, what):
    bad = P.differing(got, want)
    assert not bad, (what, bad)


CASES = C.cases()


@pytest.mark.parametrize('rules', [P.SIMPLE, P.STREAM])
def test_round_trip(rules, run_job):
    """many_reports' rows, culled at privacy 1 and written as texts that stay in HBM, parsed from
    those device pointers: the rows come back member by member with speed_bin -1, with the same
    files and row offsets, no line refused; the parsed rows written again give byte-identical
    texts and names; the result survives the text and the cull calls."""
    r = run_job('round_trip')[rules]
    kept, texts, p = r['kept'], r['texts'], r['parse']
    assert len(kept) > 1000 and texts['n_files'] > 2
    want = kept.copy()
    assert (want['speed_bin'] >= 0).all()
    want['speed_bin'] = -1
    assert p['rows'].tobytes() == want.tobytes()
    assert p['n_files'] == texts['n_files'] and p['n_rows'] == len(kept)
    assert p['file'].tobytes() == texts['file'].tobytes() and p['row_off'].tobytes() == texts['row_off'].tobytes()
    assert p['n_bad'] == 0 and p['n_bad_names'] == 0 and (p['first_bad'], p['first_bad_file'], p['first_bad_reason']) == (-1, -1, 0)
    assert p['n_headers'] == p['n_files'] and p['n_lines'] == p['n_rows'] + p['n_files']
    assert not p['file_status'].any() and set(p['line_status'].tolist()) == {P.ROW, P.HEADER}
    for k in ('text', 'names', 'text_off', 'name_off', 'row_off', 'file'):
        assert r['texts_again'][k].tobytes() == texts[k].tobytes(), k
    for k in ('parse_after', 'parse_after_cull'):
        _same(r[k], p, k)
    if rules == P.SIMPLE:
        h = r['headerless']
        assert h['n_headers'] == 0 and h['n_lines'] == h['n_rows'] == len(kept) and h['n_bad'] == 0
        assert h['rows'].tobytes() == want.tobytes() and h['row_off'].tobytes() == texts['row_off'].tobytes()
        assert h['file'].tobytes() == texts['file'].tobytes()


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_cases(case, run_job):
    """Statuses, rows, counts and first_bad* equal the restatement's exactly: the host copies and
    the device buffers of a parse of host text, and the device buffers of a parse of device text
    with OTR_TILE_PARSE_NO_HOST (no host array in the result)."""
    got = run_job('cases')[case['name']]
    want = want_of(case)
    for k in ('host', 'host_device', 'device'):
        _same(got[k], want, (case['name'], k))
    assert not set(got['no_host_keys']) & set(P.ARRAYS), got['no_host_keys']
    print('%s: %d lines, %d rows, device ms %.3f' % (case['name'], want['n_lines'], want['n_rows'], got['ms']))


def test_merge(run_job):
    """The files of two batches (ragged_city's even and odd traces) parsed in one call, the same
    names twice, and culled together at privacy 2: the texts are report_tiles of both halves' host
    lines together, which is not what culling the halves one by one gives."""
    r = run_job('merge')
    a, b = (h['lines'] for h in r['halves'])
    assert set(a) & set(b), 'the halves share no file name'
    assert r['parse']['n_bad'] == 0 and r['parse']['n_bad_names'] == 0
    assert r['parse']['n_files'] == len(a) + len(b) and r['parse']['n_rows'] == sum(len(h['rows']) for h in r['halves'])
    both = {k: a.get(k, []) + b.get(k, []) for k in set(a) | set(b)}
    want = {k: sr.COLUMNS + '\n' + ''.join(v) for k, v in sr.report_tiles(both, 2).items()}
    assert want and r['payloads'] == want
    apart = {}
    for half in (a, b):
        for k, v in sr.report_tiles(half, 2).items():
            apart[k] = apart.get(k, sr.COLUMNS + '\n') + ''.join(v)
    assert apart != want, 'the fixture does not tell a merged cull from two separate ones'


def test_report_match_dir(run_job):
    """A directory written by write_tiles and one in the reference's header-less form both come
    back from report_match_dir as the texts report_tiles gives for the same lines; the two
    directories together as those of every line twice; a line or a name the rows cannot express
    is a ValueError naming the file, the line and the reason, and nothing is reported."""
    r = run_job('match_dir')
    tiles = r['tiles']
    assert len(tiles) > 5
    for privacy in (1, 2):
        want = {k: sr.COLUMNS + '\n' + ''.join(v) for k, v in sr.report_tiles(tiles, privacy).items()}
        assert want and r[privacy]['with'] == want and r[privacy]['without'] == want
        twice = {k: sr.COLUMNS + '\n' + ''.join(v)
                 for k, v in sr.report_tiles({k: v + v for k, v in tiles.items()}, privacy).items()}
        assert r[privacy]['both'] == twice and twice != want
    assert sum(len(v) for v in sr.report_tiles(tiles, 2).values()) < sum(len(v) for v in tiles.values())
    last, n = r['last']
    assert r['bad_line'] and repr(last) in r['bad_line'] and 'U_COUNT' in r['bad_line'], r['bad_line']
    assert '(line %d of the file)' % n in r['bad_line']
    assert r['bad_name'] and "'notes.txt'" in r['bad_name'] and 'not a tile file name' in r['bad_name'], r['bad_name']
    assert r['none'] == {}


def test_refusals(run_job):
    """Every refusal of the call as a whole is a ValueError (OTR_BAD_REQUEST) naming its cause, from
    host and from device offsets, and leaves the previous result as it was: its device pointers
    still hold it, and the same call gives it again.  (The line limit, 2^31 - 1 lines, needs 2 GiB
    of text: it is not run here.)"""
    r = run_job('refusals')
    words = {'quantisation': 'quantisation', 'rules': 'unknown rules', 'source': '255 bytes', 'mode': '255 bytes',
             'text_off_start': 'ascend', 'name_off_start': 'ascend', 'text_off_descends': 'ascend',
             'name_off_descends': 'ascend', 'device_text_off_start': 'ascend', 'text_too_large': 'too large'}
    assert set(r['refused']) == set(words)
    for k, w in words.items():
        assert r['refused'][k] and w in r['refused'][k], (k, r['refused'][k])
    case = [c for c in CASES if c['name'] == 'fields_0'][0]
    want = want_of(case)
    _same(r['first'], want, 'first')
    _same(r['after'], want, 'device copies after the refusals')
    _same(r['rows_again'], want, 'again')
