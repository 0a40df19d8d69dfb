"""Rate of the session store's push path (otr_sessions_push), host to host.

Replays the traces of bench.py's deployed-configuration workload (c2dep: the metro graph, 100
probes every 15 s, sigma 10 m, mode defaults) as one arrival stream: coordinates narrowed to
float32, key = trace number, points in order of their time (stable), stream time in
milliseconds.  The stream is pushed in chunks of `--chunk-s` seconds of stream time (1 and 10 by
default) into a store with the reporter's gates (500 m, 10 points, 60 s), and punctuated at the
end.  Per chunk size: probes/s over the wall time of all pushes (input arrays on the host,
windows and reports back on the host), rounds per chunk, windows per round, and the split of
the wall time into the matcher's batches (match_ms) and everything else (session kernels, copies,
host).
One warm-up replay, then `--repeats` timed ones: median, minimum and maximum are reported.
`--tile-store` replays every chunk size a second time with a tile store open (quantisation
3600, privacy 2): otr_tile_store_add_session after every push, inside the timed loop, and one
flush after the final punctuate; the summed add device_ms, the flush device_ms and the rows held
at the flush are reported beside the plain run's probes/s.

`--text sv|json` renders the stream as raw messages ("uuid,lat,lon,time,accuracy" lines, or the
objects of `@json@id@latitude@longitude@timestamp@accuracy`; floats as '%.9g') and feeds every chunk
through otr_sessions_push_text instead: the text is the only input, no point is parsed on the
host.  The formatter's parse_ms and total_ms, summed over the pushes, are reported beside the
push's times; and the whole stream is formatted alone as one text (otr_format_messages: warm-up,
then `--repeats` steps) for its messages/s and input GB/s, for SV next to K11's parse_ms from
otr_ingest(OTR_INGEST_JAVA_SV) on the same text.  `--graph city` replays the small city graph.

    python -m reporter_amd.tools.sessions_rate --traces 2000 --out profiles/sessions_c2dep.json
    python -m reporter_amd.tools.sessions_rate --traces 2000 --text json --out profiles/formatter_c2dep_json.json

`--restore` replays the stream in 10 s chunks to its midpoint and times, on the store as it stands
there (one warm-up, `--repeats` timed; median [min, max] of the wall time and of the device time:
the call's own device_ms, or HIP events on the matcher's stream around the call): the snapshot,
the export as records, take-all with remove, the restore from the snapshot's arrays and the
restore from the records; beside them the store's sessions, points and record bytes and one plain
device-to-device copy of as many bytes.  With OTR_LIB naming a library built before these calls
existed it times the snapshot alone (the comparand in profiles/sessions_restore_c2dep.json).

    python -m reporter_amd.tools.sessions_rate --traces 2000 --tile-store --out profiles/tile_store_c2dep.json
    python -m reporter_amd.tools.sessions_rate --traces 2000 --restore --out profiles/sessions_restore_c2dep.json

`--names` runs the same stream through a store with the uuid directory (otr_sessions_open_named,
uuid_bytes 36): every point carries the 36-byte name 'veh-' + its key in 32 digits (with `--text`
the names are the uuids of the text).  It also reports `name_cost`: the stream's chunks through
otr_sessions_advance on a store whose gates never pass (no window, so no matching), with and without
names, HIP events on the matcher's stream around every call, summed per replay: the difference is
the device time of the name kernels and of the names' copies.

    python -m reporter_amd.tools.sessions_rate --traces 2000 --names --out profiles/session_names_c2dep.json

`--tile-store --text` (no value after `--text`) measures the last step of the chain, the flush to
finished file payloads, in one process on two fills of the store: the replay's own rows (10 s
chunks, privacy 2) and a seeded add_rows of `--tile-rows` rows over 300 files at privacy 1.  One
warm-up of each path (their payloads are compared there), then `--repeats` timed runs alternating:
the host path tile_store_flush + stream_tile_payloads, and the device path tile_store_flush_text +
stream_tile_payloads_device, both as host wall time ending in the {name: text} dict, the device
path's device_ms (flush + text stage) beside it; median [min, max].

    python -m reporter_amd.tools.sessions_rate --traces 2000 --tile-store --text --out profiles/tile_text_c2dep.json

`--tile-store --text --parse` measures the way back (K21) on the same two fills: one flush with texts,
then otr_tiles_parse of those texts from the device pointers (device_ms) and from the host arrays to
host arrays (wall time), beside otr_tiles_text of the same rows in HBM (K19's device_ms); one warm-up,
`--repeats` timed runs, median [min, max].

    python -m reporter_amd.tools.sessions_rate --traces 2000 --tile-store --text --parse --out profiles/tile_parse_c2dep.json

`--tile-store --records` times the tile store's state leaving and coming back (K20) on a store with
the times: export_records, restore_records from device and from host arrays, and snapshot +
restore, on the replay's held rows at the stream's midpoint and on `--tile-rows` synthetic rows,
each beside a plain device-to-device copy of the record bytes and beside the host path (snapshot to
the host plus the Python restatement, on at most 65536 rows); and one add on a store with the
times against the same add on a plain store.

    python -m reporter_amd.tools.sessions_rate --traces 2000 --tile-store --records --out profiles/tile_records_c2dep.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
T_BEGIN = 1483228800


def stream(tr):
    """The arrival stream of a gen.Traces batch and the chunk boundaries' stream times."""
    key = np.repeat(np.arange(tr.n_traces, dtype=np.uint64) + 1, np.diff(tr.offsets))
    tm = np.asarray(tr.time, np.int64)
    order = np.argsort(tm, kind='stable')
    acc = np.full(len(order), 10, np.int32) if tr.accuracy is None else np.ceil(tr.accuracy[order]).astype(np.int32)
    return {'key': key[order], 'lat': np.asarray(tr.lat)[order].astype(np.float32),
            'lon': np.asarray(tr.lon)[order].astype(np.float32), 'accuracy': acc, 'time': tm[order],
            'timestamp': tm[order] * 1000}


TEXT_FORMATS = {'sv': {'type': 'sv', 'separator': ',', 'uuid_index': 0, 'lat_index': 1, 'lon_index': 2,
                       'time_index': 3, 'accuracy_index': 4, 'time_format': 0},
                'json': {'type': 'json', 'uuid_key': 'id', 'lat_key': 'latitude', 'lon_key': 'longitude',
                         'time_key': 'timestamp', 'accuracy_key': 'accuracy', 'time_format': 0}}


def render(pts, kind):
    """The stream as one message per point (bytes, no newline)."""
    shape = ('veh-%d,%.9g,%.9g,%d,%d' if kind == 'sv' else
             '{"id":"veh-%d","latitude":%.9g,"longitude":%.9g,"timestamp":%d,"accuracy":%d}')
    return [(shape % (k, la, lo, t, a)).encode() for k, la, lo, t, a in zip(
        pts['key'].tolist(), pts['lat'].astype(np.float64).tolist(), pts['lon'].astype(np.float64).tolist(),
        pts['time'].tolist(), pts['accuracy'].tolist())]


def text_chunks(msgs, pts, cuts):
    """(text, offsets, timestamps) per chunk, as Matcher.sessions_push_text takes them."""
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        off = np.concatenate([[0], np.cumsum([len(x) for x in msgs[a:b]])]).astype(np.int64)
        out.append((b''.join(msgs[a:b]), off, pts['timestamp'][a:b]))
    return out


def formatter_rates(m, msgs, kind, repeats):
    """otr_format_messages on the whole stream as one newline-separated text: a warm-up, then
    `repeats` steps; for SV also K11's parse on the same text."""
    text = b'\n'.join(msgs) + b'\n'
    fmt = TEXT_FORMATS[kind]
    m.format_messages(text, fmt, arrays=False)
    runs = [m.format_messages(text, fmt, arrays=False) for _ in range(repeats)]
    assert runs[0]['n_points'] == len(msgs), (runs[0]['n_points'], len(msgs))
    parse = sorted(r['parse_ms'] for r in runs)
    total = sorted(r['total_ms'] for r in runs)
    med = float(np.median(parse))
    out = {'messages': len(msgs), 'bytes': len(text), 'bytes_per_message': round(len(text) / len(msgs), 1),
           'parse_ms_median_min_max': [round(med, 4), round(parse[0], 4), round(parse[-1], 4)],
           'total_ms_median_min_max': [round(float(np.median(total)), 4), round(total[0], 4), round(total[-1], 4)],
           'parse_messages_per_s': round(len(msgs) / (1e-3 * med), 1), 'parse_GB_per_s': round(len(text) / (1e6 * med), 3),
           'total_messages_per_s': round(len(msgs) / (1e-3 * float(np.median(total))), 1)}
    if kind == 'sv':
        from reporter_amd import _lib
        kw = dict(rules=_lib.OTR_INGEST_JAVA_SV, separator=',', uuid_index=0, lat_index=1, lon_index=2, time_index=3,
                  accuracy_index=4, time_format=_lib.OTR_TIME_EPOCH, inactivity=120)
        m.ingest(text, **kw)
        k11 = sorted(m.ingest(text, **kw)[0].parse_ms for _ in range(repeats))
        out['k11_parse_ms_median_min_max'] = [round(float(np.median(k11)), 4), round(k11[0], 4), round(k11[-1], 4)]
    return out


NAME_BYTES = 36


def stream_names(pts):
    """One 36-byte name per point: 'veh-' and the key in 32 digits."""
    from reporter_amd import _lib
    data, off, ln = _lib.pack_names([b'veh-%032d' % k for k in pts['key'].tolist()])
    return {'bytes': data, 'off': off, 'len': ln}


def names_chunk(names, a, b):
    """The names of points a .. b-1 over their own bytes."""
    lo, hi = int(names['off'][a]), int(names['off'][b - 1]) + int(names['len'][b - 1])
    return {'bytes': names['bytes'][lo:hi], 'off': names['off'][a:b] - lo, 'len': names['len'][a:b]}


def name_cost(m, pts, cuts, max_points, names, repeats):
    """The chunks through sessions_advance on a store that never reports, plain and named: the
    summed device time (HIP events around every call) of a replay, median [min, max]."""
    import torch
    stream = torch.cuda.ExternalStream(m.stream)
    chunks = [({k: v[a:b] for k, v in pts.items()}, names_chunk(names, a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
    out = {}
    for kind in ('plain', 'named'):
        sums = []
        for _ in range(repeats + 1):
            m.sessions_open(int(pts['key'].max()) + 1, max_points, report_dist=1e9, report_count=1 << 30,
                            uuid_bytes=NAME_BYTES if kind == 'named' else 0)
            total = 0.0
            for c, nm in chunks:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                b, _ = m.sessions_advance(c, names=nm if kind == 'named' else None)
                e1.record(stream)
                e1.synchronize()
                assert b.n_traces == 0
                total += e0.elapsed_time(e1)
            m.sessions_close()
            sums.append(total)
        v = sorted(sums[1:])
        out[kind + '_advance_ms_median_min_max'] = [round(float(np.median(v)), 3), round(v[0], 3), round(v[-1], 3)]
    out['names_ms'] = round(out['named_advance_ms_median_min_max'][0] - out['plain_advance_ms_median_min_max'][0], 3)
    out['chunks'] = len(chunks)
    return out


def replay(m, pts, cuts, max_points, batch_ms, tile_rows=0, text=None, names=None, hold=False):
    """One replay: a fresh store, every chunk pushed, a final punctuate.  tile_rows > 0: a tile
    store of that many rows takes every result (add_session) and is flushed at the end.
    text: (kind, chunks of text_chunks): every chunk goes through sessions_push_text.
    names: stream_names' dict, or True with text: the store has the uuid directory.
    hold: the tile store is neither flushed nor closed (the caller does both)."""
    m.sessions_open(int(pts['key'].max()) + 1, max_points, uuid_bytes=NAME_BYTES if names is not None else 0)
    if tile_rows:
        m.tile_store_open(tile_rows, 3600, 2)
    add_ms = []
    chunks = text[1] if text else [{k: v[a:b] for k, v in pts.items()} for a, b in zip(cuts[:-1], cuts[1:])]
    nchunks = None if text or names is None else [names_chunk(names, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    rounds = windows = reports = 0
    dev_ms = match_ms = parse_ms = format_ms = 0.0
    t0 = time.perf_counter()
    for i, c in enumerate(chunks):
        if text:
            f, r = m.sessions_push_text(c[0], TEXT_FORMATS[text[0]], msg_off=c[1], timestamp=c[2], arrays=False)
            parse_ms += f['parse_ms']
            format_ms += f['total_ms']
        else:
            r = m.sessions_push(c, names=nchunks[i] if nchunks else None)
        rounds += r['n_rounds']
        windows += r['n_windows']
        reports += r['n_reports']
        dev_ms += r['device_ms']
        match_ms += r['match_ms']
        if tile_rows:
            add_ms.append(m.tile_store_add_session()['device_ms'])
    wall = time.perf_counter() - t0
    ev = m.sessions_punctuate(int(pts['timestamp'][-1]) + 10 ** 9)
    tile = None
    if tile_rows:
        add_ms.append(m.tile_store_add_session()['device_ms'])
    if tile_rows and not hold:
        t1 = time.perf_counter()
        fl = m.tile_store_flush()
        tile = {'adds': len(add_ms), 'add_ms': float(np.sum(add_ms)), 'add_ms_max': float(np.max(add_ms)),
                'flush_ms': fl['device_ms'], 'flush_wall_ms': 1e3 * (time.perf_counter() - t1),
                'rows_held': fl['n_rows_in'], 'rows_kept': fl['n_rows'], 'files': fl['n_files'],
                'files_empty': fl['n_files_empty']}
        m.tile_store_close()
    m.sessions_close()
    return {'tile': tile, 'wall_s': wall, 'parse_ms': parse_ms, 'format_ms': format_ms, 'rounds': rounds, 'windows': windows, 'reports': reports, 'stream_ms': dev_ms, 'match_ms': match_ms,
            'evicted': ev['n_evicted'], 'eviction_windows': ev['n_windows'], 'chunks': len(chunks)}


def seeded_rows(n, files=300, seed=19):
    """n tile rows over `files` files of one hour, a few thousand pairs a file: ids of 11 to 12 digits,
    a next id on three rows of four, times of 10 digits (about 80 bytes of text a row)."""
    from reporter_amd import _lib
    rng = np.random.RandomState(seed)
    rows = np.zeros(n, _lib.TILE_ROW)
    tile = rng.randint(0, files, n).astype(np.uint64)
    index = rng.randint(0, 4000, n).astype(np.uint64)
    rows['id'] = np.uint64(1) | (np.uint64(700000) + tile) << np.uint64(3) | index << np.uint64(25)
    rows['next_id'] = rows['id'] + (np.uint64(1) << np.uint64(25))
    rows['next_id'][rng.randint(0, 4, n) == 0] = 0x3fffffffffff
    rows['file'] = (np.uint64(T_BEGIN // 3600) << np.uint64(25)) | (np.uint64(1) << np.uint64(22)) | \
        ((rows['id'] >> np.uint64(3)) & np.uint64(0x3fffff))
    rows['start'] = T_BEGIN + rng.randint(0, 3600, n)
    rows['end'] = rows['start'] + rng.randint(1, 120, n)
    rows['duration'] = rows['end'] - rows['start']
    rows['length'] = rng.randint(20, 1500, n)
    rows['queue_length'] = rng.randint(0, 4, n) // 3 * rng.randint(0, 100, n)
    return rows


def tile_text_rates(m, fill, close, repeats):
    """The flush to file payloads both ways on the store `fill` leaves open (`close` closes it):
    one warm-up each, then `repeats` timed runs alternating."""
    from reporter_amd import simple_reporter as sr

    def host():
        fill()
        t0 = time.perf_counter()
        fl = m.tile_store_flush()
        p = sr.stream_tile_payloads(fl, 'auto', 'reporter')
        wall = 1e3 * (time.perf_counter() - t0)
        close()
        return p, {'wall_ms': wall, 'flush_ms': fl['device_ms'], 'rows_held': fl['n_rows_in'], 'rows_kept': fl['n_rows'],
                   'files': fl['n_files']}

    def device():
        fill()
        fl = {}
        t0 = time.perf_counter()
        p = sr.stream_tile_payloads_device(m, 'auto', 'reporter', flush_out=fl)
        wall = 1e3 * (time.perf_counter() - t0)
        close()
        return p, {'wall_ms': wall, 'flush_ms': fl['device_ms'], 'text_ms': fl['text_ms'],
                   'device_ms': fl['device_ms'] + fl['text_ms'], 'text_bytes': fl['n_text_bytes']}

    (pa, a), (pb, b) = host(), device()
    if pa != pb:
        raise RuntimeError('the device texts differ from stream_tile_payloads')
    del pa, pb
    runs_a, runs_b = [], []
    for _ in range(repeats):
        runs_a.append(host()[1])
        runs_b.append(device()[1])

    def med(runs, k):
        v = sorted(x[k] for x in runs)
        return [round(float(np.median(v)), 3), round(float(v[0]), 3), round(float(v[-1]), 3)]

    return {'rows_held': a['rows_held'], 'rows_kept': a['rows_kept'], 'files': a['files'], 'text_bytes': b['text_bytes'],
            'host_path': {'what': 'tile_store_flush + stream_tile_payloads', 'wall_ms_median_min_max': med(runs_a, 'wall_ms'),
                          'flush_ms_median_min_max': med(runs_a, 'flush_ms')},
            'device_path': {'what': 'tile_store_flush_text + stream_tile_payloads_device',
                            'wall_ms_median_min_max': med(runs_b, 'wall_ms'),
                            'device_ms_median_min_max': med(runs_b, 'device_ms'),
                            'flush_ms_median_min_max': med(runs_b, 'flush_ms'),
                            'text_ms_median_min_max': med(runs_b, 'text_ms')}}


def tile_parse_rates(m, fill, close, repeats):
    """K21 on the texts K19 wrote for the store `fill` leaves open (`close` closes it): one flush
    with texts, then otr_tiles_parse of those texts, one warm-up and `repeats` timed runs each way:
    from the device pointers with device copies only (device_ms), and from the host arrays to the
    host arrays (wall time); beside them otr_tiles_text of the parsed rows in HBM, the same rows
    K19 wrote the texts from (device_ms)."""
    fill()
    fl = m.tile_store_flush_text('reporter', 'auto')
    kw = dict(quantisation=fl['quantisation'], rules=1, source='reporter', mode='auto')
    host_args = {k: fl[k] for k in ('text', 'text_off', 'names', 'name_off')}

    def device():
        return m.tiles_parse(text=fl['d_text'], text_off=fl['d_text_off'], names=fl['d_names'], name_off=fl['d_name_off'],
                             device=True, n_files=fl['n_files'], host=False, **kw)

    def host():
        t0 = time.perf_counter()
        r = m.tiles_parse(**host_args, **kw)
        return r, 1e3 * (time.perf_counter() - t0)

    r = device()
    if r['n_bad'] or r['n_bad_names'] or r['n_rows'] != fl['n_rows'] or host()[0]['n_rows'] != fl['n_rows']:
        raise RuntimeError('the texts of the flush do not parse back into its rows')
    dev_ms, wall_ms, host_dev_ms, text_ms = [], [], [], []
    for _ in range(repeats):
        dev_ms.append(device()['device_ms'])
        h, w = host()
        wall_ms.append(w)
        host_dev_ms.append(h['device_ms'])
    p = device()
    m.tiles_text(device_ptr=p['d_rows'], n=p['n_rows'], host=False, **kw)
    for _ in range(repeats):
        text_ms.append(m.tiles_text(device_ptr=p['d_rows'], n=p['n_rows'], host=False, **kw)['device_ms'])
    close()

    def med(v):
        v = sorted(v)
        return [round(float(np.median(v)), 3), round(float(v[0]), 3), round(float(v[-1]), 3)]

    return {'rows': fl['n_rows'], 'files': fl['n_files'], 'text_bytes': fl['n_text_bytes'], 'lines': r['n_lines'],
            'k19_flush_text_ms': round(fl['text_ms'], 3),
            'k19_tiles_text_device_ms_median_min_max': med(text_ms),
            'k21_device_text_device_ms_median_min_max': med(dev_ms),
            'k21_host_to_host_wall_ms_median_min_max': med(wall_ms),
            'k21_host_to_host_device_ms_median_min_max': med(host_dev_ms)}


def restore_rates(m, pts, max_points, repeats):
    """The store at the stream's midpoint (10 s chunks): snapshot, export, take-all, restore from
    the SoA and from records, each timed `repeats` times after a warm-up."""
    import torch
    n = len(pts['key'])
    sec = (pts['time'] - pts['time'][0]) // 10
    cuts = [0] + (np.flatnonzero(np.diff(sec)) + 1).tolist() + [n]
    cuts = [c for c in cuts if c <= n // 2]
    m.sessions_open(int(pts['key'].max()) + 1, max_points)
    for a, b in zip(cuts[:-1], cuts[1:]):
        m.sessions_push({k: v[a:b] for k, v in pts.items()})
    stream = torch.cuda.ExternalStream(m.stream)
    times = {}

    def timed(name, f, *a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        r = f(*a, **kw)
        wall = 1e3 * (time.perf_counter() - t0)
        e1.record(stream)
        e1.synchronize()
        dev = r['device_ms'] if isinstance(r, dict) and 'device_ms' in r else e0.elapsed_time(e1)
        times.setdefault(name, []).append((wall, float(dev)))
        return r

    from reporter_amd import _lib
    has_restore = hasattr(_lib.lib(), 'otr_sessions_restore')   # (a library from before K17: the snapshot alone)
    for _ in range(repeats + 1):
        snap = timed('snapshot', m.sessions_snapshot)
        if not has_restore:
            continue
        rec = timed('export_records', m.sessions_export_records)
        taken = timed('take_all', m.sessions_take, 1, 0)
        timed('restore', m.sessions_restore, taken)
        m.sessions_take(1, 0)
        timed('restore_records', m.sessions_restore_records, rec['key'], rec['rec_off'], rec['bytes'])
    out = {'points_pushed': cuts[-1], 'sessions': len(snap['key']), 'points': len(snap['time'])}
    if has_restore:
        nb = len(rec['bytes'])
        out['record_bytes'] = nb
        src = torch.zeros(max(nb, 1), dtype=torch.uint8, device='cuda')
        dst = torch.empty_like(src)
        cp = []
        for _ in range(repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            e1.synchronize()
            cp.append(e0.elapsed_time(e1))
        cp = sorted(cp[1:])
        out['device_copy_ms_median_min_max'] = [round(float(np.median(cp)), 4), round(cp[0], 4), round(cp[-1], 4)]
        after = m.sessions_snapshot()
        assert all(np.array_equal(after[k], snap[k]) for k in snap), 'the store changed over the repeats'
    for name, v in times.items():
        wall, dev = sorted(x[0] for x in v[1:]), sorted(x[1] for x in v[1:])
        out[name] = {'wall_ms_median_min_max': [round(float(np.median(wall)), 4), round(wall[0], 4), round(wall[-1], 4)],
                     'device_ms_median_min_max': [round(float(np.median(dev)), 4), round(dev[0], 4), round(dev[-1], 4)]}
    m.sessions_close()
    return out


def synthetic_reports(n, files=300, q=3600):
    """n valid reports over `files` (bucket, tile) files, one row each, as one window."""
    k = np.arange(n, dtype=np.int64)
    tile = (k % files).astype(np.uint64)
    idx = ((k // files) % 50).astype(np.uint64)
    sid = np.uint64(1) | (tile << np.uint64(3))
    t0 = T_BEGIN + 10.0 + (k % 3000) + 0.25 * (k % 4)
    return {'rep_off': np.array([0, n], np.int64), 'id': sid | (idx << np.uint64(25)),
            'next_id': sid | ((idx + np.uint64(1)) << np.uint64(25)), 't0': t0, 't1': t0 + 2.5 + (k % 7),
            'length': (40 + k % 400).astype(np.int32), 'queue_length': (k % 3).astype(np.int32)}


def records_rates(m, M, fill, repeats, slice_size=20000, host_rows=1 << 16):
    """fill(m, times) leaves m's tile store open and filled.  Device time (HIP events on the
    matcher's stream around the call, so host copies are inside) and wall time of the export, of
    restore_records from the export's device arrays and from its host arrays, of snapshot + restore
    into a second matcher's store, beside a plain device-to-device copy of the record bytes; and
    the host path on the first `host_rows` held rows: snapshot to the host plus the Python
    restatement (tests/tile_records_ref.py)."""
    import torch
    from tests import tile_records_ref as X
    fill(m, True)
    n = m.tile_store_snapshot(host=False)['n_rows']
    m2 = M.Matcher()

    def timed(f, matcher=m):
        s = torch.cuda.ExternalStream(matcher.stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(s)
        r = f()
        e1.record(s)
        e1.synchronize()
        return r, e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0)

    def mmm(v):
        v = sorted(v)
        return [round(float(np.median(v)), 3), round(v[0], 3), round(v[-1], 3)]

    t = {k: [] for k in ('export', 'restore_records_device', 'restore_records_host', 'snapshot_device', 'restore_rows_device',
                         'copy_d2d')}
    w = {k: [] for k in t}
    for i in range(repeats + 1):
        rec, a, b = timed(lambda: m.tile_store_export_records(slice_size))
        snap, c, d = timed(lambda: m.tile_store_snapshot(host=False))
        runs = {'export': (a, b), 'snapshot_device': (c, d)}
        for kind in ('restore_records_device', 'restore_records_host', 'restore_rows_device'):
            m2.tile_store_open(max(n, 1), 3600, 2, times=True)
            if kind == 'restore_rows_device':
                r, a, b = timed(lambda: m2.tile_store_restore(snap, device=True), m2)
            else:
                r, a, b = timed(lambda: m2.tile_store_restore_records(rec, device=kind.endswith('device')), m2)
            assert r['n_rows'] == n, (kind, r, n)
            m2.tile_store_close()
            runs[kind] = (a, b)
        src = torch.empty(max(rec['n_bytes'], 1), dtype=torch.uint8, device='cuda')
        dst = torch.empty_like(src)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        runs['copy_d2d'] = (e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0))
        if i:   # the first pass is the warm-up
            for k, (a, b) in runs.items():
                t[k].append(a)
                w[k].append(b)
    out = {'rows': n, 'slice_size': slice_size, 'slices': rec['n_slices'], 'files': rec['n_tiles'],
           'record_bytes': rec['n_bytes'], 'snapshot_bytes': 72 * n}
    for k in t:
        out[k + '_device_ms_median_min_max'] = mmm(t[k])
        out[k + '_wall_ms_median_min_max'] = mmm(w[k])
    # the host path: the rows and times to the host, the restatement writes and reads the bytes
    t0 = time.perf_counter()
    s = m.tile_store_snapshot()
    snap_ms = 1e3 * (time.perf_counter() - t0)
    h = min(n, host_rows)
    held = (s['rows'][:h], s['t0'][:h], s['t1'][:h])
    t0 = time.perf_counter()
    hrec = X.export(held, 3600, slice_size)
    exp_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    X.restore_records(X.empty_held(), hrec, 3600, h)
    res_ms = 1e3 * (time.perf_counter() - t0)
    out['host_path'] = {'snapshot_to_host_wall_ms': round(snap_ms, 3), 'rows_restated': h,
                        'python_export_wall_ms': round(exp_ms, 1), 'python_restore_wall_ms': round(res_ms, 1)}
    m.tile_store_close()
    return out


def add_times(m, reports, max_rows, repeats):
    """The same add on a plain store and on a store with the times: device_ms, median [min, max]."""
    out = {}
    for times in (False, True):
        v = []
        for i in range(repeats + 1):
            m.tile_store_open(max_rows, 3600, 2, times=times)
            r = m.tile_store_add_reports(reports)
            m.tile_store_close()
            if i:
                v.append(r['device_ms'])
        v = sorted(v)
        out['timed_add_ms' if times else 'plain_add_ms'] = [round(float(np.median(v)), 3), round(v[0], 3), round(v[-1], 3)]
    out['rows'] = r['n_rows_added']
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--traces', type=int, default=2000, help='traces of the c2dep workload (bench.py --json-traces)')
    ap.add_argument('--chunk-s', type=int, nargs='+', default=[1, 10])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--max-points', type=int, default=128)
    ap.add_argument('--graphs', default=os.path.join(ROOT, 'build', 'graphs'))
    ap.add_argument('--tile-store', action='store_true',
                    help='also replay with a tile store: add_session after every push, one flush at the end')
    ap.add_argument('--tile-rows', type=int, default=1 << 22, help='max_rows of that store')
    ap.add_argument('--text', choices=['sv', 'json', 'tiles'], nargs='?', const='tiles', default=None,
                    help='sv, json: render the stream as messages and push them through otr_sessions_push_text; '
                         'no value, with --tile-store: time the flush to file payloads on the host and on the device')
    ap.add_argument('--parse', action='store_true',
                    help='with --tile-store --text: time otr_tiles_parse (K21) on the texts of the flush instead')
    ap.add_argument('--restore', action='store_true',
                    help='time snapshot, export, take-all and the two restores on the store at the midpoint')
    ap.add_argument('--records', action='store_true',
                    help='with --tile-store: time export, restore_records and snapshot + restore of the tile store')
    ap.add_argument('--names', action='store_true',
                    help='the store has the uuid directory: every point is pushed with a 36-byte name')
    ap.add_argument('--graph', choices=['metro', 'city'], default='metro')
    ap.add_argument('--format-traces', type=int, default=0,
                    help='with --text: traces of the stream formatted alone (default: --traces)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from reporter_amd import matcher as M
    from reporter_amd.tools import gen
    gpath = gen.graph_path(args.graph, args.graphs)
    tr = gen.make_traces(gpath, args.traces, 100, 15, 10.0, 2, 0.0, 0.0, None, t_begin=T_BEGIN, t_spread=1800)
    M.configure(M.default_config(gpath))
    m = M.Matcher()
    pts = stream(tr)
    n = len(pts['key'])
    # the device batch's fixed cost on this machine: a batch of one trace, timed alone
    one = tr.subset([0])
    m.match_batch(one, copy_out=False, copy_reports=True)
    tb = []
    for _ in range(20):
        t0 = time.perf_counter()
        m.match_batch(one, copy_out=False, copy_reports=True)
        tb.append(1e3 * (time.perf_counter() - t0))
    batch_ms = float(np.median(tb))
    if args.restore:
        res = {'workload': 'c2dep: %s graph, %d traces x 100 probes @15 s, sigma 10 m, deployed configuration, '
                           '10 s chunks to the midpoint' % (args.graph, args.traces),
               'method': '1 warm-up, %d timed; median [min, max]; device_ms of the call, or HIP events on the '
                         "matcher's stream around it" % args.repeats,
               'restore': restore_rates(m, pts, args.max_points, args.repeats)}
        line = json.dumps(res, indent=1)
        print(line)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(line + '\n')
        return
    if args.records:
        if not args.tile_store:
            ap.error('--records goes with --tile-store')
        sec = (pts['time'] - pts['time'][0]) // 10
        cuts = [0] + (np.flatnonzero(np.diff(sec)) + 1).tolist() + [n]
        half = cuts[:len(cuts) // 2 + 1]
        syn = synthetic_reports(args.tile_rows)

        def fill_replay(mm, times):
            mm.sessions_open(int(pts['key'].max()) + 1, args.max_points)
            mm.tile_store_open(args.tile_rows, 3600, 2, times=times)
            for a, b in zip(half[:-1], half[1:]):
                mm.sessions_push({k: v[a:b] for k, v in pts.items()})
                mm.tile_store_add_session()
            mm.sessions_close()

        def fill_synthetic(mm, times):
            mm.tile_store_open(args.tile_rows, 3600, 2, times=times)
            mm.tile_store_add_reports(syn)

        res = {'workload': 'c2dep: %s graph, %d traces x 100 probes @15 s, sigma 10 m, deployed configuration, 10 s '
                           'chunks to the midpoint; and %d synthetic reports over 300 files'
                           % (args.graph, args.traces, args.tile_rows),
               'method': '1 warm-up pass, %d timed; median [min, max]; device time: HIP events on the matcher\'s stream '
                         'around the call (its copies to the host included); restores go into a second matcher\'s '
                         'empty store with the times' % args.repeats,
               'tile_records': {'replay_midpoint': records_rates(m, M, fill_replay, args.repeats),
                                'synthetic': records_rates(m, M, fill_synthetic, args.repeats),
                                'add_timed_against_plain': add_times(m, syn, args.tile_rows, args.repeats)}}
        line = json.dumps(res, indent=1)
        print(line)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(line + '\n')
        return
    if args.text == 'tiles':
        if not args.tile_store:
            ap.error('--text without a value goes with --tile-store')
        sec = (pts['time'] - pts['time'][0]) // 10
        cuts = [0] + (np.flatnonzero(np.diff(sec)) + 1).tolist() + [n]
        rows = seeded_rows(args.tile_rows)

        def fill_rows():
            m.tile_store_open(args.tile_rows, 3600, 1)
            m.tile_store_add_rows(rows)

        if args.parse:
            res = {'workload': 'c2dep: %s graph, %d traces x 100 probes @15 s, sigma 10 m, deployed configuration; and '
                               '%d seeded rows over 300 files' % (args.graph, args.traces, args.tile_rows),
                   'method': 'one process; one flush with texts per leg, then 1 warm-up and %d timed runs of each call '
                             'on those texts; device_ms: the call\'s HIP events (its copies included); wall: host '
                             'arrays in to host arrays out; median [min, max]' % args.repeats,
                   'tile_parse': {
                       'replay_10_s_privacy_2': tile_parse_rates(
                           m, lambda: replay(m, pts, cuts, args.max_points, batch_ms, args.tile_rows, hold=True),
                           m.tile_store_close, args.repeats),
                       'add_rows_privacy_1': tile_parse_rates(m, fill_rows, m.tile_store_close, args.repeats)}}
            line = json.dumps(res, indent=1)
            print(line)
            if args.out:
                with open(args.out, 'w') as f:
                    f.write(line + '\n')
            return
        res = {'workload': 'c2dep: %s graph, %d traces x 100 probes @15 s, sigma 10 m, deployed configuration; and '
                           '%d seeded rows over 300 files' % (args.graph, args.traces, args.tile_rows),
               'method': 'one process; 1 warm-up of each path, then %d timed runs alternating; host wall time from '
                         'the flush call to the {name: text} dict; median [min, max]' % args.repeats,
               'tile_text': {
                   'replay_10_s_privacy_2': tile_text_rates(
                       m, lambda: replay(m, pts, cuts, args.max_points, batch_ms, args.tile_rows, hold=True),
                       m.tile_store_close, args.repeats),
                   'add_rows_privacy_1': tile_text_rates(m, fill_rows, m.tile_store_close, args.repeats)}}
        line = json.dumps(res, indent=1)
        print(line)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(line + '\n')
        return
    msgs = render(pts, args.text) if args.text else None
    res = {'workload': 'c2dep: %s graph, %d traces x 100 probes @15 s, sigma 10 m, deployed configuration' % (args.graph, args.traces),
           'probes': n, 'gates': '500 m, 10 points, 60 s; session_gap 60000; max_points %d' % args.max_points,
           'method': 'arrays on the host -> otr_sessions_push per chunk -> windows and reports on the host; '
                     '1 warm-up replay, %d timed; median [min, max]' % args.repeats,
           'smallest_batch_ms': round(batch_ms, 3), 'chunks': {}}
    if args.text:
        res['text'] = args.text
        res['method'] = res['method'].replace('arrays on the host -> otr_sessions_push',
                                              'message text on the host -> otr_sessions_push_text')
        alone = msgs
        if args.format_traces > args.traces:
            alone = render(stream(gen.make_traces(gpath, args.format_traces, 100, 15, 10.0, 2, 0.0, 0.0, None,
                                                  t_begin=T_BEGIN, t_spread=1800)), args.text)
        res['formatter'] = formatter_rates(m, alone, args.text, max(args.repeats, 5))
    names = (True if args.text else stream_names(pts)) if args.names else None
    if args.names:
        res['names'] = 'uuid directory, uuid_bytes %d' % NAME_BYTES
    for cs in args.chunk_s:
        sec = (pts['time'] - pts['time'][0]) // cs
        cuts = [0] + (np.flatnonzero(np.diff(sec)) + 1).tolist() + [n]
        text = (args.text, text_chunks(msgs, pts, cuts)) if args.text else None
        replay(m, pts, cuts, args.max_points, batch_ms, text=text, names=names)
        runs = [replay(m, pts, cuts, args.max_points, batch_ms, text=text, names=names) for _ in range(args.repeats)]
        rate = sorted(n / r['wall_s'] for r in runs)
        r = runs[0]
        wall = float(np.median([x['wall_s'] for x in runs]))
        res['chunks']['%d_s' % cs] = {
            'chunks': r['chunks'], 'points_per_chunk': round(n / r['chunks'], 1),
            'probes_per_s': round(float(np.median(rate)), 1), 'probes_per_s_min_max': [round(rate[0], 1), round(rate[-1], 1)],
            'wall_ms': round(1e3 * wall, 1), 'rounds_per_chunk': round(r['rounds'] / r['chunks'], 3),
            'windows_per_round': round(r['windows'] / max(r['rounds'], 1), 2), 'windows': r['windows'],
            'reports': r['reports'], 'evicted_at_end': r['evicted'],
            'stream_ms': round(float(np.median([x['stream_ms'] for x in runs])), 1),
            'match_ms': round(float(np.median([x['match_ms'] for x in runs])), 1),
            'rounds_times_smallest_batch_ms': round(r['rounds'] * batch_ms, 1)}
        if args.text:
            res['chunks']['%d_s' % cs].update(
                format_parse_ms=round(float(np.median([x['parse_ms'] for x in runs])), 2),
                format_total_ms=round(float(np.median([x['format_ms'] for x in runs])), 2))
        if args.names and not args.text:
            res['chunks']['%d_s' % cs]['name_cost'] = name_cost(m, pts, cuts, args.max_points, names, args.repeats)
        if args.tile_store:
            replay(m, pts, cuts, args.max_points, batch_ms, args.tile_rows, text, names)
            truns = [replay(m, pts, cuts, args.max_points, batch_ms, args.tile_rows, text, names)
                     for _ in range(args.repeats)]
            trate = sorted(n / x['wall_s'] for x in truns)
            t = truns[0]['tile']

            def med(k, src=None):
                v = sorted(x['tile'][k] if src is None else x[src] for x in truns)
                return [round(float(np.median(v)), 3), round(float(v[0]), 3), round(float(v[-1]), 3)]

            res['chunks']['%d_s' % cs]['tile_store'] = {
                'probes_per_s': round(float(np.median(trate)), 1),
                'probes_per_s_min_max': [round(trate[0], 1), round(trate[-1], 1)],
                'adds': t['adds'], 'add_ms_sum_median_min_max': med('add_ms'),
                'add_ms_largest_median_min_max': med('add_ms_max'), 'flush_ms_median_min_max': med('flush_ms'),
                'flush_wall_ms_median_min_max': med('flush_wall_ms'),
                'match_ms_median_min_max': med(None, 'match_ms'), 'rows_held': t['rows_held'],
                'rows_kept': t['rows_kept'], 'files': t['files'], 'files_empty': t['files_empty']}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
