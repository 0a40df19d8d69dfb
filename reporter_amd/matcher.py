"""Host-side handle over libotr: configuration and the batched matching API.

Mirrors the reference's process model: `configure()` once per process
(valhalla.Configure, reporter_service.py:284), one `Matcher` per thread
(reporter_service.py:51-52).
"""
import ctypes
import json
import os
import tempfile

import numpy as np

from . import _lib

P = ctypes.POINTER

MODES = {'auto': 0, 'bicycle': 1, 'pedestrian': 2}


class NameRefusal(ValueError):
    """A chunk refused by the session store's uuid directory: point is the arrival index in the
    chunk, reason an _lib.OTR_NAME_E_* value, message the arrival index of the point's message
    after sessions_push_text (-1 otherwise)."""

    def __init__(self, text, point, reason, message=-1):
        super().__init__(text)
        self.point, self.reason, self.message = point, reason, message


OTR_KEYS = ('speed_kph', 'queue_kph', 'delta')  # engine keys, not meili's


def default_config(graph_path, device=0, **options):
    """Valhalla-style config dict of the reference deployment: valhalla_build_config's meili
    section (per-mode turn_penalty_factor auto 200 / bicycle 140 / pedestrian 100) with the
    Dockerfile's overrides (sigma_z 4.07, beta 3, max_route_distance_factor 5,
    max_route_time_factor 2; Dockerfile:14-17,42-49).  `options` apply to every mode, as a
    request's match_options override the configured values (generate_test_trace.py:44-52
    sends turn_penalty_factor 0, for example); speed_kph / queue_kph go to the otr section."""
    d = {'sigma_z': 4.07, 'beta': 3, 'max_route_distance_factor': 5, 'max_route_time_factor': 2,
         'breakage_distance': 2000, 'interpolation_distance': 10, 'search_radius': 50,
         'max_search_radius': 100, 'gps_accuracy': 5.0, 'turn_penalty_factor': 0, 'max_candidates': 32}
    modes = {'auto': {'turn_penalty_factor': 200, 'search_radius': 50},
             'bicycle': {'turn_penalty_factor': 140},
             'pedestrian': {'turn_penalty_factor': 100, 'search_radius': 50}}
    otr = {'graph': os.path.abspath(graph_path), 'device': device}
    for k, v in options.items():
        if k in OTR_KEYS:
            otr[k] = v
        else:
            d[k] = v
            for m in modes.values():
                m[k] = v
    return {'meili': dict(default=d, **modes), 'otr': otr}


def configure(config):
    """Configure from a path or a dict; raises RuntimeError on failure."""
    L = _lib.lib()
    if isinstance(config, dict):
        s = json.dumps(config).encode()
        rc = L.otr_configure_json(s, len(s))
    else:
        rc = L.otr_configure(os.fspath(config).encode())
    if rc != 0:
        raise RuntimeError('otr_configure failed (%d): %s' % (rc, _lib.last_error()))


def coalesce(max_traces, max_wait_us=2000):
    """Coalesce concurrent report_json calls of all threads into shared device batches
    (otr_coalesce); max_traces <= 0 stops it."""
    rc = _lib.lib().otr_coalesce(int(max_traces), int(max_wait_us))
    if rc != 0:
        raise RuntimeError('otr_coalesce failed (%d): %s' % (rc, _lib.last_error()))


def graph_info():
    a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    rc = _lib.lib().otr_graph_info(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    if rc != 0:
        raise RuntimeError('not configured')
    return a.value, b.value, c.value


def session_key(uuid_bytes):
    """otr_uuid_key: the session store's key of a uuid (K11's 64-bit hash of its bytes; a str
    is taken as UTF-8, as the changelog's String keys are)."""
    b = uuid_bytes.encode() if isinstance(uuid_bytes, str) else bytes(uuid_bytes)
    return int(_lib.lib().otr_uuid_key(b, len(b)))


def tile_slice_key(start, tile_id, slice_):
    """otr_tile_slice_key: the anonymise_tile changelog's String key of a slice record,
    "{start}_{tile_id}.{slice}" (bytes)."""
    buf = ctypes.create_string_buffer(64)
    n = _lib.lib().otr_tile_slice_key(int(start), int(tile_id), int(slice_), buf, 64)
    if n < 0:
        raise RuntimeError('otr_tile_slice_key failed')
    return buf.raw[:n]


def tile_slice_key_parse(text):
    """otr_tile_slice_key_parse: (start, tile_id, slice) of a changelog key exactly as
    Long.toString / Integer.toString print it; ValueError for anything else."""
    b = text.encode() if isinstance(text, str) else bytes(text)
    a, t, s = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
    if _lib.lib().otr_tile_slice_key_parse(b, len(b), ctypes.byref(a), ctypes.byref(t), ctypes.byref(s)) != 0:
        raise ValueError('not a tile slice key: %r' % b)
    return a.value, t.value, s.value


JAVA_TIME_PATTERN = 'yyyy-MM-dd HH:mm:ss'


def formatter_from_spec(spec):
    """The reference's --formatter strings (Formatter.GetFormatter, Formatter.java:36-51) as a
    format dict for Matcher.format_messages: the first character separates the arguments,
    'sv' takes separator, uuid, lat, lon, time and accuracy indices and an optional time
    pattern, 'json' the five keys in that order and an optional pattern.  The separator regex
    is accepted only as one literal byte, optionally backslash-escaped; the only pattern is
    'yyyy-MM-dd HH:mm:ss'.  Anything else raises ValueError naming it."""
    if not isinstance(spec, str) or len(spec) < 2:
        raise ValueError('formatter spec %r: too short' % (spec,))
    if spec[0] in '.$|()[]{}^?*+\\':
        raise ValueError('formatter spec %r: the argument separator %r is a regex, not a literal' % (spec, spec[0]))
    args = spec[1:].split(spec[0])
    while args and args[-1] == '':   # String.split drops trailing empty strings
        args.pop()

    def pattern(p):
        if p is None:
            return _lib.OTR_TIME_EPOCH
        if p != JAVA_TIME_PATTERN:
            raise ValueError('formatter spec %r: unsupported time pattern %r' % (spec, p))
        return _lib.OTR_TIME_YMDHMS

    if args and args[0] == 'sv':
        if len(args) < 7:
            raise ValueError('formatter spec %r: sv needs a separator and five indices' % (spec,))
        sep = args[1]
        if len(sep) == 2 and sep[0] == '\\' and not sep[1].isalnum():
            sep = sep[1]
        if len(sep) != 1 or ord(sep) > 255 or ord(sep) < 1 or (sep in '.$|()[{^?*+\\' and len(args[1]) == 1):
            raise ValueError('formatter spec %r: separator %r is not one literal byte' % (spec, args[1]))
        try:
            idx = [int(a) for a in args[2:7]]
        except ValueError:
            raise ValueError('formatter spec %r: an index is not an integer' % (spec,))
        if min(idx) < 0:
            raise ValueError('formatter spec %r: negative index' % (spec,))
        return {'type': 'sv', 'separator': sep, 'uuid_index': idx[0], 'lat_index': idx[1], 'lon_index': idx[2],
                'time_index': idx[3], 'accuracy_index': idx[4],
                'time_format': pattern(args[7] if len(args) > 7 else None)}
    if args and args[0] == 'json':
        if len(args) < 6:
            raise ValueError('formatter spec %r: json needs five keys' % (spec,))
        keys = args[1:6]
        for k in keys:
            b = k.encode()
            if not 1 <= len(b) <= 64 or b'"' in b or b'\\' in b:
                raise ValueError('formatter spec %r: key %r is not 1..64 bytes without quote or backslash'
                                 % (spec, k))
        return {'type': 'json', 'uuid_key': keys[0], 'lat_key': keys[1], 'lon_key': keys[2], 'time_key': keys[3],
                'accuracy_key': keys[4], 'time_format': pattern(args[6] if len(args) > 6 else None)}
    raise ValueError('formatter spec %r: unsupported raw format parser' % (spec,))


class IngestedBatch:
    """The traces otr_ingest left in HBM, in the shape match_batch takes."""

    def __init__(self, r):
        b = r.batch
        self.n_traces = int(r.n_traces)
        self.n_probes = int(r.n_probes)
        self.arrays = {'trace_offsets': b.trace_offsets, 'lat': b.lat, 'lon': b.lon, 'time': b.time,
                       'accuracy': b.accuracy, 'mode': b.mode}
        self.uuid_off = r.d_trace_uuid_off
        self.uuid_len = r.d_trace_uuid_len


class Matcher:
    def __init__(self):
        self._L = _lib.lib()
        self._h = self._L.otr_matcher_new()
        self._keep = []

    def close(self):
        if self._h:
            self._L.otr_matcher_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return self._L.otr_matcher_stream(self._h)

    # --- JSON drop-in entry points ------------------------------------------------
    def match_json(self, trace_json):
        """SegmentMatcher.Match(json) -> str (reporter_service.py:240)."""
        s = trace_json.encode() if isinstance(trace_json, str) else trace_json
        out, n = ctypes.c_void_p(), ctypes.c_size_t()
        rc = self._L.otr_match(self._h, s, len(s), ctypes.byref(out), ctypes.byref(n))
        body = _lib.take_string(out, n)
        if rc != 0:
            raise RuntimeError(json.loads(body).get('error', body) if body else _lib.last_error())
        return body

    def report_json(self, trace_json, threshold_sec=-1):
        """POST /report: returns (http_code, body) exactly as handle_request (209-245)."""
        s = trace_json.encode() if isinstance(trace_json, str) else trace_json
        out, n = ctypes.c_void_p(), ctypes.c_size_t()
        rc = self._L.otr_report(self._h, s, len(s), threshold_sec, ctypes.byref(out), ctypes.byref(n))
        return rc, _lib.take_string(out, n)

    def report_json_batch(self, bodies, threshold_sec=-1):
        """Many POST /report bodies in shared device batches (otr_report_batch):
        [(http_code, body)], item i exactly as report_json(bodies[i])."""
        enc = [b.encode() if isinstance(b, str) else bytes(b) for b in bodies]
        n = len(enc)
        arr = (ctypes.c_char_p * max(n, 1))(*enc)
        lens = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in enc])
        codes = (ctypes.c_int32 * max(n, 1))()
        outs = (ctypes.c_void_p * max(n, 1))()
        olens = (ctypes.c_size_t * max(n, 1))()
        rc = self._L.otr_report_batch(self._h, n, arr, lens, threshold_sec, codes, outs, olens)
        if rc != 0:
            raise RuntimeError('otr_report_batch failed (%d): %s' % (rc, _lib.last_error()))
        res = []
        for i in range(n):
            res.append((codes[i], _lib.take_string(ctypes.c_void_p(outs[i]), ctypes.c_size_t(olens[i]))))
        return res

    # --- batched API ----------------------------------------------------------------
    def match_batch(self, traces, report_levels=(0, 1), transition_levels=(0, 1), threshold_sec=15,
                    quantisation=3600, hist_base_time=0, hist_hours=0, copy_out=True, timing=False,
                    device_arrays=None, hist_device=None, tile_rows=False, tile_rules=0, host_arrays=None,
                    copy_reports=False, route_work=False, matched_points=False, edge_traversals=False):
        """Match a gen.Traces-like SoA batch.  With device_arrays (dict of device
        pointers: trace_offsets, lat, lon, time, accuracy, mode) the inputs are
        already resident in HBM; host_arrays: the same as host pointers (e.g. pinned
        buffers the caller keeps alive).  copy_reports: segments, reports and stats
        come back to the host (the JSON path's copy-out).  route_work: the LDS route
        tiers count their work (route_tier_work; instrumentation, ~7% of the first tier).
        matched_points: every probe's matched point is computed too (K12); read it with
        matched_points() / matched_points_result() before the next batch.  edge_traversals:
        when the vehicle entered and left each edge of the matched route is computed too (K13);
        read it with edge_traversals() / edge_traversals_result() / edge_observations()."""
        b = _lib.TraceBatch()
        b.n_traces = int(traces.n_traces)
        arrs = device_arrays if device_arrays is not None else host_arrays
        if arrs is not None:
            b.memory = _lib.OTR_MEM_DEVICE if device_arrays is not None else _lib.OTR_MEM_HOST
            b.trace_offsets = arrs['trace_offsets']
            b.lat = arrs['lat']
            b.lon = arrs['lon']
            b.time = arrs['time']
            b.accuracy = arrs.get('accuracy') or None
            b.mode = arrs['mode']
        else:
            b.memory = _lib.OTR_MEM_HOST
            keep = [np.ascontiguousarray(traces.offsets, np.int64), np.ascontiguousarray(traces.lat, np.float64),
                    np.ascontiguousarray(traces.lon, np.float64), np.ascontiguousarray(traces.time, np.int64),
                    np.ascontiguousarray(traces.mode, np.uint8)]
            acc = None if traces.accuracy is None else np.ascontiguousarray(traces.accuracy, np.float32)
            self._keep = keep + [acc]
            b.trace_offsets, b.lat, b.lon, b.time, b.mode = [k.ctypes.data for k in keep]
            b.accuracy = acc.ctypes.data if acc is not None else None
        b.report_levels = _lib.levels_mask(report_levels)
        b.transition_levels = _lib.levels_mask(transition_levels)
        b.threshold_sec = threshold_sec
        b.quantisation = quantisation
        b.hist_base_time = hist_base_time
        b.hist_hours = hist_hours
        b.hist_device = hist_device
        b.tile_rules = int(tile_rules)
        b.flags = (_lib.OTR_BATCH_COPY_OUT if copy_out else 0) | (_lib.OTR_BATCH_TIMING if timing else 0) | \
            (_lib.OTR_BATCH_TILE_ROWS if tile_rows else 0) | (_lib.OTR_BATCH_COPY_REPORTS if copy_reports else 0) | \
            (_lib.OTR_BATCH_ROUTE_WORK if route_work else 0) | \
            (_lib.OTR_BATCH_MATCHED_POINTS if matched_points else 0) | \
            (_lib.OTR_BATCH_EDGE_TRAVERSALS if edge_traversals else 0)
        r = _lib.BatchResult()
        rc = self._L.otr_match_batch(self._h, ctypes.byref(b), ctypes.byref(r))
        if rc != 0:
            raise RuntimeError('otr_match_batch failed (%d): %s' % (rc, _lib.last_error()))
        r._owner = self  # the host arrays belong to this matcher: keep it alive with the result
        return r

    def matched_points_result(self):
        """otr_matched_points: the PointResult of the last match_batch(..., matched_points=True)
        (host pointers with copy_out, device pointers d_* always; valid until the next batch).
        Raises RuntimeError when that batch did not ask for points."""
        r = _lib.PointResult()
        rc = self._L.otr_matched_points(self._h, ctypes.byref(r))
        if rc != 0:
            raise RuntimeError('otr_matched_points failed (%d): %s' % (rc, _lib.last_error()))
        r._owner = self
        return r

    def matched_points(self):
        """Every probe's matched point of the last match_batch(..., matched_points=True,
        copy_out=True): a dict of numpy arrays (host copies) kind, edge, frac, lat, lon, dist,
        state, pos_mm, one entry per probe in input order (include/otr.h otr_point_result)."""
        r = self.matched_points_result()
        if r.n_probes > 0 and not r.kind:
            raise RuntimeError('matched_points: the batch ran without copy_out (device arrays only: '
                               'matched_points_result())')
        return _lib.points_to_numpy(r)

    def edge_traversals_result(self):
        """otr_edge_traversals: the TraversalResult of the last match_batch(..., edge_traversals=True)
        (host pointers with copy_out, device pointers d_* always; valid until the next batch).
        Raises RuntimeError when that batch did not ask for traversals."""
        r = _lib.TraversalResult()
        rc = self._L.otr_edge_traversals(self._h, ctypes.byref(r))
        if rc != 0:
            raise RuntimeError('otr_edge_traversals failed (%d): %s' % (rc, _lib.last_error()))
        r._owner = self
        return r

    def edge_traversals(self):
        """The edge traversals of the last match_batch(..., edge_traversals=True, copy_out=True): a
        dict of numpy arrays (host copies) trace_off (n_traces + 1), edge, way, seg_id, first_state,
        f0, f1, s0_mm, s1_mm, t_enter, t_exit (include/otr.h otr_traversal_result)."""
        r = self.edge_traversals_result()
        if not r.trace_off:
            raise RuntimeError('edge_traversals: the batch ran without copy_out (device arrays only: '
                               'edge_traversals_result())')
        return _lib.traversals_to_numpy(r)

    def edge_observations(self, quantisation=3600):
        """otr_edge_observations: (device pointer, n) of the per-edge speed entries (otr_hist_entry,
        _lib.HIST_ENTRY) of the last batch's complete traversals, in traversal order; matcher-owned
        until the next batch or call.  Feed them to simple_reporter.hist_reduce(m, ptr, n, ...)."""
        ptr, n = ctypes.c_void_p(), ctypes.c_int64()
        rc = self._L.otr_edge_observations(self._h, int(quantisation), ctypes.byref(ptr), ctypes.byref(n))
        if rc != 0:
            raise RuntimeError('otr_edge_observations failed (%d): %s' % (rc, _lib.last_error()))
        return int(ptr.value or 0), int(n.value)

    def ingest(self, text, rules=0, separator='|', uuid_index=1, time_index=0, lat_index=9, lon_index=10,
               accuracy_index=5, time_format=None, inactivity=120, mode='auto', bbox=None, device_ptr=None,
               nbytes=None):
        """Probe text → windowed traces in HBM (include/otr.h otr_ingest).  text: bytes
        (host), or device_ptr + nbytes for text already in HBM.  Defaults: the raw-feed
        valuer and time pattern of simple_reporter.py:352-353.  Returns (IngestResult,
        batch) where batch is a device-array handle for match_batch(batch, device_arrays=
        batch.arrays).  Raises ValueError with the line number where the reference raises."""
        f = _lib.IngestFormat()
        f.rules = int(rules)
        f.separator = ord(separator) if isinstance(separator, str) else int(separator)
        f.uuid_index, f.time_index, f.lat_index, f.lon_index, f.accuracy_index = (
            uuid_index, time_index, lat_index, lon_index, accuracy_index)
        if time_format is None:
            time_format = _lib.OTR_TIME_EPOCH if rules == _lib.OTR_INGEST_SHARD else _lib.OTR_TIME_YMDHMS
        f.time_format = int(time_format)
        if not 0 <= int(inactivity) < 1 << 31:   # an int32 in the C-ABI: refused, never wrapped
            raise ValueError('inactivity out of range: %r' % (inactivity,))
        f.inactivity = int(inactivity)
        f.mode = {'auto': 0, 'bicycle': 1, 'pedestrian': 2}[mode] if isinstance(mode, str) else int(mode)
        if bbox is not None:
            f.use_bbox = 1
            for k in range(4):
                f.bbox[k] = float(bbox[k])
        r = _lib.IngestResult()
        if device_ptr is not None:
            rc = self._L.otr_ingest(self._h, ctypes.c_void_p(device_ptr), int(nbytes), _lib.OTR_MEM_DEVICE,
                                    ctypes.byref(f), ctypes.byref(r))
        else:
            self._keep = [text]
            rc = self._L.otr_ingest(self._h, ctypes.c_char_p(text), len(text), _lib.OTR_MEM_HOST, ctypes.byref(f),
                                    ctypes.byref(r))
        if rc != 0:
            if r.bad_line >= 0:
                raise ValueError('line %d: %s' % (r.bad_line, _lib.INGEST_REASONS.get(r.bad_reason, r.bad_reason)))
            raise RuntimeError('otr_ingest failed (%d): %s' % (rc, _lib.last_error()))
        return r, IngestedBatch(r)

    # --- session store (include/otr.h otr_sessions_*) ---------------
    def _check(self, rc, what, refused=ValueError):
        if rc == _lib.OTR_BAD_REQUEST:
            raise refused('%s refused: %s' % (what, _lib.last_error()))
        if rc != 0:
            raise RuntimeError('%s failed (%d): %s' % (what, rc, _lib.last_error()))

    def sessions_open(self, max_sessions, max_points, report_dist=500.0, report_count=10, report_time=60,
                      session_gap=60000, mode='auto', report_levels=(0, 1), transition_levels=(0, 1),
                      threshold_sec=15, batch_probes=0, uuid_bytes=0):
        """Open this matcher's session store (defaults: BatchingProcessor's gates).  uuid_bytes > 0:
        with the uuid directory (otr_sessions_open_named): every point and every restored session
        then comes with a name of at most that many bytes."""
        c = _lib.SessionConfig()
        c.max_sessions, c.max_points = int(max_sessions), int(max_points)
        c.report_dist, c.report_count, c.report_time = float(report_dist), int(report_count), int(report_time)
        c.session_gap = int(session_gap)
        c.mode = MODES[mode] if isinstance(mode, str) else int(mode)
        c.report_levels = _lib.levels_mask(report_levels)
        c.transition_levels = _lib.levels_mask(transition_levels)
        c.threshold_sec = int(threshold_sec)
        c.batch_probes = int(batch_probes)
        if uuid_bytes:
            self._check(self._L.otr_sessions_open_named(self._h, ctypes.byref(c), int(uuid_bytes)),
                        'otr_sessions_open_named')
        else:
            self._check(self._L.otr_sessions_open(self._h, ctypes.byref(c)), 'otr_sessions_open')
        self.session_uuid_bytes = int(uuid_bytes)   # 0: the open store has no uuid directory

    def sessions_close(self):
        self._check(self._L.otr_sessions_close(self._h), 'otr_sessions_close')

    def _session_points(self, points, device):
        """points: dict of key, lat, lon, accuracy, time, timestamp: numpy arrays, or device
        pointers plus 'n' with device=True."""
        p = _lib.SessionPoints()
        if device:
            p.n, p.memory = int(points['n']), _lib.OTR_MEM_DEVICE
            for k, _ in _lib.SESSION_POINT_FIELDS:
                setattr(p, k, points[k])
        else:
            keep = [np.ascontiguousarray(points[k], dt) for k, dt in _lib.SESSION_POINT_FIELDS]
            if len({len(a) for a in keep}) != 1:
                raise ValueError('session points: arrays of different lengths')
            self._keep = keep
            p.n, p.memory = len(keep[0]), _lib.OTR_MEM_HOST
            for (k, _), a in zip(_lib.SESSION_POINT_FIELDS, keep):
                setattr(p, k, a.ctypes.data)
        return p

    def _session_names(self, names, device):
        """names: a sequence of bytes objects (host), or a dict of 'bytes', 'off', 'len' (numpy
        arrays, or device pointers with device=True) and optionally 'n_bytes'."""
        s = _lib.SessionNames()
        if device:
            s.bytes, s.n_bytes = int(names['bytes']) or None, int(names['n_bytes'])
            s.off, s.len = int(names['off']) or None, int(names['len']) or None
            return s
        if isinstance(names, dict):
            data = np.ascontiguousarray(names['bytes'], np.uint8)
            off, ln = np.ascontiguousarray(names['off'], np.int64), np.ascontiguousarray(names['len'], np.int32)
            n_bytes = int(names.get('n_bytes', len(data)))
        else:
            data, off, ln = _lib.pack_names(names)
            n_bytes = len(data)
        self._keep_names = [data, off, ln]
        s.bytes, s.n_bytes = (data.ctypes.data if len(data) else None), n_bytes
        s.off, s.len = off.ctypes.data, ln.ctypes.data
        return s

    def sessions_last_refusal(self):
        """otr_sessions_last_refusal: {'point', 'message', 'reason'} of the last named call
        (reason 0: it was not refused for a name)."""
        r = _lib.SessionNameRefusal()
        self._check(self._L.otr_sessions_last_refusal(self._h, ctypes.byref(r)), 'otr_sessions_last_refusal')
        return {'point': int(r.point), 'message': int(r.message), 'reason': int(r.reason)}

    def _check_named(self, rc, what):
        """_check, a name refusal raising NameRefusal (a ValueError carrying point and reason)."""
        if rc == _lib.OTR_BAD_REQUEST:
            text = _lib.last_error()
            r = _lib.SessionNameRefusal()
            if self._L.otr_sessions_last_refusal(self._h, ctypes.byref(r)) == 0 and r.reason:
                raise NameRefusal('%s refused: point %d: name %s (%s)' % (
                    what, r.point, _lib.NAME_REASONS.get(r.reason, r.reason), text), int(r.point), int(r.reason),
                    int(r.message))
            raise ValueError('%s refused: %s' % (what, text))
        self._check(rc, what)

    def sessions_push(self, points, device=False, names=None):
        """otr_sessions_push: the chunk's windows and reports as a dict of numpy arrays
        (_lib.session_result_to_numpy).  A refused chunk raises ValueError.  names (a store with a
        uuid directory): one name per point (_session_names); a name refusal raises NameRefusal."""
        p, r = self._session_points(points, device), _lib.SessionResult()
        if names is not None:
            nm = self._session_names(names, device)
            self._check_named(self._L.otr_sessions_push_named(self._h, ctypes.byref(p), ctypes.byref(nm),
                                                              ctypes.byref(r)), 'otr_sessions_push_named')
        else:
            self._check(self._L.otr_sessions_push(self._h, ctypes.byref(p), ctypes.byref(r)), 'otr_sessions_push')
        return _lib.session_result_to_numpy(r)

    def sessions_names(self):
        """otr_sessions_names: the names of the sessions of the last sessions_snapshot,
        sessions_take or sessions_export_records, in its order, as a list of bytes."""
        r = _lib.SessionNameList()
        self._check(self._L.otr_sessions_names(self._h, ctypes.byref(r)), 'otr_sessions_names')
        return _lib.names_to_list(r)

    # --- stream formatter (include/otr.h otr_format_messages) ---------
    def _message_args(self, text, fmt, msg_off, timestamp, device_ptr, nbytes):
        """(otr_message_format, otr_messages) of a format dict (formatter_from_spec) and a chunk:
        text as bytes with numpy msg_off / timestamp, or device_ptr + nbytes with msg_off and
        timestamp as (device address, count) pairs; an int timestamp is every message's."""
        f = _lib.MessageFormat()
        f.type = {'sv': _lib.OTR_FORMAT_SV, 'json': _lib.OTR_FORMAT_JSON}[fmt['type']]
        f.time_format = int(fmt.get('time_format', _lib.OTR_TIME_EPOCH))
        keep = []
        if fmt['type'] == 'sv':
            sep = fmt['separator']
            f.separator = ord(sep) if isinstance(sep, (str, bytes)) else int(sep)
            for k in ('uuid_index', 'time_index', 'lat_index', 'lon_index', 'accuracy_index'):
                setattr(f, k, int(fmt[k]))
        else:
            for k in ('uuid_key', 'lat_key', 'lon_key', 'time_key', 'accuracy_key'):
                v = fmt[k]
                if v is not None:
                    v = v.encode() if isinstance(v, str) else bytes(v)
                    keep.append(v)
                setattr(f, k, v)
        m = _lib.Messages()
        if device_ptr is not None:
            m.text, m.len, m.memory = device_ptr or None, int(nbytes), _lib.OTR_MEM_DEVICE
            if msg_off is not None:
                m.msg_off, m.n_messages = int(msg_off[0]), int(msg_off[1])
            if isinstance(timestamp, (int, np.integer)):
                m.timestamp_all = int(timestamp)
            else:
                m.timestamp = int(timestamp[0])   # (address, count)
        else:
            keep.append(text)
            m.text = ctypes.cast(ctypes.c_char_p(text), ctypes.c_void_p)
            m.len, m.memory = len(text), _lib.OTR_MEM_HOST
            if msg_off is not None:
                off = np.ascontiguousarray(msg_off, np.int64)
                if len(off) < 1:
                    raise ValueError('msg_off needs n_messages + 1 offsets')
                keep.append(off)
                m.msg_off, m.n_messages = off.ctypes.data, len(off) - 1
            if isinstance(timestamp, (int, np.integer)):
                m.timestamp_all = int(timestamp)
            else:
                ts = np.ascontiguousarray(timestamp, np.int64)
                keep.append(ts)
                m.timestamp = ts.ctypes.data
                n = int(m.n_messages) if msg_off is not None else \
                    text.count(b'\n') + (1 if text and not text.endswith(b'\n') else 0)
                if len(ts) != n:
                    raise ValueError('timestamp: %d values for %d messages' % (len(ts), n))
        self._keep = keep
        return f, m

    def format_messages(self, text, fmt, msg_off=None, timestamp=0, device_ptr=None, nbytes=None, arrays=True):
        """otr_format_messages: raw messages → keyed points in HBM.  Returns the dict of
        _lib.format_result_to_numpy: host copies (none with arrays=False) plus 'device', the
        result struct whose arrays stay in HBM.  A refused chunk raises ValueError."""
        f, m = self._message_args(text, fmt, msg_off, timestamp, device_ptr, nbytes)
        r = _lib.FormatResult()
        self._check(self._L.otr_format_messages(self._h, ctypes.byref(f), ctypes.byref(m), ctypes.byref(r)),
                    'otr_format_messages')
        return _lib.format_result_to_numpy(r, arrays)

    def sessions_push_text(self, text, fmt, msg_off=None, timestamp=0, device_ptr=None, nbytes=None, arrays=True):
        """otr_sessions_push_text: the chunk's messages formatted and pushed into the session
        store without a point crossing to the host.  Returns (format dict, session dict); the
        format dict's host copies are made after the push (none with arrays=False)."""
        f, m = self._message_args(text, fmt, msg_off, timestamp, device_ptr, nbytes)
        r, s = _lib.FormatResult(), _lib.SessionResult()
        self._check_named(self._L.otr_sessions_push_text(self._h, ctypes.byref(f), ctypes.byref(m), ctypes.byref(r),
                                                         ctypes.byref(s)), 'otr_sessions_push_text')
        return _lib.format_result_to_numpy(r, arrays), _lib.session_result_to_numpy(s)

    def sessions_punctuate(self, ts):
        r = _lib.SessionResult()
        self._check(self._L.otr_sessions_punctuate(self._h, int(ts), ctypes.byref(r)), 'otr_sessions_punctuate')
        return _lib.session_result_to_numpy(r)

    def sessions_advance(self, points=None, device=False, names=None):
        """otr_sessions_advance: a new chunk (with names on a store with a uuid directory), or None
        to continue the current one.  Returns (TraceBatch in HBM, windows dict); n_traces == 0: the
        chunk is consumed."""
        b = _lib.TraceBatch()
        p = ctypes.byref(self._session_points(points, device)) if points is not None else None
        if names is not None:
            nm = self._session_names(names, device)
            self._check_named(self._L.otr_sessions_advance_named(self._h, p, ctypes.byref(nm), ctypes.byref(b)),
                              'otr_sessions_advance_named')
        else:
            self._check(self._L.otr_sessions_advance(self._h, p, ctypes.byref(b)), 'otr_sessions_advance')
        return b, self.sessions_windows()

    def sessions_commit(self, shape_used, status=None):
        su = np.ascontiguousarray(shape_used, np.int32)
        st = np.zeros(len(su), np.int32) if status is None else np.ascontiguousarray(status, np.int32)
        self._check(self._L.otr_sessions_commit(self._h, su.ctypes.data, st.ctypes.data, _lib.OTR_MEM_HOST),
                    'otr_sessions_commit')
        return self.sessions_windows()

    def sessions_windows(self):
        r = _lib.SessionResult()
        self._check(self._L.otr_sessions_windows(self._h, ctypes.byref(r)), 'otr_sessions_windows')
        return _lib.session_result_to_numpy(r)

    def sessions_snapshot(self):
        """Every live session in key order: key, point_off, max_sep, last_update, lat, lon,
        accuracy, time (numpy copies)."""
        r = _lib.SessionSnapshot()
        self._check(self._L.otr_sessions_snapshot(self._h, ctypes.byref(r)), 'otr_sessions_snapshot')
        return _lib.snapshot_to_numpy(r)

    # --- restore, export and move (include/otr.h otr_sessions_restore ...) --
    def _restore_check(self, rc, r, what):
        if rc == _lib.OTR_BAD_REQUEST and r.bad_reason:
            where = 'session %d: ' % r.bad_session if r.bad_session >= 0 else ''
            raise ValueError('%s refused: %s%s (%s)' % (what, where, _lib.RESTORE_NAMED_REASONS.get(r.bad_reason, r.bad_reason),
                                                       _lib.last_error()))
        self._check(rc, what)
        return {k: getattr(r, k) for k in ('n_sessions', 'n_points', 'n_live', 'device_ms')}

    def sessions_restore(self, snapshot, device=False, names=None):
        """otr_sessions_restore: the sessions of a snapshot dict (sessions_snapshot's layout)
        merged into the open store, all or nothing.  device=True: the dict holds device
        pointers plus 'n_sessions' and 'n_points'.  A refusal raises ValueError carrying the
        lowest refused index and the reason (_lib.RESTORE_REASONS)."""
        s, r = _lib.SessionSnapshot(), _lib.SessionRestoreResult()
        if device:
            s.n_sessions, s.n_points = int(snapshot['n_sessions']), int(snapshot['n_points'])
            for k, ct, _ in _lib.SNAPSHOT_FIELDS:
                setattr(s, k, ctypes.cast(ctypes.c_void_p(int(snapshot[k]) or None), P(ct)))
        else:
            keep = [np.ascontiguousarray(snapshot[k], dt) for k, _, dt in _lib.SNAPSHOT_FIELDS]
            per_session = {k: a for (k, _, _), a in zip(_lib.SNAPSHOT_FIELDS, keep)}
            ns, npt = len(per_session['key']), len(per_session['time'])
            if len(per_session['point_off']) != ns + 1 or any(len(per_session[k]) != ns for k in ('max_sep', 'last_update')) \
                    or any(len(per_session[k]) != npt for k in ('lat', 'lon', 'accuracy')):
                raise ValueError('session snapshot: arrays of different lengths')
            self._keep = keep
            s.n_sessions, s.n_points = ns, npt
            for (k, ct, _), a in zip(_lib.SNAPSHOT_FIELDS, keep):
                setattr(s, k, ctypes.cast(ctypes.c_void_p(a.ctypes.data), P(ct)))
        mem = _lib.OTR_MEM_DEVICE if device else _lib.OTR_MEM_HOST
        if names is not None:   # one name per session (a store with a uuid directory)
            nm = self._session_names(names, device)
            rc = self._L.otr_sessions_restore_named(self._h, ctypes.byref(s), ctypes.byref(nm), mem, ctypes.byref(r))
            return self._restore_check(rc, r, 'otr_sessions_restore_named')
        rc = self._L.otr_sessions_restore(self._h, ctypes.byref(s), mem, ctypes.byref(r))
        return self._restore_check(rc, r, 'otr_sessions_restore')

    def sessions_restore_records(self, key, rec_off, data, device=False, n_records=None, n_bytes=None, names=None):
        """otr_sessions_restore_records: sessions as Batch.Serder's value bytes.  key: uint64 per
        record (session_key of the changelog key), rec_off: n + 1 byte offsets, data: the bytes
        (bytes or uint8 array).  device=True: the three are device addresses, with n_records and
        n_bytes; the bytes may start at any address."""
        c, r = _lib.SessionRecords(), _lib.SessionRestoreResult()
        if device:
            c.n_records, c.n_bytes, c.memory = int(n_records), int(n_bytes), _lib.OTR_MEM_DEVICE
            c.key, c.rec_off, c.bytes = int(key) or None, int(rec_off) or None, int(data) or None
        else:
            k = np.ascontiguousarray(key, np.uint64)
            o = np.ascontiguousarray(rec_off, np.int64)
            d = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
            if len(o) != len(k) + 1:
                raise ValueError('session records: rec_off needs n_records + 1 offsets')
            self._keep = [k, o, d]
            c.n_records, c.n_bytes, c.memory = len(k), len(d), _lib.OTR_MEM_HOST
            c.key, c.rec_off, c.bytes = k.ctypes.data, o.ctypes.data, (d.ctypes.data if len(d) else None)
        if names is not None:   # one name per record: its changelog key
            nm = self._session_names(names, device)
            rc = self._L.otr_sessions_restore_records_named(self._h, ctypes.byref(c), ctypes.byref(nm), ctypes.byref(r))
            return self._restore_check(rc, r, 'otr_sessions_restore_records_named')
        rc = self._L.otr_sessions_restore_records(self._h, ctypes.byref(c), ctypes.byref(r))
        return self._restore_check(rc, r, 'otr_sessions_restore_records')

    def sessions_export_records(self):
        """otr_sessions_export_records: every live session in ascending key order as records:
        numpy copies of key, rec_off and bytes, and 'device' with the same arrays in HBM."""
        r = _lib.SessionRecords()
        self._check(self._L.otr_sessions_export_records(self._h, ctypes.byref(r)), 'otr_sessions_export_records')
        return _lib.records_to_numpy(r)

    def sessions_take(self, n_parts, part, remove=True):
        """otr_sessions_take: the sessions with key % n_parts == part as a snapshot dict;
        remove=True also deletes them from the store (no report is made)."""
        r = _lib.SessionSnapshot()
        self._check(self._L.otr_sessions_take(self._h, int(n_parts), int(part), 1 if remove else 0, ctypes.byref(r)),
                    'otr_sessions_take')
        return _lib.snapshot_to_numpy(r)

    # --- tile store (include/otr.h otr_tile_store_*) -----------------
    def tile_store_open(self, max_rows, quantisation=3600, privacy=1, times=False):
        """Open this matcher's tile store: the streaming path's anonymiser stage in HBM.
        times=True (otr_tile_store_open_ex with OTR_TILE_STORE_TIMES): the store keeps every
        report's t0 and t1 beside its rows, which tile_store_export_records needs."""
        c = _lib.TileStoreConfig()
        c.max_rows, c.quantisation, c.privacy = int(max_rows), int(quantisation), int(privacy)
        if times:
            self._check(self._L.otr_tile_store_open_ex(self._h, ctypes.byref(c), _lib.OTR_TILE_STORE_TIMES),
                        'otr_tile_store_open_ex')
        else:
            self._check(self._L.otr_tile_store_open(self._h, ctypes.byref(c)), 'otr_tile_store_open')
        self._tile_quantisation = int(quantisation)
        self._tile_times = bool(times)

    # --- tile store: snapshot, restore, records (include/otr.h) --------
    def _tile_restore_check(self, rc, r, what):
        if rc == _lib.OTR_BAD_REQUEST and r.bad_reason:
            where = 'slice %d: ' % r.bad_slice if r.bad_slice >= 0 else \
                'map entry %d: ' % r.bad_tile if r.bad_tile >= 0 else ''
            e = ValueError('%s refused: %s%s (%s)' % (what, where, _lib.TILE_RESTORE_REASONS.get(r.bad_reason, r.bad_reason),
                                                     _lib.last_error()))
            e.result = _lib.tile_restore_to_dict(r)
            raise e
        self._check(rc, what)
        return _lib.tile_restore_to_dict(r)

    def tile_store_snapshot(self, host=True):
        """otr_tile_store_snapshot: the held rows in arrival order (rows, and t0 / t1 or None),
        n_rows, quantisation, flags and the device pointers d_rows, d_t0, d_t1 (matcher-owned
        until its next tile-store call); host=False: device pointers only.  The store is untouched."""
        r = _lib.TileSnapshot()
        self._check(self._L.otr_tile_store_snapshot(self._h, 0 if host else _lib.OTR_TILE_SNAPSHOT_NO_HOST,
                                                    ctypes.byref(r)), 'otr_tile_store_snapshot')
        return _lib.tile_snapshot_to_numpy(r, host)

    def tile_store_restore(self, snapshot, device=False):
        """otr_tile_store_restore: the rows of a snapshot dict appended to the held rows, all or
        nothing.  device=True: the dict's d_rows, d_t0, d_t1 and n_rows are used.  A refusal
        raises ValueError (its .result holds bad_slice and bad_reason)."""
        s, r = _lib.TileSnapshot(), _lib.TileRestoreResult()
        if device:
            s.n_rows = int(snapshot['n_rows'])
            s.rows, s.t0, s.t1 = (int(snapshot.get('d_' + k) or 0) or None for k in ('rows', 't0', 't1'))
        else:
            rows = np.ascontiguousarray(snapshot['rows'], dtype=_lib.TILE_ROW)
            keep = [rows]
            s.n_rows, s.rows = len(rows), (rows.ctypes.data if len(rows) else None)
            if snapshot.get('t0') is not None:
                a, b = (np.ascontiguousarray(snapshot[k], np.float64) for k in ('t0', 't1'))
                if len(a) != len(rows) or len(b) != len(rows):
                    raise ValueError('tile snapshot: arrays of different lengths')
                keep += [a, b]
                s.t0, s.t1 = (a.ctypes.data, b.ctypes.data) if len(rows) else (None, None)
            self._keep = keep
        rc = self._L.otr_tile_store_restore(self._h, ctypes.byref(s), _lib.OTR_MEM_DEVICE if device else _lib.OTR_MEM_HOST,
                                            ctypes.byref(r))
        return self._tile_restore_check(rc, r, 'otr_tile_store_restore')

    def tile_store_export_records(self, slice_size=20000):
        """otr_tile_store_export_records (a store opened with times=True): the held rows as the
        reference's slice records and map entries, _lib.tile_records_to_numpy's dict plus the
        store's 'quantisation'.  The store is untouched."""
        r = _lib.TileRecords()
        self._check(self._L.otr_tile_store_export_records(self._h, int(slice_size), ctypes.byref(r)),
                    'otr_tile_store_export_records')
        out = _lib.tile_records_to_numpy(r)
        out['quantisation'] = self._tile_quantisation
        return out

    def tile_store_restore_records(self, records, device=False, use_map=True):
        """otr_tile_store_restore_records.  records: dict of start, tile_id, slice, rec_off, bytes,
        slice_size and, with use_map, map_bytes (missing or None: no map); device=True: the
        dict's d_* device addresses with n_slices, n_bytes and n_tiles.  The bytes may start at
        any address.  Returns the restore's counts; a refusal raises ValueError (.result)."""
        c, r = _lib.TileRecords(), _lib.TileRestoreResult()
        c.slice_size = int(records['slice_size'])
        has_map = use_map and records.get('d_map_bytes' if device else 'map_bytes') is not None
        if device:
            c.n_slices, c.n_bytes, c.memory = int(records['n_slices']), int(records['n_bytes']), _lib.OTR_MEM_DEVICE
            for k in ('start', 'tile_id', 'slice', 'rec_off', 'bytes'):
                setattr(c, k, int(records['d_' + k]) or None)
            c.n_tiles = int(records['n_tiles']) if has_map else -1
            c.map_bytes = (int(records['d_map_bytes']) or None) if has_map else None
        else:
            st = np.ascontiguousarray(records['start'], np.int64)
            ti = np.ascontiguousarray(records['tile_id'], np.int64)
            sl = np.ascontiguousarray(records['slice'], np.int32)
            of = np.ascontiguousarray(records['rec_off'], np.int64)
            data = records['bytes']
            d = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
            if len(of) != len(st) + 1 or len(ti) != len(st) or len(sl) != len(st):
                raise ValueError('tile records: arrays of different lengths')
            keep = [st, ti, sl, of, d]
            c.n_slices, c.n_bytes, c.memory = len(st), len(d), _lib.OTR_MEM_HOST
            c.start, c.tile_id, c.slice = (a.ctypes.data if len(st) else None for a in (st, ti, sl))
            c.rec_off, c.bytes = of.ctypes.data, (d.ctypes.data if len(d) else None)
            c.n_tiles = -1
            if has_map:
                mb = records['map_bytes']
                mp = np.frombuffer(mb, np.uint8) if isinstance(mb, (bytes, bytearray)) else np.ascontiguousarray(mb, np.uint8)
                if len(mp) % 20:
                    raise ValueError('tile records: map_bytes is not a multiple of 20 bytes')
                keep.append(mp)
                c.n_tiles, c.map_bytes = len(mp) // 20, (mp.ctypes.data if len(mp) else None)
            self._keep = keep
        rc = self._L.otr_tile_store_restore_records(self._h, ctypes.byref(c), ctypes.byref(r))
        return self._tile_restore_check(rc, r, 'otr_tile_store_restore_records')

    def tile_store_close(self):
        self._check(self._L.otr_tile_store_close(self._h), 'otr_tile_store_close')

    def tile_store_add_session(self):
        """otr_tile_store_add_session: the reports of the last sessions_push / sessions_punctuate
        into the store, in forward order.  Returns the add's counts (dict); an add past
        max_rows raises ValueError and leaves the store as it was."""
        r = _lib.TileAddResult()
        self._check(self._L.otr_tile_store_add_session(self._h, ctypes.byref(r)), 'otr_tile_store_add_session')
        return _lib.tile_add_to_dict(r)

    def tile_store_add_reports(self, reports, device=False):
        """otr_tile_store_add_reports.  reports: dict of rep_off (n_windows + 1), id, next_id, t0,
        t1, length, queue_length: numpy arrays (a sessions_push result dict as it is), or
        device pointers plus 'n_windows' with device=True."""
        r = _lib.TileAddResult()
        names = ['rep_off'] + [k for k, _, _ in _lib.SESSION_REPORT_FIELDS]
        if device:
            nw, mem = int(reports['n_windows']), _lib.OTR_MEM_DEVICE
            ptrs = [reports[k] or None for k in names]
        else:
            types = [np.int64] + [dt for _, _, dt in _lib.SESSION_REPORT_FIELDS]
            keep = [np.ascontiguousarray(reports[k], dt) for k, dt in zip(names, types)]
            if len({len(a) for a in keep[1:]}) != 1 or len(keep[0]) < 1:
                raise ValueError('tile store reports: arrays of different lengths')
            self._keep = keep
            nw, mem = len(keep[0]) - 1, _lib.OTR_MEM_HOST
            ptrs = [a.ctypes.data for a in keep]
        self._check(self._L.otr_tile_store_add_reports(self._h, nw, *ptrs, mem, ctypes.byref(r)),
                    'otr_tile_store_add_reports')
        return _lib.tile_add_to_dict(r)

    def tile_store_add_rows(self, rows=None, device_ptr=None, n=None):
        """otr_tile_store_add_rows: finished rows (numpy _lib.TILE_ROW, or device_ptr and n)."""
        r = _lib.TileAddResult()
        if device_ptr is not None:
            rc = self._L.otr_tile_store_add_rows(self._h, device_ptr or None, int(n), _lib.OTR_MEM_DEVICE,
                                                 ctypes.byref(r))
        else:
            rows = np.ascontiguousarray(rows, dtype=_lib.TILE_ROW)
            self._keep = [rows]
            rc = self._L.otr_tile_store_add_rows(self._h, rows.ctypes.data if len(rows) else None, len(rows),
                                                 _lib.OTR_MEM_HOST, ctypes.byref(r))
        self._check(rc, 'otr_tile_store_add_rows')
        return _lib.tile_add_to_dict(r)

    def tile_store_flush(self):
        """otr_tile_store_flush: everything added since the last flush as cleaned files: numpy
        copies of rows, file, row_off, n_unclean, the counts, the store's quantisation and the
        device pointers d_* (matcher-owned until its next tile-store or cull call)."""
        r = _lib.TileFlushResult()
        self._check(self._L.otr_tile_store_flush(self._h, ctypes.byref(r)), 'otr_tile_store_flush')
        out = _lib.tile_flush_to_numpy(r)
        out['quantisation'] = self._tile_quantisation
        return out

    # --- tile file texts (include/otr.h otr_tiles_text) ----------------
    @staticmethod
    def _tag_bytes(x):
        return x if isinstance(x, (bytes, bytearray)) else str(x).encode()

    def tiles_text(self, rows=None, quantisation=3600, rules=0, source='smpl_rprt', mode='auto', device_ptr=None,
                   n=None, host=True):
        """otr_tiles_text: the file texts and names of rows grouped by file (numpy _lib.TILE_ROW,
        or device_ptr and n), written on the device.  Returns _lib.tile_text_to_numpy's dict:
        text and names (uint8), text_off, name_off, file, row_off, the counts and the device
        pointers d_* (matcher-owned until its next tile call); host=False: device pointers only."""
        r = _lib.TileTextResult()
        flags = 0 if host else _lib.OTR_TILE_TEXT_NO_HOST
        args = (int(quantisation), int(rules), self._tag_bytes(source), self._tag_bytes(mode), flags, ctypes.byref(r))
        if device_ptr is not None:
            rc = self._L.otr_tiles_text(self._h, device_ptr or None, int(n), _lib.OTR_MEM_DEVICE, *args)
        else:
            rows = np.ascontiguousarray(rows, dtype=_lib.TILE_ROW)
            self._keep = [rows]
            rc = self._L.otr_tiles_text(self._h, rows.ctypes.data if len(rows) else None, len(rows),
                                        _lib.OTR_MEM_HOST, *args)
        self._check(rc, 'otr_tiles_text')
        return _lib.tile_text_to_numpy(r, host)

    def tile_store_flush_text(self, source='reporter', mode='auto', host=True):
        """otr_tile_store_flush_text: the flush with the files' texts written on the device.
        Returns tile_store_flush's dict without 'rows' (they stay in HBM, d_rows), plus text,
        text_off, names, name_off, n_text_bytes, n_name_bytes, text_ms and the device pointers
        d_text, d_text_off, d_names, d_name_off; host=False: no text or names on the host."""
        fl, r = _lib.TileFlushResult(), _lib.TileTextResult()
        self._check(self._L.otr_tile_store_flush_text(self._h, self._tag_bytes(source), self._tag_bytes(mode),
                                                      0 if host else _lib.OTR_TILE_TEXT_NO_HOST, ctypes.byref(fl),
                                                      ctypes.byref(r)), 'otr_tile_store_flush_text')
        out = _lib.tile_flush_to_numpy(fl)
        del out['rows']
        out['quantisation'] = self._tile_quantisation
        text = _lib.tile_text_to_numpy(r, host)
        out['text_ms'] = text['device_ms']
        for k in ('text', 'text_off', 'names', 'name_off', 'n_text_bytes', 'n_name_bytes', 'd_text', 'd_text_off',
                  'd_names', 'd_name_off'):
            if k in text:
                out[k] = text[k]
        return out

    # --- tile file texts read back (include/otr.h otr_tiles_parse) -----
    def tiles_parse(self, text=None, text_off=None, names=None, name_off=None, device=False, n_files=None,
                    quantisation=3600, rules=0, source='smpl_rprt', mode='auto', host=True):
        """otr_tiles_parse: the texts of many tile files (text and names: bytes or numpy uint8,
        text_off and name_off: int64 of n_files + 1, the shape tiles_text returns; or with
        device=True four device pointers and n_files) to rows in HBM grouped by file.  Returns
        _lib.tile_parse_to_numpy's dict: the counts, first_bad*, the device pointers d_* (owned by
        the matcher until its next tiles_parse) and, with host=True, numpy copies of rows, row_off,
        file, file_status, file_line_off and line_status.  Lines and names that are not rows are
        reported there, not raised; ValueError only for arguments the call refuses as a whole."""
        c, r = _lib.TileTexts(), _lib.TileParseResult()
        if device:
            c.n_files, c.memory = int(n_files), _lib.OTR_MEM_DEVICE
            c.text, c.text_off, c.names, c.name_off = (int(x) or None for x in (text, text_off, names, name_off))
        else:
            def u8(x):
                return np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, np.uint8)
            t, nm = u8(text if text is not None else b''), u8(names if names is not None else b'')
            to = np.ascontiguousarray(text_off if text_off is not None else [0], np.int64)
            no = np.ascontiguousarray(name_off if name_off is not None else [0], np.int64)
            if len(to) != len(no) or len(to) < 1:
                raise ValueError('tiles_parse: text_off and name_off hold n_files + 1 offsets each')
            if int(to[-1]) > len(t) or int(no[-1]) > len(nm):
                raise ValueError('tiles_parse: the offsets run past the text or the names')
            self._keep = [t, nm, to, no]
            c.n_files, c.memory = len(to) - 1, _lib.OTR_MEM_HOST
            c.text, c.names = (t.ctypes.data if len(t) else None), (nm.ctypes.data if len(nm) else None)
            c.text_off, c.name_off = to.ctypes.data, no.ctypes.data
        rc = self._L.otr_tiles_parse(self._h, ctypes.byref(c), int(quantisation), int(rules), self._tag_bytes(source),
                                     self._tag_bytes(mode), 0 if host else _lib.OTR_TILE_PARSE_NO_HOST,
                                     ctypes.byref(r))
        self._check(rc, 'otr_tiles_parse')
        return _lib.tile_parse_to_numpy(r, host)

    def match_batch_numpy(self, traces, **kw):
        r = self.match_batch(traces, copy_out=True, **kw)
        return _lib.result_to_numpy(r)
