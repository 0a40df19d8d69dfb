"""ctypes binding of libotr.so (include/otr.h).  No fallback: if the HIP library is
missing or cannot load, every entry point raises — the product never silently runs
anything else."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('OTR_LIB') or os.path.join(_HERE, 'libotr.so')
P = ctypes.POINTER

OTR_OK = 0
OTR_MEM_HOST = 0
OTR_MEM_DEVICE = 1
OTR_BATCH_COPY_OUT = 1
OTR_BATCH_TIMING = 2
OTR_BATCH_COPY_REPORTS = 4
OTR_BATCH_TILE_ROWS = 8
OTR_BATCH_ROUTE_WORK = 16
OTR_BATCH_MATCHED_POINTS = 32
OTR_BATCH_EDGE_TRAVERSALS = 64
OTR_BAD_REQUEST = 400
POINT_UNMATCHED, POINT_STATE, POINT_INTERPOLATED = 0, 1, 2
OTR_TILE_RULES_SIMPLE = 0
OTR_TILE_RULES_STREAM = 1
OTR_TILE_TEXT_NO_HOST = 1
OTR_TILE_STORE_TIMES = 1
OTR_TILE_SNAPSHOT_NO_HOST = 1
OTR_TILE_RESTORE_E_LAYOUT, OTR_TILE_RESTORE_E_KEY, OTR_TILE_RESTORE_E_COUNT, OTR_TILE_RESTORE_E_SEGMENT = 1, 2, 3, 4
OTR_TILE_RESTORE_E_DUPLICATE, OTR_TILE_RESTORE_E_MAP, OTR_TILE_RESTORE_E_FULL, OTR_TILE_RESTORE_E_ROW = 5, 6, 7, 8
TILE_RESTORE_REASONS = {1: 'layout', 2: 'key', 3: 'count', 4: 'segment', 5: 'duplicate', 6: 'map', 7: 'full',
                        8: 'row'}
OTR_INGEST_SHARD = 0
OTR_INGEST_RAW = 1
OTR_INGEST_JAVA_SV = 2
OTR_TIME_EPOCH = 0
OTR_TIME_YMDHMS = 1
INGEST_REASONS = {1: 'fields', 2: 'float', 3: 'int', 4: 'time', 5: 'uuid', 6: 'precision', 7: 'collision',
                  8: 'accuracy'}
OTR_FORMAT_SV = 0
OTR_FORMAT_JSON = 1
OTR_FORMAT_UNSUPPORTED = 32   # reasons below are drops (the reference throws), from here on unsupported
FORMAT_REASONS = {1: 'fields', 2: 'float', 3: 'int', 4: 'time', 5: 'accuracy', 6: 'json', 7: 'root', 8: 'missing',
                  32: 'precision', 33: 'accuracy range', 34: 'depth', 35: 'trailing', 36: 'escape', 37: 'number',
                  38: 'kind', 39: 'no id'}
OTR_NO_ID = 0xFFFFFFFFFFFFFFFF
OTR_RESTORE_E_LAYOUT, OTR_RESTORE_E_KEY, OTR_RESTORE_E_COUNT = 1, 2, 3
OTR_RESTORE_E_DUPLICATE, OTR_RESTORE_E_LIVE, OTR_RESTORE_E_FULL = 4, 5, 6
OTR_RESTORE_E_NAME = 7
RESTORE_REASONS = {1: 'layout', 2: 'key', 3: 'count', 4: 'duplicate', 5: 'live', 6: 'full'}
RESTORE_NAMED_REASONS = {**RESTORE_REASONS, 7: 'name'}   # the _named restores have one more
OTR_NAME_E_LONG, OTR_NAME_E_COLLISION, OTR_NAME_E_LAYOUT = 1, 2, 3
NAME_REASONS = {1: 'long', 2: 'collision', 3: 'layout'}
HIST_BINS = 8
KMAX = 64
STAGES = ['states', 'candidates', 'link', 'route', 'route_big', 'viterbi', 'paths', 'paths_big', 'segments',
          'histogram']
VITERBI_VARIANT = 15  # kernel_ms slot of the k_viterbi instance code (otr.h OTR_VITERBI_VARIANT)

# every symbol include/otr.h declares
EXPORTS = ['otr_configure', 'otr_configure_json', 'otr_matcher_new', 'otr_matcher_free', 'otr_match',
           'otr_report', 'otr_report_segments', 'otr_free', 'otr_last_error', 'otr_match_batch',
           'otr_graph_info', 'otr_matcher_stream', 'otr_device', 'otr_report_batch', 'otr_coalesce',
           'otr_tiles_cull', 'otr_tiles_format', 'otr_ingest', 'otr_report_lists_device', 'otr_hist_reduce',
           'otr_tilehier_row', 'otr_tilehier_col', 'otr_tilehier_file', 'otr_tilehier_files', 'otr_flatten',
           'otr_max_batch_probes', 'otr_launch_max_items', 'otr_service_stats', 'otr_matched_points',
           'otr_edge_traversals', 'otr_edge_observations', 'otr_sessions_open', 'otr_sessions_close',
           'otr_sessions_push', 'otr_sessions_punctuate', 'otr_sessions_advance', 'otr_sessions_commit',
           'otr_sessions_windows', 'otr_sessions_snapshot', 'otr_tile_store_open', 'otr_tile_store_close',
           'otr_tile_store_add_session', 'otr_tile_store_add_reports', 'otr_tile_store_add_rows',
           'otr_tile_store_flush', 'otr_format_messages', 'otr_sessions_push_text', 'otr_sessions_restore',
           'otr_sessions_restore_records', 'otr_sessions_export_records', 'otr_sessions_take', 'otr_uuid_key',
           'otr_sessions_open_named', 'otr_sessions_push_named', 'otr_sessions_advance_named',
           'otr_sessions_last_refusal', 'otr_sessions_names', 'otr_sessions_restore_named',
           'otr_sessions_restore_records_named', 'otr_tiles_text', 'otr_tile_store_flush_text',
           'otr_tile_store_open_ex', 'otr_tile_store_snapshot', 'otr_tile_store_restore',
           'otr_tile_store_export_records', 'otr_tile_store_restore_records', 'otr_tile_slice_key',
           'otr_tile_slice_key_parse', 'otr_tiles_parse']


class ServiceSplit(ctypes.Structure):
    """otr_service_split (include/otr.h): the JSON request path's host split."""
    _fields_ = [('calls', ctypes.c_int64), ('items', ctypes.c_int64), ('device_batches', ctypes.c_int64),
                ('scan_s', ctypes.c_double), ('soa_s', ctypes.c_double), ('device_s', ctypes.c_double),
                ('format_s', ctypes.c_double), ('total_s', ctypes.c_double)]


class FlatGraph(ctypes.Structure):
    """otr_flat_graph (include/otr.h): decoded road-graph arrays for otr_flatten."""
    _fields_ = [('n_nodes', ctypes.c_uint32), ('node_ll', ctypes.c_void_p), ('n_edges', ctypes.c_uint32),
                ('edge_src', ctypes.c_void_p), ('edge_dst', ctypes.c_void_p), ('edge_attr', ctypes.c_void_p),
                ('edge_seg', ctypes.c_void_p), ('edge_way', ctypes.c_void_p), ('shape_off', ctypes.c_void_p),
                ('shape_ll', ctypes.c_void_p), ('n_segments', ctypes.c_uint32), ('seg_id', ctypes.c_void_p),
                ('seg_len', ctypes.c_void_p), ('cell_deg', ctypes.c_double)]


class FlatStats(ctypes.Structure):
    _fields_ = [('n_nodes', ctypes.c_uint32), ('n_edges', ctypes.c_uint32), ('n_contracted_edges', ctypes.c_uint32),
                ('n_merged_nodes', ctypes.c_uint32)]


class TraceBatch(ctypes.Structure):
    _fields_ = [('n_traces', ctypes.c_int32), ('memory', ctypes.c_int32),
                ('trace_offsets', ctypes.c_void_p), ('lat', ctypes.c_void_p), ('lon', ctypes.c_void_p),
                ('time', ctypes.c_void_p), ('accuracy', ctypes.c_void_p), ('mode', ctypes.c_void_p),
                ('report_levels', ctypes.c_uint32), ('transition_levels', ctypes.c_uint32),
                ('threshold_sec', ctypes.c_int32), ('quantisation', ctypes.c_int32),
                ('hist_base_time', ctypes.c_int64), ('hist_hours', ctypes.c_int32), ('flags', ctypes.c_int32),
                ('hist_device', ctypes.c_void_p), ('tile_rules', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class IngestFormat(ctypes.Structure):
    _fields_ = [('rules', ctypes.c_int32), ('separator', ctypes.c_int32), ('uuid_index', ctypes.c_int32),
                ('time_index', ctypes.c_int32), ('lat_index', ctypes.c_int32), ('lon_index', ctypes.c_int32),
                ('accuracy_index', ctypes.c_int32), ('time_format', ctypes.c_int32), ('inactivity', ctypes.c_int32),
                ('mode', ctypes.c_int32), ('use_bbox', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('bbox', ctypes.c_double * 4)]


class IngestResult(ctypes.Structure):
    _fields_ = [('n_lines', ctypes.c_int64), ('n_kept', ctypes.c_int64), ('n_probes', ctypes.c_int64),
                ('n_traces', ctypes.c_int32), ('n_uuids', ctypes.c_int32), ('bad_line', ctypes.c_int64),
                ('bad_reason', ctypes.c_int32), ('parse_ms', ctypes.c_float), ('total_ms', ctypes.c_float),
                ('reserved', ctypes.c_int32), ('batch', TraceBatch),
                ('d_trace_uuid_off', ctypes.c_void_p), ('d_trace_uuid_len', ctypes.c_void_p)]


class BatchResult(ctypes.Structure):
    _fields_ = [('n_traces', ctypes.c_int32), ('n_probes', ctypes.c_int64), ('n_states', ctypes.c_int64),
                ('n_route', ctypes.c_int64), ('n_seg', ctypes.c_int64), ('n_rep', ctypes.c_int64),
                ('n_rows', ctypes.c_int64), ('status', ctypes.c_int32), ('n_overflow_traces', ctypes.c_int32),
                ('trace_state_off', P(ctypes.c_int64)), ('state_probe', P(ctypes.c_int64)),
                ('cand_count', P(ctypes.c_int32)), ('cand_edge', P(ctypes.c_uint32)),
                ('cand_p', P(ctypes.c_double)), ('cand_sqd', P(ctypes.c_double)),
                ('winner', P(ctypes.c_int32)), ('subpath', P(ctypes.c_int32)),
                ('trace_route_off', P(ctypes.c_int64)), ('route_edge', P(ctypes.c_uint32)),
                ('trace_seg_off', P(ctypes.c_int64)), ('seg_id', P(ctypes.c_uint64)),
                ('seg_start', P(ctypes.c_double)), ('seg_end', P(ctypes.c_double)),
                ('seg_length', P(ctypes.c_int32)), ('seg_queue', P(ctypes.c_int32)),
                ('seg_internal', P(ctypes.c_uint8)), ('seg_begin_shape', P(ctypes.c_int32)),
                ('seg_end_shape', P(ctypes.c_int32)), ('seg_way_off', P(ctypes.c_int64)),
                ('seg_way', P(ctypes.c_uint32)), ('trace_rep_off', P(ctypes.c_int64)),
                ('rep_id', P(ctypes.c_uint64)), ('rep_next', P(ctypes.c_uint64)),
                ('rep_t0', P(ctypes.c_double)), ('rep_t1', P(ctypes.c_double)),
                ('rep_length', P(ctypes.c_int32)), ('rep_queue', P(ctypes.c_int32)),
                ('shape_used', P(ctypes.c_int32)), ('stats', P(ctypes.c_int32)),
                ('stats_len', P(ctypes.c_double)), ('d_hist', ctypes.c_void_p), ('hist_len', ctypes.c_int64),
                ('counters', ctypes.c_uint64 * 24), ('kernel_ms', ctypes.c_float * 16),
                ('trace_status', P(ctypes.c_int32)), ('d_rows', ctypes.c_void_p),
                ('route_tier_code', ctypes.c_int32 * 16), ('route_tier_ms', ctypes.c_float * 16),
                ('route_tier_work', (ctypes.c_uint64 * 4) * 16)]


# the per-probe arrays of otr_point_result, in the struct's order
POINT_FIELDS = [('kind', ctypes.c_uint8, np.uint8), ('edge', ctypes.c_uint32, np.uint32),
                ('frac', ctypes.c_double, np.float64), ('lat', ctypes.c_double, np.float64),
                ('lon', ctypes.c_double, np.float64), ('dist', ctypes.c_double, np.float64),
                ('state', ctypes.c_int64, np.int64), ('pos_mm', ctypes.c_int64, np.int64)]


class PointResult(ctypes.Structure):
    """otr_point_result (include/otr.h): every probe's matched point, host and device arrays."""
    _fields_ = ([('n_probes', ctypes.c_int64), ('kernel_ms', ctypes.c_float), ('reserved', ctypes.c_int32)] +
                [(k, P(ct)) for k, ct, _ in POINT_FIELDS] + [('d_' + k, ctypes.c_void_p) for k, _, _ in POINT_FIELDS])


# the arrays of otr_traversal_result, in the struct's order (trace_off has n_traces + 1 elements,
# the others n_traversals)
TRAVERSAL_FIELDS = [('trace_off', ctypes.c_int64, np.int64), ('edge', ctypes.c_uint32, np.uint32),
                    ('way', ctypes.c_uint32, np.uint32), ('seg_id', ctypes.c_uint64, np.uint64),
                    ('first_state', ctypes.c_int64, np.int64), ('f0', ctypes.c_double, np.float64),
                    ('f1', ctypes.c_double, np.float64), ('s0_mm', ctypes.c_int64, np.int64),
                    ('s1_mm', ctypes.c_int64, np.int64), ('t_enter', ctypes.c_double, np.float64),
                    ('t_exit', ctypes.c_double, np.float64)]


class TraversalResult(ctypes.Structure):
    """otr_traversal_result (include/otr.h): the edge traversals of the matched routes, host and
    device arrays."""
    _fields_ = ([('n_traversals', ctypes.c_int64), ('n_traces', ctypes.c_int64), ('kernel_ms', ctypes.c_float),
                 ('reserved', ctypes.c_int32)] + [(k, P(ct)) for k, ct, _ in TRAVERSAL_FIELDS] +
                [('d_' + k, ctypes.c_void_p) for k, _, _ in TRAVERSAL_FIELDS])


class SessionConfig(ctypes.Structure):
    """otr_session_config (include/otr.h): the session store's sizes, gates and report options."""
    _fields_ = [('max_sessions', ctypes.c_int32), ('max_points', ctypes.c_int32), ('report_dist', ctypes.c_float),
                ('report_count', ctypes.c_int32), ('report_time', ctypes.c_int64), ('session_gap', ctypes.c_int64),
                ('mode', ctypes.c_int32), ('report_levels', ctypes.c_uint32), ('transition_levels', ctypes.c_uint32),
                ('threshold_sec', ctypes.c_int32), ('batch_probes', ctypes.c_int64)]


# the arrays of otr_session_points, in the struct's order
SESSION_POINT_FIELDS = [('key', np.uint64), ('lat', np.float32), ('lon', np.float32), ('accuracy', np.int32),
                        ('time', np.int64), ('timestamp', np.int64)]


class SessionPoints(ctypes.Structure):
    _fields_ = ([('n', ctypes.c_int64), ('memory', ctypes.c_int32), ('reserved', ctypes.c_int32)] +
                [(k, ctypes.c_void_p) for k, _ in SESSION_POINT_FIELDS])


# the per-window and per-report arrays of otr_session_result, in the struct's order
SESSION_WINDOW_FIELDS = [('key', ctypes.c_uint64, np.uint64), ('trigger', ctypes.c_int64, np.int64),
                         ('n_points', ctypes.c_int32, np.int32), ('shape_used', ctypes.c_int32, np.int32),
                         ('status', ctypes.c_int32, np.int32), ('trimmed', ctypes.c_int32, np.int32),
                         ('rep_off', ctypes.c_int64, np.int64)]
SESSION_REPORT_FIELDS = [('id', ctypes.c_uint64, np.uint64), ('next_id', ctypes.c_uint64, np.uint64),
                         ('t0', ctypes.c_double, np.float64), ('t1', ctypes.c_double, np.float64),
                         ('length', ctypes.c_int32, np.int32), ('queue_length', ctypes.c_int32, np.int32)]
SESSION_COUNTS = ['n_windows', 'n_reports', 'n_rounds', 'n_live', 'n_forced', 'n_dropped', 'n_evicted', 'n_rebuilds']


class MessageFormat(ctypes.Structure):
    """otr_message_format (include/otr.h): the stream formatter's SV or JSON message layout."""
    _fields_ = [('type', ctypes.c_int32), ('separator', ctypes.c_int32), ('uuid_index', ctypes.c_int32),
                ('time_index', ctypes.c_int32), ('lat_index', ctypes.c_int32), ('lon_index', ctypes.c_int32),
                ('accuracy_index', ctypes.c_int32), ('time_format', ctypes.c_int32), ('uuid_key', ctypes.c_char_p),
                ('lat_key', ctypes.c_char_p), ('lon_key', ctypes.c_char_p), ('time_key', ctypes.c_char_p),
                ('accuracy_key', ctypes.c_char_p)]


class Messages(ctypes.Structure):
    """otr_messages (include/otr.h): a chunk of raw messages, host or device memory."""
    _fields_ = [('text', ctypes.c_void_p), ('len', ctypes.c_int64), ('memory', ctypes.c_int32),
                ('reserved', ctypes.c_int32), ('msg_off', ctypes.c_void_p), ('n_messages', ctypes.c_int64),
                ('timestamp', ctypes.c_void_p), ('timestamp_all', ctypes.c_int64)]


FORMAT_COUNTS = ['n_messages', 'n_points', 'n_dropped', 'n_unsupported', 'first_bad']


class FormatResult(ctypes.Structure):
    """otr_format_result (include/otr.h): the kept messages as keyed points in HBM."""
    _fields_ = ([(k, ctypes.c_int64) for k in FORMAT_COUNTS] +
                [('first_bad_reason', ctypes.c_int32), ('parse_ms', ctypes.c_float), ('total_ms', ctypes.c_float),
                 ('reserved', ctypes.c_int32), ('points', SessionPoints), ('d_message', ctypes.c_void_p),
                 ('d_uuid_off', ctypes.c_void_p), ('d_uuid_len', ctypes.c_void_p), ('d_status', ctypes.c_void_p)])


class SessionResult(ctypes.Structure):
    """otr_session_result (include/otr.h): the windows of a session call and their reports."""
    _fields_ = ([('n_windows', ctypes.c_int64), ('n_reports', ctypes.c_int64)] +
                [(k, ctypes.c_int32) for k in SESSION_COUNTS[2:]] +
                [('device_ms', ctypes.c_float), ('match_ms', ctypes.c_float)] +
                [(k, P(ct)) for k, ct, _ in SESSION_WINDOW_FIELDS + SESSION_REPORT_FIELDS] +
                [('d_' + k, ctypes.c_void_p) for k, _, _ in SESSION_WINDOW_FIELDS + SESSION_REPORT_FIELDS])


SNAPSHOT_FIELDS = [('key', ctypes.c_uint64, np.uint64), ('point_off', ctypes.c_int64, np.int64),
                   ('max_sep', ctypes.c_float, np.float32), ('last_update', ctypes.c_int64, np.int64),
                   ('lat', ctypes.c_float, np.float32), ('lon', ctypes.c_float, np.float32),
                   ('accuracy', ctypes.c_int32, np.int32), ('time', ctypes.c_int64, np.int64)]


class SessionSnapshot(ctypes.Structure):
    """otr_session_snapshot (include/otr.h): every live session in key order."""
    _fields_ = ([('n_sessions', ctypes.c_int64), ('n_points', ctypes.c_int64)] +
                [(k, P(ct)) for k, ct, _ in SNAPSHOT_FIELDS])


class SessionRecords(ctypes.Structure):
    """otr_session_records (include/otr.h): sessions as the byte values Batch.Serder writes."""
    _fields_ = [('n_records', ctypes.c_int64), ('n_bytes', ctypes.c_int64), ('memory', ctypes.c_int32),
                ('reserved', ctypes.c_int32), ('key', ctypes.c_void_p), ('rec_off', ctypes.c_void_p),
                ('bytes', ctypes.c_void_p), ('d_key', ctypes.c_void_p), ('d_rec_off', ctypes.c_void_p),
                ('d_bytes', ctypes.c_void_p)]


class SessionRestoreResult(ctypes.Structure):
    """otr_session_restore_result (include/otr.h): what a restore did, or why it was refused."""
    _fields_ = [('n_sessions', ctypes.c_int64), ('n_points', ctypes.c_int64), ('bad_session', ctypes.c_int64),
                ('bad_reason', ctypes.c_int32), ('n_live', ctypes.c_int32), ('device_ms', ctypes.c_float),
                ('reserved', ctypes.c_int32)]


class SessionNames(ctypes.Structure):
    """otr_session_names (include/otr.h): one name per point or per session."""
    _fields_ = [('bytes', ctypes.c_void_p), ('n_bytes', ctypes.c_int64), ('off', ctypes.c_void_p),
                ('len', ctypes.c_void_p)]


class SessionNameRefusal(ctypes.Structure):
    """otr_session_name_refusal (include/otr.h): the last named call's name refusal."""
    _fields_ = [('point', ctypes.c_int64), ('message', ctypes.c_int64), ('reason', ctypes.c_int32),
                ('reserved', ctypes.c_int32)]


class SessionNameList(ctypes.Structure):
    """otr_session_name_list (include/otr.h): the names of the last listing, host and device."""
    _fields_ = [('n', ctypes.c_int64), ('n_bytes', ctypes.c_int64), ('off', ctypes.c_void_p),
                ('bytes', ctypes.c_void_p), ('d_off', ctypes.c_void_p), ('d_bytes', ctypes.c_void_p)]


class TileStoreConfig(ctypes.Structure):
    """otr_tile_store_config (include/otr.h)."""
    _fields_ = [('max_rows', ctypes.c_int64), ('quantisation', ctypes.c_int32), ('privacy', ctypes.c_int32)]


TILE_ADD_COUNTS = ['n_reports', 'n_valid', 'n_rows_added', 'n_rows']


class TileAddResult(ctypes.Structure):
    """otr_tile_add_result (include/otr.h): what one add did to the tile store."""
    _fields_ = ([(k, ctypes.c_int64) for k in TILE_ADD_COUNTS] +
                [('device_ms', ctypes.c_float), ('reserved', ctypes.c_int32)])


# the arrays of otr_tile_flush_result, in the struct's order (rows: TILE_ROW records)
TILE_FLUSH_FIELDS = ['rows', 'file', 'row_off', 'n_unclean']
TILE_FLUSH_COUNTS = ['n_rows_in', 'n_rows', 'n_files', 'n_files_empty']


class TileFlushResult(ctypes.Structure):
    """otr_tile_flush_result (include/otr.h): the flush's cleaned files, host and device arrays."""
    _fields_ = ([('n_rows_in', ctypes.c_int64), ('n_rows', ctypes.c_int64), ('n_files', ctypes.c_int32),
                 ('n_files_empty', ctypes.c_int32), ('device_ms', ctypes.c_float), ('reserved', ctypes.c_int32)] +
                [(k, ctypes.c_void_p) for k in TILE_FLUSH_FIELDS] +
                [('d_' + k, ctypes.c_void_p) for k in TILE_FLUSH_FIELDS])


# the arrays of otr_tile_text_result, in the struct's order
TILE_TEXT_FIELDS = ['text', 'text_off', 'names', 'name_off', 'file', 'row_off']
TILE_TEXT_COUNTS = ['n_rows', 'n_text_bytes', 'n_name_bytes', 'n_files']


class TileTextResult(ctypes.Structure):
    """otr_tile_text_result (include/otr.h): the files' texts and names, host and device arrays."""
    _fields_ = ([('n_rows', ctypes.c_int64), ('n_text_bytes', ctypes.c_int64), ('n_name_bytes', ctypes.c_int64),
                 ('n_files', ctypes.c_int32), ('reserved', ctypes.c_int32), ('device_ms', ctypes.c_float),
                 ('reserved2', ctypes.c_int32)] +
                [(k, ctypes.c_void_p) for k in TILE_TEXT_FIELDS] +
                [('d_' + k, ctypes.c_void_p) for k in TILE_TEXT_FIELDS])


class TileTexts(ctypes.Structure):
    """otr_tile_texts (include/otr.h): the texts and names of many tile files, K19's output shape."""
    _fields_ = [('text', ctypes.c_void_p), ('text_off', ctypes.c_void_p), ('names', ctypes.c_void_p),
                ('name_off', ctypes.c_void_p), ('n_files', ctypes.c_int32), ('memory', ctypes.c_int32)]


# the arrays of otr_tile_parse_result, in the struct's order (rows: TILE_ROW records)
TILE_PARSE_FIELDS = ['rows', 'row_off', 'file', 'file_status', 'file_line_off', 'line_status']
TILE_PARSE_COUNTS = ['n_lines', 'n_rows', 'n_headers', 'n_bad', 'n_bad_names', 'first_bad', 'first_bad_file',
                     'first_bad_reason', 'n_files']
# OTR_TILE_LINE_*
TILE_LINE = {'ROW': 0, 'HEADER': 1, 'E_FIELDS': 2, 'U_NAME': 32, 'U_END': 33, 'U_HEADER': 34, 'U_FIELDS': 35,
             'U_NUMBER': 36, 'U_NEXT': 37, 'U_COUNT': 38, 'U_TAG': 39}
TILE_LINE_NAME = {v: k for k, v in TILE_LINE.items()}
OTR_TILE_LINE_UNSUPPORTED = 32
OTR_TILE_PARSE_NO_HOST = 1


class TileParseResult(ctypes.Structure):
    """otr_tile_parse_result (include/otr.h): the rows read back from tile file texts."""
    _fields_ = ([(k, ctypes.c_int64) for k in TILE_PARSE_COUNTS[:6]] +
                [('first_bad_file', ctypes.c_int32), ('first_bad_reason', ctypes.c_int32),
                 ('device_ms', ctypes.c_float), ('n_files', ctypes.c_int32)] +
                [(k, ctypes.c_void_p) for k in TILE_PARSE_FIELDS] +
                [('d_' + k, ctypes.c_void_p) for k in TILE_PARSE_FIELDS])


def tile_parse_to_numpy(r, host=True):
    """An otr_tile_parse_result: its counts, device_ms and device pointers d_*, and with host=True
    copies of rows (TILE_ROW), row_off and file_line_off (int64), file (uint64), file_status and
    line_status (uint8)."""
    nf = int(r.n_files)
    out = {k: int(getattr(r, k)) for k in TILE_PARSE_COUNTS}
    out['device_ms'] = float(r.device_ms)
    if host:
        out['rows'] = _copy(r.rows, int(r.n_rows), TILE_ROW)
        out['row_off'] = _copy(r.row_off, nf + 1, np.int64)
        out['file'] = _copy(r.file, nf, np.uint64)
        out['file_status'] = _copy(r.file_status, nf, np.uint8)
        out['file_line_off'] = _copy(r.file_line_off, nf + 1, np.int64)
        out['line_status'] = _copy(r.line_status, int(r.n_lines), np.uint8)
    for k in TILE_PARSE_FIELDS:
        out['d_' + k] = int(getattr(r, 'd_' + k) or 0)
    return out


class TileSnapshot(ctypes.Structure):
    """otr_tile_snapshot (include/otr.h): the held rows in arrival order, with their times."""
    _fields_ = [('n_rows', ctypes.c_int64), ('quantisation', ctypes.c_int32), ('flags', ctypes.c_int32),
                ('rows', ctypes.c_void_p), ('t0', ctypes.c_void_p), ('t1', ctypes.c_void_p),
                ('d_rows', ctypes.c_void_p), ('d_t0', ctypes.c_void_p), ('d_t1', ctypes.c_void_p)]


TILE_RESTORE_COUNTS = ['n_slices', 'n_rows', 'n_unreferenced_slices', 'n_unreferenced_rows', 'n_missing_slices',
                       'n_rows_held', 'bad_slice', 'bad_tile']


class TileRestoreResult(ctypes.Structure):
    """otr_tile_restore_result (include/otr.h): what a tile restore did, or why it was refused."""
    _fields_ = ([(k, ctypes.c_int64) for k in TILE_RESTORE_COUNTS] +
                [('bad_reason', ctypes.c_int32), ('device_ms', ctypes.c_float)])


# the arrays of otr_tile_records, in the struct's order
TILE_RECORD_FIELDS = ['start', 'tile_id', 'slice', 'rec_off', 'bytes', 'names', 'name_off', 'map_bytes']


class TileRecords(ctypes.Structure):
    """otr_tile_records (include/otr.h): the tile store as Segment.ListSerder slice records and
    the slice map's entries."""
    _fields_ = ([('n_slices', ctypes.c_int64), ('n_bytes', ctypes.c_int64), ('n_name_bytes', ctypes.c_int64),
                 ('n_tiles', ctypes.c_int64), ('slice_size', ctypes.c_int32), ('memory', ctypes.c_int32)] +
                [(k, ctypes.c_void_p) for k in TILE_RECORD_FIELDS] +
                [('d_' + k, ctypes.c_void_p) for k in TILE_RECORD_FIELDS])


def _copy(ptr, n, dt):
    """n records of dtype dt at the host address ptr, copied."""
    if n <= 0 or not ptr:
        return np.zeros(max(n, 0), dt)
    return np.frombuffer(ctypes.string_at(ptr, n * np.dtype(dt).itemsize), dtype=dt).copy()


def tile_add_to_dict(r):
    out = {k: int(getattr(r, k)) for k in TILE_ADD_COUNTS}
    out['device_ms'] = float(r.device_ms)
    return out


def tile_flush_to_numpy(r):
    """Host arrays of an otr_tile_flush_result (copies), its counts and its device pointers."""
    nf = int(r.n_files)
    out = {k: int(getattr(r, k)) for k in TILE_FLUSH_COUNTS}
    out['device_ms'] = float(r.device_ms)
    out['rows'] = _copy(r.rows, int(r.n_rows), TILE_ROW)
    out['file'] = _copy(r.file, nf, np.uint64)
    out['row_off'] = _copy(r.row_off, nf + 1, np.int64)
    out['n_unclean'] = _copy(r.n_unclean, nf, np.int64)
    for k in TILE_FLUSH_FIELDS:
        out['d_' + k] = int(getattr(r, 'd_' + k) or 0)
    return out


def tile_snapshot_to_numpy(r, host=True):
    """An otr_tile_snapshot: n_rows, quantisation, flags, the device pointers d_rows, d_t0, d_t1
    and with host=True copies of rows and, from a store with the times, t0 and t1 (else None)."""
    n = int(r.n_rows)
    out = {'n_rows': n, 'quantisation': int(r.quantisation), 'flags': int(r.flags)}
    for k in ('rows', 't0', 't1'):
        out['d_' + k] = int(getattr(r, 'd_' + k) or 0)
    if host:
        timed = bool(r.flags & OTR_TILE_STORE_TIMES)
        out['rows'] = _copy(r.rows, n, TILE_ROW)
        out['t0'] = _copy(r.t0, n, np.float64) if timed else None
        out['t1'] = _copy(r.t1, n, np.float64) if timed else None
    return out


def tile_restore_to_dict(r):
    out = {k: int(getattr(r, k)) for k in TILE_RESTORE_COUNTS}
    out['bad_reason'], out['device_ms'] = int(r.bad_reason), float(r.device_ms)
    return out


def tile_records_to_numpy(r):
    """An otr_tile_records export: host copies of start, tile_id, rec_off, name_off (int64), slice
    (int32), bytes, names, map_bytes (uint8), the counts, slice_size and the device pointers d_*."""
    ns, nt = int(r.n_slices), int(r.n_tiles)
    out = {'n_slices': ns, 'n_bytes': int(r.n_bytes), 'n_name_bytes': int(r.n_name_bytes), 'n_tiles': nt,
           'slice_size': int(r.slice_size)}
    out['start'] = _copy(r.start, ns, np.int64)
    out['tile_id'] = _copy(r.tile_id, ns, np.int64)
    out['slice'] = _copy(r.slice, ns, np.int32)
    out['rec_off'] = _copy(r.rec_off, ns + 1, np.int64)
    out['name_off'] = _copy(r.name_off, ns + 1, np.int64)
    out['bytes'] = _bytes(r.bytes, int(r.n_bytes))
    out['names'] = _bytes(r.names, int(r.n_name_bytes))
    out['map_bytes'] = _bytes(r.map_bytes, 20 * max(nt, 0))
    for k in TILE_RECORD_FIELDS:
        out['d_' + k] = int(getattr(r, 'd_' + k) or 0)
    return out


def _bytes(ptr, n):
    """n bytes at the host address ptr as a numpy uint8 array (one copy, also beyond 2 GiB)."""
    out = np.empty(max(n, 0), np.uint8)
    if n > 0 and ptr:
        ctypes.memmove(out.ctypes.data, ptr, n)
    return out


def tile_text_to_numpy(r, host=True):
    """An otr_tile_text_result: its counts, device_ms and device pointers d_*, and with host=True
    copies of text and names (uint8), text_off, name_off, row_off (int64) and file (uint64)."""
    nf = int(r.n_files)
    out = {k: int(getattr(r, k)) for k in TILE_TEXT_COUNTS}
    out['device_ms'] = float(r.device_ms)
    if host:
        out['text'] = _bytes(r.text, int(r.n_text_bytes))
        out['names'] = _bytes(r.names, int(r.n_name_bytes))
        out['text_off'] = _copy(r.text_off, nf + 1, np.int64)
        out['name_off'] = _copy(r.name_off, nf + 1, np.int64)
        out['row_off'] = _copy(r.row_off, nf + 1, np.int64)
        out['file'] = _copy(r.file, nf, np.uint64)
    for k in TILE_TEXT_FIELDS:
        out['d_' + k] = int(getattr(r, 'd_' + k) or 0)
    return out


def device_to_numpy(ptr, n, dt):
    """n records of dtype dt at the device address ptr, copied to the host (through the HIP
    runtime libotr links; the producing call has drained its stream)."""
    out = np.zeros(max(int(n), 0), dt)
    if len(out) and ptr:
        L = lib()
        L.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        rc = L.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2)  # hipMemcpyDeviceToHost
        if rc != 0:
            raise RuntimeError('hipMemcpy failed (%d)' % rc)
    return out


# the per-point arrays of otr_format_result beside its points, and the per-message one
FORMAT_POINT_FIELDS = [('d_message', 'message', np.int64), ('d_uuid_off', 'uuid_off', np.int64),
                       ('d_uuid_len', 'uuid_len', np.int32)]


def format_result_to_numpy(r, arrays=True):
    """An otr_format_result as host copies: counts, times, the points (key, lat, lon, accuracy,
    time, timestamp), message, uuid_off, uuid_len per point and status per message; 'device'
    holds the result struct, its arrays in HBM (valid until the matcher's next formatter call).
    arrays=False: counts, times and 'device' only, nothing copied."""
    out = {k: int(getattr(r, k)) for k in FORMAT_COUNTS}
    out['first_bad_reason'] = int(r.first_bad_reason)
    out['parse_ms'], out['total_ms'] = float(r.parse_ms), float(r.total_ms)
    out['device'] = r
    if not arrays:
        return out
    n = int(r.n_points)
    for k, dt in SESSION_POINT_FIELDS:
        out[k] = device_to_numpy(getattr(r.points, k), n, dt)
    for src, k, dt in FORMAT_POINT_FIELDS:
        out[k] = device_to_numpy(getattr(r, src), n, dt)
    out['status'] = device_to_numpy(r.d_status, int(r.n_messages), np.int32)
    return out


def session_result_to_numpy(r):
    """Host arrays of an otr_session_result (copies) and its counts."""
    nw, nr = int(r.n_windows), int(r.n_reports)
    out = {k: _arr(getattr(r, k), nw + 1 if k == 'rep_off' else nw, dt) for k, _, dt in SESSION_WINDOW_FIELDS}
    if not r.rep_off:
        out['rep_off'] = np.zeros(1, np.int64)
    out.update({k: _arr(getattr(r, k), nr, dt) for k, _, dt in SESSION_REPORT_FIELDS})
    out.update({k: int(getattr(r, k)) for k in SESSION_COUNTS})
    out['device_ms'] = float(r.device_ms)
    out['match_ms'] = float(r.match_ms)
    return out


def snapshot_to_numpy(r):
    ns, npt = int(r.n_sessions), int(r.n_points)
    per_session = ('key', 'max_sep', 'last_update')
    return {k: _arr(getattr(r, k), ns + 1 if k == 'point_off' else (ns if k in per_session else npt), dt)
            for k, _, dt in SNAPSHOT_FIELDS}


def pack_names(names):
    """(bytes uint8, off int64, len int32) of a sequence of bytes objects, packed end to end."""
    names = [bytes(x) for x in names]
    ln = np.array([len(x) for x in names], np.int32)
    off = np.zeros(len(names), np.int64)
    if len(names):
        off[1:] = np.cumsum(ln[:-1], dtype=np.int64)
    return np.frombuffer(b''.join(names), np.uint8).copy(), off, ln


def names_to_list(r):
    """An otr_session_name_list as a list of bytes objects (host copies)."""
    n = int(r.n)
    off = _copy(r.off, n + 1, np.int64)
    data = ctypes.string_at(r.bytes, int(r.n_bytes)) if r.bytes and r.n_bytes else b''
    return [data[int(off[i]):int(off[i + 1])] for i in range(n)]


def records_to_numpy(r):
    """An exported otr_session_records as host copies (key, rec_off, bytes); 'device' holds the
    struct, whose d_* arrays stay in HBM until the matcher's next session call."""
    n, nb = int(r.n_records), int(r.n_bytes)

    def arr(ptr, count, dt):
        if not ptr or count == 0:
            return np.zeros(count, dt)
        return np.ctypeslib.as_array(ctypes.cast(ptr, P(np.ctypeslib.as_ctypes_type(dt))), shape=(count,)).copy()
    off = arr(r.rec_off, n + 1, np.int64)
    return {'key': arr(r.key, n, np.uint64), 'rec_off': off if len(off) else np.zeros(1, np.int64),
            'bytes': arr(r.bytes, nb, np.uint8), 'device': r}


# otr_hist_entry (include/otr.h), 32 bytes
HIST_ENTRY = np.dtype([('file', '<u8'), ('id', '<u8'), ('next_id', '<u8'), ('speed_bin', '<u4'), ('count', '<u4')])

# otr_tile_row (include/otr.h), 56 bytes
TILE_ROW = np.dtype([('file', '<u8'), ('id', '<u8'), ('next_id', '<u8'), ('start', '<i8'), ('end', '<i8'),
                     ('duration', '<i4'), ('length', '<i4'), ('queue_length', '<i4'), ('speed_bin', '<i4')])


_L = None


def lib():
    """Load libotr.so once.  torch (if installed) is imported first so that the
    process holds a single HIP runtime (libotr links the one torch ships)."""
    global _L
    if _L is not None:
        return _L
    if not os.path.exists(LIB_PATH):
        raise RuntimeError('reporter_amd/libotr.so is not built: run `python __graft_entry__.py build` '
                           '(the HIP path has no fallback)')
    try:
        import torch  # noqa: F401  (shares its libamdhip64 with libotr)
    except Exception:
        pass
    L = ctypes.CDLL(LIB_PATH)
    L.otr_configure.argtypes = [ctypes.c_char_p]
    L.otr_configure_json.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.otr_matcher_new.restype = ctypes.c_void_p
    L.otr_matcher_free.argtypes = [ctypes.c_void_p]
    L.otr_match.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_void_p),
                            P(ctypes.c_size_t)]
    L.otr_report.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, P(ctypes.c_void_p),
                             P(ctypes.c_size_t)]
    L.otr_report_segments.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                      ctypes.c_int, P(ctypes.c_int32), ctypes.c_int, P(ctypes.c_int32),
                                      ctypes.c_int, P(ctypes.c_void_p), P(ctypes.c_size_t)]
    L.otr_free.argtypes = [ctypes.c_void_p]
    L.otr_last_error.restype = ctypes.c_char_p
    L.otr_match_batch.argtypes = [ctypes.c_void_p, P(TraceBatch), P(BatchResult)]
    if hasattr(L, 'otr_matched_points'):  # (an A/B build of an earlier round may lack it)
        L.otr_matched_points.argtypes = [ctypes.c_void_p, P(PointResult)]
    if hasattr(L, 'otr_edge_traversals'):
        L.otr_edge_traversals.argtypes = [ctypes.c_void_p, P(TraversalResult)]
        L.otr_edge_observations.argtypes = [ctypes.c_void_p, ctypes.c_int32, P(ctypes.c_void_p), P(ctypes.c_int64)]
    if hasattr(L, 'otr_sessions_open'):  # (an A/B build of an earlier round may lack them)
        L.otr_sessions_open.argtypes = [ctypes.c_void_p, P(SessionConfig)]
        L.otr_sessions_close.argtypes = [ctypes.c_void_p]
        L.otr_sessions_push.argtypes = [ctypes.c_void_p, P(SessionPoints), P(SessionResult)]
        L.otr_sessions_punctuate.argtypes = [ctypes.c_void_p, ctypes.c_int64, P(SessionResult)]
        L.otr_sessions_advance.argtypes = [ctypes.c_void_p, P(SessionPoints), P(TraceBatch)]
        L.otr_sessions_commit.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
        L.otr_sessions_windows.argtypes = [ctypes.c_void_p, P(SessionResult)]
        L.otr_sessions_snapshot.argtypes = [ctypes.c_void_p, P(SessionSnapshot)]
    if hasattr(L, 'otr_sessions_restore'):
        L.otr_sessions_restore.argtypes = [ctypes.c_void_p, P(SessionSnapshot), ctypes.c_int32,
                                           P(SessionRestoreResult)]
        L.otr_sessions_restore_records.argtypes = [ctypes.c_void_p, P(SessionRecords), P(SessionRestoreResult)]
        L.otr_sessions_export_records.argtypes = [ctypes.c_void_p, P(SessionRecords)]
        L.otr_sessions_take.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                        P(SessionSnapshot)]
        L.otr_uuid_key.argtypes = [ctypes.c_char_p, ctypes.c_int64]
        L.otr_uuid_key.restype = ctypes.c_uint64
    if hasattr(L, 'otr_sessions_open_named'):
        L.otr_sessions_open_named.argtypes = [ctypes.c_void_p, P(SessionConfig), ctypes.c_int32]
        L.otr_sessions_push_named.argtypes = [ctypes.c_void_p, P(SessionPoints), P(SessionNames), P(SessionResult)]
        L.otr_sessions_advance_named.argtypes = [ctypes.c_void_p, P(SessionPoints), P(SessionNames), P(TraceBatch)]
        L.otr_sessions_last_refusal.argtypes = [ctypes.c_void_p, P(SessionNameRefusal)]
        L.otr_sessions_names.argtypes = [ctypes.c_void_p, P(SessionNameList)]
        L.otr_sessions_restore_named.argtypes = [ctypes.c_void_p, P(SessionSnapshot), P(SessionNames), ctypes.c_int32,
                                                 P(SessionRestoreResult)]
        L.otr_sessions_restore_records_named.argtypes = [ctypes.c_void_p, P(SessionRecords), P(SessionNames),
                                                         P(SessionRestoreResult)]
    if hasattr(L, 'otr_tile_store_open'):  # (an A/B build of an earlier round may lack them)
        L.otr_tile_store_open.argtypes = [ctypes.c_void_p, P(TileStoreConfig)]
        L.otr_tile_store_close.argtypes = [ctypes.c_void_p]
        L.otr_tile_store_add_session.argtypes = [ctypes.c_void_p, P(TileAddResult)]
        L.otr_tile_store_add_reports.argtypes = [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 7 + \
            [ctypes.c_int32, P(TileAddResult)]
        L.otr_tile_store_add_rows.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                              P(TileAddResult)]
        L.otr_tile_store_flush.argtypes = [ctypes.c_void_p, P(TileFlushResult)]
    if hasattr(L, 'otr_tiles_text'):
        L.otr_tiles_text.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                     ctypes.c_int32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int32,
                                     P(TileTextResult)]
        L.otr_tile_store_flush_text.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int32,
                                                P(TileFlushResult), P(TileTextResult)]
    if hasattr(L, 'otr_tiles_parse'):
        L.otr_tiles_parse.argtypes = [ctypes.c_void_p, P(TileTexts), ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p,
                                      ctypes.c_char_p, ctypes.c_int32, P(TileParseResult)]
    if hasattr(L, 'otr_tile_store_open_ex'):
        L.otr_tile_store_open_ex.argtypes = [ctypes.c_void_p, P(TileStoreConfig), ctypes.c_int32]
        L.otr_tile_store_snapshot.argtypes = [ctypes.c_void_p, ctypes.c_int32, P(TileSnapshot)]
        L.otr_tile_store_restore.argtypes = [ctypes.c_void_p, P(TileSnapshot), ctypes.c_int32, P(TileRestoreResult)]
        L.otr_tile_store_export_records.argtypes = [ctypes.c_void_p, ctypes.c_int32, P(TileRecords)]
        L.otr_tile_store_restore_records.argtypes = [ctypes.c_void_p, P(TileRecords), P(TileRestoreResult)]
        L.otr_tile_slice_key.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_char_p,
                                         ctypes.c_int64]
        L.otr_tile_slice_key_parse.argtypes = [ctypes.c_char_p, ctypes.c_int64, P(ctypes.c_int64), P(ctypes.c_int64),
                                               P(ctypes.c_int32)]
    if hasattr(L, 'otr_format_messages'):
        L.otr_format_messages.argtypes = [ctypes.c_void_p, P(MessageFormat), P(Messages), P(FormatResult)]
        L.otr_sessions_push_text.argtypes = [ctypes.c_void_p, P(MessageFormat), P(Messages), P(FormatResult),
                                             P(SessionResult)]
    L.otr_graph_info.argtypes = [P(ctypes.c_int64), P(ctypes.c_int64), P(ctypes.c_int64)]
    L.otr_matcher_stream.argtypes = [ctypes.c_void_p]
    L.otr_matcher_stream.restype = ctypes.c_void_p
    L.otr_report_batch.argtypes = [ctypes.c_void_p, ctypes.c_int32, P(ctypes.c_char_p), P(ctypes.c_size_t),
                                   ctypes.c_int, P(ctypes.c_int32), P(ctypes.c_void_p), P(ctypes.c_size_t)]
    L.otr_coalesce.argtypes = [ctypes.c_int32, ctypes.c_int32]
    if hasattr(L, 'otr_service_stats'):  # (an A/B build of an earlier round may lack it)
        L.otr_service_stats.argtypes = [P(ServiceSplit), ctypes.c_int]
    L.otr_tiles_cull.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                 ctypes.c_int32, P(ctypes.c_void_p), P(ctypes.c_int64)]
    L.otr_tiles_format.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_char_p, ctypes.c_char_p,
                                   ctypes.c_int32, P(ctypes.c_void_p), P(ctypes.c_size_t)]
    L.otr_ingest.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, P(IngestFormat),
                             P(IngestResult)]
    if hasattr(L, 'otr_max_batch_probes'):  # (an A/B build of an earlier round may lack them)
        L.otr_max_batch_probes.restype = ctypes.c_int64
        L.otr_launch_max_items.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]
        L.otr_launch_max_items.restype = ctypes.c_uint64
    L.otr_tilehier_row.argtypes = [ctypes.c_int32, ctypes.c_double]
    L.otr_tilehier_row.restype = ctypes.c_int32
    L.otr_tilehier_col.argtypes = [ctypes.c_int32, ctypes.c_double]
    L.otr_tilehier_col.restype = ctypes.c_int32
    L.otr_tilehier_file.argtypes = [ctypes.c_int32, ctypes.c_int64, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    L.otr_tilehier_files.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_char_p,
                                 P(ctypes.c_void_p), P(ctypes.c_size_t)]
    L.otr_flatten.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p]
    L.otr_hist_reduce.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                  ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, P(ctypes.c_int64)]
    _L = L
    return L


def last_error():
    return lib().otr_last_error().decode('utf-8', 'replace')


def take_string(ptr, n):
    """Copy a library-owned output string and release it with otr_free."""
    if not ptr.value:
        return ''
    s = ctypes.string_at(ptr.value, n.value).decode('utf-8')
    lib().otr_free(ptr.value)
    return s


def levels_mask(levels):
    m = 0
    for l in levels:
        l = int(l)
        if 0 <= l < 32:
            m |= 1 << l
    return m


def _arr(p, n, dt):
    if n <= 0 or not p:
        return np.zeros(max(n, 0), dt)
    return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True)


def result_to_numpy(r):
    """Host arrays of an OTR_BATCH_COPY_OUT result (same keys as oracle.pyoracle.match_batch)."""
    nt, ns, nseg, nrep = r.n_traces, r.n_states, r.n_seg, r.n_rep
    out = dict(
        trace_state_off=_arr(r.trace_state_off, nt + 1, np.int64),
        state_probe=_arr(r.state_probe, ns, np.int64),
        cand_count=_arr(r.cand_count, ns, np.int32),
        cand_edge=_arr(r.cand_edge, ns * KMAX, np.uint32).reshape(ns, KMAX),
        cand_p=_arr(r.cand_p, ns * KMAX, np.float64).reshape(ns, KMAX),
        cand_sqd=_arr(r.cand_sqd, ns * KMAX, np.float64).reshape(ns, KMAX),
        winner=_arr(r.winner, ns, np.int32), subpath=_arr(r.subpath, ns, np.int32),
        trace_route_off=_arr(r.trace_route_off, nt + 1, np.int64),
        route_edge=_arr(r.route_edge, r.n_route, np.uint32),
        trace_seg_off=_arr(r.trace_seg_off, nt + 1, np.int64),
        seg_id=_arr(r.seg_id, nseg, np.uint64), seg_start=_arr(r.seg_start, nseg, np.float64),
        seg_end=_arr(r.seg_end, nseg, np.float64), seg_length=_arr(r.seg_length, nseg, np.int32),
        seg_queue=_arr(r.seg_queue, nseg, np.int32), seg_internal=_arr(r.seg_internal, nseg, np.uint8),
        seg_begin_shape=_arr(r.seg_begin_shape, nseg, np.int32),
        seg_end_shape=_arr(r.seg_end_shape, nseg, np.int32),
        seg_way_off=_arr(r.seg_way_off, nseg + 1, np.int64),
        trace_rep_off=_arr(r.trace_rep_off, nt + 1, np.int64),
        rep_id=_arr(r.rep_id, nrep, np.uint64), rep_next=_arr(r.rep_next, nrep, np.uint64),
        rep_t0=_arr(r.rep_t0, nrep, np.float64), rep_t1=_arr(r.rep_t1, nrep, np.float64),
        rep_length=_arr(r.rep_length, nrep, np.int32), rep_queue=_arr(r.rep_queue, nrep, np.int32),
        shape_used=_arr(r.shape_used, nt, np.int32),
        stats=_arr(r.stats, nt * 7, np.int32).reshape(nt, 7),
        stats_len=_arr(r.stats_len, nt * 2, np.float64).reshape(nt, 2),
    )
    out['seg_way'] = _arr(r.seg_way, int(out['seg_way_off'][-1]) if nseg else 0, np.uint32)
    out['counters'] = list(r.counters)
    out['n_rows'] = r.n_rows
    out['status'] = r.status
    out['n_overflow'] = r.n_overflow_traces
    return out


def points_to_numpy(r):
    """Host arrays of an otr_point_result (copies): kind, edge, frac, lat, lon, dist, state, pos_mm."""
    return {k: _arr(getattr(r, k), int(r.n_probes), dt) for k, _, dt in POINT_FIELDS}


def traversals_to_numpy(r):
    """Host arrays of an otr_traversal_result (copies): trace_off, edge, way, seg_id, first_state,
    f0, f1, s0_mm, s1_mm, t_enter, t_exit."""
    return {k: _arr(getattr(r, k), int(r.n_traces) + 1 if k == 'trace_off' else int(r.n_traversals), dt)
            for k, _, dt in TRAVERSAL_FIELDS}


def service_stats(reset=False):
    """otr_service_stats: the JSON path's host split since the last reset (dict)."""
    st = ServiceSplit()
    lib().otr_service_stats(ctypes.byref(st), 1 if reset else 0)
    return {k: getattr(st, k) for k, _ in ServiceSplit._fields_}
