/*
 * otr.h — C-ABI of libotr.so, the MI355X-native drop-in for Open Traffic Reporter's
 * matching hot path (trace JSON → map-match → OSMLR segment / speed JSON).
 *
 * Plain C: pointers, sizes, status codes.  No torch or HIP types cross this line.
 * Every entry point names the reference interface it replaces.
 *
 * Threading: otr_configure() is process-global and not thread-safe (call once, as
 * reporter_service.py:284 / simple_reporter.py:132 call valhalla.Configure once).
 * An otr_matcher is owned by one thread at a time (reporter_service.py:51-52 keeps
 * one valhalla.SegmentMatcher per thread); matchers share the read-only graph that
 * otr_configure placed in HBM.
 */
#ifndef OTR_H
#define OTR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (HTTP codes of reporter_service.py:209-245 are kept) ---- */
#define OTR_OK 0
#define OTR_BAD_REQUEST 400   /* reporter_service.py:214,219,225,231,235 */
#define OTR_MATCH_ERROR 500   /* reporter_service.py:244-245 */
#define OTR_NOT_CONFIGURED 503
#define OTR_DEVICE_ERROR 504

typedef struct otr_matcher otr_matcher;

/* Replaces valhalla.Configure(conf_path) (reporter_service.py:284, simple_reporter.py:132).
 * Reads a Valhalla-style JSON config: {"meili": {"default": {...}, "auto": {...}, ...},
 * "otr": {"graph": "<flattened graph file>", "device": 0}} (meili values:
 * Dockerfile:14-17,42-49).  Loads the graph once and uploads it to HBM.  Returns
 * OTR_OK or an error code; otr_last_error() holds the message. */
int otr_configure(const char* config_json_path);

/* Same, with the config given as a JSON string (for embedders without files). */
int otr_configure_json(const char* config_json, size_t len);

/* Replaces valhalla.SegmentMatcher() (reporter_service.py:52, simple_reporter.py:133). */
otr_matcher* otr_matcher_new(void);
void otr_matcher_free(otr_matcher* m);

/* Replaces SegmentMatcher.Match(json) -> str (reporter_service.py:240,
 * simple_reporter.py:166): trace JSON in, {"segments":[...],"mode":...} out
 * (schema README.md:288-300).  *out is owned by the library: release with otr_free.
 * Returns OTR_OK, or an error code with *out = {"error":"..."}. */
int otr_match(otr_matcher* m, const char* json, size_t len, char** out, size_t* out_len);

/* Replaces the HTTP POST /report round trip (Batch.java:68 → reporter_service.py
 * handle_request 209-245): request validation, Match, then report() with
 * report_levels / transition_levels from match_options (reporter_service.py:228-235).
 * Returns 200 with the report() JSON, or 400/500 with {"error":"..."} carrying the
 * reference's messages.  threshold_sec < 0 selects THRESHOLD_SEC or 15
 * (reporter_service.py:55-58). */
int otr_report(otr_matcher* m, const char* json, size_t len, int threshold_sec, char** out, size_t* out_len);

/* report() alone (reporter_service.py:79-179) over a Match() output string and the
 * original trace JSON; for callers that already hold a match (simple_reporter.py:168). */
int otr_report_segments(const char* match_json, size_t match_len, const char* trace_json, size_t trace_len,
                        int threshold_sec, const int32_t* report_levels, int n_report_levels,
                        const int32_t* transition_levels, int n_transition_levels, char** out, size_t* out_len);

/* n POST /report bodies at once (the reference serves one per HTTP request,
 * reporter_service.py:209-245; a batching caller such as BatchingProcessor.java:58-141
 * holds many).  Bodies are scanned on host threads, grouped by the options that must
 * be uniform within a device batch (report/transition levels, match_options
 * overrides) and matched in shared device batches.  codes[i] / outs[i] / out_lens[i]
 * are exactly what otr_report returns for bodies[i] (release each outs[i] with
 * otr_free).  Returns OTR_OK once every item has its code. */
int otr_report_batch(otr_matcher* m, int32_t n, const char* const* bodies, const size_t* lens, int threshold_sec,
                     int32_t* codes, char** outs, size_t* out_lens);

/* Process-wide request coalescing (SURVEY §8b threading row): while enabled,
 * otr_report calls from any number of threads are handed to one dispatcher thread
 * that runs them as shared device batches of up to max_traces, waiting at most
 * max_wait_us after the first queued request.  Each caller still blocks until its
 * own response is ready and receives exactly what the uncoalesced call returns.
 * max_traces <= 0 drains the queue and stops the dispatcher. */
int otr_coalesce(int32_t max_traces, int32_t max_wait_us);

/* Where the JSON request path's host time goes (new; diagnostics for the drop-in
 * callers of otr_report / otr_report_batch / the coalescer): summed over every internal
 * request-processing call of the process since the last reset — calls (a batch call, or
 * one coalesced batch), items (bodies), device batches, and the wall seconds of its
 * phases: scan (body parse + validation into SoA, host threads), soa (gather of each
 * device batch's arrays), device (otr_match_batch: H2D, kernels, D2H of the compacted
 * reports), format (report() bodies, host threads); total is their sum plus grouping. */
typedef struct otr_service_split {
  int64_t calls, items, device_batches;
  double scan_s, soa_s, device_s, format_s, total_s;
} otr_service_split;
int otr_service_stats(otr_service_split* out, int reset);

void otr_free(char* p);
const char* otr_last_error(void);

/* ---- batched throughput API (new; the reference matches one trace per call) ---- */

#define OTR_MEM_HOST 0
#define OTR_MEM_DEVICE 1

typedef struct otr_trace_batch {
  int32_t n_traces;
  int32_t memory;              /* OTR_MEM_HOST or OTR_MEM_DEVICE (pointers in HBM) */
  const int64_t* trace_offsets;  /* n_traces+1 probe offsets */
  const double* lat;
  const double* lon;
  const int64_t* time;         /* epoch seconds */
  const float* accuracy;       /* metres, NULL or <0 entries = not given */
  const uint8_t* mode;         /* per trace: 0 auto, 1 bicycle, 2 pedestrian */
  uint32_t report_levels;      /* bit mask of OSMLR levels, simple_reporter --report-levels */
  uint32_t transition_levels;  /* bit mask, --transition-levels */
  int32_t threshold_sec;       /* report() tail threshold, 15 */
  int32_t quantisation;        /* hour bucket seconds, 3600 (simple_reporter.py:343) */
  int64_t hist_base_time;      /* histogram covers [base, base + hist_hours*quantisation) */
  int32_t hist_hours;
  int32_t flags;               /* OTR_BATCH_* */
  uint32_t* hist_device;       /* optional caller-owned device histogram (else library-owned) */
  int32_t tile_rules;          /* OTR_TILE_RULES_* for OTR_BATCH_TILE_ROWS */
  int32_t reserved;
} otr_trace_batch;

#define OTR_BATCH_COPY_OUT 1   /* fill the host arrays of otr_batch_result */
#define OTR_BATCH_TIMING 2     /* record per-kernel HIP-event timings */
#define OTR_BATCH_COPY_REPORTS 4  /* host copies of segments, reports, stats only (the JSON path) */
#define OTR_BATCH_TILE_ROWS 8  /* also emit simple_reporter tile rows on device (d_rows / n_rows) */
#define OTR_BATCH_ROUTE_WORK 16  /* count the LDS route tiers' work (route_tier_work, counters
                                    3, 4, 9, 10, 13, 14): instrumentation, ~7% of the first tier */
#define OTR_BATCH_MATCHED_POINTS 32  /* also compute every probe's matched point (K12): read it
                                        with otr_matched_points after the call */
#define OTR_BATCH_EDGE_TRAVERSALS 64  /* also compute the edge traversals of the matched route
                                         (K13): read them with otr_edge_traversals and
                                         otr_edge_observations after the call */

/* One simple_reporter tile line (simple_reporter.py:188-195) in binary form: the line
 * "id,next_id,duration,1,length,queue_length,start,end,source,MODE" of the file
 * "{b*q}_{(b+1)*q-1}/{level}/{tile_index}" (q = quantisation). */
typedef struct otr_tile_row {
  uint64_t file;       /* bucket b << 25 | level << 22 | tile index (get_tile_level/_index, :45-49) */
  uint64_t id;         /* segment id */
  uint64_t next_id;    /* next segment id, or INVALID_SEGMENT_ID 0x3fffffffffff (:43,193) */
  int64_t start;       /* floor(t0) */
  int64_t end;         /* ceil(t1) */
  int32_t duration;    /* int(round(t1 - t0)), Python 2 rounding (:179) */
  int32_t length;
  int32_t queue_length;
  int32_t speed_bin;   /* min(int(length / (t1 - t0) * 3.6 / 20), 7): the report's 20 km/h speed bin;
                          -1 in a row read back from a tile file's text (otr_tiles_parse below): the
                          text holds floor(t0), ceil(t1) and the rounded duration, not t0 and t1, so
                          the bin cannot be recovered.  The cull's two orders and the file texts
                          never read it. */
} otr_tile_row;
#define OTR_INVALID_SEGMENT_ID 0x3fffffffffffull

/* Which reference path the tile rows follow.
 * OTR_TILE_RULES_SIMPLE: simple_reporter.py:176-196 (t1 - t0 > .5, floor/ceil hour buckets,
 *   bucket-span limit), files sorted as text lines (:218).
 * OTR_TILE_RULES_STREAM: the Java streaming path — Segment.valid (Segment.java:38-40) as
 *   BatchingProcessor.forward applies it (:119-126), TimeQuantisedTile.getTiles buckets
 *   (TimeQuantisedTile.java:26-35), files sorted by Segment.compareTo (numeric id,
 *   next_id; stable: arrival order within a pair) and written by
 *   Segment.appendToStringBuffer (Segment.java:59-74) as AnonymisingProcessor.store does. */
#define OTR_TILE_RULES_SIMPLE 0
#define OTR_TILE_RULES_STREAM 1

#define OTR_NO_ID 0xFFFFFFFFFFFFFFFFull

/* kernel_ms slots (OTR_STAGE_LINK: K_link, the per-state search inputs and the task records) */
enum { OTR_STAGE_STATES = 0, OTR_STAGE_CANDIDATES, OTR_STAGE_LINK, OTR_STAGE_ROUTE, OTR_STAGE_ROUTE_BIG,
       OTR_STAGE_VITERBI, OTR_STAGE_PATHS, OTR_STAGE_PATHS_BIG, OTR_STAGE_SEGMENTS, OTR_STAGE_HISTOGRAM,
       OTR_STAGE_TOTAL };
/* kernel_ms[OTR_VITERBI_VARIANT] is not a time: the host writes there, with or without
 * OTR_BATCH_TIMING, which k_viterbi instance the batch ran: 11 one trace per wave with the
 * predecessor scan split over the wave's halves (k_viterbi<1, true>: every mode keeps <= 32
 * candidates and the batch has fewer than OTR_VIT_SPLIT traces, default 8192), 20 two traces
 * per wave (k_viterbi<2>: <= 32 candidates, larger batches; OTR_VIT_SPLIT=0 selects it at any
 * size), 10 one trace per wave (k_viterbi<1>: some mode keeps more than 32 candidates).
 * (counters[15], the one counter word no kernel counts into, is pinned to 0 together with
 * every route_tier_* slot by tests/golden/route_tier_slots.json, so the code lives here.) */
#define OTR_VITERBI_VARIANT 15
#define OTR_HIST_BINS 8       /* speed bins of 20 km/h: [0,20) … [140,∞) */

/* All pointers below are owned by the matcher and stay valid until the next batch
 * call or otr_matcher_free.  Host arrays are filled only with OTR_BATCH_COPY_OUT;
 * the device histogram is always produced. */
typedef struct otr_batch_result {
  int32_t n_traces;
  int64_t n_probes;
  int64_t n_states;
  int64_t n_route;
  int64_t n_seg;
  int64_t n_rep;
  int64_t n_rows;              /* simple_reporter tile rows (after filter + hour fan-out) */
  int32_t status;              /* OTR_OK or first error */
  int32_t n_overflow_traces;   /* traces whose search exceeded the largest LDS table */
  /* host copies (OTR_BATCH_COPY_OUT) — same layout as oracle/oracle.h orc_result */
  int64_t* trace_state_off;  int64_t* state_probe;  int32_t* cand_count;
  uint32_t* cand_edge;  double* cand_p;  double* cand_sqd;   /* n_states * 64 slots */
  int32_t* winner;  int32_t* subpath;
  int64_t* trace_route_off;  uint32_t* route_edge;
  int64_t* trace_seg_off;  uint64_t* seg_id;  double* seg_start;  double* seg_end;
  int32_t* seg_length;  int32_t* seg_queue;  uint8_t* seg_internal;
  int32_t* seg_begin_shape;  int32_t* seg_end_shape;  int64_t* seg_way_off;  uint32_t* seg_way;
  int64_t* trace_rep_off;  uint64_t* rep_id;  uint64_t* rep_next;  double* rep_t0;  double* rep_t1;
  int32_t* rep_length;  int32_t* rep_queue;  int32_t* shape_used;  int32_t* stats;  double* stats_len;
  /* device outputs */
  uint32_t* d_hist;            /* [hist_hours][n_segments][OTR_HIST_BINS] observation counts */
  int64_t hist_len;            /* elements */
  /* algorithmic byte counters, summed over the batch */
  uint64_t counters[24];       /* algorithmic work counters: 0 cells visited,
                                  1 shape segments tested, 2 candidates, 3 settled nodes and
                                  4 relaxed edges (first-tier route launch), 5 search tasks,
                                  6 transition entries, 7 output segments, 8 tile rows,
                                  9/10 settled/relaxed of the large-table retry, 11/12 node
                                  searches resumed from / dumped to HBM (next retry table), 13 search rounds
                                  and 14 table keys (first-tier route launch),
                                  16-21 diagnostic-build search phase cycles, 22/23 edge-state
                                  searches resumed from / dumped to HBM (next table) */
  float kernel_ms[16];         /* OTR_BATCH_TIMING: device time per stage, OTR_STAGE_*;
                                  [OTR_VITERBI_VARIANT]: the k_viterbi instance code (always) */
  int32_t* trace_status;       /* host, per trace (with COPY_OUT / COPY_REPORTS): OTR_OK, or
                                  OTR_MATCH_ERROR when its search outgrew the largest LDS table */
  otr_tile_row* d_rows;        /* OTR_BATCH_TILE_ROWS: n_rows tile rows in HBM (matcher-owned),
                                  trace by trace in report order */
  /* per route-search kernel: slot 0 the first tier (k_route<160,2>), 1..5 the LDS retry
   * tiers in order, 6 / 7 the global-memory search (32K / 1M-state slabs), 8 the 64-bit
   * label LDS tier (steps whose length and time bits exceed 32), 10 the first edge-state
   * tier (modes with turn costs), 9 / 11 the larger edge-state tables (512, then 1024 states),
   * 12 the small-search first tier (k_route<80,4>: steps expected to stay small), 13 the
   * tiny-search first tier (k_route<40,8>: at most 8 targets, tinier still), 14..15 unused.
   * code: 6,000,000 + CAP*100 + targets of an edge-state tier, CAP*10+G of an LDS tier,
   * 900000 + CAP the 64-bit tier, -1 / -2 the global tiers, 0 unused (a tier with no task
   * kind to run: the node tiers when every mode has turn costs).
   * work: searches, settled nodes (expanded states), relaxed edges, transition entries
   * written.  ms (OTR_BATCH_TIMING): HIP-event time of the kernel on the matcher's stream. */
  int32_t route_tier_code[16];
  float route_tier_ms[16];
  uint64_t route_tier_work[16][4];
} otr_batch_result;

/* At most otr_max_batch_probes() = 2^26 - 64 (67,108,800) probes per call
 * (OTR_BAD_REQUEST beyond: split the input). */
int otr_match_batch(otr_matcher* m, const otr_trace_batch* in, otr_batch_result* out);

/* The batch limit and its reason: a kernel dispatch counts its work-items in 32 bits, and
 * the per-state / per-trace kernels give every state / trace a 64-lane wave.
 * otr_launch_max_items: the most work-items one of those launches dispatches for a batch
 * of n_states states and n_traces traces (states_per_wave 1 or 2: k_prep / k_tasks);
 * a batch of otr_max_batch_probes() probes stays below 2^32.  Host-only (no device). */
int64_t otr_max_batch_probes(void);
uint64_t otr_launch_max_items(int64_t n_states, int64_t n_traces, int32_t states_per_wave);

/* ---- matched points: where on the road every probe ended up --------
 * One entry per probe of the batch, in input order.  kind: OTR_POINT_STATE the probe of an
 * HMM state that has candidates and a winner (edge / frac: the winning candidate),
 * OTR_POINT_INTERPOLATED a probe between two such states of one sub-path (projected onto
 * the winner route between them, never moving backwards), OTR_POINT_UNMATCHED everything
 * else (edge 0xFFFFFFFF, state and pos_mm -1, the rest 0).  frac: fraction of the edge's
 * length; lat / lon: the snapped coordinate; dist: metres from the probe to it; state: index
 * of the (preceding) state in the batch's state arrays; pos_mm: position along the matched
 * route from the start of the sub-path, whole millimetres.
 * Refers to the matcher's last otr_match_batch, which must have set
 * OTR_BATCH_MATCHED_POINTS (OTR_BAD_REQUEST otherwise, or when there was no batch).  The
 * pointers are owned by the matcher and stay valid until its next batch call; the host
 * arrays are filled only when that batch also set OTR_BATCH_COPY_OUT. */
#define OTR_POINT_UNMATCHED 0
#define OTR_POINT_STATE 1
#define OTR_POINT_INTERPOLATED 2

typedef struct otr_point_result {
  int64_t n_probes;
  float kernel_ms;             /* OTR_BATCH_TIMING: device time of K12 */
  int32_t reserved;
  /* host (OTR_BATCH_COPY_OUT) */
  uint8_t* kind;  uint32_t* edge;  double* frac;  double* lat;
  double* lon;  double* dist;  int64_t* state;  int64_t* pos_mm;
  /* device, always */
  uint8_t* d_kind;  uint32_t* d_edge;  double* d_frac;  double* d_lat;
  double* d_lon;  double* d_dist;  int64_t* d_state;  int64_t* d_pos_mm;
} otr_point_result;

int otr_matched_points(otr_matcher* m, otr_point_result* out);

/* ---- edge traversals: when the vehicle entered and left each edge --
 * One entry per edge portion of the matched route, densely, trace by trace: trace t owns
 * entries trace_off[t] .. trace_off[t+1]-1 (trace_off has n_traces + 1 elements), and their
 * edges are the trace's route_edge entries without the 0xFFFFFFFF separators, in order.
 * edge / way: the edge and its way id; seg_id: the OSMLR id of the edge's segment or
 * OTR_NO_ID; first_state: batch index of the first state of the entry's sub-path (entries
 * of one sub-path share it); f0 / f1: fractions of the edge's length where the traversal
 * starts and ends (0 and 1 except at the two ends of a sub-path); s0_mm / s1_mm: the same
 * places as positions along the sub-path's route, whole millimetres (an entry's s1 is its
 * successor's s0; s0 == s1 occurs and is kept); t_enter / t_exit: epoch seconds, linear in
 * route position between the states around the place, always filled.  A sub-path with one
 * state has no entry.
 * The entries of a trace whose trace_status is not OTR_OK are what its route and segments
 * are: left over from a search that gave up, in bounds but without meaning; skip them.
 * Refers to the matcher's last otr_match_batch, which must have set
 * OTR_BATCH_EDGE_TRAVERSALS (OTR_BAD_REQUEST otherwise, or when there was no batch).  The
 * pointers are owned by the matcher and stay valid until its next batch call; the host
 * arrays are filled only when that batch also set OTR_BATCH_COPY_OUT (NULL otherwise).  An
 * empty batch has n_traversals 0 and a trace_off of one zero. */
typedef struct otr_traversal_result {
  int64_t n_traversals;
  int64_t n_traces;
  float kernel_ms;             /* OTR_BATCH_TIMING: device time of K13 (count, offsets, fill) */
  int32_t reserved;
  /* host (OTR_BATCH_COPY_OUT) */
  int64_t* trace_off;  uint32_t* edge;  uint32_t* way;  uint64_t* seg_id;  int64_t* first_state;
  double* f0;  double* f1;  int64_t* s0_mm;  int64_t* s1_mm;  double* t_enter;  double* t_exit;
  /* device, always */
  int64_t* d_trace_off;  uint32_t* d_edge;  uint32_t* d_way;  uint64_t* d_seg_id;  int64_t* d_first_state;
  double* d_f0;  double* d_f1;  int64_t* d_s0_mm;  int64_t* d_s1_mm;  double* d_t_enter;  double* d_t_exit;
} otr_traversal_result;

int otr_edge_traversals(otr_matcher* m, otr_traversal_result* out);

/* simple_reporter's tile stage (simple_reporter.py:211-239) on device: sort the rows
 * by file, then in the line order of segments.sort() (:218, string order of the whole
 * line), and delete the (id, next_id) runs seen fewer than `privacy` times with the
 * reference loop's exact rule (:221-239, including its trailing-singleton quirk).
 * With rules = OTR_TILE_RULES_STREAM the order is Segment.compareTo's instead and the
 * cull is AnonymisingProcessor.clean (AnonymisingProcessor.java:155-175, same rule).
 * rows: n rows in host (OTR_MEM_HOST) or device (OTR_MEM_DEVICE) memory, e.g. the
 * d_rows of a batch or rows received from other GPUs.  *out: the kept rows, sorted,
 * in host memory owned by the matcher (valid until its next call). */
int otr_tiles_cull(otr_matcher* m, const otr_tile_row* rows, int64_t n, int32_t memory, int32_t privacy,
                   int32_t rules, const otr_tile_row** out, int64_t* n_out);

/* ---- keyed speed histogram -------------------------------------------
 * One entry per (hour-tile file, segment pair, speed bin) with its observation count:
 * the per-GPU histogram is the tile rows sort-reduced by that key; GPUs exchange entries
 * with the rank owning their (hour, tile) file (RCCL all-to-all, simple_reporter.
 * file_owner) and each owner reduces what it received and applies the privacy cull to
 * complete pairs (a pair's total count over its bins >= privacy; the reference cull's
 * trailing-singleton rule belongs to the line-based tile files, otr_tiles_cull). */
typedef struct otr_hist_entry {
  uint64_t file;       /* bucket << 25 | level << 22 | tile index, as otr_tile_row.file */
  uint64_t id;
  uint64_t next_id;    /* or OTR_INVALID_SEGMENT_ID */
  uint32_t speed_bin;  /* 20 km/h bins 0..7 */
  uint32_t count;
} otr_hist_entry;

/* Sort-reduce n entries (in: host or device memory) by (file, id, next_id, speed_bin),
 * summing counts; with privacy > 1 also drop the (file, id, next_id) pairs whose total
 * count is below privacy.  The reduced entries, in key order, are copied to `out`
 * (out_memory: host or device; room for out_cap entries, n suffices) and *n_out is
 * their number.  rows_in != 0: the input is n tile rows, count 1 each; rows read back from
 * tile file texts (otr_tiles_parse) carry speed_bin -1 and have no place in a speed histogram:
 * they would all land in the one bin 0xFFFFFFFF. */
int otr_hist_reduce(otr_matcher* m, const void* in, int64_t n, int32_t memory, int32_t rows_in, int32_t privacy,
                    otr_hist_entry* out, int64_t out_cap, int32_t out_memory, int64_t* n_out);

/* Per-edge speed entries of the edge traversals (otr_edge_traversals above), in HBM, in
 * traversal order: one otr_hist_entry per complete traversal (f0 == 0 and f1 == 1) that
 * took more than half a second: file = (floor(t_enter) / quantisation) << 25 | road level << 22 (tile index 0),
 * id the edge, next_id the edge of the next traversal of the same sub-path or
 * OTR_INVALID_SEGMENT_ID, speed_bin from (s1_mm - s0_mm) and t_exit - t_enter in 20 km/h
 * steps (7 at most), count 1.  quantisation <= 0 means 3600.  *d_entries is owned by the
 * matcher until its next batch or otr_edge_observations call and can be handed to
 * otr_hist_reduce(m, *d_entries, *n, OTR_MEM_DEVICE, 0, ...) as it is.  Same errors as
 * otr_edge_traversals. */
int otr_edge_observations(otr_matcher* m, int32_t quantisation, otr_hist_entry** d_entries, int64_t* n);

/* The CSV lines of n (host) rows in order.  OTR_TILE_RULES_SIMPLE: "id,next,duration,1,
 * length,queue,start,end,source,MODE\n" each (simple_reporter.py:188-195).
 * OTR_TILE_RULES_STREAM: "\nid,[next],duration,1,length,queue,start,end,source,MODE"
 * each, next empty when invalid (Segment.java:59-74).  mode is upper-cased as both do. */
int otr_tiles_format(const otr_tile_row* rows, int64_t n, const char* source, const char* mode, int32_t rules,
                     char** out, size_t* out_len);

/* ---- graph building (§8 f rank 1) -------------------------------------------------------
 * Tile hierarchy of the reference's py/get_tiles.py:30-102 (Valhalla baldr): levels 0/1/2
 * tile the world with 4 / 1 / 0.25 degree tiles, tile id = row * ncolumns + col.
 *   otr_tilehier_row / otr_tilehier_col: Tiles.Row / Tiles.Col (:51-72), -1 outside the world.
 *   otr_tilehier_file: Tiles.GetFile (:81-102), e.g. level 2, id 745313, "gph" ->
 *     "2/000/745/313.gph"; out gets the NUL-terminated name (cap bytes of room).
 *   otr_tilehier_files: the script's listing (:132-171) for a bbox — split at the
 *     antimeridian, levels 0, 1, 2 (Python 2 dict order), rows then columns — as
 *     newline-terminated names in *out (release with otr_free). */
int32_t otr_tilehier_row(int32_t level, double lat);
int32_t otr_tilehier_col(int32_t level, double lon);
int otr_tilehier_file(int32_t level, int64_t tile_id, const char* suffix, char* out, size_t cap);
int otr_tilehier_files(double min_lon, double min_lat, double max_lon, double max_lat, const char* suffix, char** out,
                   size_t* out_len);

/* The flattener: decoded road-graph arrays (what a Valhalla GraphTile reader yields for
 * the tiles otr_tilehier_files lists: nodes, directed edges, edge shapes, way ids, OSMLR
 * associations) -> the .otrg file otr_configure uploads (include/otr_graph_format.h).
 * Edges may come in any order; the file's edges are sorted by (src, dst), stable.
 * Edges shorter than 5 cm are contracted (their end nodes merge into the smallest node
 * id; DESIGN.md §3.4: shorter edges only narrow the exact search rounds); a
 * contracted edge's OSMLR begin/end flag moves to its segment's neighbouring edge.
 * Routing lengths are the shapes' lengths.  Decoding the .gph binary itself needs
 * Valhalla 2.3.6's GraphTile layout (UPSTREAM, absent here): out of scope. */
typedef struct otr_flat_graph {
  uint32_t n_nodes;
  const int32_t* node_ll;      /* [2*n_nodes] lat_e6, lon_e6 */
  uint32_t n_edges;
  const uint32_t* edge_src;    /* node index */
  const uint32_t* edge_dst;
  const uint32_t* edge_attr;   /* OTR_ATTR_* fields of otr_graph_format.h (access, speed, level,
                                  internal, OSMLR segment begin / end) */
  const uint32_t* edge_seg;    /* OSMLR segment index into seg_id, OTR_NO_SEGMENT; may be NULL */
  const uint32_t* edge_way;    /* OSM way id (low 32 bits); may be NULL */
  const uint32_t* shape_off;   /* [n_edges+1] into shape_ll; a shape holds both end nodes */
  const int32_t* shape_ll;     /* lat_e6, lon_e6 pairs */
  uint32_t n_segments;
  const uint64_t* seg_id;      /* OSMLR ids: level(3) | tile(22) | index(21) */
  const uint32_t* seg_len;     /* whole metres */
  double cell_deg;             /* candidate grid cell (degrees); 0 = 0.0005 (meili's 500 per tile) */
} otr_flat_graph;

typedef struct otr_flat_stats {
  uint32_t n_nodes, n_edges;          /* written */
  uint32_t n_contracted_edges;        /* edges < 5 cm (and edges inside merged clusters) */
  uint32_t n_merged_nodes;
} otr_flat_stats;

int otr_flatten(const otr_flat_graph* in, const char* out_path, otr_flat_stats* stats);

/* ---- ingest: probe text → windowed traces in HBM (§8 f rank 4) -------------------------
 * OTR_INGEST_SHARD: the "uuid,time,lat,lon,acc" lines simple_reporter.match() reads
 *   (simple_reporter.py:140-160): line.strip().split(',') into exactly 5 fields,
 *   float() coordinates, int() time and accuracy.
 * OTR_INGEST_RAW: the raw feed simple_reporter.download() reads (:99-111) followed by the
 *   shard round trip into match(): fields by index after splitting on `separator`, the
 *   bbox filter (applied before time and accuracy are parsed, as :103-105), the fast
 *   "%Y-%m-%d %H:%M:%S" time (:106-107) or epoch seconds, accuracy min(ceil(x), 1000)
 *   (:110), and coordinates as match() re-reads them from the Python 2 str() text
 *   (12 significant digits, :111).
 * OTR_INGEST_JAVA_SV: Formatter.formatSV (Formatter.java:103-114): float32 coordinates,
 *   (int)ceil accuracy, Long.parseLong or "yyyy-MM-dd HH:mm:ss" time.
 * Then, for every rule: points grouped by uuid, sorted by time (stable), split at gaps
 *   > inactivity seconds, windows of fewer than 2 points dropped (:146-160).  Traces come
 *   out in order of the first appearance of their uuid, then by time. */
#define OTR_INGEST_SHARD 0
#define OTR_INGEST_RAW 1
#define OTR_INGEST_JAVA_SV 2
#define OTR_TIME_EPOCH 0
#define OTR_TIME_YMDHMS 1
/* bad_reason: why the first rejected line (bad_line) was rejected */
#define OTR_INGEST_E_FIELDS 1     /* wrong field count / index out of range (ValueError, IndexError) */
#define OTR_INGEST_E_FLOAT 2      /* coordinate not a finite decimal number */
#define OTR_INGEST_E_INT 3        /* time or accuracy not an integer (int()) */
#define OTR_INGEST_E_TIME 4       /* date fields out of range (datetime.date) */
#define OTR_INGEST_E_UUID 5       /* uuid holds the shard separator ',' */
#define OTR_INGEST_E_PRECISION 6  /* > 19 significant digits whose rounding needs big-number arithmetic */
#define OTR_INGEST_E_COLLISION 7  /* two uuids share a 64-bit hash (never seen; refused rather than merged) */
#define OTR_INGEST_E_ACCURACY 8   /* accuracy not finite or beyond ±2^24 */

typedef struct otr_ingest_format {
  int32_t rules;          /* OTR_INGEST_* */
  int32_t separator;      /* field separator byte: ',' (SHARD, fixed), '|' (raw feed) */
  int32_t uuid_index, time_index, lat_index, lon_index, accuracy_index;  /* RAW / JAVA_SV */
  int32_t time_format;    /* OTR_TIME_* (RAW / JAVA_SV) */
  int32_t inactivity;     /* seconds (--inactivity, 120) */
  int32_t mode;           /* 0 auto, 1 bicycle, 2 pedestrian: the batch's mode (--mode) */
  int32_t use_bbox;       /* RAW: apply bbox */
  int32_t reserved;
  double bbox[4];         /* min lat, min lon, max lat, max lon (--bbox) */
} otr_ingest_format;

typedef struct otr_ingest_result {
  int64_t n_lines;        /* lines in the text */
  int64_t n_kept;         /* lines inside the bbox */
  int64_t n_probes;       /* probes in windows of >= 2 points */
  int32_t n_traces;       /* windows */
  int32_t n_uuids;
  int64_t bad_line;       /* first rejected line (0-based), -1 if none */
  int32_t bad_reason;     /* OTR_INGEST_E_* */
  float parse_ms;         /* device time of the line parse kernel (HIP events on the matcher's stream) */
  float total_ms;         /* device time from the first kernel to the last (host syncs between included) */
  int32_t reserved;
  otr_trace_batch batch;  /* memory = OTR_MEM_DEVICE: offsets, lat, lon, time, accuracy, mode in HBM
                             (matcher-owned, valid until its next otr_ingest); levels/flags zero */
  const int64_t* d_trace_uuid_off;  /* per trace: byte offset of its uuid in the text */
  const int32_t* d_trace_uuid_len;
} otr_ingest_result;

/* Parse `len` bytes of probe lines (host or device memory) into traces in HBM.  Returns
 * OTR_OK, or OTR_BAD_REQUEST with bad_line / bad_reason set where the reference raises
 * (the whole text is refused, as the reference loses the file).  The batch can be
 * passed straight to otr_match_batch after setting its levels, threshold and flags. */
int otr_ingest(otr_matcher* m, const char* text, int64_t len, int32_t memory, const otr_ingest_format* fmt,
               otr_ingest_result* out);

/* ---- session store: the streaming reporter's per-key state ----
 * What BatchingProcessor.java:58-106 and Batch.java:43-90 keep per uuid, in HBM: a session
 * of points per 64-bit key, the report gate (max separation from the first point, point
 * count, elapsed time), the trim by the report's shape_used and the eviction of sessions
 * that went quiet.  One store per matcher.  max_points bounds a session (the reference's
 * lists are unbounded): a session that reaches it after an append is reported as at
 * eviction (n >= 2 and a non-negative elapsed time; counted in n_forced) or, failing that,
 * cleared (n_dropped).  Keys have no String order: evictions go by ascending key value. */
typedef struct otr_session_config {
  int32_t max_sessions;        /* live sessions at a time; the key table has twice as many entries */
  int32_t max_points;          /* per session, >= 2 */
  float report_dist;           /* metres, 500 (compared with the float max separation) */
  int32_t report_count;        /* points, 10 */
  int64_t report_time;         /* 60, units of time */
  int64_t session_gap;         /* 60000, units of timestamp */
  int32_t mode;                /* 0 auto, 1 bicycle, 2 pedestrian: every report's mode */
  uint32_t report_levels;      /* bit masks as in otr_trace_batch */
  uint32_t transition_levels;
  int32_t threshold_sec;
  int64_t batch_probes;        /* most probes per device batch of a round; <= 0: otr_max_batch_probes() */
} otr_session_config;

/* Keyed points in arrival order, host or device memory.  Key OTR_NO_ID is refused. */
typedef struct otr_session_points {
  int64_t n;
  int32_t memory;              /* OTR_MEM_HOST or OTR_MEM_DEVICE */
  int32_t reserved;
  const uint64_t* key;
  const float* lat;            /* Point.java:15-17: float coordinates, int accuracy, long time */
  const float* lon;
  const int32_t* accuracy;
  const int64_t* time;
  const int64_t* timestamp;    /* the record's stream time (session_gap's units) */
} otr_session_points;

/* What Batch.report hands to BatchingProcessor.forward, for every window of a call.
 * Windows come in round order (a key's next window needs its previous trim), within a
 * round by ascending trigger; the reference's forward order is ascending trigger over the
 * whole chunk: sort by it to get that.  trigger: the arrival index, in the pushed chunk, of
 * the point that tripped the gate, or -1 - rank for the eviction of rank `rank` in key
 * order.  shape_used: -1 when the report has none (K7's 0 included) or the trace failed;
 * status: the trace's OTR_OK / OTR_MATCH_ERROR; trimmed: points dropped from the session's
 * front; window w owns reports rep_off[w] .. rep_off[w+1]-1 (rep_off has n_windows + 1
 * elements; a failed trace has none).  All pointers are owned by the matcher and stay
 * valid until its next session call; host and device arrays are both filled.
 * n_forced / n_dropped count this call; n_rebuilds counts the key table's rebuilds since
 * otr_sessions_open; n_live is the number of sessions after the call. */
typedef struct otr_session_result {
  int64_t n_windows;
  int64_t n_reports;
  int32_t n_rounds;
  int32_t n_live;
  int32_t n_forced;
  int32_t n_dropped;
  int32_t n_evicted;           /* punctuate: sessions deleted, reporting or not */
  int32_t n_rebuilds;
  float device_ms;             /* HIP-event time from the call's first kernel to its last */
  float match_ms;              /* host wall time of the matcher's batches inside the call */
  /* host */
  uint64_t* key;  int64_t* trigger;  int32_t* n_points;  int32_t* shape_used;  int32_t* status;
  int32_t* trimmed;  int64_t* rep_off;
  uint64_t* id;  uint64_t* next_id;  double* t0;  double* t1;  int32_t* length;  int32_t* queue_length;
  /* device */
  uint64_t* d_key;  int64_t* d_trigger;  int32_t* d_n_points;  int32_t* d_shape_used;  int32_t* d_status;
  int32_t* d_trimmed;  int64_t* d_rep_off;
  uint64_t* d_id;  uint64_t* d_next_id;  double* d_t0;  double* d_t1;  int32_t* d_length;  int32_t* d_queue_length;
} otr_session_result;

/* Every live session in ascending key order (the content of Batch.Serder): session i owns
 * points point_off[i] .. point_off[i+1]-1.  Host arrays owned by the matcher, valid until
 * its next session call. */
typedef struct otr_session_snapshot {
  int64_t n_sessions;
  int64_t n_points;
  uint64_t* key;  int64_t* point_off;  float* max_sep;  int64_t* last_update;
  float* lat;  float* lon;  int32_t* accuracy;  int64_t* time;
} otr_session_snapshot;

/* Opens the matcher's store (OTR_BAD_REQUEST when it has one, or for a config out of
 * range; OTR_DEVICE_ERROR naming the buffer when it does not fit the device). */
int otr_sessions_open(otr_matcher* m, const otr_session_config* cfg);
int otr_sessions_close(otr_matcher* m);

/* BatchingProcessor.process over a chunk of points: every key's points are appended one by
 * one; the keys whose gate passed are matched as one device batch (several beyond
 * batch_probes), trimmed, and the chunk goes on after the trigger points, round by round,
 * to its end.  Any chunking of one arrival stream gives the same windows.  A chunk that
 * would take the live sessions beyond max_sessions is refused with OTR_BAD_REQUEST and
 * the store untouched. */
int otr_sessions_push(otr_matcher* m, const otr_session_points* pts, otr_session_result* out);

/* BatchingProcessor.punctuate: every session with ts - last_update > session_gap is deleted
 * and, when it holds n >= 2 points with a non-negative elapsed time, reported. */
int otr_sessions_punctuate(otr_matcher* m, int64_t ts, otr_session_result* out);

/* The two halves of a round, for callers with their own matching policy.  Advance takes a
 * new chunk (pts) or continues the current one (pts NULL) and leaves the tripped windows
 * as a batch in HBM (memory OTR_MEM_DEVICE, levels and threshold from the config; owned by
 * the matcher until the commit); n_traces == 0: the chunk is consumed.  Commit takes one
 * shape_used and one trace status per window (host or device memory) and trims.
 * otr_sessions_windows describes the windows of the last advance (after the commit also
 * shape_used, status and trimmed; no reports). */
int otr_sessions_advance(otr_matcher* m, const otr_session_points* pts, otr_trace_batch* out);
int otr_sessions_commit(otr_matcher* m, const int32_t* shape_used, const int32_t* status, int32_t memory);
int otr_sessions_windows(otr_matcher* m, otr_session_result* out);

int otr_sessions_snapshot(otr_matcher* m, otr_session_snapshot* out);

/* ---- restore, export and move -----------------------------------
 * Sessions as the values Batch.Serder writes (Batch.java:110-116, Point.java:50-55), big-endian:
 * int32 count, float max_separation, int64 last_update, then count x (float lat, float lon,
 * int32 accuracy, int64 time): 16 + 20*count bytes.  Record i is bytes[rec_off[i] .. rec_off[i+1]);
 * bytes may start at any address and records at any offset.  key[i] is the 64-bit key of the
 * record's uuid: otr_uuid_key over the changelog key's UTF-8 bytes.  On a store with the uuid
 * directory the changelog key of record i itself is entry i of otr_sessions_names after the
 * export. */
typedef struct otr_session_records {
  int64_t n_records;  int64_t n_bytes;
  int32_t memory;     int32_t reserved;        /* OTR_MEM_HOST / OTR_MEM_DEVICE (input) */
  const uint64_t* key;  const int64_t* rec_off;  const uint8_t* bytes;
  /* export only: the same three arrays in HBM */
  const uint64_t* d_key;  const int64_t* d_rec_off;  const uint8_t* d_bytes;
} otr_session_records;

/* Why a restore is refused; where a session has several reasons the lowest value is reported. */
#define OTR_RESTORE_E_LAYOUT 1     /* snapshot: point_off[0] != 0, not non-decreasing, or its last value is not
                                      n_points.  Records: offsets not non-decreasing or beyond n_bytes, a record
                                      shorter than 16 bytes or not 16 + 20*count long (64-bit; count < 0 too) */
#define OTR_RESTORE_E_KEY 2        /* the key is OTR_NO_ID */
#define OTR_RESTORE_E_COUNT 3      /* count outside 1 .. max_points - 1 */
#define OTR_RESTORE_E_DUPLICATE 4  /* not the first occurrence of its key in the input */
#define OTR_RESTORE_E_LIVE 5       /* the key has a live session in the store */
#define OTR_RESTORE_E_FULL 6       /* live + given > max_sessions (bad_session -1) */

typedef struct otr_session_restore_result {
  int64_t n_sessions, n_points;   /* restored by this call */
  int64_t bad_session;            /* lowest refused index, -1: none (or the refusal is of the whole input) */
  int32_t bad_reason;             /* OTR_RESTORE_E_*, 0 when restored */
  int32_t n_live;                 /* after the call */
  float device_ms;  int32_t reserved;
} otr_session_restore_result;

/* Merges the given sessions into the open store (it does not replace it).  max_sep and
 * last_update are taken as stored, by bits, never recomputed (what the deserialiser does).
 * All or nothing: on any refusal the call returns OTR_BAD_REQUEST with bad_session / bad_reason
 * filled and the store untouched.  bad_session is the lowest index with any per-session reason;
 * OTR_RESTORE_E_FULL is reported only when no session has one.  A count of 0 is refused because
 * the reference never stores an empty Batch (BatchingProcessor.java:77), a count of max_points
 * because a live session never holds that many after a call.  A key that was deleted from
 * the store earlier is restorable.  Refused too (bad_session -1, bad_reason 0): no store, or an
 * advance / commit sequence or a chunk open.  memory: where the snapshot's arrays are. */
int otr_sessions_restore(otr_matcher* m, const otr_session_snapshot* snap, int32_t memory,
                         otr_session_restore_result* out);
int otr_sessions_restore_records(otr_matcher* m, const otr_session_records* recs, otr_session_restore_result* out);

/* Every live session in ascending key order as records, in host memory and in HBM (memory is
 * set to OTR_MEM_HOST).  The arrays are owned by the matcher and valid until its next session
 * call. */
int otr_sessions_export_records(otr_matcher* m, otr_session_records* out);

/* The sessions with key % n_parts == part, in ascending key order and the layout of the
 * snapshot.  The keys are K11's mixed 64-bit hash already, so the remainder spreads them evenly:
 * this is the shard rule of the uuid-sharded layout.  remove != 0 also deletes them
 * exactly as an eviction does (no report is made).  n_parts 1, part 0, remove 0 is the snapshot.
 * Refused while an advance / commit sequence or a chunk is open. */
int otr_sessions_take(otr_matcher* m, int32_t n_parts, int32_t part, int32_t remove, otr_session_snapshot* out);

/* K11's 64-bit hash of a uuid's bytes, on the host: the key of a changelog record. */
uint64_t otr_uuid_key(const char* uuid, int64_t len);

/* ---- uuid directory: the name of every live session --------------
 * The reference's store is KeyValueStore<String, Batch> (BatchingProcessor.java:21,47); ours is
 * keyed by a 64-bit hash.  A store opened with otr_sessions_open_named also keeps, in HBM and per
 * session slot, the uuid bytes of every live session (max_sessions x round_up(uuid_bytes, 16)
 * bytes and a length each).  Every point then comes with a name: a key that is live under another
 * name (two uuids sharing a hash) is refused instead of merged, snapshots, takes and exports list
 * the names (a record's changelog key is entry i of that list), restores bring them back, and
 * otr_sessions_punctuate evicts in ascending name order (unsigned bytes, a proper prefix first,
 * ties by key; trigger = -1 - rank in that order): String order for ASCII uuids, UTF-8 byte order
 * otherwise.  The store does not check key == otr_uuid_key(name): keying is the caller's choice,
 * the directory demands one name per live key.  A name belongs to a live session only: once the
 * session is deleted its key may come back under another name.  uuid_bytes: 1 .. 255, the
 * longest name (OTR_BAD_REQUEST outside that range).  A store opened with otr_sessions_open has
 * no directory and refuses the _named calls; a store with one refuses otr_sessions_push,
 * otr_sessions_advance with points, otr_sessions_restore and otr_sessions_restore_records. */
int otr_sessions_open_named(otr_matcher* m, const otr_session_config* cfg, int32_t uuid_bytes);

/* One name per point or per session, in the same memory as the arrays it goes with: name i is
 * bytes[off[i] .. off[i] + len[i]).  No byte outside [bytes, bytes + n_bytes) is read. */
typedef struct otr_session_names {
  const uint8_t* bytes;  int64_t n_bytes;
  const int64_t* off;  const int32_t* len;
} otr_session_names;

/* Why a named chunk is refused.  The refusal is that of the lowest arrival index with any reason
 * and, at that point, of the lowest value.  It comes after the chunk's own refusals (OTR_NO_ID,
 * max_sessions) and like them leaves the store and the directory untouched. */
#define OTR_NAME_E_LONG 1        /* len > uuid_bytes (0 is a valid length) */
#define OTR_NAME_E_COLLISION 2   /* the key's live session has another name (length or any byte), or the
                                    key is new in the chunk and its first-arriving point has another */
#define OTR_NAME_E_LAYOUT 3      /* off < 0, len < 0 or off + len > n_bytes */

typedef struct otr_session_name_refusal {
  int64_t point;      /* arrival index in the chunk, -1: the last named call was not refused for a name */
  int64_t message;    /* otr_sessions_push_text: the arrival index of the point's message; else -1 */
  int32_t reason;     /* OTR_NAME_E_*, 0: none */
  int32_t reserved;
} otr_session_name_refusal;

/* otr_sessions_push / otr_sessions_advance (pts non-NULL; a chunk is continued with
 * otr_sessions_advance and NULL) on a store with a directory.  An accepted chunk stores the name
 * of every key it created: that of the key's first-arriving point. */
int otr_sessions_push_named(otr_matcher* m, const otr_session_points* pts, const otr_session_names* names,
                            otr_session_result* out);
int otr_sessions_advance_named(otr_matcher* m, const otr_session_points* pts, const otr_session_names* names,
                               otr_trace_batch* out);
int otr_sessions_last_refusal(otr_matcher* m, otr_session_name_refusal* out);

/* The names of exactly the sessions of the matcher's last otr_sessions_snapshot, otr_sessions_take
 * (gathered before a removal) or otr_sessions_export_records, in that listing's order: name i is
 * bytes[off[i] .. off[i+1]).  Host and device arrays owned by the matcher, valid until its next
 * session call; refused without a directory or without such a listing. */
typedef struct otr_session_name_list {
  int64_t n;  int64_t n_bytes;
  const int64_t* off;  const uint8_t* bytes;      /* host: off has n + 1 elements */
  const int64_t* d_off;  const uint8_t* d_bytes;  /* the same in HBM */
} otr_session_name_list;
int otr_sessions_names(otr_matcher* m, otr_session_name_list* out);

/* otr_sessions_restore / otr_sessions_restore_records with one name per session (names in the
 * memory of the sessions), on a store with a directory.  One more per-session reason, last in
 * the order.  Names are stored as given. */
#define OTR_RESTORE_E_NAME 7       /* the name's layout (as OTR_NAME_E_LAYOUT) or len > uuid_bytes */
int otr_sessions_restore_named(otr_matcher* m, const otr_session_snapshot* snap, const otr_session_names* names,
                               int32_t memory, otr_session_restore_result* out);
int otr_sessions_restore_records_named(otr_matcher* m, const otr_session_records* recs,
                                       const otr_session_names* names, otr_session_restore_result* out);

/* ---- stream formatter: raw messages → keyed points in HBM -------
 * What KeyedFormattingProcessor.java:32-43 does with Formatter.formatSV / formatJSON: every
 * message ends as a point (kept), is dropped (the reference certainly throws and the
 * processor logs and goes on), or is unsupported (the reference would, or might, produce a
 * point that cannot be reproduced here without a JVM: never approximated, counted apart).
 * A message's status is 0 or its reason; reasons below OTR_FORMAT_UNSUPPORTED are drops.
 * Over a message any drop beats any unsupported reading; within a class the first in the
 * reference's evaluation order (lat, lon, time, accuracy, uuid) is reported.  The key of a
 * point is K11's 64-bit hash of the uuid bytes. */
#define OTR_FORMAT_SV   0   /* Formatter.formatSV   (Formatter.java:97-109)  */
#define OTR_FORMAT_JSON 1   /* Formatter.formatJSON (Formatter.java:111-124) */
#define OTR_FORMAT_D_FIELDS 1     /* SV: a needed field index beyond what String.split leaves */
#define OTR_FORMAT_D_FLOAT 2      /* coordinate text not a finite decimal number */
#define OTR_FORMAT_D_INT 3        /* time text not an integer (Long.parseLong, the pattern's pieces) */
#define OTR_FORMAT_D_TIME 4       /* date fields out of range; JSON: a number where the pattern needs text */
#define OTR_FORMAT_D_ACCURACY 5   /* SV: accuracy not a decimal number */
#define OTR_FORMAT_D_JSON 6       /* not one RFC 8259 value */
#define OTR_FORMAT_D_ROOT 7       /* the JSON value is not an object */
#define OTR_FORMAT_D_MISSING 8    /* a needed key is missing */
#define OTR_FORMAT_UNSUPPORTED 32
#define OTR_FORMAT_U_PRECISION 32 /* > 19 significant digits whose rounding needs big-number arithmetic */
#define OTR_FORMAT_U_ACCURACY 33  /* accuracy not finite or beyond ±2^24 */
#define OTR_FORMAT_U_DEPTH 34     /* JSON nested deeper than 64 */
#define OTR_FORMAT_U_TRAILING 35  /* non-whitespace after the JSON value */
#define OTR_FORMAT_U_ESCAPE 36    /* a backslash in a top-level key or in a needed string */
#define OTR_FORMAT_U_NUMBER 37    /* a number token the reference prints or reads in a way not pinned here */
#define OTR_FORMAT_U_KIND 38      /* a needed value of a kind whose reading is not pinned here */
#define OTR_FORMAT_U_NO_ID 39     /* the uuid hashes to OTR_NO_ID */

typedef struct otr_message_format {
  int32_t type;            /* OTR_FORMAT_* */
  int32_t separator;       /* SV: one byte */
  int32_t uuid_index, time_index, lat_index, lon_index, accuracy_index;   /* SV */
  int32_t time_format;     /* OTR_TIME_EPOCH | OTR_TIME_YMDHMS ("yyyy-MM-dd HH:mm:ss", UTC) */
  const char *uuid_key, *lat_key, *lon_key, *time_key, *accuracy_key;     /* JSON: 1..64 bytes, no '"', no '\\' */
} otr_message_format;

typedef struct otr_messages {
  const char* text;  int64_t len;  int32_t memory;  int32_t reserved;
  const int64_t* msg_off;   /* NULL: messages are the '\n'-separated lines of text (K11's line rule:
                               a final fragment counts); else n_messages+1 ascending byte offsets,
                               same memory as text */
  int64_t n_messages;       /* with msg_off */
  const int64_t* timestamp; /* per message, same memory as text; NULL: timestamp_all for every message */
  int64_t timestamp_all;
} otr_messages;

/* points: the kept messages in arrival order, memory == OTR_MEM_DEVICE; d_message: per point
 * the arrival index of its message (a session window's trigger maps back through it);
 * d_uuid_off / d_uuid_len: per point, its uuid in the text; d_status: per message.  All of it
 * is owned by the matcher and valid until its next formatter call (it survives an
 * otr_sessions_push that consumes it). */
typedef struct otr_format_result {
  int64_t n_messages;
  int64_t n_points;
  int64_t n_dropped;
  int64_t n_unsupported;
  int64_t first_bad;          /* first message dropped or unsupported, -1 if none */
  int32_t first_bad_reason;   /* OTR_FORMAT_D_* / OTR_FORMAT_U_* */
  float parse_ms;             /* device time of k_format_parse (HIP events on the matcher's stream) */
  float total_ms;             /* from the first kernel to the last (host syncs between included) */
  int32_t reserved;
  otr_session_points points;
  const int64_t* d_message;
  const int64_t* d_uuid_off;
  const int32_t* d_uuid_len;
  const int32_t* d_status;
} otr_format_result;

/* Text → keyed points in HBM.  OTR_BAD_REQUEST, nothing changed: a bad format struct, a key
 * out of range, offsets that do not ascend, text or message count beyond otr_ingest's
 * limits, or two different uuids of the chunk sharing a hash (first_bad set, reason
 * OTR_INGEST_E_COLLISION).  Everything else is decided per message. */
int otr_format_messages(otr_matcher* m, const otr_message_format* fmt, const otr_messages* msgs,
                        otr_format_result* out);

/* The same, then otr_sessions_push of those device points: no point crosses to the host in
 * between.  Refusals are those of otr_sessions_push plus the formatter's own. */
int otr_sessions_push_text(otr_matcher* m, const otr_message_format* fmt, const otr_messages* msgs,
                           otr_format_result* fmt_out, otr_session_result* session_out);

/* ---- tile store: the streaming reporter's anonymiser stage ------
 * What sits between BatchingProcessor.forward (BatchingProcessor.java:108-141) and the tile
 * files of AnonymisingProcessor.process / punctuate (AnonymisingProcessor.java:119-175,
 * 222-266), in HBM: reports that pass Segment.valid are fanned out over their time buckets
 * (TimeQuantisedTile.java:26-35) into OTR_TILE_RULES_STREAM rows, exactly the rows
 * otr_match_batch writes with OTR_BATCH_TILE_ROWS, kept in arrival order across any number
 * of adds, and only the flush sorts every (bucket, tile) file by Segment.compareTo, cleans it
 * for privacy (clean, :155-175, over everything added since the last flush) and hands the
 * files out.  One store per matcher, independent of the session store; its rows live in a
 * buffer of their own and survive every other call on the matcher. */
typedef struct otr_tile_store_config {
  int64_t max_rows;      /* rows held between two flushes, 1 .. 1<<27 (sizeof(otr_tile_row) bytes each) */
  int32_t quantisation;  /* bucket seconds, >= 60 (AnonymisingProcessor.java:78-80) */
  int32_t privacy;       /* observations a pair needs, >= 1 (:72-74) */
} otr_tile_store_config;

typedef struct otr_tile_add_result {
  int64_t n_reports, n_valid;    /* reports read / passing Segment.valid (forward()'s `reported`) */
  int64_t n_rows_added, n_rows;  /* n_rows: held after the call */
  float device_ms;               /* HIP-event time from the call's first device operation to its last */
  int32_t reserved;
} otr_tile_add_result;

/* The flush's files: listed file f owns rows row_off[f] .. row_off[f+1]-1 (row_off has
 * n_files + 1 elements), files by ascending `file`, within a file Segment.compareTo order
 * (numeric id, next_id), stable in arrival order across all adds.  n_unclean: the file's rows
 * before clean (the reference's log line).  Files cleaned to nothing are counted in
 * n_files_empty and not listed.  Host and device copies, owned by the matcher until its
 * next tile-store or otr_tiles_cull call. */
typedef struct otr_tile_flush_result {
  int64_t n_rows_in, n_rows;     /* before / after clean */
  int32_t n_files, n_files_empty;
  float device_ms;
  int32_t reserved;
  const otr_tile_row* rows;  const uint64_t* file;  const int64_t* row_off;  const int64_t* n_unclean;
  const otr_tile_row* d_rows;  const uint64_t* d_file;  const int64_t* d_row_off;  const int64_t* d_n_unclean;
} otr_tile_flush_result;

/* Opens the matcher's tile store (OTR_BAD_REQUEST when it has one, or for a config out of
 * range; OTR_DEVICE_ERROR naming the buffer when it does not fit the device).  Every other
 * call below returns OTR_BAD_REQUEST on a matcher without a store. */
int otr_tile_store_open(otr_matcher* m, const otr_tile_store_config* cfg);
int otr_tile_store_close(otr_matcher* m);

/* Adds the reports of the matcher's last otr_sessions_push / otr_sessions_punctuate result,
 * read from its device arrays, in the reference's forward order: windows by ascending trigger
 * (stable), the windows of an eviction in rank order, a window's reports in order, a report's
 * buckets ascending.  Refused when there is no such result or it was added already.
 * An add that would take the store beyond max_rows is refused with OTR_BAD_REQUEST (the
 * message names max_rows) and the store untouched: flush, then add again. */
int otr_tile_store_add_session(otr_matcher* m, otr_tile_add_result* out);

/* The same from plain arrays in host or device memory, windows in the order given: window w
 * owns reports rep_off[w] .. rep_off[w+1]-1 (rep_off[0] == 0, ascending); next_id OTR_NO_ID: none. */
int otr_tile_store_add_reports(otr_matcher* m, int64_t n_windows, const int64_t* rep_off, const uint64_t* id,
                               const uint64_t* next_id, const double* t0, const double* t1, const int32_t* length,
                               const int32_t* queue_length, int32_t memory, otr_tile_add_result* out);

/* Appends n finished rows (host or device memory), e.g. those received from another GPU. */
int otr_tile_store_add_rows(otr_matcher* m, const otr_tile_row* rows, int64_t n, int32_t memory,
                            otr_tile_add_result* out);

/* Everything added since the last flush as cleaned files; the store is empty afterwards.  A
 * flush of an empty store returns zero files. */
int otr_tile_store_flush(otr_matcher* m, otr_tile_flush_result* out);

/* ---- tile file texts: rows in HBM to payload bytes ---------------
 * What AnonymisingProcessor.store (AnonymisingProcessor.java:177-183) and simple_reporter.py
 * (:188-196, 252-253) hand to S3, HTTP or a directory, written on the device: one byte buffer
 * holding every file's text, file f at text[text_off[f] .. text_off[f+1]), and one holding the
 * file names "{b*q}_{(b+1)*q-1}/{level}/{tile}" (q the quantisation; both products in uint64
 * modulo 2^64, printed unsigned), name f at names[name_off[f] .. name_off[f+1]).  With H the
 * column line segment_id,next_segment_id,duration,count,length,queue_length,minimum_timestamp,
 * maximum_timestamp,source,vehicle_type a file's text is
 *   OTR_TILE_RULES_STREAM: H, then per row "\n" and the fields (no trailing newline; next_id left
 *     out when it is OTR_INVALID_SEGMENT_ID),
 *   OTR_TILE_RULES_SIMPLE: H "\n", then per row the fields and "\n" (next_id always printed),
 * the rows' bytes being exactly those of otr_tiles_format.  source and mode: at most 255 bytes
 * each, null = empty; mode's ASCII a-z are upper-cased.  Host and device copies, owned by the
 * matcher until its next tile-store, otr_tiles_text or otr_tiles_cull call. */
typedef struct otr_tile_text_result {
  int64_t n_rows, n_text_bytes, n_name_bytes;
  int32_t n_files, reserved;
  float device_ms; int32_t reserved2;  /* HIP-event time of the text stage */
  const uint8_t* text;  const int64_t* text_off;  /* n_files + 1 */
  const uint8_t* names; const int64_t* name_off;  /* n_files + 1 */
  const uint64_t* file; const int64_t* row_off;   /* n_files, n_files + 1 */
  const uint8_t* d_text;  const int64_t* d_text_off;
  const uint8_t* d_names; const int64_t* d_name_off;
  const uint64_t* d_file; const int64_t* d_row_off;
} otr_tile_text_result;

#define OTR_TILE_TEXT_NO_HOST 1   /* leave the host pointers null: device copies only */

/* The texts of n rows (host or device memory) in which the rows of one file are adjacent, as
 * otr_tiles_cull and the flush leave them: every run of equal `file` is one file, so a file
 * value that recurs after another file is a second file of the same name.  n == 0: zero files,
 * text_off = {0}.  OTR_BAD_REQUEST for quantisation < 1, unknown rules, or a source or mode
 * longer than 255 bytes. */
int otr_tiles_text(otr_matcher* m, const otr_tile_row* rows, int64_t n, int32_t memory, int32_t quantisation,
                   int32_t rules, const char* source, const char* mode, int32_t flags, otr_tile_text_result* out);

/* otr_tile_store_flush (same counts, same file table, the store empty afterwards), then the
 * texts of the kept rows under OTR_TILE_RULES_STREAM and the store's quantisation, written from
 * their device copy: flush->rows is null, no row crosses to the host.  A refusal (source or
 * mode too long) or a failure of the text stage leaves the store as it was.  A flush of an empty
 * store returns zero files and no text. */
int otr_tile_store_flush_text(otr_matcher* m, const char* source, const char* mode, int32_t flags,
                              otr_tile_flush_result* flush, otr_tile_text_result* out);

/* ---- tile file texts read back: payload bytes to rows in HBM -------
 * The inverse of otr_tiles_text, for simple_reporter.py --match-dir (report(), :211-254, reads the
 * tile files match() appended to a directory earlier, :199-206): the byte buffer of many tile
 * files with their names and offsets, in the shape otr_tile_text_result has, to otr_tile_row
 * records in HBM grouped by file, every line that is not a row named with its reason.
 *
 * THE RULE: a line becomes a row if and only if writing that row back (otr_tiles_format, the
 * same rules, source and mode) reproduces the line's bytes; a file name is accepted if and only
 * if it is the name otr_tiles_text gives the resulting `file` value at the caller's quantisation
 * without wrapping modulo 2^64.  Nothing is approximated: a numeral that is not the canonical
 * decimal ("01", "+1", "-0", " 1", "1.0") would sort elsewhere in the reference than its row does
 * here, and a line the reference would carry through as opaque text but a row cannot express is
 * counted and reported, never turned into a row.  (A source or mode that holds a ',' gives lines
 * of more than 10 fields: they are OTR_TILE_LINE_U_FIELDS.)
 *
 * Lines.  File f is T = text[text_off[f] .. text_off[f+1]), split at every '\n' into pieces
 * p0..pk; an empty T has no line.  With H the column line of otr_tiles_text:
 *   OTR_TILE_RULES_SIMPLE (line = piece "\n"): p0..p(k-1) are lines, pk only if it is not empty,
 *     and then it is an unterminated final line (U_END: ''.join(segments), :253, would glue it to
 *     its successor after the sort).  H is optional: write_tiles and the uploaded bodies have it,
 *     the reference's match-dir files do not.
 *   OTR_TILE_RULES_STREAM (row = "\n" piece): p0..pk are all lines, p0 must be H, and an empty
 *     piece (one left by a trailing "\n" included) is a line and is bad.
 * A p0 that equals H is OTR_TILE_LINE_HEADER; H anywhere else is U_HEADER.  Line indices are
 * global over the files in order, headers included.  The first status that applies, in the order
 * of the values below, is a line's status, except that every line of a file whose name was
 * refused is U_NAME (its lines are not parsed).  Values >= OTR_TILE_LINE_UNSUPPORTED mean "the
 * reference would carry this line; rows cannot". */
#define OTR_TILE_LINE_ROW 0        /* became a row */
#define OTR_TILE_LINE_HEADER 1     /* the column line, first of its file: skipped */
#define OTR_TILE_LINE_E_FIELDS 2   /* fewer than 2 comma-separated fields (the empty line included):
                                      report() raises IndexError (:224-227) and the file is lost */
#define OTR_TILE_LINE_UNSUPPORTED 32
#define OTR_TILE_LINE_U_NAME 32    /* the file's name was refused */
#define OTR_TILE_LINE_U_END 33     /* SIMPLE: the final line has no "\n" */
#define OTR_TILE_LINE_U_HEADER 34  /* the column line misplaced, or missing under STREAM */
#define OTR_TILE_LINE_U_FIELDS 35  /* not exactly 10 fields */
#define OTR_TILE_LINE_U_NUMBER 36  /* a numeric field is not the canonical decimal ("-"? then digits,
                                      no leading zero, no "-0") of a value its row member holds: id and
                                      next_id uint64 without sign, duration, length and queue_length
                                      int32, start and end int64 (an empty next_id is U_NEXT's) */
#define OTR_TILE_LINE_U_NEXT 37    /* next_id empty under SIMPLE, or spelled 70368744177663 under STREAM
                                      (otr_tiles_text leaves it out there; empty under STREAM is
                                      OTR_INVALID_SEGMENT_ID) */
#define OTR_TILE_LINE_U_COUNT 38   /* the fourth field is not "1" */
#define OTR_TILE_LINE_U_TAG 39     /* source or vehicle_type is not byte-equal to the caller's source and
                                      upper-cased mode (a "\r" before the newline lands here) */

/* The input: otr_tiles_text's output shape.  A name is "{a}_{b}/{level}/{tile}", four canonical
 * unsigned decimals with a % q == 0, b == a + q - 1, a / q < 2^39, level <= 7, tile < 2^22 (q the
 * quantisation); no directory prefix. */
typedef struct otr_tile_texts {
  const uint8_t* text;  const int64_t* text_off;   /* n_files + 1, ascending from 0 */
  const uint8_t* names; const int64_t* name_off;   /* n_files + 1, ascending from 0 */
  int32_t n_files, memory;                         /* OTR_MEM_*: one memory for all four */
} otr_tile_texts;

/* Rows are grouped by file in line order: file f's are rows[row_off[f] .. row_off[f+1]), each with
 * `file` = file[f] (from the name alone: the reference never compares the ids with the path
 * either) and speed_bin -1.  A file whose name was refused has file[f] = OTR_NO_ID,
 * file_status[f] = 1 and no rows.  Lines file_line_off[f] .. file_line_off[f+1]-1 are file f's.
 * first_bad: the lowest line with a status >= OTR_TILE_LINE_E_FIELDS (-1, -1, 0: none).  Host copies
 * unless OTR_TILE_PARSE_NO_HOST, device copies always; all owned by the matcher until its next
 * otr_tiles_parse: they survive otr_tiles_cull, otr_tiles_text and the tile store calls, so
 * d_rows can go to any of them with OTR_MEM_DEVICE. */
typedef struct otr_tile_parse_result {
  int64_t n_lines, n_rows, n_headers, n_bad, n_bad_names;
  int64_t first_bad;  int32_t first_bad_file, first_bad_reason;
  float device_ms;  int32_t n_files;
  const otr_tile_row* rows;    const int64_t* row_off;       /* n_rows, n_files + 1 */
  const uint64_t* file;        const uint8_t* file_status;   /* n_files */
  const int64_t* file_line_off;                              /* n_files + 1 */
  const uint8_t* line_status;                                /* n_lines: OTR_TILE_LINE_* */
  const otr_tile_row* d_rows;  const int64_t* d_row_off;
  const uint64_t* d_file;      const uint8_t* d_file_status;
  const int64_t* d_file_line_off;
  const uint8_t* d_line_status;
} otr_tile_parse_result;

#define OTR_TILE_PARSE_NO_HOST 1   /* leave the host pointers null: device copies only */

/* Device text is read where the caller's pointers say (one device-to-device copy pads it to whole
 * 16-byte chunks, as otr_ingest does), never through the host.  OTR_BAD_REQUEST, with the previous
 * result left as it was, for quantisation < 1, unknown rules, a source or mode longer than 255
 * bytes, n_files < 0, offsets that do not ascend from 0, and sizes beyond otr_ingest's: text of
 * 2^40 bytes or of 2^31 - 1 sixteen-byte chunks, or 2^31 - 1 lines.  Everything else is decided per
 * line and per file; n_files == 0 gives zero lines. */
int otr_tiles_parse(otr_matcher* m, const otr_tile_texts* in, int32_t quantisation, int32_t rules,
                    const char* source, const char* mode, int32_t flags, otr_tile_parse_result* out);

/* ---- tile store: snapshot, restore, Segment.ListSerder records ----
 * The reference keeps the anonymiser's state in two Kafka state stores with changelogs
 * (AnonymisingProcessor.java:47-59): anonymise_tile, String "{time_range_start}_{tile_id}.{slice}"
 * -> the bytes of Segment.ListSerder (Segment.java:131-155), and anonymise_max_slice,
 * TimeQuantisedTile.Serder (TimeQuantisedTile.java:55-71) -> the current slice.  A Segment carries
 * the doubles min and max, an otr_tile_row only floor(t0), ceil(t1) and the rounded duration, so a
 * store that is to write those bytes keeps the two times beside every row. */
#define OTR_TILE_STORE_TIMES 1   /* keep t0[max_rows] and t1[max_rows] (doubles, 16 B per row) */

/* otr_tile_store_open with flags; 0 is otr_tile_store_open.  On a store with OTR_TILE_STORE_TIMES
 * every add of reports writes the report's t0 and t1 beside each of its rows (a report that spans
 * several buckets gives each of its rows the same pair), the flushes give the same results and
 * reset it the same way, and otr_tile_store_add_rows is refused with OTR_BAD_REQUEST (finished rows
 * have no times): otr_tile_store_restore takes its place. */
int otr_tile_store_open_ex(otr_matcher* m, const otr_tile_store_config* cfg, int32_t flags);

/* The held rows in arrival order; t0 / t1 per row on a store with the times, null otherwise.
 * Host and device copies, owned by the matcher until its next tile-store call. */
typedef struct otr_tile_snapshot {
  int64_t n_rows;
  int32_t quantisation;  int32_t flags;   /* the store's (output; ignored by a restore) */
  const otr_tile_row* rows;  const double* t0;  const double* t1;
  const otr_tile_row* d_rows;  const double* d_t0;  const double* d_t1;   /* output only */
} otr_tile_snapshot;
#define OTR_TILE_SNAPSHOT_NO_HOST 1   /* leave the host pointers null: device copies only */

/* Why a tile restore is refused; where an index has several reasons the lowest value is reported. */
#define OTR_TILE_RESTORE_E_LAYOUT 1     /* offsets not non-decreasing or beyond n_bytes; a record shorter than 4
                                           bytes or not 4 + 40*count long (64-bit; count < 0 too) */
#define OTR_TILE_RESTORE_E_KEY 2        /* start < 0, start % q != 0, start / q >= 2^39, tile_id outside
                                           0 .. 0x1FFFFFF, slice < 0 */
#define OTR_TILE_RESTORE_E_COUNT 3      /* count 0 (the reference never puts an empty list,
                                           AnonymisingProcessor.java:138-141) or count > slice_size */
#define OTR_TILE_RESTORE_E_SEGMENT 4    /* a segment failing Segment.valid; max >= 2^62; id & 0x1FFFFFF != tile_id;
                                           or start / q outside [(long)min / q, (long)max / q] */
#define OTR_TILE_RESTORE_E_DUPLICATE 5  /* not the first occurrence of its (start, tile_id, slice) in the input */
#define OTR_TILE_RESTORE_E_MAP 6        /* a map entry with an invalid key (as E_KEY), a negative value or a
                                           repeated key (bad_slice -1, bad_tile the lowest such entry); reported
                                           only when no slice record has a reason */
#define OTR_TILE_RESTORE_E_FULL 7       /* held + restored rows > max_rows (bad_slice -1); only when nothing
                                           above applies */
#define OTR_TILE_RESTORE_E_ROW 8        /* otr_tile_store_restore on a store with the times: a row that is not
                                           the row its report gives (bad_slice: the lowest such row) */

typedef struct otr_tile_restore_result {
  int64_t n_slices, n_rows;             /* restored by this call */
  int64_t n_unreferenced_slices, n_unreferenced_rows;   /* valid records the map does not name: not restored */
  int64_t n_missing_slices;             /* slices the map names and the input lacks */
  int64_t n_rows_held;                  /* after the call */
  int64_t bad_slice;                    /* lowest refused record (otr_tile_store_restore: row), -1: none */
  int64_t bad_tile;                     /* lowest refused map entry, -1: none */
  int32_t bad_reason;                   /* OTR_TILE_RESTORE_E_*, 0 when restored */
  float device_ms;
} otr_tile_restore_result;

/* flags: 0 or OTR_TILE_SNAPSHOT_NO_HOST.  The store is untouched; an empty store gives n_rows 0. */
int otr_tile_store_snapshot(otr_matcher* m, int32_t flags, otr_tile_snapshot* out);

/* Appends snap's n_rows rows (host or device arrays) to the held rows, all or nothing.  A plain
 * store takes the rows as they are, exactly as otr_tile_store_add_rows does, and ignores any
 * times.  A store with the times requires them, and every row must equal, bit for bit in all nine
 * fields, the row an add derives from (row.file >> 25, id, next_id, t0, t1, length, queue_length):
 * the report passes Segment.valid and the bucket lies in its span.  Otherwise OTR_BAD_REQUEST with
 * OTR_TILE_RESTORE_E_ROW and the lowest such index in bad_slice; OTR_TILE_RESTORE_E_FULL when
 * held + given > max_rows and no row is refused. */
int otr_tile_store_restore(otr_matcher* m, const otr_tile_snapshot* snap, int32_t memory,
                           otr_tile_restore_result* out);

/* The held rows as the reference's records, in `file` order (bucket << 25 | level << 22 | tile
 * index; time_range_start = bucket * q, tile_id = level | index << 3 = id & 0x1FFFFFF).  A file
 * with n held rows gives slice records s = 0 .. ceil(n / S) - 1 holding its rows
 * [sS, min((s+1)S, n)) in arrival order, and one map entry with value n / S (floor): when n is a
 * multiple of S the slice the map names has no record yet, the reference's state after its S-th
 * add (AnonymisingProcessor.java:147-151).  Slice record i is bytes[rec_off[i] .. rec_off[i+1]):
 * int32 count, then count x (int64 id, int64 next_id, double min, double max, int32 length,
 * int32 queue), big-endian, 4 + 40*count bytes (Segment.java:82-89, 145-148); next_id
 * OTR_INVALID_SEGMENT_ID for none, min and max the kept t0 and t1 by bits.  Its key is
 * (start[i], tile_id[i], slice[i]), and as the changelog's String names[name_off[i] ..
 * name_off[i+1]).  map_bytes: 20 bytes per map entry, int64 start, int64 tile_id (the
 * TimeQuantisedTile.Serder key), int32 slice (Kafka's integer value), big-endian.  Slices ascend
 * by (file, slice), map entries by file.
 * As an input (otr_tile_store_restore_records): n_slices, n_bytes, slice_size (the largest count
 * accepted), memory, start, tile_id, slice, rec_off, bytes (any address, records at any offset),
 * n_tiles and map_bytes (n_tiles < 0: no map); names and the d_ pointers are ignored. */
typedef struct otr_tile_records {
  int64_t n_slices, n_bytes, n_name_bytes;
  int64_t n_tiles;
  int32_t slice_size;  int32_t memory;   /* OTR_MEM_HOST / OTR_MEM_DEVICE (input; an export sets host) */
  const int64_t* start;  const int64_t* tile_id;  const int32_t* slice;  const int64_t* rec_off;  /* n_slices + 1 */
  const uint8_t* bytes;  const uint8_t* names;  const int64_t* name_off;  const uint8_t* map_bytes;
  /* export only: the same arrays in HBM */
  const int64_t* d_start;  const int64_t* d_tile_id;  const int32_t* d_slice;  const int64_t* d_rec_off;
  const uint8_t* d_bytes;  const uint8_t* d_names;  const int64_t* d_name_off;  const uint8_t* d_map_bytes;
} otr_tile_records;

/* A store with the times only (OTR_BAD_REQUEST naming OTR_TILE_STORE_TIMES otherwise);
 * slice_size >= 1, the reference's SLICE_SIZE is 20000 (AnonymisingProcessor.java:45).  The store
 * is untouched.  An empty store gives zero slices and rec_off = {0}.  Host and device arrays,
 * owned by the matcher until its next tile-store call. */
int otr_tile_store_export_records(otr_matcher* m, int32_t slice_size, otr_tile_records* out);

/* Appends the rows of the referenced slice records in (file, slice, position) order, each row
 * derived from its segment exactly as an add derives it; a plain store keeps the rows only.  With
 * a map a record is referenced when its (start, tile_id) has an entry and slice <= its value;
 * unreferenced records are validated like the rest and not restored (the reference's punctuate
 * deletes them with a warning, :258-265), slices the map names and the input lacks are accepted
 * and counted (:242-243).  Without a map every record is referenced.  All or nothing: on a refusal
 * OTR_BAD_REQUEST, the store untouched, bad_slice / bad_reason the lowest refused index and the
 * lowest of its reasons.  ListSerder's own deserialiser returns an empty list (Segment.java:165-167)
 * and so loses every restored slice; this call restores what the serialiser wrote. */
int otr_tile_store_restore_records(otr_matcher* m, const otr_tile_records* in, otr_tile_restore_result* out);

/* The changelog's String key of a slice: Long.toString(start) "_" Long.toString(tile_id) "."
 * Integer.toString(slice).  Returns its length (at most 52, no terminator counted; one is written
 * when it fits) or -1 when cap is too small.  The parse accepts exactly what those print: an
 * optional '-', no '+', no leading zeros, no spaces; returns 0, or nonzero for anything else. */
int otr_tile_slice_key(int64_t start, int64_t tile_id, int32_t slice, char* buf, int64_t cap);
int otr_tile_slice_key_parse(const char* text, int64_t len, int64_t* start, int64_t* tile_id, int32_t* slice);

/* report() (reporter_service.py:79-179) over n segment lists at once, evaluated by the
 * device code of the segment scan K7 (otr_report.h compiled for gfx950, one thread per
 * list) — what pins the device tail against the reference's own report() outputs.  Host
 * arrays; list c holds segments seg_off[c] .. seg_off[c+1]-1 (seg_id OTR_NO_ID: no id;
 * has_length 0: no length) and its reports go to rep_* from index seg_off[c]; per list:
 * n_rep, shape_used (-1 absent), counts[6] (successful, unreported, discontinuities,
 * invalid_speeds, invalid_times, unassociated), lengths[2], length_set[2]. */
int otr_report_lists_device(int32_t n, const int64_t* seg_off, const uint64_t* seg_id, const double* start,
                            const double* end, const uint8_t* internal, const int32_t* queue,
                            const uint8_t* has_length, const int32_t* length, const int32_t* begin_shape,
                            const int64_t* end_time, const double* threshold, const uint32_t* report_levels,
                            const uint32_t* transition_levels, uint64_t* rep_id, uint64_t* rep_next, double* rep_t0,
                            double* rep_t1, int32_t* rep_length, int32_t* rep_queue, int32_t* n_rep,
                            int32_t* shape_used, int32_t* counts, double* lengths, int32_t* length_set);

/* graph facts for callers sizing histograms */
int otr_graph_info(int64_t* n_nodes, int64_t* n_edges, int64_t* n_segments);

/* device + stream the matcher runs on (hipStream_t as void*), for callers that
 * place inputs in HBM themselves and bracket timing */
void* otr_matcher_stream(otr_matcher* m);
int otr_device(void);

#ifdef __cplusplus
}
#endif
#endif
