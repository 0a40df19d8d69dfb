// otr_engine.h — host-side engine: HBM graph replica, per-matcher workspace and the stages
// that run on it.  Internal C++ interface between the C-ABI in otr_api.cpp and the units that
// define Matcher's members: otr_engine.hip (configure, the workspace, the batched pipeline
// K0..K9, K12, K13, report_lists_device), otr_tiles.hip (tile cull K10, keyed histogram),
// otr_text.hip (probe ingest K11, stream formatter K16), otr_sessions.hip (K14, K17, K18) and
// otr_tilestore.hip (K15, K19, K20).
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/otr.h"
#include "otr_device.h"
#include "otr_hostdev.h"
#include "otr_tiers.h"

namespace otr {

struct Config {
  ModeParams mp;
  std::string graph_path;
  int device = 0;
};

ModeParams default_mode_params();
void finalize_params(MatchParams* p);
const char* check_params(const MatchParams& p);  // nullptr when the engine can honour p

// The configured graph, resident in HBM (one replica per process/GPU).  A reconfigure
// builds the new replica aside and swaps it in under the exclusive lock; batches hold
// the shared lock for their whole run, so no kernel ever sees a freed array.
struct GraphState {
  bool ready = false;
  int device = 0;
  DevGraph dg{};
  ModeParams defaults{};
  std::vector<void*> allocs;
  uint64_t n_nodes = 0, n_edges = 0, n_segments = 0;
  // host copy of the few arrays the JSON path needs
  std::vector<unsigned long long> seg_id;
  std::shared_mutex mu;
};

GraphState& graph_state();
int engine_configure(const Config& cfg, std::string* err);

struct ReportLists {
  int32_t n;
  const int64_t* seg_off;
  const unsigned long long* seg_id;
  const double *start, *end;
  const uint8_t* internal;
  const int32_t* queue;
  const uint8_t* has_length;
  const int32_t *length, *begin_shape;
  const int64_t* end_time;
  const double* threshold;
  const uint32_t *rl, *tl;
  unsigned long long *rep_id, *rep_next;
  double *rep_t0, *rep_t1;
  int32_t *rep_length, *rep_queue, *n_rep, *shape_used, *counts;
  double* lengths;
  int32_t* length_set;
};

int report_lists_device(const ReportLists& h, std::string* err);

// one tier of global-memory search slabs (otr_general.h), owned by a matcher
struct GSlab {
  uint32_t* key = nullptr;
  unsigned long long* lab = nullptr;
  uint32_t* qmark = nullptr;
  uint32_t* fr = nullptr;
  uint32_t* touched = nullptr;
};

// turn cost table (mm) of a turn_penalty_factor: factor * exp(-deg / 45) for deg 0..180
// (oracle orc_turn_table: the same operations)
void turn_table(double factor, int32_t* tab181);

uint64_t uuid_key_host(const char* uuid, int64_t len);  // K11's uuid_hash over host bytes

struct SessionStore;                    // otr_sessions.hip (K14)
void sessions_destroy(SessionStore* s);  // frees the store's device memory

// the reports of a session store's last push / punctuate result, in HBM (for the tile
// store's add_session): valid until the store's next session call
struct SessionReports {
  int64_t n_windows, n_reports;
  const int64_t *trigger, *rep_off;
  const unsigned long long *id, *next_id;
  const double *t0, *t1;
  const int32_t *length, *queue_length;
  bool* added;  // set once a tile store has taken them
};
bool sessions_last_reports(SessionStore* s, SessionReports* out);  // false: no such result

struct TileStore;                      // otr_tilestore.hip (K15)
void tile_store_destroy(TileStore* s);  // frees the store's device memory

struct TileText;                      // otr_tilestore.hip (K19): the buffers of the file texts
void tile_text_destroy(TileText* t);  // frees them

struct TileParse;                       // otr_tilestore.hip (K21): the rows read back from file texts
void tile_parse_destroy(TileParse* t);  // frees them

// what cull_device leaves in the matcher's cull slots
struct CulledRows {
  const otr_tile_row* sorted;  // all n rows in file, then rule order
  const otr_tile_row* kept;    // the n_kept rows the cull keeps, same order
  const int64_t* kept_incl;    // [n] inclusive count of kept rows along `sorted`
  int64_t n_kept;
};

struct Matcher {
  hipStream_t stream = nullptr;
  SessionStore* ses = nullptr;  // the session store (otr_sessions_open), owned
  TileStore* tst = nullptr;     // the tile store (otr_tile_store_open), owned
  TileText* ttx = nullptr;      // the file texts of the last otr_tiles_text / flush_text, owned
  TileParse* tpx = nullptr;     // the rows of the last otr_tiles_parse, owned
  DevPool pool{PoolOwner::matcher, nullptr, 0};  // the workspace slots (otr_slots.h), sized at first use
  GSlab gslab[2];
  // the turn cost tables last uploaded and the device buffer that holds them: a batch with the
  // same parameters and the same buffer uploads nothing
  std::vector<int32_t> h_turn;
  const int32_t* turn_dev = nullptr;
  // the same for K7's arguments, which k_compact reads from device memory (copy-out only)
  std::vector<char> seg_args;
  const void* seg_args_dev = nullptr;
  // The pinned mailbox (mapped host memory, allocated once, one per matcher so that streams
  // stay independent): every scalar the host reads of a batch or of a histogram reduce
  // arrives here, one record per host wait.  post_wait gathers the runs (8-byte words, eight
  // runs at most, kMailWords in all) with k_post, waits for the stream and leaves them back to
  // back in mail[]; post only queues the gather, into dst.  Nothing is copied into pageable
  // memory, and no wait has more than one device-to-host operation.
  static constexpr int kMailWords = 512;
  unsigned long long* mail = nullptr;
  struct MailRun {
    const void* src;
    int words;
  };
  int post(std::initializer_list<MailRun> runs, unsigned long long* dst, std::string* err);
  int post_wait(std::initializer_list<MailRun> runs, std::string* err);
  // pinned host copy of the batch's drain slab (per-trace output counts, folded counters)
  unsigned long long* h_drain = nullptr;
  size_t h_drain_words = 0;
  // host result storage (OTR_BATCH_COPY_OUT)
  std::vector<int64_t> h_trace_state_off, h_state_probe, h_trace_route_off, h_trace_seg_off, h_seg_way_off,
      h_trace_rep_off;
  std::vector<int32_t> h_cand_count, h_winner, h_subpath, h_seg_length, h_seg_queue, h_seg_bshape, h_seg_eshape,
      h_rep_length, h_rep_queue, h_shape_used, h_stats, h_trace_status;
  std::vector<uint32_t> h_cand_edge, h_route_edge, h_seg_way;
  std::vector<double> h_cand_p, h_cand_sqd, h_seg_start, h_seg_end, h_rep_t0, h_rep_t1, h_stats_len;
  std::vector<unsigned long long> h_seg_id, h_rep_id, h_rep_next;
  std::vector<uint8_t> h_seg_internal;
  std::vector<otr_tile_row> h_tile_rows;
  // matched points (K12) of the last batch: whether it asked for them, and the result
  // otr_matched_points hands out (device arrays in the matcher's slots, host copies here)
  bool pts_have = false;
  otr_point_result pts{};
  std::vector<uint8_t> h_pt_kind;
  std::vector<uint32_t> h_pt_edge;
  std::vector<double> h_pt_frac, h_pt_lat, h_pt_lon, h_pt_dist;
  std::vector<int64_t> h_pt_state, h_pt_pos;
  // edge traversals (K13) of the last batch, kept the same way for otr_edge_traversals and
  // otr_edge_observations
  bool trv_have = false;
  otr_traversal_result trv{};
  std::vector<int64_t> h_tr_off, h_tr_first, h_tr_s0, h_tr_s1;
  std::vector<uint32_t> h_tr_edge, h_tr_way;
  std::vector<uint64_t> h_tr_seg;
  std::vector<double> h_tr_f0, h_tr_f1, h_tr_t0, h_tr_t1;
  // 0..19 the batch stages and, from kEvents' layout (otr_tiers.h), a pair per route tier slot and
  // K12's and K13's pairs: otr_engine.hip; 20..23 ingest and the formatter: otr_text.hip
  hipEvent_t ev[kEvents];
  bool ev_init = false;

  template <class T>
  T* need(int slot, size_t n);
  // optional workspace (the retry tiers' resume dumps, the spatial sort's copy): taken
  // only while the device keeps a reserve free for the mandatory buffers of later stages,
  // nullptr otherwise (the searches then restart: same results)
  template <class T>
  T* want(int slot, size_t n);
  // frees the optional workspace after the stream drains (a mandatory need() that cannot
  // allocate retries once after it); not while the route stage's kernels hold it
  bool release_optional();
  bool opt_busy = false;
  // entry points: a device allocation failure inside returns OTR_DEVICE_ERROR (no kernel
  // runs on a missing buffer): each body runs under guarded() (otr_hostdev.h)
  int run(const otr_trace_batch* in, const ModeParams& mp, otr_batch_result* out, std::string* err);
  int matched_points(otr_point_result* out, std::string* err) const;  // of the last run (host only)
  int edge_traversals(otr_traversal_result* out, std::string* err) const;  // of the last run (host only)
  int edge_observations(int quantisation, otr_hist_entry** d_entries, int64_t* n, std::string* err);
  int tiles_cull(const otr_tile_row* rows, int64_t n, int memory, int privacy, int rules, const otr_tile_row** out,
                 int64_t* n_out, std::string* err);
  int hist_reduce(const void* in, int64_t n, int memory, int rows_in, int privacy, const otr_hist_entry** out,
                  int64_t* n_out, std::string* err);
  // sort + cull of rows already in HBM, results left in HBM (the tile store's flush)
  int cull_device(const otr_tile_row* d_in, int64_t n, int privacy, int rules, CulledRows* out, std::string* err);
  int copy_out(void* dst, const void* src, size_t bytes, int dst_memory, std::string* err);
  int ingest(const char* text, int64_t len, int memory, const otr_ingest_format* fmt, otr_ingest_result* out,
             std::string* err);
  // the stream formatter (K16, otr_formatter.h): raw messages → keyed points in HBM
  int format_messages(const otr_message_format* fmt, const otr_messages* msgs, otr_format_result* out,
                      std::string* err);
  // the session store (K14, otr_sessions.hip)
  // (uuid_bytes > 0: with the uuid directory, K18; names: non-null on such a store only)
  int sessions_open(const otr_session_config* cfg, int32_t uuid_bytes, std::string* err);
  int sessions_close(std::string* err);
  int sessions_push(const otr_session_points* pts, const otr_session_names* names, otr_session_result* out,
                    std::string* err);
  int sessions_punctuate(int64_t ts, otr_session_result* out, std::string* err);
  int sessions_advance(const otr_session_points* pts, const otr_session_names* names, otr_trace_batch* out,
                       std::string* err);
  int sessions_commit(const int32_t* shape_used, const int32_t* status, int memory, std::string* err);
  int sessions_windows(otr_session_result* out, std::string* err);
  int sessions_snapshot(otr_session_snapshot* out, std::string* err);
  // restore, export and move (K17)
  int sessions_restore(const otr_session_snapshot* snap, const otr_session_names* names, int memory,
                       otr_session_restore_result* out, std::string* err);
  int sessions_restore_records(const otr_session_records* recs, const otr_session_names* names,
                               otr_session_restore_result* out, std::string* err);
  int sessions_export_records(otr_session_records* out, std::string* err);
  int sessions_take(int n_parts, int part, int remove, otr_session_snapshot* out, std::string* err);
  // the uuid directory (K18): whether the store has one, the names of the last listing, the last
  // name refusal (and, after a refused otr_sessions_push_text, its message from d_message)
  bool sessions_named() const;
  int sessions_names(otr_session_name_list* out, std::string* err);
  int sessions_last_refusal(otr_session_name_refusal* out, std::string* err);
  void sessions_refusal_message(const int64_t* d_message);
  void sessions_refusal_clear();
  // the formatter's copy of the last chunk's text (S_IN_TEXT) and its length: what
  // otr_format_result's d_uuid_off / d_uuid_len index
  const uint8_t* fmt_text = nullptr;
  int64_t fmt_text_len = 0;
  // the tile store (K15, otr_tilestore.hip)
  int tile_store_open(const otr_tile_store_config* cfg, int flags, std::string* err);
  int tile_store_snapshot(int flags, otr_tile_snapshot* out, std::string* err);
  int tile_store_restore(const otr_tile_snapshot* snap, int memory, otr_tile_restore_result* out, std::string* err);
  int tile_store_export_records(int32_t slice_size, otr_tile_records* out, std::string* err);
  int tile_store_restore_records(const otr_tile_records* in, otr_tile_restore_result* out, std::string* err);
  int tile_store_close(std::string* err);
  int tile_store_add_session(otr_tile_add_result* out, std::string* err);
  int tile_store_add_reports(int64_t n_windows, const int64_t* rep_off, const uint64_t* id, const uint64_t* next_id,
                             const double* t0, const double* t1, const int32_t* length, const int32_t* queue_length,
                             int memory, otr_tile_add_result* out, std::string* err);
  int tile_store_add_rows(const otr_tile_row* rows, int64_t n, int memory, otr_tile_add_result* out, std::string* err);
  int tile_store_flush(otr_tile_flush_result* out, std::string* err);
  // tile file texts (K19, otr_tiletext.h; otr_tilestore.hip)
  int tiles_text(const otr_tile_row* rows, int64_t n, int memory, int quantisation, int rules, const char* source,
                 const char* mode, int flags, otr_tile_text_result* out, std::string* err);
  int tile_store_flush_text(const char* source, const char* mode, int flags, otr_tile_flush_result* flush,
                            otr_tile_text_result* out, std::string* err);
  // tile file texts read back (K21, otr_tileparse.h; otr_tilestore.hip)
  int tiles_parse(const otr_tile_texts* in, int quantisation, int rules, const char* source, const char* mode,
                  int flags, otr_tile_parse_result* out, std::string* err);
  ~Matcher();
};

}  // namespace otr
