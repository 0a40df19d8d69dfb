// otr_sessions.hip — host side of the session store (K14, otr_sessions.h): the store's
// device memory, the passes of a chunk (insert, assign, group), the rounds (advance, gather,
// match, commit), punctuate and the snapshot; restore, export as records and take (K17).
// include/otr.h otr_sessions_* for the rules.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "otr_devscan.h"
#include "otr_engine.h"
#include "otr_launch.h"
#include "otr_sessions.h"

namespace otr {

namespace {

// growable buffers of a chunk, a round and a result
enum SesBuf {
  B_KEY, B_LAT, B_LON, B_ACC, B_TIME, B_TS, B_ENTRY, B_NEW, B_RANK, B_LANE_SLOT, B_IDX, B_SORT_SLOT, B_SORT_IDX,
  B_HEAD, B_SEG_INCL, B_SEG_SLOT, B_SEG_CUR, B_SEG_END, B_TRIP, B_TRIP_INCL, B_TMP,
  B_W_SLOT, B_W_TRIG, B_W_N, B_W_KEY, B_W_SU, B_W_STATUS, B_W_TRIM, B_W_SU_OUT,
  B_G_OFF, B_G_LAT, B_G_LON, B_G_TIME, B_G_ACC, B_G_MODE, B_SUB_OFF,
  B_FLAG, B_FLAG_INCL, B_L_KEY, B_L_SLOT, B_L_KEY2, B_L_SLOT2, B_L_REP, B_L_REP_INCL, B_L_N,
  B_S_LAT, B_S_LON, B_S_ACC,
  B_R_KEY, B_R_TRIG, B_R_N, B_R_SU, B_R_STATUS, B_R_TRIM, B_R_OFF, B_R_ID, B_R_NEXT, B_R_T0, B_R_T1, B_R_LEN,
  B_R_QUEUE,
  B_RS_KEY, B_RS_OFF, B_RS_SEP, B_RS_LAST, B_RS_BYTES, B_RS_BAD, B_X_LEN, B_X_OFF, B_X_BYTES,
  B_NM_BYTES, B_NM_OFF, B_NM_LEN, B_NL_LEN, B_NL_OFF, B_NL_BYTES, B_NS_KEY, B_NS_KEY2, B_NS_PERM, B_NS_PERM2,
  B_NUM
};
const char* const kBufName[B_NUM] = {
    "chunk key", "chunk lat", "chunk lon", "chunk accuracy", "chunk time", "chunk timestamp", "lane entry",
    "lane creator", "creator rank", "lane session", "lane index", "sorted session", "sorted index", "segment head",
    "segment rank", "segment session", "segment cursor", "segment end", "trigger flag", "trigger rank",
    "scan / sort workspace", "window session", "window trigger", "window size", "window key", "window shape_used in",
    "window status", "window trimmed", "window shape_used", "batch offsets", "batch lat", "batch lon", "batch time",
    "batch accuracy", "batch mode", "sub-batch offsets", "session flag", "session rank", "list key", "list session",
    "sorted list key", "sorted list session", "eviction report flag", "eviction report rank", "list size",
    "snapshot lat", "snapshot lon", "snapshot accuracy", "result key", "result trigger", "result size",
    "result shape_used", "result status", "result trimmed", "result report offsets", "result id", "result next id",
    "result t0", "result t1", "result length", "result queue length", "restore key", "restore offsets",
    "restore max_sep", "restore last_update", "restore bytes", "restore refusal", "record lengths", "record offsets",
    "record bytes", "name bytes", "name offsets", "name lengths", "listed name lengths", "listed name offsets",
    "listed name bytes", "name sort key", "sorted name sort key", "name order", "sorted name order"};

}  // namespace

struct SessionStore : DevPool {  // the growable buffers: the pool's slots, by SesBuf
  SessionStore() : DevPool(PoolOwner::sessions, kBufName, B_NUM) {}
  otr_session_config cfg{};
  hipStream_t stream = nullptr;
  std::vector<void*> fixed;
  SesTable tab{}, spare{};
  SesStore st{};
  int32_t* free_list = nullptr;
  int32_t* cnt = nullptr;
  int32_t h_cnt[SES_WORDS] = {0, 0, 0, 0, 0};
  int32_t n_rebuilds = 0;
  hipEvent_t ev[2];
  bool ev_init = false;
  // the chunk and the round
  SesChunk ch{};
  int32_t n_seg = 0, W = 0, n_list = 0;
  int64_t P = 0;
  bool chunk_open = false, pending = false;
  std::vector<unsigned long long> w_key;
  std::vector<int64_t> w_trig, w_n;
  std::vector<int32_t> w_su, w_status, w_trim;
  // what a call returns
  std::vector<unsigned long long> r_key, r_id, r_next;
  std::vector<int64_t> r_trig, r_off;
  std::vector<int32_t> r_n, r_su, r_status, r_trim, r_len, r_queue;
  std::vector<double> r_t0, r_t1;
  int32_t r_rounds = 0, r_evicted = 0, forced0 = 0, dropped0 = 0;
  double r_match_ms = 0.0;
  // the last push / punctuate result's reports are in the B_R_* buffers (res_have), and
  // whether a tile store has taken them
  bool res_have = false, res_added = false;
  // snapshot
  std::vector<unsigned long long> s_key;
  std::vector<int64_t> s_off, s_last, s_time, all_last;
  std::vector<float> s_sep, s_lat, s_lon, all_sep;
  std::vector<int32_t> s_acc, s_slot;
  // exported records
  std::vector<int64_t> x_off;
  std::vector<uint8_t> x_bytes;
  // K18: the uuid directory (dir.row == 0: none), its scratch words per table entry, the names
  // of the last listing and the last name refusal
  SesDir dir{};
  int32_t* name_first = nullptr;
  std::vector<int64_t> nl_off;
  std::vector<uint8_t> nl_bytes;
  bool names_have = false;
  otr_session_name_refusal refusal{-1, -1, 0, 0};
  bool named() const { return dir.row > 0; }

  int32_t live() const { return cfg.max_sessions - h_cnt[SES_NFREE]; }

  template <class T>
  T* fix(size_t n, const char* name) {
    void* p = nullptr;
    const size_t bytes = (n ? n : 1) * sizeof(T);
    if (hipMalloc(&p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      throw DeviceOom{PoolOwner::sessions, name, -1, bytes};
    }
    fixed.push_back(p);
    return (T*)p;
  }

  // inclusive sum of 32- or 64-bit counts, the workspace in B_TMP
  template <class T>
  int scan(const T* in, T* out, int64_t n, std::string* err) {
    return pool_scan(*this, B_TMP, in, out, n, stream, err);
  }
  int alloc(std::string* err);
  int rebuild(std::string* err);
  int chunk_begin(const otr_session_points* pts, const SesNamesIn* nm, std::string* err);
  int names_in(const otr_session_names* names, int64_t n, int memory, SesNamesIn* out, std::string* err);
  int names_list(std::string* err);
  int name_order(std::string* err);
  int round(std::string* err);
  int gather(std::string* err);
  int commit(const int32_t* su, const int32_t* status, int memory, std::string* err);
  int match(Matcher& m, std::string* err);
  void result_begin();
  void result_round();
  int result_end(otr_session_result* out, bool with_device, std::string* err);
  void fill_batch(otr_trace_batch* bt);
  int list_sessions(int stale_only, int64_t ts, std::string* err);
  int list_flagged(std::string* err);
  int snapshot_list(otr_session_snapshot* out, std::string* err);
  template <bool REC>
  int restore(SesGiven g, const SesNamesIn* nm, otr_session_restore_result* out, std::string* err);
  int release_list(const int32_t* list, int32_t n, std::string* err);
};

void sessions_destroy(SessionStore* s) {
  if (!s) return;
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (void* p : s->fixed) (void)hipFree(p);
  s->release();
  if (s->ev_init)
    for (auto& e : s->ev) (void)hipEventDestroy(e);
  delete s;
}

int SessionStore::alloc(std::string* err) {
  const size_t ms = (size_t)cfg.max_sessions, cap = 2 * ms, np = ms * (size_t)cfg.max_points;
  tab.cap = spare.cap = (uint32_t)cap;
  tab.key = fix<unsigned long long>(cap, "key table");
  tab.slot = fix<int32_t>(cap, "key table sessions");
  spare.key = fix<unsigned long long>(cap, "spare key table");
  spare.slot = fix<int32_t>(cap, "spare key table sessions");
  st.max_sessions = cfg.max_sessions;
  st.max_points = cfg.max_points;
  st.n = fix<int32_t>(ms, "session sizes");
  st.max_sep = fix<float>(ms, "session max_sep");
  st.last = fix<int64_t>(ms, "session last_update");
  st.skey = fix<unsigned long long>(ms, "session keys");
  st.entry = fix<int32_t>(ms, "session entries");
  st.lat = fix<float>(np, "session points lat");
  st.lon = fix<float>(np, "session points lon");
  st.acc = fix<int32_t>(np, "session points accuracy");
  st.time = fix<int64_t>(np, "session points time");
  free_list = fix<int32_t>(ms, "free sessions");
  cnt = fix<int32_t>(SES_WORDS, "store counters");
  if (dir.uuid_bytes > 0) {
    dir.row = name_row_bytes(dir.uuid_bytes);
    dir.bytes = fix<uint8_t>(ms * (size_t)dir.row, "session names");
    dir.len = fix<int32_t>(ms, "session name lengths");
    name_first = fix<int32_t>(cap, "name scratch words");
    HIPCHK(hipMemsetAsync(dir.bytes, 0, ms * (size_t)dir.row, stream));
    HIPCHK(hipMemsetAsync(dir.len, 0, 4 * ms, stream));
    HIPCHK(hipMemsetAsync(name_first, 0x7F, 4 * cap, stream));
  }
  HIPCHK(hipMemsetAsync(tab.key, 0xFF, 8 * cap, stream));
  HIPCHK(hipMemsetAsync(tab.slot, 0xFF, 4 * cap, stream));
  HIPCHK(hipMemsetAsync(st.n, 0, 4 * ms, stream));
  HIPCHK(hipMemsetAsync(st.max_sep, 0, 4 * ms, stream));
  HIPCHK(hipMemsetAsync(st.last, 0, 8 * ms, stream));
  HIPCHK(hipMemsetAsync(st.skey, 0xFF, 8 * ms, stream));
  std::vector<int32_t> fl(ms);
  for (size_t i = 0; i < ms; ++i) fl[i] = (int32_t)(ms - 1 - i);  // session 0 on top
  h_cnt[SES_NFREE] = cfg.max_sessions;
  HIPCHK(hipMemcpyAsync(free_list, fl.data(), 4 * ms, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(cnt, h_cnt, sizeof(h_cnt), hipMemcpyHostToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream));
  for (auto& e : ev) HIPCHK(hipEventCreate(&e));
  ev_init = true;
  return OTR_OK;
}

// live + dead entries beyond half the table: the live ones into the spare table
int SessionStore::rebuild(std::string* err) {
  HIPCHK(hipMemsetAsync(spare.key, 0xFF, 8 * (size_t)spare.cap, stream));
  HIPCHK(hipMemsetAsync(spare.slot, 0xFF, 4 * (size_t)spare.cap, stream));
  k_ses_rebuild<<<grid_ceil1(tab.cap, 256), 256, 0, stream>>>(tab, spare, st);
  HIPCHK(hipGetLastError());
  std::swap(tab, spare);
  h_cnt[SES_DEAD] = 0;
  HIPCHK(hipMemsetAsync(cnt + SES_DEAD, 0, 4, stream));
  ++n_rebuilds;
  return OTR_OK;
}

// the names of a call in device memory (copied when they are the host's)
int SessionStore::names_in(const otr_session_names* names, int64_t n, int memory, SesNamesIn* out, std::string* err) {
  *out = SesNamesIn{nullptr, 0, nullptr, nullptr};
  if (n <= 0) return OTR_OK;
  if (!names->off || !names->len || (names->n_bytes > 0 && !names->bytes)) {
    if (err) *err = "null argument";
    return OTR_BAD_REQUEST;
  }
  if (names->n_bytes < 0 || names->n_bytes > (int64_t)1 << 40) {
    if (err) *err = "name bytes out of range (2^40 at most)";
    return OTR_BAD_REQUEST;
  }
  out->n_bytes = names->n_bytes;
  if (memory == OTR_MEM_DEVICE) {
    out->bytes = names->bytes;
    out->off = names->off;
    out->len = names->len;
    return OTR_OK;
  }
  uint8_t* bytes = get<uint8_t>(B_NM_BYTES, names->n_bytes);
  int64_t* off = get<int64_t>(B_NM_OFF, n);
  int32_t* len = get<int32_t>(B_NM_LEN, n);
  if (names->n_bytes > 0)
    HIPCHK(hipMemcpyAsync(bytes, names->bytes, (size_t)names->n_bytes, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(off, names->off, 8 * (size_t)n, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(len, names->len, 4 * (size_t)n, hipMemcpyHostToDevice, stream));
  out->bytes = bytes;
  out->off = off;
  out->len = len;
  return OTR_OK;
}

int SessionStore::chunk_begin(const otr_session_points* pts, const SesNamesIn* nm, std::string* err) {
  int rc;
  const int64_t n = pts->n;
  W = 0;
  if (n <= 0) return OTR_OK;
  if (n > (int64_t)1 << 30) {
    if (err) *err = "too many points for one chunk (2^30 at most)";
    return OTR_BAD_REQUEST;
  }
  if (h_cnt[SES_DEAD] > 0 && live() + h_cnt[SES_DEAD] > cfg.max_sessions && (rc = rebuild(err))) return rc;
  unsigned long long* key = get<unsigned long long>(B_KEY, n);
  float* lat = get<float>(B_LAT, n);
  float* lon = get<float>(B_LON, n);
  int32_t* acc = get<int32_t>(B_ACC, n);
  int64_t* time = get<int64_t>(B_TIME, n);
  int64_t* ts = get<int64_t>(B_TS, n);
  int32_t* entry = get<int32_t>(B_ENTRY, n);
  int32_t* fresh = get<int32_t>(B_NEW, n);
  int32_t* rank = get<int32_t>(B_RANK, n);
  uint32_t* lane_slot = get<uint32_t>(B_LANE_SLOT, n);
  int32_t* idx = get<int32_t>(B_IDX, n);
  uint32_t* sorted_slot = get<uint32_t>(B_SORT_SLOT, n);
  int32_t* sorted_idx = get<int32_t>(B_SORT_IDX, n);
  int32_t* head = get<int32_t>(B_HEAD, n);
  int32_t* seg_incl = get<int32_t>(B_SEG_INCL, n);
  int32_t* trip = get<int32_t>(B_TRIP, n);
  get<int32_t>(B_TRIP_INCL, n);
  const hipMemcpyKind kind = pts->memory == OTR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIPCHK(hipMemcpyAsync(key, pts->key, 8 * n, kind, stream));
  HIPCHK(hipMemcpyAsync(lat, pts->lat, 4 * n, kind, stream));
  HIPCHK(hipMemcpyAsync(lon, pts->lon, 4 * n, kind, stream));
  HIPCHK(hipMemcpyAsync(acc, pts->accuracy, 4 * n, kind, stream));
  HIPCHK(hipMemcpyAsync(time, pts->time, 8 * n, kind, stream));
  HIPCHK(hipMemcpyAsync(ts, pts->timestamp, 8 * n, kind, stream));
  ch = SesChunk{n, key, lat, lon, acc, time, ts};
  const unsigned g = grid_ceil1(n, 256);
  // 1. keys into the table
  HIPCHK(hipMemsetAsync(cnt + SES_FLAGS, 0, 4, stream));
  k_ses_insert<<<g, 256, 0, stream>>>(tab, ch, entry, fresh, cnt);
  if ((rc = scan(fresh, rank, n, err))) return rc;
  int32_t n_new = 0, flags = 0;
  unsigned long long h_bad = kSesNoBad;
  if (nm) {  // K18: the names against the directory, read back with the chunk's own refusals
    unsigned long long* bad = get<unsigned long long>(B_RS_BAD, 1);
    HIPCHK(hipMemsetAsync(bad, 0xFF, 8, stream));
    k_ses_name_first<<<g, 256, 0, stream>>>(tab, n, entry, name_first);
    k_ses_name_check<<<g, 256, 0, stream>>>(tab, dir, *nm, n, entry, name_first, bad);
    HIPCHK(hipMemcpyAsync(&h_bad, bad, 8, hipMemcpyDeviceToHost, stream));
  }
  if ((rc = read_back(stream, err, fetch(&n_new, rank + (n - 1)), fetch(&flags, cnt + SES_FLAGS)))) return rc;
  const bool own = flags || n_new > h_cnt[SES_NFREE];
  if (own || h_bad != kSesNoBad) {
    if (nm) k_ses_name_unmark<<<g, 256, 0, stream>>>(n, entry, fresh, name_first);
    k_ses_rollback<<<g, 256, 0, stream>>>(tab, n, entry, fresh);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    if (!own) {
      static const char* const why[] = {"", "name longer than uuid_bytes", "the key is live under another name",
                                        "name layout"};
      refusal.point = (int64_t)(h_bad >> 8);
      refusal.reason = (int32_t)(h_bad & 0xFF);
      if (err) *err = "point " + std::to_string(refusal.point) + ": " + why[refusal.reason & 3];
    } else if (err)
      *err = (flags & kSesFlagNoId) ? "key OTR_NO_ID is the store's empty mark"
                                    : "the chunk would take the live sessions beyond max_sessions (" +
                                          std::to_string(live()) + " live, " + std::to_string(cfg.max_sessions) +
                                          " at most)";
    return OTR_BAD_REQUEST;
  }
  // 2. storage for the new keys, 3. the chunk grouped by session, arrival order kept
  if (n_new) {
    k_ses_assign<<<g, 256, 0, stream>>>(tab, st, ch, entry, fresh, rank, free_list, h_cnt[SES_NFREE]);
    k_ses_add<<<1, 1, 0, stream>>>(cnt + SES_NFREE, -n_new);
    h_cnt[SES_NFREE] -= n_new;
    if (nm) k_ses_name_write<<<g, 256, 0, stream>>>(tab, dir, *nm, n, entry, fresh, name_first);
  }
  k_ses_lane_slot<<<g, 256, 0, stream>>>(tab, n, entry, lane_slot, idx);
  int bits = 1;
  while (bits < 32 && ((int64_t)1 << bits) < (int64_t)cfg.max_sessions) ++bits;
  if ((rc = pool_sort(*this, B_TMP, lane_slot, sorted_slot, idx, sorted_idx, n, 0, bits, stream, err))) return rc;
  k_ses_heads<<<g, 256, 0, stream>>>(sorted_slot, n, head);
  if ((rc = scan(head, seg_incl, n, err))) return rc;
  if ((rc = read_back(stream, err, fetch(&n_seg, seg_incl + (n - 1))))) return rc;
  int32_t* seg_slot = get<int32_t>(B_SEG_SLOT, n_seg);
  int32_t* seg_cur = get<int32_t>(B_SEG_CUR, n_seg);
  int32_t* seg_end = get<int32_t>(B_SEG_END, n_seg);
  k_ses_segments<<<g, 256, 0, stream>>>(sorted_slot, seg_incl, n, seg_slot, seg_cur, seg_end);
  HIPCHK(hipMemsetAsync(trip, 0, 4 * n, stream));
  HIPCHK(hipGetLastError());
  chunk_open = true;
  return OTR_OK;
}

int SessionStore::release_list(const int32_t* list, int32_t n, std::string* err) {
  k_ses_release<<<grid_ceil1(n, 256), 256, 0, stream>>>(n, list, tab, st, free_list, cnt);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h_cnt, cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return OTR_OK;
}

// offsets, then one wave per window (win_slot / win_n of W windows are in place)
int SessionStore::gather(std::string* err) {
  int rc;
  int64_t* off = get<int64_t>(B_G_OFF, (size_t)W + 1);
  HIPCHK(hipMemsetAsync(off, 0, 8, stream));
  if ((rc = scan((int64_t*)b[B_W_N].p, off + 1, W, err))) return rc;
  w_key.resize(W);
  w_trig.resize(W);
  w_n.resize(W);
  HIPCHK(hipMemcpyAsync(&P, off + W, 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(w_key.data(), b[B_W_KEY].p, 8 * (size_t)W, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(w_trig.data(), b[B_W_TRIG].p, 8 * (size_t)W, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(w_n.data(), b[B_W_N].p, 8 * (size_t)W, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  double* lat = get<double>(B_G_LAT, P);
  double* lon = get<double>(B_G_LON, P);
  int64_t* time = get<int64_t>(B_G_TIME, P);
  float* acc = get<float>(B_G_ACC, P);
  uint8_t* mode = get<uint8_t>(B_G_MODE, W);
  k_ses_gather<false><<<(unsigned)W, 64, 0, stream>>>(W, (const int32_t*)b[B_W_SLOT].p, off, st, lat, lon, time, acc,
                                                      mode, (uint8_t)cfg.mode, nullptr, nullptr, nullptr);
  HIPCHK(hipGetLastError());
  w_su.assign(W, -1);
  w_status.assign(W, OTR_OK);
  w_trim.assign(W, 0);
  return OTR_OK;
}

// one round: advance every key with unconsumed points, list the tripped ones by trigger
int SessionStore::round(std::string* err) {
  int rc;
  const int64_t n = ch.n;
  int32_t* trip = (int32_t*)b[B_TRIP].p;
  int32_t* trip_incl = (int32_t*)b[B_TRIP_INCL].p;
  const SesGate gate{cfg.report_dist, cfg.report_count, cfg.report_time};
  k_ses_advance<<<grid_ceil1(n_seg, 64), 64, 0, stream>>>(n_seg, (const int32_t*)b[B_SEG_SLOT].p,
                                                          (int32_t*)b[B_SEG_CUR].p, (const int32_t*)b[B_SEG_END].p,
                                                          (const int32_t*)b[B_SORT_IDX].p, ch, st, gate, trip, cnt);
  if ((rc = scan(trip, trip_incl, n, err))) return rc;
  if ((rc = read_back(stream, err, fetch(&W, trip_incl + (n - 1))))) return rc;
  if (W == 0) {  // the chunk is consumed: sessions left empty are deleted
    chunk_open = false;
    return release_list((const int32_t*)b[B_SEG_SLOT].p, n_seg, err);
  }
  int32_t* win_slot = get<int32_t>(B_W_SLOT, W);
  int64_t* win_trig = get<int64_t>(B_W_TRIG, W);
  int64_t* win_n = get<int64_t>(B_W_N, W);
  unsigned long long* win_key = get<unsigned long long>(B_W_KEY, W);
  k_ses_windows<<<grid_ceil1(n, 256), 256, 0, stream>>>(n, trip, trip_incl, (const uint32_t*)b[B_LANE_SLOT].p, st,
                                                        win_slot, win_trig, win_n, win_key);
  if ((rc = gather(err))) return rc;
  pending = true;
  return OTR_OK;
}

void SessionStore::fill_batch(otr_trace_batch* bt) {
  memset(bt, 0, sizeof(*bt));
  bt->memory = OTR_MEM_DEVICE;
  bt->report_levels = cfg.report_levels;
  bt->transition_levels = cfg.transition_levels;
  bt->threshold_sec = cfg.threshold_sec;
  bt->quantisation = 3600;
  bt->n_traces = W;
  bt->trace_offsets = (const int64_t*)b[B_G_OFF].p;
  if (W > 0) {
    bt->lat = (const double*)b[B_G_LAT].p;
    bt->lon = (const double*)b[B_G_LON].p;
    bt->time = (const int64_t*)b[B_G_TIME].p;
    bt->accuracy = (const float*)b[B_G_ACC].p;
    bt->mode = (const uint8_t*)b[B_G_MODE].p;
  }
}

int SessionStore::commit(const int32_t* su, const int32_t* status, int memory, std::string* err) {
  int32_t* d_su = get<int32_t>(B_W_SU, W);
  int32_t* d_status = get<int32_t>(B_W_STATUS, W);
  int32_t* d_su_out = get<int32_t>(B_W_SU_OUT, W);
  int32_t* d_trim = get<int32_t>(B_W_TRIM, W);
  const hipMemcpyKind kind = memory == OTR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIPCHK(hipMemcpyAsync(d_su, su, 4 * (size_t)W, kind, stream));
  HIPCHK(hipMemcpyAsync(d_status, status, 4 * (size_t)W, kind, stream));
  k_ses_commit<<<(unsigned)W, 64, 0, stream>>>(W, (const int32_t*)b[B_W_SLOT].p, d_su, d_status, st, d_su_out, d_trim);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(w_su.data(), d_su_out, 4 * (size_t)W, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(w_trim.data(), d_trim, 4 * (size_t)W, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(w_status.data(), d_status, 4 * (size_t)W, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  pending = false;
  return OTR_OK;
}

void SessionStore::result_begin() {
  res_have = false;
  for (auto* v : {&r_key, &r_id, &r_next}) v->clear();
  for (auto* v : {&r_trig, &r_off}) v->clear();
  for (auto* v : {&r_n, &r_su, &r_status, &r_trim, &r_len, &r_queue}) v->clear();
  r_t0.clear();
  r_t1.clear();
  r_off.push_back(0);
  r_rounds = 0;
  r_evicted = 0;
  r_match_ms = 0.0;
  forced0 = h_cnt[SES_FORCED];
  dropped0 = h_cnt[SES_DROPPED];
}

// the windows of the round into the call's result (their reports are already in r_id ...
// with one r_off entry per window)
void SessionStore::result_round() {
  for (int32_t w = 0; w < W; ++w) {
    r_key.push_back(w_key[w]);
    r_trig.push_back(w_trig[w]);
    r_n.push_back((int32_t)w_n[w]);
    r_su.push_back(w_su[w]);
    r_status.push_back(w_status[w]);
    r_trim.push_back(w_trim[w]);
  }
}

// the windows of the round through the matcher, in device batches of at most batch_probes
// probes: shape_used, status and the reports of every window
int SessionStore::match(Matcher& m, std::string* err) {
  const int64_t limit = cfg.batch_probes > 0 ? std::min<int64_t>(cfg.batch_probes, kMaxBatchProbes) : kMaxBatchProbes;
  std::vector<int64_t> sub;
  int32_t w0 = 0;
  int64_t p0 = 0;
  while (w0 < W) {
    int32_t w1 = w0 + 1;
    int64_t np = w_n[w0];
    while (w1 < W && np + w_n[w1] <= limit) np += w_n[w1++];
    otr_trace_batch bt;
    fill_batch(&bt);
    bt.flags = OTR_BATCH_COPY_REPORTS;
    bt.n_traces = w1 - w0;
    if (w0 > 0 || w1 < W) {  // offsets from zero for this part
      sub.assign(1, 0);
      for (int32_t w = w0; w < w1; ++w) sub.push_back(sub.back() + w_n[w]);
      int64_t* d_sub = get<int64_t>(B_SUB_OFF, sub.size());
      HIPCHK(hipMemcpyAsync(d_sub, sub.data(), 8 * sub.size(), hipMemcpyHostToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));
      bt.trace_offsets = d_sub;
      bt.lat += p0;
      bt.lon += p0;
      bt.time += p0;
      bt.accuracy += p0;
      bt.mode += w0;
    }
    otr_batch_result br;
    std::string e2;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = m.run(&bt, graph_state().defaults, &br, &e2);
    r_match_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int32_t w = w0; w < w1; ++w) {
      const int32_t t = w - w0;
      const int32_t status = rc != OTR_OK ? rc : br.trace_status[t];
      w_status[w] = status;
      w_su[w] = status == OTR_OK ? br.shape_used[t] : -1;
      if (status == OTR_OK)
        for (int64_t k = br.trace_rep_off[t]; k < br.trace_rep_off[t + 1]; ++k) {
          r_id.push_back(br.rep_id[k]);
          r_next.push_back(br.rep_next[k]);
          r_t0.push_back(br.rep_t0[k]);
          r_t1.push_back(br.rep_t1[k]);
          r_len.push_back(br.rep_length[k]);
          r_queue.push_back(br.rep_queue[k]);
        }
      r_off.push_back((int64_t)r_id.size());
    }
    if (rc != OTR_OK && err) *err = e2;
    p0 += np;
    w0 = w1;
  }
  return OTR_OK;
}

int SessionStore::result_end(otr_session_result* out, bool with_device, std::string* err) {
  memset(out, 0, sizeof(*out));
  const size_t nw = r_key.size(), nr = r_id.size();
  out->n_windows = (int64_t)nw;
  out->n_reports = (int64_t)nr;
  out->n_rounds = r_rounds;
  out->n_live = live();
  out->n_forced = h_cnt[SES_FORCED] - forced0;
  out->n_dropped = h_cnt[SES_DROPPED] - dropped0;
  out->n_evicted = r_evicted;
  out->n_rebuilds = n_rebuilds;
  out->match_ms = (float)r_match_ms;
  auto P_ = [](auto& v) { return v.empty() ? nullptr : v.data(); };
  out->key = (uint64_t*)P_(r_key);
  out->trigger = P_(r_trig);
  out->n_points = P_(r_n);
  out->shape_used = P_(r_su);
  out->status = P_(r_status);
  out->trimmed = P_(r_trim);
  out->rep_off = P_(r_off);
  out->id = (uint64_t*)P_(r_id);
  out->next_id = (uint64_t*)P_(r_next);
  out->t0 = P_(r_t0);
  out->t1 = P_(r_t1);
  out->length = P_(r_len);
  out->queue_length = P_(r_queue);
  if (!with_device) return OTR_OK;
  auto up = [&](int slot, auto& v, auto** dst) -> int {
    using T = typename std::remove_reference_t<decltype(v)>::value_type;
    T* d = get<T>(slot, v.size());
    if (!v.empty()) HIPCHK(hipMemcpyAsync(d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, stream));
    *dst = d;
    return OTR_OK;
  };
  int rc;
  unsigned long long *dk, *di, *dn;
  if ((rc = up(B_R_KEY, r_key, &dk)) || (rc = up(B_R_TRIG, r_trig, &out->d_trigger)) ||
      (rc = up(B_R_N, r_n, &out->d_n_points)) || (rc = up(B_R_SU, r_su, &out->d_shape_used)) ||
      (rc = up(B_R_STATUS, r_status, &out->d_status)) || (rc = up(B_R_TRIM, r_trim, &out->d_trimmed)) ||
      (rc = up(B_R_OFF, r_off, &out->d_rep_off)) || (rc = up(B_R_ID, r_id, &di)) ||
      (rc = up(B_R_NEXT, r_next, &dn)) || (rc = up(B_R_T0, r_t0, &out->d_t0)) || (rc = up(B_R_T1, r_t1, &out->d_t1)) ||
      (rc = up(B_R_LEN, r_len, &out->d_length)) || (rc = up(B_R_QUEUE, r_queue, &out->d_queue_length)))
    return rc;
  out->d_key = (uint64_t*)dk;
  out->d_id = (uint64_t*)di;
  out->d_next_id = (uint64_t*)dn;
  HIPCHK(hipEventRecord(ev[1], stream));
  HIPCHK(hipStreamSynchronize(stream));
  HIPCHK(hipEventElapsedTime(&out->device_ms, ev[0], ev[1]));
  res_have = true;
  res_added = false;
  return OTR_OK;
}

bool sessions_last_reports(SessionStore* s, SessionReports* out) {
  if (!s || !s->res_have) return false;
  out->n_windows = (int64_t)s->r_key.size();
  out->n_reports = (int64_t)s->r_id.size();
  out->trigger = (const int64_t*)s->b[B_R_TRIG].p;
  out->rep_off = (const int64_t*)s->b[B_R_OFF].p;
  out->id = (const unsigned long long*)s->b[B_R_ID].p;
  out->next_id = (const unsigned long long*)s->b[B_R_NEXT].p;
  out->t0 = (const double*)s->b[B_R_T0].p;
  out->t1 = (const double*)s->b[B_R_T1].p;
  out->length = (const int32_t*)s->b[B_R_LEN].p;
  out->queue_length = (const int32_t*)s->b[B_R_QUEUE].p;
  out->added = &s->res_added;
  return true;
}

// sessions (all live ones, or the stale ones at ts) in ascending key order: n_list of them
// in B_L_KEY2 / B_L_SLOT2
int SessionStore::list_sessions(int stale_only, int64_t ts, std::string* err) {
  const int32_t ms = cfg.max_sessions;
  int32_t* flag = get<int32_t>(B_FLAG, ms);
  k_ses_flag<<<grid_ceil1(ms, 256), 256, 0, stream>>>(st, stale_only, ts, cfg.session_gap, flag);
  return list_flagged(err);
}

// the sessions flagged in B_FLAG, in ascending key order
int SessionStore::list_flagged(std::string* err) {
  int rc;
  const int32_t ms = cfg.max_sessions;
  int32_t* flag = (int32_t*)b[B_FLAG].p;
  int32_t* incl = get<int32_t>(B_FLAG_INCL, ms);
  if ((rc = scan(flag, incl, ms, err))) return rc;
  if ((rc = read_back(stream, err, fetch(&n_list, incl + (ms - 1))))) return rc;
  if (n_list == 0) return OTR_OK;
  unsigned long long* key = get<unsigned long long>(B_L_KEY, n_list);
  int32_t* slot = get<int32_t>(B_L_SLOT, n_list);
  unsigned long long* key2 = get<unsigned long long>(B_L_KEY2, n_list);
  int32_t* slot2 = get<int32_t>(B_L_SLOT2, n_list);
  k_ses_list<<<grid_ceil1(ms, 256), 256, 0, stream>>>(st, flag, incl, key, slot);
  if ((rc = pool_sort(*this, B_TMP, key, key2, slot, slot2, n_list, 0, 64, stream, err))) return rc;
  HIPCHK(hipGetLastError());
  return OTR_OK;
}

// K18: the names of the sessions listed in B_L_SLOT2, in the listing's order, in HBM
// (B_NL_OFF / B_NL_BYTES) and in nl_off / nl_bytes
int SessionStore::names_list(std::string* err) {
  int rc;
  const int32_t ns = n_list;
  nl_off.assign((size_t)ns + 1, 0);
  nl_bytes.clear();
  int64_t* off = get<int64_t>(B_NL_OFF, (size_t)ns + 1);
  get<uint8_t>(B_NL_BYTES, 0);
  HIPCHK(hipMemsetAsync(off, 0, 8, stream));
  names_have = true;
  if (ns == 0) {
    HIPCHK(hipStreamSynchronize(stream));
    return OTR_OK;
  }
  const int32_t* list = (const int32_t*)b[B_L_SLOT2].p;
  int64_t* len = get<int64_t>(B_NL_LEN, ns);
  k_ses_name_len<<<grid_ceil1(ns, 256), 256, 0, stream>>>(ns, list, dir, len);
  if ((rc = scan(len, off + 1, ns, err))) return rc;
  HIPCHK(hipMemcpyAsync(nl_off.data(), off, 8 * ((size_t)ns + 1), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  const int64_t nb = nl_off[ns];
  uint8_t* bytes = get<uint8_t>(B_NL_BYTES, nb);
  k_ses_name_gather<<<grid_ceil1(ns, 256), 256, 0, stream>>>(ns, list, off, dir, bytes);
  HIPCHK(hipGetLastError());
  nl_bytes.resize((size_t)nb);
  if (nb > 0) HIPCHK(hipMemcpyAsync(nl_bytes.data(), bytes, (size_t)nb, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return OTR_OK;
}

// K18: the key-ordered list of B_L_KEY2 / B_L_SLOT2 into ascending name order (ties keep the
// key order): stable LSD passes over a permutation, the length first, then the sort words of
// the rows from the last to the first
int SessionStore::name_order(std::string* err) {
  int rc;
  const int32_t ns = n_list;
  if (ns < 2) return OTR_OK;
  const unsigned g = grid_ceil1(ns, 256);
  unsigned long long* key = get<unsigned long long>(B_NS_KEY, ns);
  unsigned long long* key2 = get<unsigned long long>(B_NS_KEY2, ns);
  int32_t* perm = get<int32_t>(B_NS_PERM, ns);
  int32_t* perm2 = get<int32_t>(B_NS_PERM2, ns);
  int32_t* list = (int32_t*)b[B_L_SLOT2].p;
  unsigned long long* lkey = (unsigned long long*)b[B_L_KEY2].p;
  Workspace tmp;  // one for every pass, sized before the first launch
  if ((rc = sort_bytes(key, key2, perm, perm2, ns, 0, 64, &tmp.bytes, stream, err))) return rc;
  tmp.p = get<char>(B_TMP, tmp.bytes);
  k_ses_iota<<<g, 256, 0, stream>>>(ns, perm);
  for (int32_t w = -1, pass = 0; pass <= name_sort_words(dir.uuid_bytes); ++pass) {
    k_ses_name_sort_key<<<g, 256, 0, stream>>>(ns, list, perm, dir, w, key);
    if ((rc = sort_pairs(tmp, key, key2, perm, perm2, ns, 0, w < 0 ? 9 : 64, stream, err))) return rc;
    std::swap(perm, perm2);
    w = w < 0 ? name_sort_words(dir.uuid_bytes) - 1 : w - 1;
  }
  // (the unsorted list's buffers are free by now)
  int32_t* list_out = (int32_t*)b[B_L_SLOT].p;
  unsigned long long* key_out = (unsigned long long*)b[B_L_KEY].p;
  k_ses_permute<<<g, 256, 0, stream>>>(ns, perm, list, lkey, list_out, key_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(list, list_out, 4 * (size_t)ns, hipMemcpyDeviceToDevice, stream));
  HIPCHK(hipMemcpyAsync(lkey, key_out, 8 * (size_t)ns, hipMemcpyDeviceToDevice, stream));
  return OTR_OK;
}

// the sessions listed in B_L_KEY2 / B_L_SLOT2 as a snapshot in the store's host arrays
int SessionStore::snapshot_list(otr_session_snapshot* out, std::string* err) {
  int rc;
  memset(out, 0, sizeof(*out));
  const int32_t ns = n_list;
  s_off.assign((size_t)ns + 1, 0);
  out->point_off = s_off.data();
  if (named() && (rc = names_list(err))) return rc;
  if (ns == 0) return OTR_OK;
  const int32_t* list = (const int32_t*)b[B_L_SLOT2].p;
  int32_t* rep = get<int32_t>(B_L_REP, ns);
  int64_t* cnt_n = get<int64_t>(B_L_N, ns);
  // (B_SUB_OFF, not the batch's offsets: an advance's empty batch stays what it is)
  int64_t* off = get<int64_t>(B_SUB_OFF, (size_t)ns + 1);
  k_ses_evict_gate<<<grid_ceil1(ns, 256), 256, 0, stream>>>(ns, list, st, rep, cnt_n);
  HIPCHK(hipMemsetAsync(off, 0, 8, stream));
  if ((rc = scan(cnt_n, off + 1, ns, err))) return rc;
  const size_t ms = (size_t)cfg.max_sessions;
  s_key.resize(ns);
  s_slot.resize(ns);
  all_sep.resize(ms);
  all_last.resize(ms);
  HIPCHK(hipMemcpyAsync(s_off.data(), off, 8 * ((size_t)ns + 1), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(s_key.data(), b[B_L_KEY2].p, 8 * (size_t)ns, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(s_slot.data(), list, 4 * (size_t)ns, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(all_sep.data(), st.max_sep, 4 * ms, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(all_last.data(), st.last, 8 * ms, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  const int64_t np = s_off[ns];
  float* lat = get<float>(B_S_LAT, np);
  float* lon = get<float>(B_S_LON, np);
  int32_t* acc = get<int32_t>(B_S_ACC, np);
  int64_t* time = get<int64_t>(B_G_TIME, np);
  k_ses_gather<true><<<(unsigned)ns, 64, 0, stream>>>(ns, list, off, st, nullptr, nullptr, time, nullptr, nullptr, 0,
                                                      lat, lon, acc);
  HIPCHK(hipGetLastError());
  s_lat.resize(np);
  s_lon.resize(np);
  s_acc.resize(np);
  s_time.resize(np);
  HIPCHK(hipMemcpyAsync(s_lat.data(), lat, 4 * (size_t)np, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(s_lon.data(), lon, 4 * (size_t)np, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(s_acc.data(), acc, 4 * (size_t)np, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(s_time.data(), time, 8 * (size_t)np, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  s_sep.resize(ns);
  s_last.resize(ns);
  for (int32_t i = 0; i < ns; ++i) {
    s_sep[i] = all_sep[s_slot[i]];
    s_last[i] = all_last[s_slot[i]];
  }
  out->n_sessions = ns;
  out->n_points = np;
  out->key = (uint64_t*)s_key.data();
  out->max_sep = s_sep.data();
  out->last_update = s_last.data();
  out->lat = s_lat.data();
  out->lon = s_lon.data();
  out->accuracy = s_acc.data();
  out->time = s_time.data();
  return OTR_OK;
}

// K17: the given sessions (device arrays) merged into the store, all or nothing
template <bool REC>
int SessionStore::restore(SesGiven g, const SesNamesIn* nm, otr_session_restore_result* out, std::string* err) {
  int rc;
  const int64_t n = g.n;
  out->n_live = live();
  if (n == 0) return OTR_OK;
  if (h_cnt[SES_DEAD] > 0 && live() + h_cnt[SES_DEAD] > cfg.max_sessions && (rc = rebuild(err))) return rc;
  int32_t* entry = get<int32_t>(B_ENTRY, n);
  int32_t* fresh = get<int32_t>(B_NEW, n);
  unsigned long long* bad = get<unsigned long long>(B_RS_BAD, 1);
  int32_t* first = spare.slot;  // scratch: the spare table is only used inside a rebuild
  HIPCHK(hipMemsetAsync(first, 0x7F, 4 * (size_t)spare.cap, stream));
  HIPCHK(hipMemsetAsync(bad, 0xFF, 8, stream));
  HIPCHK(hipMemsetAsync(cnt + SES_FLAGS, 0, 4, stream));
  const unsigned grid = grid_ceil1(n, 256);
  k_ses_restore_check<REC><<<grid, 256, 0, stream>>>(tab, g, cfg.max_points, first, entry, fresh, bad, cnt);
  if (nm) k_ses_restore_name_check<<<grid, 256, 0, stream>>>(dir, *nm, n, bad);
  HIPCHK(hipGetLastError());
  unsigned long long h_bad = kSesNoBad;
  int32_t flags = 0;
  if ((rc = read_back(stream, err, fetch(&h_bad, bad), fetch(&flags, cnt + SES_FLAGS)))) return rc;
  if (flags) {
    // more keys than the table has room for (a refusal either way): lanes that found no entry
    // could not see each other, so the occurrences of a key are counted here
    std::vector<unsigned long long> keys((size_t)n);
    HIPCHK(hipMemcpyAsync(keys.data(), g.key, 8 * (size_t)n, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    std::vector<std::pair<unsigned long long, int64_t>> order((size_t)n);
    for (int64_t i = 0; i < n; ++i) order[i] = {keys[i], i};
    std::sort(order.begin(), order.end());
    for (int64_t i = 1; i < n; ++i)
      if (order[i].first == order[i - 1].first)
        h_bad = std::min(h_bad, ((unsigned long long)order[i].second << 8) | OTR_RESTORE_E_DUPLICATE);
  }
  const bool full = n > (int64_t)h_cnt[SES_NFREE];
  if (h_bad != kSesNoBad || full || flags) {
    k_ses_rollback<<<grid, 256, 0, stream>>>(tab, n, entry, fresh);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    static const char* const why[] = {"",
                                      "layout",
                                      "key OTR_NO_ID is the store's empty mark",
                                      "count outside 1 .. max_points - 1",
                                      "duplicate key",
                                      "the key has a live session",
                                      "",
                                      "name layout or longer than uuid_bytes"};
    if (h_bad != kSesNoBad) {
      out->bad_session = (int64_t)(h_bad >> 8);
      out->bad_reason = (int32_t)(h_bad & 0xFF);
      if (err) *err = "session " + std::to_string(out->bad_session) + ": " + why[out->bad_reason];
    } else {
      out->bad_reason = OTR_RESTORE_E_FULL;
      if (err)
        *err = "the restore would take the live sessions beyond max_sessions (" + std::to_string(live()) + " live, " +
               std::to_string(n) + " given, " + std::to_string(cfg.max_sessions) + " at most)";
    }
    return OTR_BAD_REQUEST;
  }
  k_ses_restore_copy<REC><<<(unsigned)n, 64, 0, stream>>>(tab, st, g, entry, free_list, h_cnt[SES_NFREE]);
  if (nm) k_ses_restore_name_copy<<<grid, 256, 0, stream>>>(dir, *nm, n, free_list, h_cnt[SES_NFREE]);
  k_ses_add<<<1, 1, 0, stream>>>(cnt + SES_NFREE, -(int32_t)n);
  HIPCHK(hipGetLastError());
  h_cnt[SES_NFREE] -= (int32_t)n;
  out->n_sessions = n;
  out->n_live = live();
  return OTR_OK;
}

// ---- the matcher's entry points -------------------------------------------------------------

namespace {

// the session calls' preconditions, then the shared guard (an allocation failure of the store's
// pool or of the matcher's, which the rounds and the formatter reach into, ends here)
template <class F>
int guarded(Matcher& m, std::string* err, bool need_store, F&& f, bool keep_names = false) {
  if (need_store && !m.ses) {
    if (err) *err = "no session store: call otr_sessions_open first";
    return OTR_BAD_REQUEST;
  }
  if (m.ses && !keep_names) m.ses->names_have = false;  // a listing's names last until the next session call
  return otr::guarded(m.stream, err, f);
}

int bad(std::string* err, const char* what) {
  if (err) *err = what;
  return OTR_BAD_REQUEST;
}

bool points_ok(const otr_session_points* p) {
  return p->n <= 0 || (p->key && p->lat && p->lon && p->accuracy && p->time && p->timestamp);
}

// K18: a store with a directory takes its points and sessions with names, a plain one without
const char* names_mismatch(const SessionStore& s, bool given) {
  if (s.named() && !given) return "the store has a uuid directory: use the _named call";
  if (!s.named() && given) return "the store has no uuid directory: open it with otr_sessions_open_named";
  return nullptr;
}

}  // namespace

bool Matcher::sessions_named() const { return ses && ses->named(); }

int Matcher::sessions_open(const otr_session_config* cfg, int32_t uuid_bytes, std::string* err) {
  if (ses) return bad(err, "the matcher already has a session store");
  if (uuid_bytes < 0 || uuid_bytes > 255) return bad(err, "uuid_bytes outside 1 .. 255");
  if (cfg->max_sessions < 1 || cfg->max_sessions > (1 << 30) || cfg->max_points < 2 || cfg->mode < 0 ||
      cfg->mode > 2 || (int64_t)cfg->max_sessions * cfg->max_points > ((int64_t)1 << 40) || cfg->report_count < 0)
    return bad(err, "session config out of range");
  HIPCHK(hipSetDevice(graph_state().device));
  if (!stream) HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  SessionStore* s = new SessionStore();
  s->cfg = *cfg;
  s->stream = stream;
  s->dir.uuid_bytes = uuid_bytes;
  const int rc = guarded(*this, err, false, [&] { return s->alloc(err); });
  if (rc != OTR_OK) {
    sessions_destroy(s);
    return rc;
  }
  ses = s;
  return OTR_OK;
}

int Matcher::sessions_close(std::string* err) {
  if (!ses) return bad(err, "no session store");
  sessions_destroy(ses);
  ses = nullptr;
  return OTR_OK;
}

int Matcher::sessions_advance(const otr_session_points* pts, const otr_session_names* names, otr_trace_batch* out,
                              std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    SessionStore& s = *ses;
    int rc;
    HIPCHK(hipSetDevice(graph_state().device));
    if (names) s.refusal = otr_session_name_refusal{-1, -1, 0, 0};
    if (s.pending) return bad(err, "the last advance has not been committed");
    if (pts) {
      if (const char* w = names_mismatch(s, names != nullptr)) return bad(err, w);
      if (s.chunk_open) return bad(err, "the current chunk is not consumed");
      if (!points_ok(pts)) return bad(err, "null argument");
      SesNamesIn nm;
      if (names && (rc = s.names_in(names, pts->n, pts->memory, &nm, err))) return rc;
      if ((rc = s.chunk_begin(pts, names ? &nm : nullptr, err))) return rc;
    }
    s.W = 0;
    if (s.chunk_open && (rc = s.round(err))) return rc;
    if (s.W == 0) {
      int64_t* off = s.get<int64_t>(B_G_OFF, 1);
      HIPCHK(hipMemsetAsync(off, 0, 8, stream));
      HIPCHK(hipStreamSynchronize(stream));
    }
    s.fill_batch(out);
    return OTR_OK;
  });
}

int Matcher::sessions_commit(const int32_t* shape_used, const int32_t* status, int memory, std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    HIPCHK(hipSetDevice(graph_state().device));
    if (!ses->pending) return bad(err, "nothing to commit: no advance with windows is open");
    if (!shape_used || !status) return bad(err, "null argument");
    return ses->commit(shape_used, status, memory, err);
  });
}

int Matcher::sessions_windows(otr_session_result* out, std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    SessionStore& s = *ses;
    s.result_begin();
    s.result_round();
    for (int32_t w = 0; w < s.W; ++w) s.r_off.push_back(0);
    return s.result_end(out, false, err);
  });
}

int Matcher::sessions_push(const otr_session_points* pts, const otr_session_names* names, otr_session_result* out,
                           std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    SessionStore& s = *ses;
    int rc;
    if (names) s.refusal = otr_session_name_refusal{-1, -1, 0, 0};
    if (const char* w = names_mismatch(s, names != nullptr)) return bad(err, w);
    if (!graph_state().ready) {
      if (err) *err = "otr_configure has not been called";
      return OTR_NOT_CONFIGURED;
    }
    HIPCHK(hipSetDevice(graph_state().device));
    if (s.pending || s.chunk_open) return bad(err, "an advance / commit sequence is open");
    if (!points_ok(pts)) return bad(err, "null argument");
    s.result_begin();
    HIPCHK(hipEventRecord(s.ev[0], stream));
    SesNamesIn nm;
    if (names && (rc = s.names_in(names, pts->n, pts->memory, &nm, err))) return rc;
    if ((rc = s.chunk_begin(pts, names ? &nm : nullptr, err))) return rc;
    while (s.chunk_open) {
      if ((rc = s.round(err))) return rc;
      if (s.W == 0) break;
      ++s.r_rounds;
      if ((rc = s.match(*this, err))) return rc;
      if ((rc = s.commit(s.w_su.data(), s.w_status.data(), OTR_MEM_HOST, err))) return rc;
      s.result_round();
    }
    s.W = 0;
    return s.result_end(out, true, err);
  });
}

int Matcher::sessions_punctuate(int64_t ts, otr_session_result* out, std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    SessionStore& s = *ses;
    int rc;
    if (!graph_state().ready) {
      if (err) *err = "otr_configure has not been called";
      return OTR_NOT_CONFIGURED;
    }
    HIPCHK(hipSetDevice(graph_state().device));
    if (s.pending || s.chunk_open) return bad(err, "an advance / commit sequence is open");
    s.result_begin();
    s.W = 0;
    HIPCHK(hipEventRecord(s.ev[0], stream));
    if ((rc = s.list_sessions(1, ts, err))) return rc;
    if (s.named() && (rc = s.name_order(err))) return rc;
    const int32_t ne = s.n_list;
    if (ne > 0) {
      const int32_t* list = (const int32_t*)s.b[B_L_SLOT2].p;
      int32_t* rep = s.get<int32_t>(B_L_REP, ne);
      int32_t* rep_incl = s.get<int32_t>(B_L_REP_INCL, ne);
      int64_t* cnt_n = s.get<int64_t>(B_L_N, ne);
      k_ses_evict_gate<<<grid_ceil1(ne, 256), 256, 0, stream>>>(ne, list, s.st, rep, cnt_n);
      if ((rc = s.scan(rep, rep_incl, ne, err))) return rc;
      if ((rc = read_back(stream, err, fetch(&s.W, rep_incl + (ne - 1))))) return rc;
      if (s.W > 0) {
        int32_t* win_slot = s.get<int32_t>(B_W_SLOT, s.W);
        int64_t* win_trig = s.get<int64_t>(B_W_TRIG, s.W);
        int64_t* win_n = s.get<int64_t>(B_W_N, s.W);
        unsigned long long* win_key = s.get<unsigned long long>(B_W_KEY, s.W);
        k_ses_evict_windows<<<grid_ceil1(ne, 256), 256, 0, stream>>>(
            ne, list, (const unsigned long long*)s.b[B_L_KEY2].p, rep, rep_incl, cnt_n, win_slot, win_trig, win_n,
            win_key);
        if ((rc = s.gather(err))) return rc;
        s.r_rounds = 1;
        if ((rc = s.match(*this, err))) return rc;
        for (int32_t w = 0; w < s.W; ++w) {  // the session is deleted whatever the report used
          s.w_trim[w] = (int32_t)s.w_n[w];
          if (s.w_su[w] <= 0) s.w_su[w] = -1;
        }
        s.result_round();
      }
      k_ses_clear<<<grid_ceil1(ne, 256), 256, 0, stream>>>(ne, list, s.st);
      if ((rc = s.release_list(list, ne, err))) return rc;
      s.r_evicted = ne;
    }
    s.W = 0;
    return s.result_end(out, true, err);
  });
}

int Matcher::sessions_snapshot(otr_session_snapshot* out, std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    SessionStore& s = *ses;
    int rc;
    HIPCHK(hipSetDevice(graph_state().device));
    if (s.pending) return bad(err, "the last advance has not been committed");
    if ((rc = s.list_sessions(0, 0, err))) return rc;
    return s.snapshot_list(out, err);
  });
}

// ---- K17: restore, export and move ------------------------------------------------------------

namespace {

void restore_result_begin(otr_session_restore_result* out) {
  memset(out, 0, sizeof(*out));
  out->bad_session = -1;
}

}  // namespace

int Matcher::sessions_restore(const otr_session_snapshot* snap, const otr_session_names* names, int memory,
                              otr_session_restore_result* out, std::string* err) {
  restore_result_begin(out);
  return guarded(*this, err, true, [&]() -> int {
    SessionStore& s = *ses;
    int rc;
    HIPCHK(hipSetDevice(graph_state().device));
    out->n_live = s.live();
    if (const char* w = names_mismatch(s, names != nullptr)) return bad(err, w);
    if (s.pending || s.chunk_open) return bad(err, "an advance / commit sequence is open");
    const int64_t n = snap->n_sessions, np = snap->n_points;
    if (n < 0 || np < 0 || n > (int64_t)1 << 30 || np > (int64_t)1 << 40)
      return bad(err, "too many sessions for one restore (2^30 at most)");
    if (n == 0) {
      if (np == 0) return OTR_OK;
      out->bad_reason = OTR_RESTORE_E_LAYOUT;
      return bad(err, "layout: points without sessions");
    }
    if (!snap->key || !snap->point_off || !snap->max_sep || !snap->last_update ||
        (np > 0 && (!snap->lat || !snap->lon || !snap->accuracy || !snap->time)))
      return bad(err, "null argument");
    SesGiven g{};
    g.n = n;
    g.total = np;
    HIPCHK(hipEventRecord(s.ev[0], stream));
    if (memory == OTR_MEM_DEVICE) {
      g.key = (const unsigned long long*)snap->key;
      g.off = snap->point_off;
      g.max_sep = snap->max_sep;
      g.last = snap->last_update;
      g.lat = snap->lat;
      g.lon = snap->lon;
      g.acc = snap->accuracy;
      g.time = snap->time;
    } else {
      unsigned long long* key = s.get<unsigned long long>(B_RS_KEY, n);
      int64_t* off = s.get<int64_t>(B_RS_OFF, (size_t)n + 1);
      float* sep = s.get<float>(B_RS_SEP, n);
      int64_t* last = s.get<int64_t>(B_RS_LAST, n);
      float* lat = s.get<float>(B_LAT, np);
      float* lon = s.get<float>(B_LON, np);
      int32_t* acc = s.get<int32_t>(B_ACC, np);
      int64_t* time = s.get<int64_t>(B_TIME, np);
      HIPCHK(hipMemcpyAsync(key, snap->key, 8 * (size_t)n, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(off, snap->point_off, 8 * ((size_t)n + 1), hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(sep, snap->max_sep, 4 * (size_t)n, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(last, snap->last_update, 8 * (size_t)n, hipMemcpyHostToDevice, stream));
      if (np > 0) {
        HIPCHK(hipMemcpyAsync(lat, snap->lat, 4 * (size_t)np, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(lon, snap->lon, 4 * (size_t)np, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(acc, snap->accuracy, 4 * (size_t)np, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(time, snap->time, 8 * (size_t)np, hipMemcpyHostToDevice, stream));
      }
      g.key = key;
      g.off = off;
      g.max_sep = sep;
      g.last = last;
      g.lat = lat;
      g.lon = lon;
      g.acc = acc;
      g.time = time;
    }
    SesNamesIn nm;
    if (names && (rc = s.names_in(names, n, memory, &nm, err))) return rc;
    if ((rc = s.restore<false>(g, names ? &nm : nullptr, out, err))) return rc;
    out->n_points = np;
    HIPCHK(hipEventRecord(s.ev[1], stream));
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipEventElapsedTime(&out->device_ms, s.ev[0], s.ev[1]));
    return OTR_OK;
  });
}

int Matcher::sessions_restore_records(const otr_session_records* recs, const otr_session_names* names,
                                      otr_session_restore_result* out, std::string* err) {
  restore_result_begin(out);
  return guarded(*this, err, true, [&]() -> int {
    SessionStore& s = *ses;
    int rc;
    HIPCHK(hipSetDevice(graph_state().device));
    out->n_live = s.live();
    if (const char* w = names_mismatch(s, names != nullptr)) return bad(err, w);
    if (s.pending || s.chunk_open) return bad(err, "an advance / commit sequence is open");
    const int64_t n = recs->n_records, nb = recs->n_bytes;
    if (n < 0 || nb < 0 || n > (int64_t)1 << 30 || nb > (int64_t)1 << 44)
      return bad(err, "too many sessions for one restore (2^30 at most)");
    if (n == 0) return OTR_OK;
    if (!recs->key || !recs->rec_off || (nb > 0 && !recs->bytes)) return bad(err, "null argument");
    SesGiven g{};
    g.n = n;
    g.total = nb;
    HIPCHK(hipEventRecord(s.ev[0], stream));
    if (recs->memory == OTR_MEM_DEVICE) {
      g.key = (const unsigned long long*)recs->key;
      g.off = recs->rec_off;
      g.bytes = recs->bytes;
    } else {
      unsigned long long* key = s.get<unsigned long long>(B_RS_KEY, n);
      int64_t* off = s.get<int64_t>(B_RS_OFF, (size_t)n + 1);
      uint8_t* bytes = s.get<uint8_t>(B_RS_BYTES, nb);
      HIPCHK(hipMemcpyAsync(key, recs->key, 8 * (size_t)n, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(off, recs->rec_off, 8 * ((size_t)n + 1), hipMemcpyHostToDevice, stream));
      if (nb > 0) HIPCHK(hipMemcpyAsync(bytes, recs->bytes, (size_t)nb, hipMemcpyHostToDevice, stream));
      g.key = key;
      g.off = off;
      g.bytes = bytes;
    }
    SesNamesIn nm;
    if (names && (rc = s.names_in(names, n, recs->memory, &nm, err))) return rc;
    if ((rc = s.restore<true>(g, names ? &nm : nullptr, out, err))) return rc;
    int64_t ends[2] = {0, 0};  // every record was as long as its count says
    HIPCHK(hipMemcpyAsync(&ends[0], g.off, 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(&ends[1], g.off + n, 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipEventRecord(s.ev[1], stream));
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipEventElapsedTime(&out->device_ms, s.ev[0], s.ev[1]));
    out->n_points = (ends[1] - ends[0] - kRecHeader * n) / kRecPoint;
    return OTR_OK;
  });
}

int Matcher::sessions_export_records(otr_session_records* out, std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    SessionStore& s = *ses;
    int rc;
    HIPCHK(hipSetDevice(graph_state().device));
    if (s.pending) return bad(err, "the last advance has not been committed");
    memset(out, 0, sizeof(*out));
    out->memory = OTR_MEM_HOST;
    if ((rc = s.list_sessions(0, 0, err))) return rc;
    const int32_t ns = s.n_list;
    s.x_off.assign((size_t)ns + 1, 0);
    int64_t* off = s.get<int64_t>(B_X_OFF, (size_t)ns + 1);
    HIPCHK(hipMemsetAsync(off, 0, 8, stream));
    out->rec_off = s.x_off.data();
    out->d_rec_off = off;
    if (s.named() && (rc = s.names_list(err))) return rc;
    if (ns == 0) {
      HIPCHK(hipStreamSynchronize(stream));
      return OTR_OK;
    }
    const int32_t* list = (const int32_t*)s.b[B_L_SLOT2].p;
    int64_t* len = s.get<int64_t>(B_X_LEN, ns);
    k_ses_record_len<<<grid_ceil1(ns, 256), 256, 0, stream>>>(ns, list, s.st, len);
    if ((rc = s.scan(len, off + 1, ns, err))) return rc;
    s.s_key.resize(ns);
    HIPCHK(hipMemcpyAsync(s.x_off.data(), off, 8 * ((size_t)ns + 1), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(s.s_key.data(), s.b[B_L_KEY2].p, 8 * (size_t)ns, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    const int64_t nb = s.x_off[ns];
    uint8_t* bytes = s.get<uint8_t>(B_X_BYTES, nb);
    k_ses_encode<<<(unsigned)ns, 64, 0, stream>>>(ns, list, off, s.st, bytes);
    HIPCHK(hipGetLastError());
    s.x_bytes.resize((size_t)nb);
    HIPCHK(hipMemcpyAsync(s.x_bytes.data(), bytes, (size_t)nb, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    out->n_records = ns;
    out->n_bytes = nb;
    out->key = (const uint64_t*)s.s_key.data();
    out->bytes = s.x_bytes.data();
    out->d_key = (const uint64_t*)s.b[B_L_KEY2].p;
    out->d_bytes = bytes;
    return OTR_OK;
  });
}

int Matcher::sessions_take(int n_parts, int part, int remove, otr_session_snapshot* out, std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    SessionStore& s = *ses;
    int rc;
    HIPCHK(hipSetDevice(graph_state().device));
    if (s.pending || s.chunk_open) return bad(err, "an advance / commit sequence is open");
    if (n_parts < 1 || part < 0 || part >= n_parts) return bad(err, "part out of range");
    const int32_t ms = s.cfg.max_sessions;
    int32_t* flag = s.get<int32_t>(B_FLAG, ms);
    k_ses_flag_part<<<grid_ceil1(ms, 256), 256, 0, stream>>>(s.st, (uint32_t)n_parts, (uint32_t)part, flag);
    if ((rc = s.list_flagged(err))) return rc;
    if ((rc = s.snapshot_list(out, err))) return rc;
    if (remove && s.n_list > 0) {  // deleted as an eviction deletes, without a report
      const int32_t* list = (const int32_t*)s.b[B_L_SLOT2].p;
      k_ses_clear<<<grid_ceil1(s.n_list, 256), 256, 0, stream>>>(s.n_list, list, s.st);
      if ((rc = s.release_list(list, s.n_list, err))) return rc;
    }
    return OTR_OK;
  });
}

// ---- K18: the names of a listing, the last name refusal ----------------------------------------

int Matcher::sessions_names(otr_session_name_list* out, std::string* err) {
  return guarded(
      *this, err, true,
      [&]() -> int {
        SessionStore& s = *ses;
        memset(out, 0, sizeof(*out));
        if (!s.named()) return bad(err, "the store has no uuid directory: open it with otr_sessions_open_named");
        if (!s.names_have)
          return bad(err, "no listing: call otr_sessions_snapshot, otr_sessions_take or otr_sessions_export_records");
        out->n = (int64_t)s.nl_off.size() - 1;
        out->n_bytes = s.nl_off.back();
        out->off = s.nl_off.data();
        out->bytes = s.nl_bytes.data();
        out->d_off = (const int64_t*)s.b[B_NL_OFF].p;
        out->d_bytes = (const uint8_t*)s.b[B_NL_BYTES].p;
        return OTR_OK;
      },
      true);
}

int Matcher::sessions_last_refusal(otr_session_name_refusal* out, std::string* err) {
  return guarded(
      *this, err, true,
      [&]() -> int {
        *out = ses->refusal;
        return OTR_OK;
      },
      true);
}

void Matcher::sessions_refusal_clear() {
  if (ses) ses->refusal = otr_session_name_refusal{-1, -1, 0, 0};
}

// otr_sessions_push_text: the message of the refused point
void Matcher::sessions_refusal_message(const int64_t* d_message) {
  if (!ses || !ses->refusal.reason || !d_message) return;
  int64_t msg = -1;
  if (hipMemcpy(&msg, d_message + ses->refusal.point, 8, hipMemcpyDeviceToHost) == hipSuccess) ses->refusal.message = msg;
}

}  // namespace otr
