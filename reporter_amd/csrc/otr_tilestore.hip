// otr_tilestore.hip — host side of the tile store (K15, otr_tilestore.h): the store's row
// buffer, the two passes of an add (count, scan, capacity check, write) and the flush (the
// matcher's device cull, then the per-file table), and of the tile file texts (K19,
// otr_tiletext.h): lengths, scans, one emit pass, of the store's snapshot, restore and
// changelog records (K20, otr_tile_records.h), and of the file texts read back into rows (K21,
// otr_tileparse.h): newline list, line table, one parse pass, compaction.  include/otr.h
// otr_tile_store_*, otr_tiles_text and otr_tiles_parse for the rules.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "otr_devscan.h"
#include "otr_engine.h"
#include "otr_tilestore.h"
#include "otr_tiletext.h"
#include "otr_tile_records.h"
// (K21 launches K11's two newline kernels; the rest of otr_ingest.h's kernels stay in otr_text.hip)
#define OTR_INGEST_NEWLINES_ONLY
#include "otr_tileparse.h"

namespace otr {

namespace {

DeviceOom tst_oom(const char* name, size_t bytes) { return DeviceOom{PoolOwner::tile_store, name, -1, bytes}; }

constexpr int64_t kTstMaxRows = (int64_t)1 << 27;

// growable buffers of an add, of a flush's file table (the rows are not among them) and of
// the file texts
enum TstBuf {
  T_OFF, T_ID, T_NEXT, T_T0, T_T1, T_LEN, T_QUEUE, T_KEY_A, T_KEY_B, T_IDX_A, T_IDX_B, T_CNT, T_ROW_OFF, T_TMP,
  T_F_HEAD, T_F_INCL, T_F_START, T_F_LISTED, T_F_LINCL, T_F_FILE, T_F_ROW_OFF, T_F_UNCLEAN,
  T_X_ROWS, T_X_TAG, T_X_LEN, T_X_OFF, T_X_TEXT_OFF, T_X_NAME_LEN, T_X_NAME_OFF, T_X_TEXT, T_X_NAMES,
  // K20: a snapshot (and a restore's staging), an export's outputs, a record restore's input and work
  T_S_ROWS, T_S_T0, T_S_T1, T_S_VERDICT,
  T_E_SHEAD, T_E_SINCL, T_E_POS, T_E_START, T_E_TILE, T_E_SLICE, T_E_REC_LEN, T_E_REC_OFF, T_E_NAME_LEN, T_E_NAME_OFF,
  T_E_BYTES, T_E_NAMES, T_E_MAP,
  T_I_START, T_I_TILE, T_I_SLICE, T_I_OFF, T_I_BYTES, T_I_MAP, T_I_COUNT, T_I_KEY_OK, T_I_FILE, T_I_FILE_A, T_I_FILE_B,
  T_I_SLICE_KEY, T_I_SLICE_B, T_I_IDX_A, T_I_IDX_B, T_I_IDX_C, T_I_WORDS, T_I_REF, T_I_ROW_OFF,
  T_M_FILE_A, T_M_FILE_B, T_M_IDX_A, T_M_IDX_B, T_M_VALUE, T_M_OK,
  // K21: a parse's inputs and work, then its six results
  T_P_TEXT, T_P_TEXT_OFF, T_P_NAMES, T_P_NAME_OFF, T_P_TAG, T_P_CNT, T_P_CSCAN, T_P_NL, T_P_NL_LO, T_P_LINE_CNT,
  T_P_LINE_INCL, T_P_SLOT, T_P_ROW_INCL, T_P_HEAD_INCL, T_P_BAD_INCL, T_P_BAD,
  T_P_ROWS, T_P_ROW_OFF, T_P_FILE, T_P_FILE_STATUS, T_P_FILE_LINE_OFF, T_P_LINE_STATUS,
  T_NUM
};
const char* const kTstName[T_NUM] = {
    "report offsets", "report id", "report next id", "report t0", "report t1", "report length", "report queue length",
    "window order key", "sorted window order key", "window index", "window order", "window row counts",
    "window row offsets", "scan / sort workspace", "file head", "file rank", "file start", "file listed",
    "listed file rank", "file table files", "file table row offsets", "file table unclean counts",
    "text rows", "text tag", "text row lengths", "text row offsets", "file text offsets", "file name lengths",
    "file name offsets", "file texts", "file names",
    "snapshot rows", "snapshot t0", "snapshot t1", "restore verdict",
    "slice heads", "slice ranks", "slice positions", "slice starts", "slice tile ids", "slice numbers",
    "record lengths", "record offsets", "slice name lengths", "slice name offsets", "record bytes", "slice names",
    "map entries",
    "input starts", "input tile ids", "input slices", "input record offsets", "input record bytes", "input map entries",
    "input counts", "input key flags", "input file keys", "input file keys in slice order", "sorted input file keys",
    "input slice keys", "sorted input slice keys", "input index", "input slice order", "input order",
    "restore verdict and counters", "referenced counts", "restored row offsets",
    "map file keys", "sorted map file keys", "map index", "map order", "map values", "map key flags",
    "parse text", "parse text offsets", "parse names", "parse name offsets", "parse tag", "newline counts",
    "newline ranks", "newline positions", "file newline ranks", "file line counts", "file line ranks",
    "line row slots", "line row ranks", "line header ranks", "line refusal ranks", "first refused line",
    "parsed rows", "parsed row offsets", "parsed files", "parsed file status", "parsed file line offsets",
    "parsed line status"};

}  // namespace

// the growable buffers (the pool's slots, by TstBuf), the stream they are used on and a pair
// of events
struct TstBufs : DevPool {
  TstBufs() : DevPool(PoolOwner::tile_store, kTstName, T_NUM) {}
  hipStream_t stream = nullptr;
  hipEvent_t ev[2];
  bool ev_init = false;
  int scan64(const int64_t* in, int64_t* out, int64_t n, std::string* err) {
    return pool_scan(*this, T_TMP, in, out, n, stream, err);
  }
  int events(std::string* err) {
    if (ev_init) return OTR_OK;
    for (auto& e : ev) HIPCHK(hipEventCreate(&e));
    ev_init = true;
    return OTR_OK;
  }
  int finish(float* device_ms, std::string* err);
  void release() {
    if (stream) (void)hipStreamSynchronize(stream);
    DevPool::release();
    if (ev_init)
      for (auto& e : ev) (void)hipEventDestroy(e);
  }
};

// The file texts of the last otr_tiles_text / otr_tile_store_flush_text (K19): device buffers
// and the host copies the result points to.
struct TileText : TstBufs {
  std::vector<uint8_t> h_tag;
  std::unique_ptr<uint8_t[]> h_text;  // grown, never zero-filled
  size_t h_text_cap = 0;
  std::vector<uint8_t> h_names;
  std::vector<int64_t> h_text_off, h_name_off, h_row_off;
  std::vector<unsigned long long> h_file;

  int table(const otr_tile_row* d_rows, int64_t n, const unsigned long long** d_file, const int64_t** d_row_off,
            int64_t* n_files, std::string* err);
  int write(const otr_tile_row* d_rows, int64_t n, const unsigned long long* d_file, const int64_t* d_row_off,
            int64_t n_files, int64_t quantisation, int rules, int flags, otr_tile_text_result* out, std::string* err);
};

void tile_text_destroy(TileText* t) {
  if (!t) return;
  t->release();
  delete t;
}

// The rows of the last otr_tiles_parse (K21): a pool of its own, so that its results survive the
// cull, the texts and the tile store calls, and the host copies the result points to.
struct TileParse : TstBufs {
  std::vector<otr_tile_row> h_rows;
  std::vector<int64_t> h_row_off, h_file_line_off;
  std::vector<unsigned long long> h_file;
  std::vector<uint8_t> h_file_status, h_line_status;
};

void tile_parse_destroy(TileParse* t) {
  if (!t) return;
  t->release();
  delete t;
}

struct TileStore : TstBufs {
  otr_tile_store_config cfg{};
  otr_tile_row* rows = nullptr;  // [max_rows], the store's own allocation
  unsigned long long* counters = nullptr;
  int64_t n_rows = 0;
  int flags = 0;         // OTR_TILE_STORE_*
  double* t0 = nullptr;  // [max_rows] each with OTR_TILE_STORE_TIMES
  double* t1 = nullptr;
  // what a flush returns
  std::vector<otr_tile_row> h_rows;
  std::vector<unsigned long long> h_file;
  std::vector<int64_t> h_row_off, h_unclean;
  // what a snapshot and an export return (K20)
  std::vector<otr_tile_row> h_snap_rows;
  std::vector<double> h_snap_t0, h_snap_t1;
  std::vector<int64_t> h_start, h_tile, h_rec_off, h_name_off;
  std::vector<int32_t> h_slice;
  std::vector<uint8_t> h_bytes, h_names, h_map;

  bool timed() const { return (flags & OTR_TILE_STORE_TIMES) != 0; }
  int sort_pairs(const unsigned long long* k_in, unsigned long long* k_out, const int32_t* v_in, int32_t* v_out,
                 int64_t n, std::string* err);
  int snapshot(int sflags, otr_tile_snapshot* out, std::string* err);
  int restore(const otr_tile_snapshot* snap, int memory, otr_tile_restore_result* out, std::string* err);
  int export_records(int32_t slice_size, otr_tile_records* out, std::string* err);
  int restore_records(const otr_tile_records* in, otr_tile_restore_result* out, std::string* err);

  int alloc(std::string* err);
  int add(const StoreArgs& in, int64_t n_reports, otr_tile_add_result* out, std::string* err);
  void add_result(otr_tile_add_result* out, int64_t n_reports, int64_t n_valid, int64_t added) const;
  int flush(Matcher& m, TileText* text, int flags, otr_tile_flush_result* out, otr_tile_text_result* text_out,
            std::string* err);
};

void tile_store_destroy(TileStore* s) {
  if (!s) return;
  s->release();
  if (s->rows) (void)hipFree(s->rows);
  if (s->counters) (void)hipFree(s->counters);
  if (s->t0) (void)hipFree(s->t0);
  if (s->t1) (void)hipFree(s->t1);
  delete s;
}

int TileStore::alloc(std::string* err) {
  const size_t bytes = sizeof(otr_tile_row) * (size_t)cfg.max_rows;
  if (hipMalloc((void**)&rows, bytes) != hipSuccess) {
    (void)hipGetLastError();
    rows = nullptr;
    throw tst_oom("tile store rows", bytes);
  }
  if (hipMalloc((void**)&counters, 8 * TST_WORDS) != hipSuccess) {
    (void)hipGetLastError();
    counters = nullptr;
    throw tst_oom("tile store counters", 8 * TST_WORDS);
  }
  if (timed()) {
    const size_t tb = sizeof(double) * (size_t)cfg.max_rows;
    if (hipMalloc((void**)&t0, tb) != hipSuccess || hipMalloc((void**)&t1, tb) != hipSuccess) {
      (void)hipGetLastError();
      throw tst_oom("tile store times", 2 * tb);
    }
  }
  return events(err);
}

void TileStore::add_result(otr_tile_add_result* out, int64_t n_reports, int64_t n_valid, int64_t added) const {
  memset(out, 0, sizeof(*out));
  out->n_reports = n_reports;
  out->n_valid = n_valid;
  out->n_rows_added = added;
  out->n_rows = n_rows;
}

// ev[0] was recorded at the call's start
int TstBufs::finish(float* device_ms, std::string* err) {
  HIPCHK(hipEventRecord(ev[1], stream));
  HIPCHK(hipStreamSynchronize(stream));
  HIPCHK(hipEventElapsedTime(device_ms, ev[0], ev[1]));
  return OTR_OK;
}

// in: the windows, their order and the report arrays in HBM (ev[0] recorded).  Pass 1 counts
// every window's rows, the scan places them, and only a total that fits is written.
int TileStore::add(const StoreArgs& in, int64_t n_reports, otr_tile_add_result* out, std::string* err) {
  int rc;
  const int64_t W = in.n_windows;
  StoreArgs a = in;
  a.quantisation = cfg.quantisation;
  a.row_cnt = get<int64_t>(T_CNT, W);
  int64_t* off = get<int64_t>(T_ROW_OFF, (size_t)W + 1);
  a.counters = counters;
  a.row_off = off;
  a.rows = rows + n_rows;
  a.row_t0 = timed() ? t0 + n_rows : nullptr;
  a.row_t1 = timed() ? t1 + n_rows : nullptr;
  const unsigned blocks = grid_ceil1(W, kStoreWaves);
  HIPCHK(hipMemsetAsync(counters, 0, 8 * TST_WORDS, stream));
  HIPCHK(hipMemsetAsync(off, 0, 8, stream));
  k_store_rows<false><<<blocks, 256, 0, stream>>>(a);
  HIPCHK(hipGetLastError());
  if ((rc = scan64(a.row_cnt, off + 1, W, err))) return rc;
  int64_t total = 0;
  unsigned long long h_cnt[TST_WORDS] = {0, 0};
  HIPCHK(hipMemcpyAsync(&total, off + W, 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(h_cnt, counters, sizeof(h_cnt), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (h_cnt[TST_BAD_OFF]) {
    if (err) *err = "rep_off does not start at 0 or is not ascending";
    return OTR_BAD_REQUEST;
  }
  if (total < 0 || total > cfg.max_rows - n_rows) {
    if (err)
      *err = "the add would take the tile store beyond max_rows (" + std::to_string(n_rows) + " rows held, " +
             (total >= (int64_t)kStoreBucketClamp ? std::string("more than ") + std::to_string(kTstMaxRows)
                                                  : std::to_string(total)) +
             " to add, max_rows " + std::to_string(cfg.max_rows) + "): flush first";
    return OTR_BAD_REQUEST;
  }
  if (total > 0) {
    if (timed())
      k_store_rows<true, true><<<blocks, 256, 0, stream>>>(a);
    else
      k_store_rows<true><<<blocks, 256, 0, stream>>>(a);
    HIPCHK(hipGetLastError());
  }
  float ms = 0.f;
  if ((rc = finish(&ms, err))) return rc;
  n_rows += total;
  add_result(out, n_reports, (int64_t)h_cnt[TST_VALID], total);
  out->device_ms = ms;
  return OTR_OK;
}

// ---- the matcher's entry points -------------------------------------------------------------

namespace {

int bad(std::string* err, const std::string& what) {
  if (err) *err = what;
  return OTR_BAD_REQUEST;
}

// the tile store calls' precondition, then the shared guard (an allocation failure of the
// store's pool or of the matcher's, which the flush reaches into, ends here)
template <class F>
int guarded(Matcher& m, std::string* err, bool need_store, F&& f) {
  if (need_store && !m.tst) return bad(err, "no tile store: call otr_tile_store_open first");
  return otr::guarded(m.stream, err, f);
}

}  // namespace

int Matcher::tile_store_open(const otr_tile_store_config* cfg, int flags, std::string* err) {
  if (flags & ~OTR_TILE_STORE_TIMES) return bad(err, "unknown tile store flags");
  if (tst) return bad(err, "the matcher already has a tile store");
  if (cfg->max_rows < 1 || cfg->max_rows > kTstMaxRows || cfg->quantisation < 60 || cfg->privacy < 1)
    return bad(err, "tile store config out of range (max_rows 1 .. 1<<27, quantisation >= 60, privacy >= 1)");
  HIPCHK(hipSetDevice(graph_state().device));
  if (!stream) HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  TileStore* s = new TileStore();
  s->cfg = *cfg;
  s->flags = flags;
  s->stream = stream;
  const int rc = guarded(*this, err, false, [&] { return s->alloc(err); });
  if (rc != OTR_OK) {
    tile_store_destroy(s);
    return rc;
  }
  tst = s;
  return OTR_OK;
}

int Matcher::tile_store_close(std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    tile_store_destroy(tst);
    tst = nullptr;
    return OTR_OK;
  });
}

int Matcher::tile_store_add_session(otr_tile_add_result* out, std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    TileStore& s = *tst;
    int rc;
    SessionReports sr;
    if (!sessions_last_reports(ses, &sr))
      return bad(err, "no session result to add: call otr_sessions_push or otr_sessions_punctuate first");
    if (*sr.added) return bad(err, "the last session result was already added");
    HIPCHK(hipSetDevice(graph_state().device));
    const int64_t W = sr.n_windows;
    if (W >= (int64_t)INT32_MAX) return bad(err, "too many windows for one add");
    if (W == 0) {
      *sr.added = true;
      s.add_result(out, 0, 0, 0);
      return OTR_OK;
    }
    HIPCHK(hipEventRecord(s.ev[0], stream));
    // the forward order: a stable sort of the windows by trigger (an eviction's by rank)
    unsigned long long* key_a = s.get<unsigned long long>(T_KEY_A, W);
    unsigned long long* key_b = s.get<unsigned long long>(T_KEY_B, W);
    int32_t* idx_a = s.get<int32_t>(T_IDX_A, W);
    int32_t* idx_b = s.get<int32_t>(T_IDX_B, W);
    k_store_order_key<<<grid_ceil1(W, 256), 256, 0, stream>>>(sr.trigger, W, key_a, idx_a);
    if ((rc = s.sort_pairs(key_a, key_b, idx_a, idx_b, W, err))) return rc;
    StoreArgs a{};
    a.n_windows = W;
    a.order = idx_b;
    a.rep_off = sr.rep_off;
    a.id = sr.id;
    a.next_id = sr.next_id;
    a.t0 = sr.t0;
    a.t1 = sr.t1;
    a.length = sr.length;
    a.queue = sr.queue_length;
    if ((rc = s.add(a, sr.n_reports, out, err))) return rc;
    *sr.added = true;
    return OTR_OK;
  });
}

int Matcher::tile_store_add_reports(int64_t n_windows, const int64_t* rep_off, const uint64_t* id,
                                    const uint64_t* next_id, const double* t0, const double* t1,
                                    const int32_t* length, const int32_t* queue_length, int memory,
                                    otr_tile_add_result* out, std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    TileStore& s = *tst;
    const int64_t W = n_windows;
    if (W >= (int64_t)INT32_MAX) return bad(err, "too many windows for one add");
    if (W <= 0) {
      s.add_result(out, 0, 0, 0);
      return OTR_OK;
    }
    if (!rep_off) return bad(err, "null argument");
    HIPCHK(hipSetDevice(graph_state().device));
    int64_t n_reports = 0;
    StoreArgs a{};
    a.n_windows = W;
    if (memory == OTR_MEM_DEVICE) {
      HIPCHK(hipMemcpy(&n_reports, rep_off + W, 8, hipMemcpyDeviceToHost));
      if (n_reports < 0) return bad(err, "rep_off does not start at 0 or is not ascending");
      if (n_reports > 0 && (!id || !next_id || !t0 || !t1 || !length || !queue_length)) return bad(err, "null argument");
      HIPCHK(hipEventRecord(s.ev[0], stream));
      a.rep_off = rep_off;
      a.id = (const unsigned long long*)id;
      a.next_id = (const unsigned long long*)next_id;
      a.t0 = t0;
      a.t1 = t1;
      a.length = length;
      a.queue = queue_length;
    } else {
      if (rep_off[0] != 0) return bad(err, "rep_off does not start at 0 or is not ascending");
      for (int64_t w = 0; w < W; ++w)
        if (rep_off[w + 1] < rep_off[w]) return bad(err, "rep_off does not start at 0 or is not ascending");
      n_reports = rep_off[W];
      if (n_reports > 0 && (!id || !next_id || !t0 || !t1 || !length || !queue_length)) return bad(err, "null argument");
      const size_t nr = (size_t)n_reports;
      int64_t* d_off = s.get<int64_t>(T_OFF, (size_t)W + 1);
      unsigned long long* d_id = s.get<unsigned long long>(T_ID, nr);
      unsigned long long* d_next = s.get<unsigned long long>(T_NEXT, nr);
      double* d_t0 = s.get<double>(T_T0, nr);
      double* d_t1 = s.get<double>(T_T1, nr);
      int32_t* d_len = s.get<int32_t>(T_LEN, nr);
      int32_t* d_queue = s.get<int32_t>(T_QUEUE, nr);
      HIPCHK(hipEventRecord(s.ev[0], stream));
      HIPCHK(hipMemcpyAsync(d_off, rep_off, 8 * ((size_t)W + 1), hipMemcpyHostToDevice, stream));
      if (nr) {
        HIPCHK(hipMemcpyAsync(d_id, id, 8 * nr, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(d_next, next_id, 8 * nr, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(d_t0, t0, 8 * nr, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(d_t1, t1, 8 * nr, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(d_len, length, 4 * nr, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(d_queue, queue_length, 4 * nr, hipMemcpyHostToDevice, stream));
      }
      a.rep_off = d_off;
      a.id = d_id;
      a.next_id = d_next;
      a.t0 = d_t0;
      a.t1 = d_t1;
      a.length = d_len;
      a.queue = d_queue;
    }
    return s.add(a, n_reports, out, err);
  });
}

int Matcher::tile_store_add_rows(const otr_tile_row* rows, int64_t n, int memory, otr_tile_add_result* out,
                                 std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    TileStore& s = *tst;
    if (s.timed())
      return bad(err, "finished rows have no times: a tile store opened with OTR_TILE_STORE_TIMES takes "
                      "otr_tile_store_restore instead");
    if (n <= 0) {
      s.add_result(out, 0, 0, 0);
      return OTR_OK;
    }
    if (!rows) return bad(err, "null argument");
    if (n > s.cfg.max_rows - s.n_rows)
      return bad(err, "the add would take the tile store beyond max_rows (" + std::to_string(s.n_rows) +
                          " rows held, " + std::to_string(n) + " to add, max_rows " +
                          std::to_string(s.cfg.max_rows) + "): flush first");
    HIPCHK(hipSetDevice(graph_state().device));
    HIPCHK(hipEventRecord(s.ev[0], stream));
    HIPCHK(hipMemcpyAsync(s.rows + s.n_rows, rows, sizeof(otr_tile_row) * (size_t)n,
                          memory == OTR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    float ms = 0.f;
    int rc;
    if ((rc = s.finish(&ms, err))) return rc;
    s.n_rows += n;
    s.add_result(out, 0, 0, n);
    out->device_ms = ms;
    return OTR_OK;
  });
}

// The flush.  text non-null (otr_tile_store_flush_text): the kept rows stay in HBM and their
// file texts are written there; the store is emptied only once that has succeeded.
int TileStore::flush(Matcher& m, TileText* text, int flags, otr_tile_flush_result* out,
                     otr_tile_text_result* text_out, std::string* err) {
  TileStore& s = *this;
  int rc;
  memset(out, 0, sizeof(*out));
  const int64_t n = s.n_rows;
  s.h_rows.clear();
  s.h_file.clear();
  s.h_unclean.clear();
  s.h_row_off.assign(1, 0);
  int64_t* d_row_off = s.get<int64_t>(T_F_ROW_OFF, 1);
  out->row_off = s.h_row_off.data();
  if (n == 0) {
    HIPCHK(hipMemsetAsync(d_row_off, 0, 8, stream));
    HIPCHK(hipStreamSynchronize(stream));
    out->d_row_off = d_row_off;
    if (text) return text->write(nullptr, 0, nullptr, d_row_off, 0, cfg.quantisation, OTR_TILE_RULES_STREAM, flags,
                                 text_out, err);
    return OTR_OK;
  }
  HIPCHK(hipEventRecord(s.ev[0], stream));
  CulledRows c;
  if ((rc = m.cull_device(s.rows, n, s.cfg.privacy, OTR_TILE_RULES_STREAM, &c, err))) return rc;
  // the files of the sorted rows, and which of them kept rows
  const unsigned g = grid_ceil1(n, 256);
  int64_t* head = s.get<int64_t>(T_F_HEAD, n);
  int64_t* head_incl = s.get<int64_t>(T_F_INCL, n);
  k_store_file_heads<<<g, 256, 0, stream>>>(c.sorted, n, head);
  if ((rc = s.scan64(head, head_incl, n, err))) return rc;
  int64_t nf = 0;
  if ((rc = read_back(stream, err, fetch(&nf, head_incl + (n - 1))))) return rc;
  if (nf < 1 || nf > n) {
    if (err) *err = "tile store file split failed";
    return OTR_DEVICE_ERROR;
  }
  int64_t* start = s.get<int64_t>(T_F_START, nf);
  int64_t* listed = s.get<int64_t>(T_F_LISTED, nf);
  int64_t* listed_incl = s.get<int64_t>(T_F_LINCL, nf);
  k_store_file_starts<<<g, 256, 0, stream>>>(head, head_incl, n, start);
  const unsigned gf = grid_ceil1(nf, 256);
  k_store_file_listed<<<gf, 256, 0, stream>>>(start, nf, n, c.kept_incl, listed);
  if ((rc = s.scan64(listed, listed_incl, nf, err))) return rc;
  int64_t nl = 0;
  if ((rc = read_back(stream, err, fetch(&nl, listed_incl + (nf - 1))))) return rc;
  if (nl < 0 || nl > nf || nl > c.n_kept || (nl == 0) != (c.n_kept == 0)) {
    if (err) *err = "tile store file table failed";
    return OTR_DEVICE_ERROR;
  }
  unsigned long long* d_file = s.get<unsigned long long>(T_F_FILE, nl);
  d_row_off = s.get<int64_t>(T_F_ROW_OFF, (size_t)nl + 1);
  int64_t* d_unclean = s.get<int64_t>(T_F_UNCLEAN, nl);
  k_store_file_table<<<gf, 256, 0, stream>>>(c.sorted, start, nf, n, c.kept_incl, listed, listed_incl, d_file,
                                             d_row_off, d_unclean);
  HIPCHK(hipGetLastError());
  if (!text) s.h_rows.resize((size_t)c.n_kept);
  s.h_file.resize((size_t)nl);
  s.h_unclean.resize((size_t)nl);
  s.h_row_off.resize((size_t)nl + 1);
  if (!text && c.n_kept > 0)
    HIPCHK(hipMemcpyAsync(s.h_rows.data(), c.kept, sizeof(otr_tile_row) * (size_t)c.n_kept, hipMemcpyDeviceToHost,
                          stream));
  if (nl > 0) {
    HIPCHK(hipMemcpyAsync(s.h_file.data(), d_file, 8 * (size_t)nl, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(s.h_unclean.data(), d_unclean, 8 * (size_t)nl, hipMemcpyDeviceToHost, stream));
  }
  HIPCHK(hipMemcpyAsync(s.h_row_off.data(), d_row_off, 8 * ((size_t)nl + 1), hipMemcpyDeviceToHost, stream));
  if ((rc = s.finish(&out->device_ms, err))) return rc;
  // (the kept rows of one listed file are adjacent and two listed files differ in `file`: the
  // text stage's file heads fall on d_row_off)
  if (text && (rc = text->write(c.kept, c.n_kept, d_file, d_row_off, nl, cfg.quantisation, OTR_TILE_RULES_STREAM,
                                flags, text_out, err)))
    return rc;
  s.n_rows = 0;  // the sorted and the kept rows are copies: the buffer is free again
  out->n_rows_in = n;
  out->n_rows = c.n_kept;
  out->n_files = (int32_t)nl;
  out->n_files_empty = (int32_t)(nf - nl);
  out->rows = s.h_rows.empty() ? nullptr : s.h_rows.data();
  out->file = s.h_file.empty() ? nullptr : (const uint64_t*)s.h_file.data();
  out->row_off = s.h_row_off.data();
  out->n_unclean = s.h_unclean.empty() ? nullptr : s.h_unclean.data();
  out->d_rows = c.kept;
  out->d_file = (const uint64_t*)d_file;
  out->d_row_off = d_row_off;
  out->d_n_unclean = d_unclean;
  return OTR_OK;
}

int Matcher::tile_store_flush(otr_tile_flush_result* out, std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    HIPCHK(hipSetDevice(graph_state().device));
    return tst->flush(*this, nullptr, 0, out, nullptr, err);
  });
}

// ---- tile file texts (K19) ---------------------------------------------------------------

// The file table of n > 0 rows that come without one: every run of equal `file` is a file.
int TileText::table(const otr_tile_row* d_rows, int64_t n, const unsigned long long** d_file,
                    const int64_t** d_row_off, int64_t* n_files, std::string* err) {
  int rc;
  const unsigned g = grid_ceil1(n, 256);
  int64_t* head = get<int64_t>(T_F_HEAD, n);
  int64_t* head_incl = get<int64_t>(T_F_INCL, n);
  k_store_file_heads<<<g, 256, 0, stream>>>(d_rows, n, head);
  if ((rc = scan64(head, head_incl, n, err))) return rc;
  int64_t nf = 0;
  if ((rc = read_back(stream, err, fetch(&nf, head_incl + (n - 1))))) return rc;
  if (nf < 1 || nf > n || nf >= (int64_t)INT32_MAX) {
    if (err) *err = "tile text file split failed";
    return OTR_DEVICE_ERROR;
  }
  int64_t* start = get<int64_t>(T_F_START, nf);
  unsigned long long* file = get<unsigned long long>(T_F_FILE, nf);
  int64_t* row_off = get<int64_t>(T_F_ROW_OFF, (size_t)nf + 1);
  k_store_file_starts<<<g, 256, 0, stream>>>(head, head_incl, n, start);
  k_tile_text_table<<<grid_ceil1(nf + 1, 256), 256, 0, stream>>>(d_rows, start, nf, n, file, row_off);
  HIPCHK(hipGetLastError());
  *d_file = file;
  *d_row_off = row_off;
  *n_files = nf;
  return OTR_OK;
}

// The texts and names of n rows in HBM whose file table is (d_file, d_row_off, n_files), all
// on the device; h_tag holds the call's tag.  Lengths, two scans, one synchronise for the two
// totals, then the emit pass and the names.
int TileText::write(const otr_tile_row* d_rows, int64_t n, const unsigned long long* d_file,
                    const int64_t* d_row_off, int64_t n_files, int64_t quantisation, int rules, int flags,
                    otr_tile_text_result* out, std::string* err) {
  int rc;
  memset(out, 0, sizeof(*out));
  if ((rc = events(err))) return rc;
  HIPCHK(hipEventRecord(ev[0], stream));
  const int64_t nf = n_files;
  const int32_t tag_len = (int32_t)h_tag.size();
  int64_t* off = get<int64_t>(T_X_OFF, (size_t)n + 1);
  int64_t* text_off = get<int64_t>(T_X_TEXT_OFF, (size_t)nf + 1);
  int64_t* name_off = get<int64_t>(T_X_NAME_OFF, (size_t)nf + 1);
  uint8_t* tag = get<uint8_t>(T_X_TAG, kTileTextTagMax);
  HIPCHK(hipMemsetAsync(off, 0, 8, stream));
  HIPCHK(hipMemsetAsync(text_off, 0, 8, stream));
  HIPCHK(hipMemsetAsync(name_off, 0, 8, stream));
  int64_t total[2] = {0, 0};  // text bytes, name bytes
  if (n > 0) {
    int64_t* len = get<int64_t>(T_X_LEN, n);
    int64_t* name_len = get<int64_t>(T_X_NAME_LEN, nf);
    HIPCHK(hipMemcpyAsync(tag, h_tag.data(), (size_t)tag_len, hipMemcpyHostToDevice, stream));
    k_tile_text_len<<<grid_ceil1(n, 256), 256, 0, stream>>>(d_rows, n, rules, tag_len, len);
    if ((rc = scan64(len, off + 1, n, err))) return rc;
    k_tile_text_files<<<grid_ceil1(nf + 1, 256), 256, 0, stream>>>(d_file, d_row_off, off, nf, quantisation, text_off,
                                                                   name_len);
    if ((rc = scan64(name_len, name_off + 1, nf, err))) return rc;
    if ((rc = read_back(stream, err, fetch(&total[0], off + n), fetch(&total[1], name_off + nf)))) return rc;
    // (a row is at least 17 bytes and at most 122 + the tag, a name 8 to 20 + 1 + 20 + 1 + 1 + 1 + 7)
    if (total[0] < 17 * n || total[0] > n * (int64_t)(122 + kTileTextTagMax + kTileTextHeader + 1) || total[1] < 8 * nf ||
        total[1] > 51 * nf) {
      if (err) *err = "tile text lengths failed";
      return OTR_DEVICE_ERROR;
    }
  }
  uint8_t* text = get<uint8_t>(T_X_TEXT, (size_t)total[0]);
  uint8_t* names = get<uint8_t>(T_X_NAMES, (size_t)total[1]);
  if (n > 0) {
    k_tile_text_emit<<<grid_ceil1(n, kTtRows), kTtRows, kTtLds, stream>>>(d_rows, n, rules, tag, tag_len, off, text);
    k_tile_text_names<<<grid_ceil1(nf, 256), 256, 0, stream>>>(d_file, name_off, nf, quantisation, names);
    HIPCHK(hipGetLastError());
  }
  const bool host = !(flags & OTR_TILE_TEXT_NO_HOST);
  if (host) {
    if (h_text_cap < (size_t)total[0] || !h_text) {
      h_text_cap = (size_t)total[0] + (size_t)total[0] / 4 + 16;
      h_text.reset();
      h_text.reset(new uint8_t[h_text_cap]);
    }
    h_names.resize((size_t)total[1] + 1);
    h_text_off.resize((size_t)nf + 1);
    h_name_off.resize((size_t)nf + 1);
    h_row_off.resize((size_t)nf + 1);
    h_file.resize((size_t)nf + 1);
    if (total[0] > 0) HIPCHK(hipMemcpyAsync(h_text.get(), text, (size_t)total[0], hipMemcpyDeviceToHost, stream));
    if (total[1] > 0) HIPCHK(hipMemcpyAsync(h_names.data(), names, (size_t)total[1], hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(h_text_off.data(), text_off, 8 * ((size_t)nf + 1), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(h_name_off.data(), name_off, 8 * ((size_t)nf + 1), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(h_row_off.data(), d_row_off, 8 * ((size_t)nf + 1), hipMemcpyDeviceToHost, stream));
    if (nf > 0) HIPCHK(hipMemcpyAsync(h_file.data(), d_file, 8 * (size_t)nf, hipMemcpyDeviceToHost, stream));
  }
  if ((rc = finish(&out->device_ms, err))) return rc;
  out->n_rows = n;
  out->n_text_bytes = total[0];
  out->n_name_bytes = total[1];
  out->n_files = (int32_t)nf;
  if (host) {
    out->text = h_text.get();
    out->text_off = h_text_off.data();
    out->names = h_names.data();
    out->name_off = h_name_off.data();
    out->file = (const uint64_t*)h_file.data();
    out->row_off = h_row_off.data();
  }
  out->d_text = text;
  out->d_text_off = text_off;
  out->d_names = names;
  out->d_name_off = name_off;
  out->d_file = (const uint64_t*)d_file;
  out->d_row_off = d_row_off;
  return OTR_OK;
}

namespace {

// the call's tag into t.h_tag; false: source or mode longer than 255 bytes
bool text_tag(std::vector<uint8_t>* tag, const char* source, const char* mode, int rules) {
  const char* src = source ? source : "";
  const char* md = mode ? mode : "";
  const size_t ls = strnlen(src, kTileTextTagPart + 1), lm = strnlen(md, kTileTextTagPart + 1);
  if (ls > (size_t)kTileTextTagPart || lm > (size_t)kTileTextTagPart) return false;
  tag->resize(kTileTextTagMax);
  tag->resize((size_t)tile_text_tag_put((const uint8_t*)src, (int32_t)ls, (const uint8_t*)md, (int32_t)lm, rules,
                                        tag->data()));
  return true;
}

// the matcher's text state, created at its first use (the device and the stream are set)
int text_state(Matcher& m, std::string* err) {
  HIPCHK(hipSetDevice(graph_state().device));
  if (!m.stream) HIPCHK(hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking));
  if (!m.ttx) m.ttx = new TileText();
  m.ttx->stream = m.stream;
  return OTR_OK;
}

const char* const kTagTooLong = "tile text: source and mode take at most 255 bytes each";

}  // namespace

int Matcher::tiles_text(const otr_tile_row* rows, int64_t n, int memory, int quantisation, int rules,
                        const char* source, const char* mode, int flags, otr_tile_text_result* out,
                        std::string* err) {
  std::vector<uint8_t> tag;
  if (quantisation < 1) return bad(err, "tile text: quantisation below 1");
  if (!tile_text_rules_ok(rules)) return bad(err, "tile text: unknown rules " + std::to_string(rules));
  if (!text_tag(&tag, source, mode, rules)) return bad(err, kTagTooLong);
  if (n < 0 || n >= (int64_t)INT32_MAX) return bad(err, "tile text: row count out of range");
  return guarded(*this, err, false, [&]() -> int {
    int rc;
    if ((rc = text_state(*this, err))) return rc;
    TileText& t = *ttx;
    t.h_tag = tag;
    const otr_tile_row* d_rows = rows;
    const unsigned long long* d_file = nullptr;
    const int64_t* d_row_off = t.get<int64_t>(T_F_ROW_OFF, 1);
    int64_t nf = 0;
    if (n > 0) {
      if (memory != OTR_MEM_DEVICE) {
        otr_tile_row* d = t.get<otr_tile_row>(T_X_ROWS, n);
        HIPCHK(hipMemcpyAsync(d, rows, sizeof(otr_tile_row) * (size_t)n, hipMemcpyHostToDevice, stream));
        d_rows = d;
      }
      if ((rc = t.table(d_rows, n, &d_file, &d_row_off, &nf, err))) return rc;
    } else {
      HIPCHK(hipMemsetAsync((void*)d_row_off, 0, 8, stream));
    }
    return t.write(d_rows, n, d_file, d_row_off, nf, quantisation, rules, flags, out, err);
  });
}

int Matcher::tile_store_flush_text(const char* source, const char* mode, int flags, otr_tile_flush_result* flush,
                                   otr_tile_text_result* out, std::string* err) {
  std::vector<uint8_t> tag;
  if (!text_tag(&tag, source, mode, OTR_TILE_RULES_STREAM)) return bad(err, kTagTooLong);
  return guarded(*this, err, true, [&]() -> int {
    int rc;
    if ((rc = text_state(*this, err))) return rc;
    ttx->h_tag = tag;
    return tst->flush(*this, ttx, flags, flush, out, err);
  });
}

// ---- tile file texts read back (K21) ------------------------------------------------------

// The sizes refused are those of Matcher::ingest (otr_text.hip): text of 2^40 bytes or of
// INT32_MAX 16-byte chunks (the chunk scan counts in int), INT32_MAX lines (the line scans do).
// Order of work: the inputs, the newline list and the line counts go to work slots; only once the
// line count has passed are the six result slots touched, so a refusal leaves the last result,
// host and device, as it was.
int Matcher::tiles_parse(const otr_tile_texts* in, int quantisation, int rules, const char* source, const char* mode,
                         int flags, otr_tile_parse_result* out, std::string* err) {
  std::vector<uint8_t> tag;
  if (quantisation < 1) return bad(err, "tile parse: quantisation below 1");
  if (!tile_text_rules_ok(rules)) return bad(err, "tile parse: unknown rules " + std::to_string(rules));
  if (!text_tag(&tag, source, mode, rules)) return bad(err, "tile parse: source and mode take at most 255 bytes each");
  const int64_t nf = in->n_files;
  if (nf < 0) return bad(err, "tile parse: n_files below 0");
  if (nf > 0 && (!in->text_off || !in->name_off)) return bad(err, "null argument");
  return guarded(*this, err, false, [&]() -> int {
    int rc;
    HIPCHK(hipSetDevice(graph_state().device));
    if (!stream) HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    if (!tpx) tpx = new TileParse();
    TileParse& t = *tpx;
    t.stream = stream;
    if ((rc = t.events(err))) return rc;
    const bool dev = in->memory == OTR_MEM_DEVICE;
    // the two offset arrays on the host: checked here, whichever memory they came from
    std::vector<int64_t> toff((size_t)nf + 1, 0), noff((size_t)nf + 1, 0);
    if (nf > 0) {
      const hipMemcpyKind k = dev ? hipMemcpyDeviceToHost : hipMemcpyHostToHost;
      HIPCHK(hipMemcpy(toff.data(), in->text_off, 8 * ((size_t)nf + 1), k));
      HIPCHK(hipMemcpy(noff.data(), in->name_off, 8 * ((size_t)nf + 1), k));
    }
    for (const auto* o : {&toff, &noff}) {
      if ((*o)[0] != 0) return bad(err, "tile parse: offsets do not ascend from 0");
      for (int64_t f = 0; f < nf; ++f)
        if ((*o)[(size_t)f + 1] < (*o)[(size_t)f]) return bad(err, "tile parse: offsets do not ascend from 0");
    }
    const int64_t len = toff[(size_t)nf], name_len = noff[(size_t)nf];
    const int64_t n_chunks = (len + 15) / 16;
    if (len >= ((int64_t)1 << 40) || n_chunks >= (int64_t)INT32_MAX) return bad(err, "tile parse: text too large");
    if ((len > 0 && !in->text) || (name_len > 0 && !in->names)) return bad(err, "null argument");
    HIPCHK(hipEventRecord(t.ev[0], stream));
    // inputs in HBM: the text padded to whole chunks, the rest as it is or uploaded
    const hipMemcpyKind up = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    TileParseIn a{};
    a.n_files = nf;
    a.rules = rules;
    a.quantisation = quantisation;
    uint8_t* d_text = t.get<uint8_t>(T_P_TEXT, 16 * (size_t)n_chunks);
    a.text = d_text;
    if (n_chunks > 0) {
      HIPCHK(hipMemsetAsync(d_text + 16 * (n_chunks - 1), 0, 16, stream));
      HIPCHK(hipMemcpyAsync(d_text, in->text, (size_t)len, up, stream));
    }
    if (dev && nf > 0) {
      a.text_off = in->text_off;
      a.names = in->names;
      a.name_off = in->name_off;
    } else {
      int64_t* d_toff = t.get<int64_t>(T_P_TEXT_OFF, (size_t)nf + 1);
      int64_t* d_noff = t.get<int64_t>(T_P_NAME_OFF, (size_t)nf + 1);
      uint8_t* d_names = t.get<uint8_t>(T_P_NAMES, (size_t)name_len);
      HIPCHK(hipMemcpyAsync(d_toff, toff.data(), 8 * ((size_t)nf + 1), hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(d_noff, noff.data(), 8 * ((size_t)nf + 1), hipMemcpyHostToDevice, stream));
      if (name_len > 0) HIPCHK(hipMemcpyAsync(d_names, in->names, (size_t)name_len, hipMemcpyHostToDevice, stream));
      a.text_off = d_toff;
      a.names = d_names;
      a.name_off = d_noff;
    }
    uint8_t* d_tag = t.get<uint8_t>(T_P_TAG, kTileTextTagMax);
    HIPCHK(hipMemcpyAsync(d_tag, tag.data(), tag.size(), hipMemcpyHostToDevice, stream));
    // the newline positions (K11's kernels)
    int64_t n_nl = 0;
    if (n_chunks > 0) {
      int64_t* cnt = t.get<int64_t>(T_P_CNT, (size_t)n_chunks);
      int64_t* cscan = t.get<int64_t>(T_P_CSCAN, (size_t)n_chunks);
      k_nl_count<<<grid_ceil(n_chunks, 256), 256, 0, stream>>>(reinterpret_cast<const uint4*>(d_text), n_chunks, cnt);
      HIPCHK(hipGetLastError());
      if ((rc = t.scan64(cnt, cscan, n_chunks, err))) return rc;
      if ((rc = read_back(stream, err, fetch(&n_nl, cscan + (n_chunks - 1))))) return rc;
      if (n_nl < 0 || n_nl > len) {
        if (err) *err = "tile parse newline count failed";
        return OTR_DEVICE_ERROR;
      }
      int64_t* nl = t.get<int64_t>(T_P_NL, (size_t)n_nl);
      if (n_nl > 0) {
        k_nl_write<<<grid_ceil(n_chunks, 256), 256, 0, stream>>>(reinterpret_cast<const uint4*>(d_text), n_chunks, cscan,
                                                                nl);
        HIPCHK(hipGetLastError());
      }
      a.nl = nl;
    } else {
      a.nl = t.get<int64_t>(T_P_NL, 1);
    }
    a.n_nl = n_nl;
    // the line table: per file its newlines and its line count, then the counts' scan
    int64_t n_lines = 0;
    int64_t* nl_lo = t.get<int64_t>(T_P_NL_LO, (size_t)nf + 1);
    int64_t* line_cnt = t.get<int64_t>(T_P_LINE_CNT, (size_t)nf);
    int64_t* line_incl = t.get<int64_t>(T_P_LINE_INCL, (size_t)nf);
    const unsigned gf = grid_ceil1(nf + 1, 256);
    if (nf > 0) {
      k_tile_parse_files<<<gf, 256, 0, stream>>>(a, nl_lo, line_cnt);
      HIPCHK(hipGetLastError());
      if ((rc = t.scan64(line_cnt, line_incl, nf, err))) return rc;
      if ((rc = read_back(stream, err, fetch(&n_lines, line_incl + (nf - 1))))) return rc;
      if (n_lines < 0 || n_lines > n_nl + nf) {
        if (err) *err = "tile parse line table failed";
        return OTR_DEVICE_ERROR;
      }
    }
    if (n_lines >= (int64_t)INT32_MAX) return bad(err, "tile parse: too many lines for one call");
    // ---- from here on the result slots are written
    int64_t* file_line_off = t.get<int64_t>(T_P_FILE_LINE_OFF, (size_t)nf + 1);
    unsigned long long* file = t.get<unsigned long long>(T_P_FILE, (size_t)nf);
    uint8_t* file_status = t.get<uint8_t>(T_P_FILE_STATUS, (size_t)nf);
    uint8_t* line_status = t.get<uint8_t>(T_P_LINE_STATUS, (size_t)n_lines);
    int64_t* row_off = t.get<int64_t>(T_P_ROW_OFF, (size_t)nf + 1);
    otr_tile_row* slot = t.get<otr_tile_row>(T_P_SLOT, (size_t)n_lines);
    int64_t* row_incl = t.get<int64_t>(T_P_ROW_INCL, (size_t)n_lines);
    int64_t* head_incl = t.get<int64_t>(T_P_HEAD_INCL, (size_t)n_lines);
    int64_t* bad_incl = t.get<int64_t>(T_P_BAD_INCL, (size_t)n_lines);
    unsigned long long* d_bad = t.get<unsigned long long>(T_P_BAD, 1);
    k_tile_parse_names<<<gf, 256, 0, stream>>>(a, line_incl, file_line_off, file, file_status);
    HIPCHK(hipGetLastError());
    int64_t n_rows = 0, n_headers = 0, n_bad = 0;
    unsigned long long h_bad = ~0ull;
    if (n_lines > 0) {
      HIPCHK(hipMemsetAsync(d_bad, 0xFF, 8, stream));
      k_tile_parse<<<grid_ceil(n_lines, 256), 256, 0, stream>>>(a, nl_lo, file_line_off, file, file_status, d_tag,
                                                                (int32_t)tag.size(), n_lines, line_status, slot, d_bad);
      HIPCHK(hipGetLastError());
      Workspace ws;
      int64_t* const three[3] = {row_incl, head_incl, bad_incl};
      if ((rc = tuple_sums<3>(&ws, TileParseColumns{line_status}, three, (int)n_lines, stream, err))) return rc;
      ws.p = t.get<char>(T_TMP, ws.bytes);
      if ((rc = tuple_sums<3>(&ws, TileParseColumns{line_status}, three, (int)n_lines, stream, err))) return rc;
      if ((rc = read_back(stream, err, fetch(&n_rows, row_incl + (n_lines - 1)), fetch(&n_headers, head_incl + (n_lines - 1)),
                          fetch(&n_bad, bad_incl + (n_lines - 1)), fetch(&h_bad, d_bad))))
        return rc;
      if (n_rows < 0 || n_headers < 0 || n_bad < 0 || n_rows + n_headers + n_bad != n_lines ||
          (n_bad == 0) != (h_bad == ~0ull) || (h_bad != ~0ull && (int64_t)(h_bad >> 8) >= n_lines)) {
        if (err) *err = "tile parse line counts failed";
        return OTR_DEVICE_ERROR;
      }
    }
    otr_tile_row* rows = t.get<otr_tile_row>(T_P_ROWS, (size_t)n_rows);
    k_tile_parse_compact<<<grid_ceil1(std::max<int64_t>(n_lines, nf + 1), 256), 256, 0, stream>>>(
        line_status, slot, row_incl, n_lines, file_line_off, nf, rows, row_off);
    HIPCHK(hipGetLastError());
    // the file table always comes to the host: the first refused line's file and the refused names
    t.h_file_line_off.resize((size_t)nf + 1);
    t.h_file_status.resize((size_t)nf + 1);
    HIPCHK(hipMemcpyAsync(t.h_file_line_off.data(), file_line_off, 8 * ((size_t)nf + 1), hipMemcpyDeviceToHost, stream));
    if (nf > 0) HIPCHK(hipMemcpyAsync(t.h_file_status.data(), file_status, (size_t)nf, hipMemcpyDeviceToHost, stream));
    const bool host = !(flags & OTR_TILE_PARSE_NO_HOST);
    if (host) {
      t.h_rows.resize((size_t)n_rows + 1);
      t.h_row_off.resize((size_t)nf + 1);
      t.h_file.resize((size_t)nf + 1);
      t.h_line_status.resize((size_t)n_lines + 1);
      if (n_rows > 0)
        HIPCHK(hipMemcpyAsync(t.h_rows.data(), rows, sizeof(otr_tile_row) * (size_t)n_rows, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipMemcpyAsync(t.h_row_off.data(), row_off, 8 * ((size_t)nf + 1), hipMemcpyDeviceToHost, stream));
      if (nf > 0) HIPCHK(hipMemcpyAsync(t.h_file.data(), file, 8 * (size_t)nf, hipMemcpyDeviceToHost, stream));
      if (n_lines > 0)
        HIPCHK(hipMemcpyAsync(t.h_line_status.data(), line_status, (size_t)n_lines, hipMemcpyDeviceToHost, stream));
    }
    float ms = 0.f;
    if ((rc = t.finish(&ms, err))) return rc;
    memset(out, 0, sizeof(*out));
    out->n_lines = n_lines;
    out->n_rows = n_rows;
    out->n_headers = n_headers;
    out->n_bad = n_bad;
    for (int64_t f = 0; f < nf; ++f) out->n_bad_names += t.h_file_status[(size_t)f];
    out->first_bad = -1;
    out->first_bad_file = -1;
    if (h_bad != ~0ull) {
      out->first_bad = (int64_t)(h_bad >> 8);
      out->first_bad_reason = (int32_t)(h_bad & 0xFF);
      out->first_bad_file = (int32_t)tile_parse_file_of(t.h_file_line_off.data(), nf, out->first_bad);
    }
    out->device_ms = ms;
    out->n_files = (int32_t)nf;
    if (host) {
      out->rows = t.h_rows.data();
      out->row_off = t.h_row_off.data();
      out->file = (const uint64_t*)t.h_file.data();
      out->file_status = t.h_file_status.data();
      out->file_line_off = t.h_file_line_off.data();
      out->line_status = t.h_line_status.data();
    }
    out->d_rows = rows;
    out->d_row_off = row_off;
    out->d_file = (const uint64_t*)file;
    out->d_file_status = file_status;
    out->d_file_line_off = file_line_off;
    out->d_line_status = line_status;
    return OTR_OK;
  });
}

// ---- snapshot, restore, Segment.ListSerder records (K20) -------------------------------------

namespace {

void restore_result(otr_tile_restore_result* out, int64_t held) {
  memset(out, 0, sizeof(*out));
  out->bad_slice = out->bad_tile = -1;
  out->n_rows_held = held;
}

hipMemcpyKind copy_in(int memory) { return memory == OTR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice; }

const char* const kTileRestoreReason[] = {"",      "layout", "key",  "count", "segment", "duplicate",
                                          "map", "full",   "row"};

}  // namespace

int TileStore::sort_pairs(const unsigned long long* k_in, unsigned long long* k_out, const int32_t* v_in,
                          int32_t* v_out, int64_t n, std::string* err) {
  return pool_sort(*this, T_TMP, k_in, k_out, v_in, v_out, n, 0, 64, stream, err);
}

int TileStore::snapshot(int sflags, otr_tile_snapshot* out, std::string* err) {
  memset(out, 0, sizeof(*out));
  out->quantisation = cfg.quantisation;
  out->flags = flags;
  const size_t n = (size_t)n_rows;
  out->n_rows = n_rows;
  if (n == 0) return OTR_OK;
  const bool host = !(sflags & OTR_TILE_SNAPSHOT_NO_HOST);
  otr_tile_row* d_rows = get<otr_tile_row>(T_S_ROWS, n);
  HIPCHK(hipMemcpyAsync(d_rows, rows, sizeof(otr_tile_row) * n, hipMemcpyDeviceToDevice, stream));
  out->d_rows = d_rows;
  if (host) {
    h_snap_rows.resize(n);
    HIPCHK(hipMemcpyAsync(h_snap_rows.data(), rows, sizeof(otr_tile_row) * n, hipMemcpyDeviceToHost, stream));
    out->rows = h_snap_rows.data();
  }
  if (timed()) {
    double* d_t0 = get<double>(T_S_T0, n);
    double* d_t1 = get<double>(T_S_T1, n);
    HIPCHK(hipMemcpyAsync(d_t0, t0, 8 * n, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_t1, t1, 8 * n, hipMemcpyDeviceToDevice, stream));
    out->d_t0 = d_t0;
    out->d_t1 = d_t1;
    if (host) {
      h_snap_t0.resize(n);
      h_snap_t1.resize(n);
      HIPCHK(hipMemcpyAsync(h_snap_t0.data(), t0, 8 * n, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipMemcpyAsync(h_snap_t1.data(), t1, 8 * n, hipMemcpyDeviceToHost, stream));
      out->t0 = h_snap_t0.data();
      out->t1 = h_snap_t1.data();
    }
  }
  HIPCHK(hipStreamSynchronize(stream));
  return OTR_OK;
}

int TileStore::restore(const otr_tile_snapshot* snap, int memory, otr_tile_restore_result* out, std::string* err) {
  int rc;
  restore_result(out, n_rows);
  const int64_t n = snap->n_rows;
  if (n < 0 || n > kTstMaxRows) return bad(err, "tile restore: row count out of range");
  if (n == 0) return OTR_OK;
  if (!snap->rows || (timed() && (!snap->t0 || !snap->t1)))
    return bad(err, timed() ? "tile restore: a store with OTR_TILE_STORE_TIMES needs rows, t0 and t1"
                            : "null argument");
  HIPCHK(hipEventRecord(ev[0], stream));
  const otr_tile_row* d_rows = snap->rows;
  const double *d_t0 = snap->t0, *d_t1 = snap->t1;
  if (timed()) {
    if (memory != OTR_MEM_DEVICE) {  // staged: nothing reaches the store before the check has passed
      otr_tile_row* r = get<otr_tile_row>(T_S_ROWS, n);
      double* a = get<double>(T_S_T0, n);
      double* b = get<double>(T_S_T1, n);
      HIPCHK(hipMemcpyAsync(r, snap->rows, sizeof(otr_tile_row) * (size_t)n, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(a, snap->t0, 8 * (size_t)n, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(b, snap->t1, 8 * (size_t)n, hipMemcpyHostToDevice, stream));
      d_rows = r;
      d_t0 = a;
      d_t1 = b;
    }
    unsigned long long* verdict = get<unsigned long long>(T_S_VERDICT, 1);
    unsigned long long h_verdict = 0;
    HIPCHK(hipMemsetAsync(verdict, 0xFF, 8, stream));
    k_tilerec_check_rows<<<grid_ceil1(n, 256), 256, 0, stream>>>(d_rows, d_t0, d_t1, n, cfg.quantisation, verdict);
    HIPCHK(hipGetLastError());
    if ((rc = read_back(stream, err, fetch(&h_verdict, verdict)))) return rc;
    if (h_verdict != kTileRecNone) {
      out->bad_slice = (int64_t)h_verdict;
      out->bad_reason = OTR_TILE_RESTORE_E_ROW;
      return bad(err, "tile restore: row " + std::to_string(out->bad_slice) +
                          " is not the row its report gives under the store's quantisation");
    }
  }
  if (n > cfg.max_rows - n_rows) {
    out->bad_reason = OTR_TILE_RESTORE_E_FULL;
    return bad(err, "the restore would take the tile store beyond max_rows (" + std::to_string(n_rows) +
                        " rows held, " + std::to_string(n) + " given, max_rows " + std::to_string(cfg.max_rows) + ")");
  }
  const hipMemcpyKind kind = (timed() || memory == OTR_MEM_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIPCHK(hipMemcpyAsync(rows + n_rows, d_rows, sizeof(otr_tile_row) * (size_t)n, kind, stream));
  if (timed()) {
    HIPCHK(hipMemcpyAsync(t0 + n_rows, d_t0, 8 * (size_t)n, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemcpyAsync(t1 + n_rows, d_t1, 8 * (size_t)n, hipMemcpyDeviceToDevice, stream));
  }
  if ((rc = finish(&out->device_ms, err))) return rc;
  n_rows += n;
  out->n_rows = n;
  out->n_rows_held = n_rows;
  return OTR_OK;
}

int TileStore::export_records(int32_t slice_size, otr_tile_records* out, std::string* err) {
  int rc;
  memset(out, 0, sizeof(*out));
  if (!timed())
    return bad(err, "the records carry the reports' times: open the tile store with OTR_TILE_STORE_TIMES");
  if (slice_size < 1) return bad(err, "tile export: slice_size below 1");
  const int64_t n = n_rows, S = slice_size, q = cfg.quantisation;
  out->slice_size = slice_size;
  out->memory = OTR_MEM_HOST;
  HIPCHK(hipEventRecord(ev[0], stream));
  int64_t* rec_off = get<int64_t>(T_E_REC_OFF, 1);
  int64_t* name_off = get<int64_t>(T_E_NAME_OFF, 1);
  int64_t nf = 0, ns = 0, total[2] = {0, 0};
  int64_t *start = nullptr, *tile = nullptr;
  int32_t* slice = nullptr;
  uint32_t* map_words = nullptr;
  if (n > 0) {
    const unsigned g = grid_ceil1(n, 256);
    unsigned long long* key_a = get<unsigned long long>(T_KEY_A, n);
    unsigned long long* key_b = get<unsigned long long>(T_KEY_B, n);
    int32_t* idx_a = get<int32_t>(T_IDX_A, n);
    int32_t* idx_b = get<int32_t>(T_IDX_B, n);
    // arrival order within a file: a stable sort by `file` alone
    k_tilerec_keys<<<g, 256, 0, stream>>>(rows, n, key_a, idx_a);
    if ((rc = sort_pairs(key_a, key_b, idx_a, idx_b, n, err))) return rc;
    int64_t* head = get<int64_t>(T_F_HEAD, n);
    int64_t* head_incl = get<int64_t>(T_F_INCL, n);
    k_tilerec_heads<<<g, 256, 0, stream>>>(key_b, n, head);
    if ((rc = scan64(head, head_incl, n, err))) return rc;
    if ((rc = read_back(stream, err, fetch(&nf, head_incl + (n - 1))))) return rc;
    if (nf < 1 || nf > n) {
      if (err) *err = "tile export file split failed";
      return OTR_DEVICE_ERROR;
    }
    int64_t* fstart = get<int64_t>(T_F_START, nf);
    int64_t* shead = get<int64_t>(T_E_SHEAD, n);
    int64_t* shead_incl = get<int64_t>(T_E_SINCL, n);
    k_store_file_starts<<<g, 256, 0, stream>>>(head, head_incl, n, fstart);
    k_tilerec_slice_heads<<<g, 256, 0, stream>>>(head_incl, fstart, n, S, shead);
    if ((rc = scan64(shead, shead_incl, n, err))) return rc;
    if ((rc = read_back(stream, err, fetch(&ns, shead_incl + (n - 1))))) return rc;
    if (ns < nf || ns > n) {
      if (err) *err = "tile export slice split failed";
      return OTR_DEVICE_ERROR;
    }
    int64_t* pos = get<int64_t>(T_E_POS, (size_t)ns + 1);
    start = get<int64_t>(T_E_START, ns);
    tile = get<int64_t>(T_E_TILE, ns);
    slice = get<int32_t>(T_E_SLICE, ns);
    map_words = get<uint32_t>(T_E_MAP, 5 * (size_t)nf);
    int64_t* rec_len = get<int64_t>(T_E_REC_LEN, ns);
    int64_t* name_len = get<int64_t>(T_E_NAME_LEN, ns);
    rec_off = get<int64_t>(T_E_REC_OFF, (size_t)ns + 1);
    name_off = get<int64_t>(T_E_NAME_OFF, (size_t)ns + 1);
    k_tilerec_table<<<g, 256, 0, stream>>>(key_b, head, head_incl, fstart, nf, shead, shead_incl, n, ns, S, q, pos,
                                           start, tile, slice, map_words);
    k_tilerec_lens<<<grid_ceil1(ns, 256), 256, 0, stream>>>(pos, start, tile, slice, ns, rec_len, name_len);
    HIPCHK(hipMemsetAsync(rec_off, 0, 8, stream));
    HIPCHK(hipMemsetAsync(name_off, 0, 8, stream));
    if ((rc = scan64(rec_len, rec_off + 1, ns, err))) return rc;
    if ((rc = scan64(name_len, name_off + 1, ns, err))) return rc;
    if ((rc = read_back(stream, err, fetch(&total[0], rec_off + ns), fetch(&total[1], name_off + ns)))) return rc;
    if (total[0] != kTileRecHeader * ns + kTileRecSegment * n || total[1] < 5 * ns || total[1] > kTileKeyMax * ns) {
      if (err) *err = "tile export lengths failed";
      return OTR_DEVICE_ERROR;
    }
    uint8_t* bytes = get<uint8_t>(T_E_BYTES, (size_t)total[0]);
    uint8_t* names = get<uint8_t>(T_E_NAMES, (size_t)total[1]);
    const int64_t n_words = total[0] / 4;
    k_tilerec_emit<<<grid_ceil1(n_words, kTileRecEmit), kTileRecEmit, 0, stream>>>(rows, t0, t1, idx_b, pos, rec_off,
                                                                                   ns, n_words, (uint32_t*)bytes);
    k_tilerec_names<<<grid_ceil1(ns, 256), 256, 0, stream>>>(start, tile, slice, name_off, ns, names);
    HIPCHK(hipGetLastError());
    h_bytes.resize((size_t)total[0]);
    h_names.resize((size_t)total[1]);
    h_map.resize((size_t)(kTileMapEntry * nf));
    HIPCHK(hipMemcpyAsync(h_bytes.data(), bytes, (size_t)total[0], hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(h_names.data(), names, (size_t)total[1], hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(h_map.data(), map_words, h_map.size(), hipMemcpyDeviceToHost, stream));
    out->bytes = h_bytes.data();
    out->names = h_names.data();
    out->map_bytes = h_map.data();
    out->d_bytes = bytes;
    out->d_names = names;
    out->d_map_bytes = (const uint8_t*)map_words;
  } else {
    HIPCHK(hipMemsetAsync(rec_off, 0, 8, stream));
    HIPCHK(hipMemsetAsync(name_off, 0, 8, stream));
  }
  h_start.resize((size_t)ns);
  h_tile.resize((size_t)ns);
  h_slice.resize((size_t)ns);
  h_rec_off.resize((size_t)ns + 1);
  h_name_off.resize((size_t)ns + 1);
  if (ns > 0) {
    HIPCHK(hipMemcpyAsync(h_start.data(), start, 8 * (size_t)ns, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(h_tile.data(), tile, 8 * (size_t)ns, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(h_slice.data(), slice, 4 * (size_t)ns, hipMemcpyDeviceToHost, stream));
  }
  HIPCHK(hipMemcpyAsync(h_rec_off.data(), rec_off, 8 * ((size_t)ns + 1), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(h_name_off.data(), name_off, 8 * ((size_t)ns + 1), hipMemcpyDeviceToHost, stream));
  float ms = 0.f;
  if ((rc = finish(&ms, err))) return rc;
  out->n_slices = ns;
  out->n_bytes = total[0];
  out->n_name_bytes = total[1];
  out->n_tiles = nf;
  out->start = ns ? h_start.data() : nullptr;
  out->tile_id = ns ? h_tile.data() : nullptr;
  out->slice = ns ? h_slice.data() : nullptr;
  out->rec_off = h_rec_off.data();
  out->name_off = h_name_off.data();
  out->d_start = start;
  out->d_tile_id = tile;
  out->d_slice = slice;
  out->d_rec_off = rec_off;
  out->d_name_off = name_off;
  return OTR_OK;
}

int TileStore::restore_records(const otr_tile_records* in, otr_tile_restore_result* out, std::string* err) {
  int rc;
  restore_result(out, n_rows);
  const int64_t n = in->n_slices, nb = in->n_bytes, nt = in->n_tiles < 0 ? -1 : in->n_tiles;
  if (n < 0 || n >= (int64_t)INT32_MAX || nb < 0 || nt >= (int64_t)INT32_MAX)
    return bad(err, "tile records: counts out of range");
  if (in->slice_size < 1) return bad(err, "tile records: slice_size below 1");
  if ((n > 0 && (!in->start || !in->tile_id || !in->slice)) || !in->rec_off || (nb > 0 && !in->bytes) ||
      (nt > 0 && !in->map_bytes))
    return bad(err, "null argument");
  HIPCHK(hipEventRecord(ev[0], stream));
  TileRecIn a{};
  a.n_slices = n;
  a.n_bytes = nb;
  a.q = cfg.quantisation;
  a.slice_size = in->slice_size;
  const uint8_t* d_map = in->map_bytes;
  if (in->memory == OTR_MEM_DEVICE) {
    a.start = in->start;
    a.tile_id = in->tile_id;
    a.slice = in->slice;
    a.rec_off = in->rec_off;
    a.bytes = in->bytes;
  } else {
    int64_t* st = get<int64_t>(T_I_START, n);
    int64_t* ti = get<int64_t>(T_I_TILE, n);
    int32_t* sl = get<int32_t>(T_I_SLICE, n);
    int64_t* of = get<int64_t>(T_I_OFF, (size_t)n + 1);
    uint8_t* by = get<uint8_t>(T_I_BYTES, (size_t)nb);
    if (n > 0) {
      HIPCHK(hipMemcpyAsync(st, in->start, 8 * (size_t)n, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(ti, in->tile_id, 8 * (size_t)n, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(sl, in->slice, 4 * (size_t)n, hipMemcpyHostToDevice, stream));
    }
    HIPCHK(hipMemcpyAsync(of, in->rec_off, 8 * ((size_t)n + 1), hipMemcpyHostToDevice, stream));
    if (nb > 0) HIPCHK(hipMemcpyAsync(by, in->bytes, (size_t)nb, hipMemcpyHostToDevice, stream));
    if (nt > 0) {
      uint8_t* mp = get<uint8_t>(T_I_MAP, (size_t)(kTileMapEntry * nt));
      HIPCHK(hipMemcpyAsync(mp, in->map_bytes, (size_t)(kTileMapEntry * nt), hipMemcpyHostToDevice, stream));
      d_map = mp;
    }
    a.start = st;
    a.tile_id = ti;
    a.slice = sl;
    a.rec_off = of;
    a.bytes = by;
  }
  // words: the records' verdict, the map's verdict, then the TRC_* counters
  unsigned long long* words = get<unsigned long long>(T_I_WORDS, 2 + TRC_WORDS);
  unsigned long long h_words[2 + TRC_WORDS];
  HIPCHK(hipMemsetAsync(words, 0xFF, 16, stream));
  HIPCHK(hipMemsetAsync(words + 2, 0, 8 * TRC_WORDS, stream));
  int32_t* count = get<int32_t>(T_I_COUNT, n);
  int32_t* key_ok = get<int32_t>(T_I_KEY_OK, n);
  unsigned long long* file_key = get<unsigned long long>(T_I_FILE, n);
  unsigned long long* file_a = get<unsigned long long>(T_I_FILE_A, n);
  unsigned long long* file_b = get<unsigned long long>(T_I_FILE_B, n);
  unsigned long long* slice_key = get<unsigned long long>(T_I_SLICE_KEY, n);
  unsigned long long* slice_b = get<unsigned long long>(T_I_SLICE_B, n);
  int32_t* idx_a = get<int32_t>(T_I_IDX_A, n);
  int32_t* idx_b = get<int32_t>(T_I_IDX_B, n);
  int32_t* order = get<int32_t>(T_I_IDX_C, n);
  if (n > 0) {
    const unsigned g = grid_ceil1(n, 256);
    k_tilerec_validate<<<grid_ceil1(n, 256 / OTR_WAVE), 256, 0, stream>>>(a, count, key_ok, file_key, slice_key, idx_a,
                                                                          words);
    HIPCHK(hipGetLastError());
    // (file, slice) order, stable: by slice, then by file
    if ((rc = sort_pairs(slice_key, slice_b, idx_a, idx_b, n, err))) return rc;
    k_tilerec_gather<<<g, 256, 0, stream>>>(file_key, idx_b, n, file_a);
    if ((rc = sort_pairs(file_a, file_b, idx_b, order, n, err))) return rc;
    k_tilerec_duplicates<<<g, 256, 0, stream>>>(file_b, order, slice_key, key_ok, n, words);
    HIPCHK(hipGetLastError());
  }
  unsigned long long* map_b = get<unsigned long long>(T_M_FILE_B, nt > 0 ? nt : 1);
  int32_t* map_order = get<int32_t>(T_M_IDX_B, nt > 0 ? nt : 1);
  int32_t* map_value = get<int32_t>(T_M_VALUE, nt > 0 ? nt : 1);
  if (nt > 0) {
    unsigned long long* map_a = get<unsigned long long>(T_M_FILE_A, nt);
    int32_t* map_idx = get<int32_t>(T_M_IDX_A, nt);
    int32_t* map_ok = get<int32_t>(T_M_OK, nt);
    const unsigned gm = grid_ceil1(nt, 256);
    k_tilerec_map_keys<<<gm, 256, 0, stream>>>(d_map, nt, a.q, map_a, map_idx, map_value, map_ok, words + 1,
                                               words + 2);
    if ((rc = sort_pairs(map_a, map_b, map_idx, map_order, nt, err))) return rc;
    k_tilerec_map_duplicates<<<gm, 256, 0, stream>>>(map_b, map_order, map_ok, nt, words + 1);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpyAsync(h_words, words, 16, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (h_words[0] != kTileRecNone) {
    out->bad_slice = (int64_t)(h_words[0] >> 8);
    out->bad_reason = (int32_t)(h_words[0] & 0xFF);
    return bad(err, "tile records: slice record " + std::to_string(out->bad_slice) + ": " +
                        kTileRestoreReason[out->bad_reason]);
  }
  if (h_words[1] != kTileRecNone) {
    out->bad_tile = (int64_t)h_words[1];
    out->bad_reason = OTR_TILE_RESTORE_E_MAP;
    return bad(err, "tile records: map entry " + std::to_string(out->bad_tile) +
                        ": invalid key, negative value or repeated key");
  }
  if (n > 0) {
    int64_t* ref = get<int64_t>(T_I_REF, n);
    int64_t* row_off = get<int64_t>(T_I_ROW_OFF, (size_t)n + 1);
    HIPCHK(hipMemsetAsync(row_off, 0, 8, stream));
    // (the slice keys' sorted copy is free again: the join reads the keys in input order)
    k_tilerec_join<<<grid_ceil1(n, 256), 256, 0, stream>>>(file_b, order, slice_key, count, n, map_b, map_order,
                                                           map_value, nt, ref, words + 2);
    HIPCHK(hipGetLastError());
    if ((rc = scan64(ref, row_off + 1, n, err))) return rc;
    HIPCHK(hipMemcpyAsync(h_words, words, sizeof(h_words), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    const int64_t total = (int64_t)h_words[2 + TRC_ROWS];
    if (total > cfg.max_rows - n_rows) {
      out->bad_reason = OTR_TILE_RESTORE_E_FULL;
      return bad(err, "the restore would take the tile store beyond max_rows (" + std::to_string(n_rows) +
                          " rows held, " + std::to_string(total) + " referenced, max_rows " +
                          std::to_string(cfg.max_rows) + ")");
    }
    if (total > 0) {
      k_tilerec_write<<<grid_ceil1(n, 256 / OTR_WAVE), 256, 0, stream>>>(a, order, ref, row_off, rows + n_rows,
                                                                         timed() ? t0 + n_rows : nullptr,
                                                                         timed() ? t1 + n_rows : nullptr);
      HIPCHK(hipGetLastError());
    }
    if ((rc = finish(&out->device_ms, err))) return rc;
    n_rows += total;
    out->n_rows = total;
    out->n_slices = (int64_t)h_words[2 + TRC_SLICES];
    out->n_unreferenced_rows = (int64_t)h_words[2 + TRC_UNREF_ROWS];
    out->n_unreferenced_slices = (int64_t)h_words[2 + TRC_UNREF_SLICES];
  } else {
    HIPCHK(hipMemcpyAsync(h_words, words, sizeof(h_words), hipMemcpyDeviceToHost, stream));
    if ((rc = finish(&out->device_ms, err))) return rc;
  }
  if (nt >= 0) out->n_missing_slices = (int64_t)h_words[2 + TRC_NAMED] - out->n_slices;
  out->n_rows_held = n_rows;
  return OTR_OK;
}

}  // namespace otr

// the changelog's String keys, on the host (include/otr.h; the rules are otr_tile_records.h's)
extern "C" int otr_tile_slice_key(int64_t start, int64_t tile_id, int32_t slice, char* buf, int64_t cap) {
  const int32_t n = otr::tile_key_len(start, tile_id, slice);
  if (!buf || cap < n) return -1;
  otr::tile_key_put(start, tile_id, slice, (uint8_t*)buf);
  if (cap > n) buf[n] = 0;
  return n;
}

extern "C" int otr_tile_slice_key_parse(const char* text, int64_t len, int64_t* start, int64_t* tile_id,
                                        int32_t* slice) {
  if (!text || !start || !tile_id || !slice) return 1;
  return otr::tile_key_parse(text, len, start, tile_id, slice) ? 0 : 1;
}

namespace otr {

int Matcher::tile_store_snapshot(int flags, otr_tile_snapshot* out, std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    HIPCHK(hipSetDevice(graph_state().device));
    return tst->snapshot(flags, out, err);
  });
}

int Matcher::tile_store_restore(const otr_tile_snapshot* snap, int memory, otr_tile_restore_result* out,
                                std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    HIPCHK(hipSetDevice(graph_state().device));
    return tst->restore(snap, memory, out, err);
  });
}

int Matcher::tile_store_export_records(int32_t slice_size, otr_tile_records* out, std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    HIPCHK(hipSetDevice(graph_state().device));
    return tst->export_records(slice_size, out, err);
  });
}

int Matcher::tile_store_restore_records(const otr_tile_records* in, otr_tile_restore_result* out, std::string* err) {
  return guarded(*this, err, true, [&]() -> int {
    HIPCHK(hipSetDevice(graph_state().device));
    return tst->restore_records(in, out, err);
  });
}

}  // namespace otr
