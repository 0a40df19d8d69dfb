// otr_text.hip — the text stages in front of the matching pipeline, on the matcher's stream
// and workspace slots (otr_slots.h): probe ingest (K11, otr_ingest.h) and the stream formatter
// (K16, otr_formatter.h), the newline index and the uuid grouping they share, and K11's uuid
// hash on the host.  Nothing here reads the route tiers' build macros.
#include <cstring>

#include "otr_devscan.h"
#include "otr_engine.h"
#include "otr_formatter.h"
#include "otr_ingest.h"
#include "otr_slots.h"
#include "otr_util_kernels.h"

namespace otr {

// ---- the text front end ingest and the formatter share -----------------------------------
// (the parts that do not branch on the caller: each takes its slots and keeps its size refusals)
// the text into d_text, zero-padded to n_chunks whole 16-byte chunks
static int text_copy(hipStream_t stream, uint8_t* d_text, const void* text, int64_t len, hipMemcpyKind kind,
                     int64_t n_chunks, std::string* err) {
  HIPCHK(hipMemsetAsync(d_text + 16 * (n_chunks - 1), 0, 16, stream));
  if (len > 0) HIPCHK(hipMemcpyAsync(d_text, text, len, kind, stream));
  return OTR_OK;
}

// the refusal word reset and the call's first event recorded behind the copies
static int text_mark(Matcher& m, unsigned long long* bad, std::string* err) {
  HIPCHK(hipMemsetAsync(bad, 0xFF, 8, m.stream));
  if (!m.ev_init) {
    for (auto& e : m.ev) HIPCHK(hipEventCreate(&e));
    m.ev_init = true;
  }
  HIPCHK(hipEventRecord(m.ev[20], m.stream));
  return OTR_OK;
}

// The newlines of d_text[0, len), len > 0: k_nl_count per chunk, the scan (tmp: the caller's
// workspace for n_chunks), then the count and the last byte read back.  n_lines follows
// Python's file iteration: a final fragment without '\n' is a line too.
static int newline_count(hipStream_t stream, const uint8_t* d_text, int64_t len, int64_t n_chunks, int64_t* cnt,
                         int64_t* cscan, Workspace tmp, int64_t* n_nl, int64_t* n_lines, std::string* err) {
  int rc;
  k_nl_count<<<grid_ceil(n_chunks, 256), 256, 0, stream>>>(reinterpret_cast<const uint4*>(d_text), n_chunks, cnt);
  if ((rc = inclusive_sum(tmp, cnt, cscan, (int)n_chunks, stream, err))) return rc;
  uint8_t last = 0;
  if ((rc = read_back(stream, err, fetch(n_nl, cscan + (n_chunks - 1)), fetch(&last, d_text + (len - 1))))) return rc;
  *n_lines = *n_nl + (last != '\n' ? 1 : 0);
  return OTR_OK;
}

// ---- K11 ingest (include/otr.h otr_ingest) ----------------------------------------------
// The uuid grouping stage, shared by K11 and the stream formatter (K16): the M kept lines
// (kidx, ascending) sorted by (hash, line), the stable sort keeping line order within a
// hash, then group heads with a byte compare of every equal-hash neighbour: a collision
// lands in *bad as (line << 8 | OTR_INGEST_E_COLLISION).
static int uuid_group_heads(hipStream_t stream, const uint64_t* hash, const int32_t* kidx, int64_t M,
                            const int64_t* uoff, const int32_t* ulen, const uint8_t* d_text, Workspace tmp,
                            uint64_t* key_a, uint64_t* key_b, int32_t* val_b, int64_t* head, unsigned long long* bad,
                            std::string* err) {
  int rc;
  k_gather_by<uint64_t><<<grid_ceil(M, 256), 256, 0, stream>>>(hash, kidx, M, key_a);
  if ((rc = sort_pairs(tmp, key_a, key_b, kidx, val_b, (int)M, 0, 64, stream, err))) return rc;
  k_group_heads<<<grid_ceil(M, 256), 256, 0, stream>>>(key_b, val_b, M, uoff, ulen, d_text, head, bad);
  return OTR_OK;
}

int Matcher::ingest(const char* text, int64_t len, int memory, const otr_ingest_format* fmt, otr_ingest_result* out,
                    std::string* err) {
  return guarded(stream, err, [&]() -> int {
    GraphState& gs = graph_state();
    HIPCHK(hipSetDevice(gs.device));
    if (!stream) HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    memset(out, 0, sizeof(*out));
    out->bad_line = -1;
    if (fmt->rules < OTR_INGEST_SHARD || fmt->rules > OTR_INGEST_JAVA_SV || fmt->mode < 0 || fmt->mode > 2 ||
        fmt->inactivity < 0 || (fmt->rules != OTR_INGEST_SHARD && (fmt->separator < 1 || fmt->separator > 255))) {
      if (err) *err = "bad ingest format";
      return OTR_BAD_REQUEST;
    }
    for (int k : {fmt->uuid_index, fmt->time_index, fmt->lat_index, fmt->lon_index, fmt->accuracy_index})
      if (fmt->rules != OTR_INGEST_SHARD && (k < 0 || k > 4096)) {
        if (err) *err = "bad ingest field index";
        return OTR_BAD_REQUEST;
      }
    out->batch.memory = OTR_MEM_DEVICE;
    if (len <= 0) return OTR_OK;
    if (len >= ((int64_t)1 << 40)) {
      if (err) *err = "ingest text too large";
      return OTR_BAD_REQUEST;
    }
    // text in HBM, zero-padded to whole 16-byte chunks
    const int64_t n_chunks = (len + 15) / 16;
    uint8_t* d_text = need<uint8_t>(S_IN_TEXT, 16 * n_chunks);
    int64_t* cnt = need<int64_t>(S_IN_CNT, n_chunks);
    int64_t* cscan = need<int64_t>(S_IN_CSCAN, n_chunks);
    unsigned long long* bad = need<unsigned long long>(S_IN_BAD, 1);
    int rc;
    if ((rc = text_copy(stream, d_text, text, len,
                        memory == OTR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, n_chunks, err)) ||
        (rc = text_mark(*this, bad, err)))
      return rc;
    Workspace tmp;
    if ((rc = scan_bytes(cnt, cscan, (int)std::min<int64_t>(n_chunks, INT32_MAX), &tmp.bytes, stream, err))) return rc;
    if (n_chunks >= INT32_MAX) {
      if (err) *err = "ingest text too large";
      return OTR_DEVICE_ERROR;
    }
    tmp.p = need<char>(S_IN_TMP, tmp.bytes);
    int64_t n_nl = 0, n_lines = 0;
    if ((rc = newline_count(stream, d_text, len, n_chunks, cnt, cscan, tmp, &n_nl, &n_lines, err))) return rc;
    out->n_lines = n_lines;
    if (n_lines >= INT32_MAX) {
      if (err) *err = "too many lines for one ingest";
      return OTR_BAD_REQUEST;
    }
    const int64_t nL = std::max<int64_t>(n_lines, 1);
    int64_t* nl = need<int64_t>(S_IN_NL, std::max<int64_t>(n_nl, 1));
    IngestLines L{};
    L.text = d_text;
    L.len = len;
    L.nl = nl;
    L.n_nl = n_nl;
    L.n_lines = n_lines;
    L.hash = need<uint64_t>(S_IN_HASH, nL);
    L.uoff = need<int64_t>(S_IN_UOFF, nL);
    L.ulen = need<int32_t>(S_IN_ULEN, nL);
    L.time = need<int64_t>(S_IN_TIME, nL);
    L.lat = need<double>(S_IN_LAT, nL);
    L.lon = need<double>(S_IN_LON, nL);
    L.acc = need<float>(S_IN_ACC, nL);
    L.keep = need<int64_t>(S_IN_KEEP, nL);
    L.bad = bad;
    int64_t* kpos = need<int64_t>(S_IN_KPOS, nL);
    int32_t* kidx = need<int32_t>(S_IN_KIDX, nL);
    if (n_nl) k_nl_write<<<grid_ceil(n_chunks, 256), 256, 0, stream>>>(reinterpret_cast<const uint4*>(d_text), n_chunks,
                                                                       cscan, nl);
    IngestFmt f{};
    f.rules = fmt->rules;
    f.sep = fmt->separator;
    f.tfmt = fmt->time_format;
    f.use_bbox = fmt->use_bbox;
    f.idx[0] = fmt->uuid_index;
    f.idx[1] = fmt->time_index;
    f.idx[2] = fmt->lat_index;
    f.idx[3] = fmt->lon_index;
    f.idx[4] = fmt->accuracy_index;
    for (int k = 0; k < 4; ++k) f.bbox[k] = fmt->bbox[k];
    HIPCHK(hipEventRecord(ev[21], stream));
    k_ingest_parse<<<grid_ceil(n_lines, 256), 256, 0, stream>>>(L, f);
    HIPCHK(hipEventRecord(ev[22], stream));
    unsigned long long hbad = ~0ull;
    if ((rc = read_back(stream, err, fetch(&hbad, bad)))) return rc;
    if (hbad != ~0ull) {
      out->bad_line = (int64_t)(hbad >> 8);
      out->bad_reason = (int32_t)(hbad & 0xFF);
      if (err) *err = "malformed probe line " + std::to_string(out->bad_line);
      return OTR_BAD_REQUEST;
    }
    // kept lines (bbox), in line order
    const int nI = (int)n_lines;
    // (the stream is drained: the workspace may grow to what the scans and sorts below need)
    if ((rc = scan_sort_bytes(L.keep, kpos, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const int32_t*)nullptr,
                              (int32_t*)nullptr, nI, &tmp.bytes, stream, err)))
      return rc;
    tmp.p = need<char>(S_IN_TMP, tmp.bytes);
    if ((rc = inclusive_sum(tmp, L.keep, kpos, nI, stream, err))) return rc;
    k_scatter_index<int32_t><<<grid_ceil(n_lines, 256), 256, 0, stream>>>(L.keep, kpos, n_lines, kidx);
    int64_t M = 0;
    if ((rc = read_back(stream, err, fetch(&M, kpos + (n_lines - 1))))) return rc;
    out->n_kept = M;
    if (M == 0) return OTR_OK;
    const int nM = (int)M;
    uint64_t* key_a = need<uint64_t>(S_IN_KEY_A, M);
    uint64_t* key_b = need<uint64_t>(S_IN_KEY_B, M);
    int32_t* val_a = need<int32_t>(S_IN_VAL_A, M);
    int32_t* val_b = need<int32_t>(S_IN_VAL_B, M);
    int64_t* head = need<int64_t>(S_IN_HEAD, M);
    int64_t* gid = need<int64_t>(S_IN_GID, M);
    int32_t* gfirst = need<int32_t>(S_IN_GFIRST, M);
    uint32_t* gkey = need<uint32_t>(S_IN_GKEY, nL);
    // 1. group by uuid: sort (hash, line) — the stable sort keeps line order within a hash
    if ((rc = uuid_group_heads(stream, L.hash, kidx, M, L.uoff, L.ulen, d_text, tmp, key_a, key_b, val_b, head, bad,
                               err)))
      return rc;
    if ((rc = inclusive_sum(tmp, head, gid, nM, stream, err))) return rc;
    k_group_first<<<grid_ceil(M, 256), 256, 0, stream>>>(head, gid, val_b, M, gfirst);
    k_group_key<<<grid_ceil(M, 256), 256, 0, stream>>>(gid, val_b, M, gfirst, gkey);
    int64_t n_uuid = 0;
    HIPCHK(hipMemcpyAsync(&n_uuid, gid + (M - 1), 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(&hbad, bad, 8, hipMemcpyDeviceToHost, stream));
    // 2. final order (first appearance of the uuid, time, line): stable LSD passes
    int64_t* tkey_a = reinterpret_cast<int64_t*>(key_a);
    int64_t* tkey_b = reinterpret_cast<int64_t*>(key_b);
    k_gather_by<int64_t><<<grid_ceil(M, 256), 256, 0, stream>>>(L.time, kidx, M, tkey_a);
    if ((rc = sort_pairs(tmp, tkey_a, tkey_b, kidx, val_a, nM, 0, 64, stream, err))) return rc;
    uint32_t* gk_a = reinterpret_cast<uint32_t*>(key_a);
    uint32_t* gk_b = reinterpret_cast<uint32_t*>(key_b);
    k_gather_by<uint32_t><<<grid_ceil(M, 256), 256, 0, stream>>>(gkey, val_a, M, gk_a);
    int end_bit = 1;
    while (end_bit < 32 && ((int64_t)1 << end_bit) < n_lines) ++end_bit;
    if ((rc = sort_pairs(tmp, gk_a, gk_b, val_a, val_b, nM, 0, end_bit, stream, err))) return rc;
    const int32_t* perm = val_b;
    // 3. windows
    k_win_heads<<<grid_ceil(M, 256), 256, 0, stream>>>(perm, M, gkey, L.time, fmt->inactivity, head);
    if ((rc = inclusive_sum(tmp, head, gid, nM, stream, err))) return rc;  // gid: window ids now
    int64_t n_win = 0;
    if ((rc = read_back(stream, err, fetch(&n_win, gid + (M - 1))))) return rc;
    if (hbad != ~0ull) {
      out->bad_line = (int64_t)(hbad >> 8);
      out->bad_reason = (int32_t)(hbad & 0xFF);
      if (err) *err = "uuid hash collision at line " + std::to_string(out->bad_line);
      return OTR_BAD_REQUEST;
    }
    out->n_uuids = (int32_t)n_uuid;
    int64_t* ws = need<int64_t>(S_IN_WS, n_win);
    int64_t* klen = need<int64_t>(S_IN_KLEN, n_win);
    int64_t* kflag = need<int64_t>(S_IN_KFLAG, n_win);
    int64_t* poff = need<int64_t>(S_IN_POFF, n_win);
    int64_t* tpos = need<int64_t>(S_IN_TPOS, n_win);
    k_scatter_index<int64_t><<<grid_ceil(M, 256), 256, 0, stream>>>(head, gid, M, ws);
    k_win_len<<<grid_ceil(n_win, 256), 256, 0, stream>>>(ws, n_win, M, klen, kflag);
    if ((rc = inclusive_sum(tmp, klen, poff, (int)n_win, stream, err))) return rc;
    if ((rc = inclusive_sum(tmp, kflag, tpos, (int)n_win, stream, err))) return rc;
    int64_t n_tr = 0, n_pr = 0;
    if ((rc = read_back(stream, err, fetch(&n_tr, tpos + (n_win - 1)), fetch(&n_pr, poff + (n_win - 1))))) return rc;
    out->n_traces = (int32_t)n_tr;
    out->n_probes = n_pr;
    if (n_tr == 0) return OTR_OK;
    IngestOut o{};
    o.trace_off = need<int64_t>(S_IN_T_OFF, n_tr + 1);
    o.lat = need<double>(S_IN_T_LAT, n_pr);
    o.lon = need<double>(S_IN_T_LON, n_pr);
    o.time = need<int64_t>(S_IN_T_TIME, n_pr);
    o.acc = need<float>(S_IN_T_ACC, n_pr);
    o.mode = need<uint8_t>(S_IN_T_MODE, n_tr);
    o.uoff = need<int64_t>(S_IN_T_UOFF, n_tr);
    o.ulen = need<int32_t>(S_IN_T_ULEN, n_tr);
    k_win_emit<<<grid_ceil(M, 256), 256, 0, stream>>>(perm, M, gid, ws, klen, poff, tpos, (int32_t)n_tr, L,
                                                      (uint8_t)fmt->mode, o);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev[23], stream));
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipEventElapsedTime(&out->parse_ms, ev[21], ev[22]));
    HIPCHK(hipEventElapsedTime(&out->total_ms, ev[20], ev[23]));
    otr_trace_batch& b = out->batch;
    b.n_traces = (int32_t)n_tr;
    b.memory = OTR_MEM_DEVICE;
    b.trace_offsets = o.trace_off;
    b.lat = o.lat;
    b.lon = o.lon;
    b.time = o.time;
    b.accuracy = o.acc;
    b.mode = o.mode;
    out->d_trace_uuid_off = o.uoff;
    out->d_trace_uuid_len = o.ulen;
    return OTR_OK;
  });
}

// ---- K16 stream formatter (include/otr.h otr_format_messages) ---------------------------
int Matcher::format_messages(const otr_message_format* fmt, const otr_messages* msgs, otr_format_result* out,
                             std::string* err) {
  return guarded(stream, err, [&]() -> int {
    GraphState& gs = graph_state();
    HIPCHK(hipSetDevice(gs.device));
    if (!stream) HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    memset(out, 0, sizeof(*out));
    out->first_bad = -1;
    out->points.memory = OTR_MEM_DEVICE;
    auto refuse = [&](const char* what) {
      if (err) *err = what;
      return OTR_BAD_REQUEST;
    };
    // the format
    MsgFmt f{};
    f.type = fmt->type;
    f.sep = fmt->separator;
    f.tfmt = fmt->time_format;
    f.idx[FM_UUID] = fmt->uuid_index;
    f.idx[FM_TIME] = fmt->time_index;
    f.idx[FM_LAT] = fmt->lat_index;
    f.idx[FM_LON] = fmt->lon_index;
    f.idx[FM_ACC] = fmt->accuracy_index;
    if ((f.type != OTR_FORMAT_SV && f.type != OTR_FORMAT_JSON) ||
        (f.tfmt != OTR_TIME_EPOCH && f.tfmt != OTR_TIME_YMDHMS))
      return refuse("bad message format");
    uint8_t h_keys[5 * 64] = {0};
    if (f.type == OTR_FORMAT_SV) {
      if (f.sep < 1 || f.sep > 255) return refuse("bad message format: separator");
      for (int k = 0; k < 5; ++k)
        if (f.idx[k] < 0 || f.idx[k] > 4096) return refuse("bad message field index");
    } else {
      const char* keys[5];
      keys[FM_UUID] = fmt->uuid_key;
      keys[FM_TIME] = fmt->time_key;
      keys[FM_LAT] = fmt->lat_key;
      keys[FM_LON] = fmt->lon_key;
      keys[FM_ACC] = fmt->accuracy_key;
      for (int k = 0; k < 5; ++k) {
        if (!keys[k]) return refuse("bad message format: null key");
        const size_t n = strnlen(keys[k], 65);
        if (n < 1 || n > 64 || memchr(keys[k], '"', n) || memchr(keys[k], '\\', n))
          return refuse("bad message key: 1..64 bytes, no quote, no backslash");
        f.klen[k] = (int)n;
        memcpy(h_keys + 64 * k, keys[k], n);
      }
    }
    // the messages
    const int64_t len = msgs->len;
    const bool given = msgs->msg_off != nullptr;
    if (len < 0 || (len > 0 && !msgs->text) || (given && msgs->n_messages < 0)) return refuse("bad messages");
    if (len >= ((int64_t)1 << 40)) return refuse("message text too large");
    if (given && msgs->n_messages >= INT32_MAX) return refuse("too many messages for one call");
    const hipMemcpyKind kind = msgs->memory == OTR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const int64_t n_chunks = std::max<int64_t>((len + 15) / 16, 1);
    if (n_chunks >= INT32_MAX) return refuse("message text too large");
    int rc;
    uint8_t* d_text = need<uint8_t>(S_IN_TEXT, 16 * n_chunks);
    unsigned long long* bad = need<unsigned long long>(S_IN_BAD, 1);
    uint8_t* d_keys = need<uint8_t>(S_FM_KEYS, sizeof(h_keys));
    f.keys = d_keys;
    if ((rc = text_copy(stream, d_text, msgs->text, len, kind, n_chunks, err))) return rc;
    HIPCHK(hipMemcpyAsync(d_keys, h_keys, sizeof(h_keys), hipMemcpyHostToDevice, stream));
    if ((rc = text_mark(*this, bad, err))) return rc;
    // message bounds: the given offsets, or K11's newline index
    int64_t n = 0, n_nl = 0;
    const int64_t* d_off = nullptr;
    const int64_t* nl = nullptr;
    Workspace tmp;
    if (given) {
      n = msgs->n_messages;
      int64_t* off = need<int64_t>(S_FM_OFF, n + 1);
      int32_t* wrong = need<int32_t>(S_FM_WRONG, 1);
      HIPCHK(hipMemcpyAsync(off, msgs->msg_off, 8 * (n + 1), kind, stream));
      HIPCHK(hipMemsetAsync(wrong, 0, 4, stream));
      k_format_check_off<<<grid_ceil(n + 1, 256), 256, 0, stream>>>(off, n, len, wrong);
      int32_t h_wrong = 0;
      if ((rc = read_back(stream, err, fetch(&h_wrong, wrong)))) return rc;
      if (h_wrong) return refuse("message offsets must ascend from >= 0 to <= len");
      d_off = off;
    } else if (len > 0) {
      int64_t* cnt = need<int64_t>(S_IN_CNT, n_chunks);
      int64_t* cscan = need<int64_t>(S_IN_CSCAN, n_chunks);
      if ((rc = scan_bytes(cnt, cscan, (int)n_chunks, &tmp.bytes, stream, err))) return rc;
      tmp.p = need<char>(S_IN_TMP, tmp.bytes);
      // (n: a final fragment without '\n' is a message too)
      if ((rc = newline_count(stream, d_text, len, n_chunks, cnt, cscan, tmp, &n_nl, &n, err))) return rc;
      if (n >= INT32_MAX) return refuse("too many messages for one call");
      int64_t* nlw = need<int64_t>(S_IN_NL, std::max<int64_t>(n_nl, 1));
      if (n_nl)
        k_nl_write<<<grid_ceil(n_chunks, 256), 256, 0, stream>>>(reinterpret_cast<const uint4*>(d_text), n_chunks,
                                                                 cscan, nlw);
      nl = nlw;
    }
    out->n_messages = n;
    if (n == 0) return OTR_OK;
    const int64_t* ts_in = nullptr;
    if (msgs->timestamp) {
      if (kind == hipMemcpyHostToDevice) {
        int64_t* t = need<int64_t>(S_FM_TSIN, n);
        HIPCHK(hipMemcpyAsync(t, msgs->timestamp, 8 * n, kind, stream));
        ts_in = t;
      } else {
        ts_in = msgs->timestamp;
      }
    }
    FormatMsgs M{};
    M.text = d_text;
    M.len = len;
    M.nl = nl;
    M.n_nl = n_nl;
    M.off = d_off;
    M.n = n;
    M.status = need<int32_t>(S_FM_STATUS, n);
    M.hash = need<uint64_t>(S_IN_HASH, n);
    M.uoff = need<int64_t>(S_IN_UOFF, n);
    M.ulen = need<int32_t>(S_IN_ULEN, n);
    M.time = need<int64_t>(S_IN_TIME, n);
    M.lat = need<float>(S_FM_P_LAT, n);
    M.lon = need<float>(S_FM_P_LON, n);
    M.acc = need<int32_t>(S_FM_P_ACC, n);
    M.flag = need<int64_t>(S_FM_FLAG, n);
    M.bad = bad;
    int64_t* scan = need<int64_t>(S_IN_KPOS, n);
    const int nI = (int)n;
    // (the stream is drained but for k_nl_write, which does not touch the workspace: it may
    // grow to what the scan and the sort below need)
    if ((rc = scan_sort_bytes(M.flag, scan, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const int32_t*)nullptr,
                              (int32_t*)nullptr, nI, &tmp.bytes, stream, err)))
      return rc;
    tmp.p = need<char>(S_IN_TMP, tmp.bytes);
    // parse → flag → scan → emit
    HIPCHK(hipEventRecord(ev[21], stream));
    k_format_parse<<<grid_ceil(n, 256), 256, 0, stream>>>(M, f);
    HIPCHK(hipEventRecord(ev[22], stream));
    if ((rc = inclusive_sum(tmp, M.flag, scan, nI, stream, err))) return rc;
    int64_t total = 0;
    unsigned long long hbad = ~0ull;
    if ((rc = read_back(stream, err, fetch(&total, scan + (n - 1)), fetch(&hbad, bad)))) return rc;
    const int64_t P = total & 0xFFFFFFFFll, n_drop = total >> 32;
    const int64_t first_bad = hbad == ~0ull ? -1 : (int64_t)(hbad >> 8);
    const int32_t first_reason = hbad == ~0ull ? 0 : (int32_t)(hbad & 0xFF);
    const int64_t nP = std::max<int64_t>(P, 1);
    FormatOut o{};
    o.key = need<unsigned long long>(S_FM_KEY, nP);
    o.lat = need<float>(S_FM_LAT, nP);
    o.lon = need<float>(S_FM_LON, nP);
    o.acc = need<int32_t>(S_FM_ACC, nP);
    o.time = need<int64_t>(S_FM_TIME, nP);
    o.ts = need<int64_t>(S_FM_TS, nP);
    o.msg = need<int64_t>(S_FM_MSG, nP);
    o.uoff = need<int64_t>(S_FM_UOFF, nP);
    o.ulen = need<int32_t>(S_FM_ULEN, nP);
    o.kidx = need<int32_t>(S_IN_KIDX, nP);
    if (P > 0) {
      k_format_emit<<<grid_ceil(n, 256), 256, 0, stream>>>(M, scan, ts_in, msgs->timestamp_all, o);
      // two different uuids of the chunk under one hash: K11's stage, K11's refusal
      uint64_t* key_a = need<uint64_t>(S_IN_KEY_A, P);
      uint64_t* key_b = need<uint64_t>(S_IN_KEY_B, P);
      int32_t* val_b = need<int32_t>(S_IN_VAL_B, P);
      int64_t* head = need<int64_t>(S_IN_HEAD, P);
      HIPCHK(hipMemsetAsync(bad, 0xFF, 8, stream));
      if ((rc = uuid_group_heads(stream, M.hash, o.kidx, P, M.uoff, M.ulen, d_text, tmp, key_a, key_b, val_b, head, bad,
                                 err)))
        return rc;
      HIPCHK(hipMemcpyAsync(&hbad, bad, 8, hipMemcpyDeviceToHost, stream));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev[23], stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (P > 0 && hbad != ~0ull) {
      out->first_bad = (int64_t)(hbad >> 8);
      out->first_bad_reason = (int32_t)(hbad & 0xFF);
      if (err) *err = "uuid hash collision at message " + std::to_string(out->first_bad);
      return OTR_BAD_REQUEST;
    }
    HIPCHK(hipEventElapsedTime(&out->parse_ms, ev[21], ev[22]));
    HIPCHK(hipEventElapsedTime(&out->total_ms, ev[20], ev[23]));
    out->n_points = P;
    out->n_dropped = n_drop;
    out->n_unsupported = n - P - n_drop;
    out->first_bad = first_bad;
    out->first_bad_reason = first_reason;
    out->points.n = P;
    out->points.key = (const uint64_t*)o.key;
    out->points.lat = o.lat;
    out->points.lon = o.lon;
    out->points.accuracy = o.acc;
    out->points.time = o.time;
    out->points.timestamp = o.ts;
    fmt_text = d_text;
    fmt_text_len = len;
    out->d_message = o.msg;
    out->d_uuid_off = o.uoff;
    out->d_uuid_len = o.ulen;
    out->d_status = M.status;
    return OTR_OK;
  });
}

// K11's uuid_hash on the host: the key of a changelog record (otr_uuid_key)
uint64_t uuid_key_host(const char* uuid, int64_t len) {
  return uuid_hash(reinterpret_cast<const uint8_t*>(uuid), 0, len > 0 ? len : 0);
}

}  // namespace otr
