// otr_tile_records.h — K20: the anonymiser's state as the reference's changelog records
// (include/otr.h otr_tile_store_export_records / _restore_records).
//   slice record (Segment.ListSerder, Segment.java:131-155), big-endian: int32 count, then
//     count x (int64 id, int64 next_id, double min, double max, int32 length, int32 queue):
//     4 + 40 * count bytes
//   map entry (TimeQuantisedTile.Serder key + Kafka's integer value): int64 start,
//     int64 tile_id, int32 slice: 20 bytes
// The per-record rules are __host__ __device__ and use no libc, so that
// tools/tilerecordcheck.cpp runs the very same functions on the CPU (under sanitizers) that the
// kernels below run on the device.  Input bytes are read one at a time: a record may start at
// any address.
#pragma once
#include <stdint.h>

#include "../../include/otr.h"
#include "otr_session_records.h"
#include "otr_tiletext.h"

#if defined(__HIPCC__)
#define OTR_TR_HD __host__ __device__ inline
#else
#define OTR_TR_HD inline
#endif

namespace otr {

constexpr int64_t kTileRecHeader = 4;
constexpr int64_t kTileRecSegment = 40;
constexpr int64_t kTileMapEntry = 20;
constexpr int64_t kTileMaxBucket = (int64_t)1 << 39;  // `file` holds the bucket in 39 bits
constexpr int kTileKeyMax = 20 + 1 + 20 + 1 + 11;     // the longest slice key text

struct TileSegment {
  uint64_t id, next_id;
  double t0, t1;
  int32_t length, queue;
};

OTR_TR_HD double tr_bits_double(uint64_t u) { return __builtin_bit_cast(double, u); }
OTR_TR_HD uint64_t tr_double_bits(double d) { return __builtin_bit_cast(uint64_t, d); }

// `file` of a valid key, and back
OTR_TR_HD uint64_t tile_rec_file(int64_t bucket, int64_t tile_id) {
  return ((uint64_t)bucket << 25) | (((uint64_t)tile_id & 7ull) << 22) | (((uint64_t)tile_id >> 3) & 0x3FFFFFull);
}
OTR_TR_HD int64_t tile_rec_tile_id(uint64_t file) {
  return (int64_t)(((file >> 22) & 7ull) | ((file & 0x3FFFFFull) << 3));
}

// Record [b, e) of a buffer of n_bytes: inside the buffer, at least a header, and as long as its
// count says, in 64 bits.  count is set once the header is readable.
OTR_TR_HD bool tile_rec_layout_ok(const uint8_t* bytes, int64_t n_bytes, int64_t b, int64_t e, int32_t* count) {
  *count = 0;
  if (b < 0 || e < b || e > n_bytes || e - b < kTileRecHeader) return false;
  *count = (int32_t)rec_get32(bytes + b);
  return kTileRecHeader + kTileRecSegment * (int64_t)*count == e - b;
}

// OTR_TILE_RESTORE_E_KEY's rule (slice: of a record; of a map entry pass 0)
OTR_TR_HD bool tile_rec_key_ok(int64_t start, int64_t tile_id, int32_t slice, int64_t q) {
  return start >= 0 && start % q == 0 && start / q < kTileMaxBucket && tile_id >= 0 && tile_id <= 0x1FFFFFF &&
         slice >= 0;
}

OTR_TR_HD TileSegment tile_rec_segment_get(const uint8_t* rec, int32_t k) {
  const uint8_t* p = rec + kTileRecHeader + kTileRecSegment * (int64_t)k;
  TileSegment s;
  s.id = rec_get64(p);
  s.next_id = rec_get64(p + 8);
  s.t0 = tr_bits_double(rec_get64(p + 16));
  s.t1 = tr_bits_double(rec_get64(p + 24));
  s.length = (int32_t)rec_get32(p + 32);
  s.queue = (int32_t)rec_get32(p + 36);
  return s;
}

OTR_TR_HD void tile_rec_segment_put(uint8_t* rec, int32_t k, const TileSegment& s) {
  uint8_t* p = rec + kTileRecHeader + kTileRecSegment * (int64_t)k;
  rec_put64(p, s.id);
  rec_put64(p + 8, s.next_id);
  rec_put64(p + 16, tr_double_bits(s.t0));
  rec_put64(p + 24, tr_double_bits(s.t1));
  rec_put32(p + 32, (uint32_t)s.length);
  rec_put32(p + 36, (uint32_t)s.queue);
}

// dword w of a record of `count` segments, in memory order (so that a little-endian dword store
// writes the big-endian bytes); seg: the segment w lies in (w >= 1: segment (w - 1) / 10)
OTR_TR_HD uint32_t tr_bswap32(uint32_t v) {
  return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24);
}
OTR_TR_HD uint32_t tile_rec_segment_word(const TileSegment& s, int32_t field) {
  uint32_t v;
  switch (field) {
    case 0: v = (uint32_t)(s.id >> 32); break;
    case 1: v = (uint32_t)s.id; break;
    case 2: v = (uint32_t)(s.next_id >> 32); break;
    case 3: v = (uint32_t)s.next_id; break;
    case 4: v = (uint32_t)(tr_double_bits(s.t0) >> 32); break;
    case 5: v = (uint32_t)tr_double_bits(s.t0); break;
    case 6: v = (uint32_t)(tr_double_bits(s.t1) >> 32); break;
    case 7: v = (uint32_t)tr_double_bits(s.t1); break;
    case 8: v = (uint32_t)s.length; break;
    default: v = (uint32_t)s.queue; break;
  }
  return tr_bswap32(v);
}

// OTR_TILE_RESTORE_E_SEGMENT's rule: Segment.valid (Segment.java:38-40), times the (long) casts
// are exact for, the key's tile, and the key's bucket within the segment's span
// (TimeQuantisedTile.getTiles, TimeQuantisedTile.java:26-35)
OTR_TR_HD bool tile_rec_segment_ok(const TileSegment& s, int64_t tile_id, int64_t bucket, int64_t q) {
  if (!(s.t0 > 0 && s.t1 > 0 && s.t1 > s.t0 && s.length > 0 && s.queue >= 0)) return false;
  if (s.t1 >= 4611686018427387904.0) return false;  // 2^62
  if ((int64_t)(s.id & 0x1FFFFFFull) != tile_id) return false;
  return bucket >= (int64_t)s.t0 / q && bucket <= (int64_t)s.t1 / q;
}

// ---- map entries and key texts ------------------------------------------------------------
OTR_TR_HD void tile_map_get(const uint8_t* p, int64_t* start, int64_t* tile_id, int32_t* value) {
  *start = (int64_t)rec_get64(p);
  *tile_id = (int64_t)rec_get64(p + 8);
  *value = (int32_t)rec_get32(p + 16);
}
OTR_TR_HD void tile_map_put(uint8_t* p, int64_t start, int64_t tile_id, int32_t value) {
  rec_put64(p, (uint64_t)start);
  rec_put64(p + 8, (uint64_t)tile_id);
  rec_put32(p + 16, (uint32_t)value);
}

OTR_TR_HD int32_t tile_key_len(int64_t start, int64_t tile_id, int32_t slice) {
  return tt_len_i64(start) + 1 + tt_len_i64(tile_id) + 1 + tt_len_i32(slice);
}
OTR_TR_HD int32_t tile_key_put(int64_t start, int64_t tile_id, int32_t slice, uint8_t* out) {
  const TtPtrSink s{out};
  int64_t pos = tt_put_i64(s, 0, start);
  s.set(pos++, (uint8_t)'_');
  pos = tt_put_i64(s, pos, tile_id);
  s.set(pos++, (uint8_t)'.');
  pos = tt_put_i32(s, pos, slice);
  return (int32_t)pos;
}

// One number as Long.toString prints it, from text[*pos] up to `stop` (not consumed) or the
// end: an optional '-', no '+', no leading zeros, no "-0", within int64.  false: anything else.
OTR_TR_HD bool tile_key_number(const char* text, int64_t len, int64_t* pos, char stop, int64_t* out) {
  int64_t p = *pos;
  const bool neg = p < len && text[p] == '-';
  if (neg) ++p;
  const int64_t d0 = p;
  uint64_t v = 0;
  const uint64_t lim = neg ? (uint64_t)1 << 63 : ((uint64_t)1 << 63) - 1;
  while (p < len && text[p] != stop) {
    const char c = text[p];
    if (c < '0' || c > '9') return false;
    const uint64_t d = (uint64_t)(c - '0');
    if (v > (lim - d) / 10ull) return false;
    v = v * 10ull + d;
    ++p;
  }
  const int64_t nd = p - d0;
  if (nd < 1 || (nd > 1 && text[d0] == '0') || (neg && v == 0)) return false;
  *out = neg ? (int64_t)(0ull - v) : (int64_t)v;
  *pos = p;
  return true;
}

OTR_TR_HD bool tile_key_parse(const char* text, int64_t len, int64_t* start, int64_t* tile_id, int32_t* slice) {
  int64_t pos = 0, sl = 0;
  if (len < 0 || !tile_key_number(text, len, &pos, '_', start) || pos >= len) return false;
  ++pos;
  if (!tile_key_number(text, len, &pos, '.', tile_id) || pos >= len) return false;
  ++pos;
  if (!tile_key_number(text, len, &pos, '\0', &sl) || pos != len) return false;
  if (sl < -2147483648ll || sl > 2147483647ll) return false;
  *slice = (int32_t)sl;
  return true;
}

}  // namespace otr

#if defined(__HIPCC__)
#include "otr_tilerow.h"

namespace otr {

// ---- export ---------------------------------------------------------------------------------
// Input: the held rows' `file` values sorted (stable, so arrival order within a file) with the
// row index as payload.  Passes are ordered by kernel boundaries only.

__global__ void k_tilerec_keys(const otr_tile_row* rows, int64_t n, unsigned long long* key, int32_t* idx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  key[i] = rows[i].file;
  idx[i] = (int32_t)i;
}

__global__ void k_tilerec_heads(const unsigned long long* key, int64_t n, int64_t* head) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) head[i] = (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
}

// sorted position j opens a slice where its rank in its file is a multiple of S
__global__ void k_tilerec_slice_heads(const int64_t* head_incl, const int64_t* fstart, int64_t n, int64_t S,
                                      int64_t* shead) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) shead[j] = ((j - fstart[head_incl[j] - 1]) % S == 0) ? 1 : 0;
}

// the slice table (pos: the slice's first sorted position, pos[n_slices] = n), the slices' keys
// and the map entries (20 bytes each, 4-byte aligned: five dword stores)
__global__ void k_tilerec_table(const unsigned long long* key, const int64_t* head, const int64_t* head_incl,
                                const int64_t* fstart, int64_t n_files, const int64_t* shead,
                                const int64_t* shead_incl, int64_t n, int64_t n_slices, int64_t S, int64_t q,
                                int64_t* pos, int64_t* start, int64_t* tile_id, int32_t* slice, uint32_t* map_words) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  if (j == 0) pos[n_slices] = n;
  if (!shead[j]) return;
  const int64_t f = head_incl[j] - 1, sl = shead_incl[j] - 1;
  const unsigned long long file = key[j];
  const int64_t st = (int64_t)(file >> 25) * q, tid = tile_rec_tile_id(file);
  pos[sl] = j;
  start[sl] = st;
  tile_id[sl] = tid;
  slice[sl] = (int32_t)((j - fstart[f]) / S);
  if (head[j]) {
    const int64_t rows_in = (f + 1 < n_files ? fstart[f + 1] : n) - j;
    uint32_t* w = map_words + 5 * f;
    w[0] = tr_bswap32((uint32_t)((uint64_t)st >> 32));
    w[1] = tr_bswap32((uint32_t)st);
    w[2] = tr_bswap32((uint32_t)((uint64_t)tid >> 32));
    w[3] = tr_bswap32((uint32_t)tid);
    w[4] = tr_bswap32((uint32_t)(rows_in / S));
  }
}

__global__ void k_tilerec_lens(const int64_t* pos, const int64_t* start, const int64_t* tile_id,
                               const int32_t* slice, int64_t n_slices, int64_t* rec_len, int64_t* name_len) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slices) return;
  rec_len[s] = kTileRecHeader + kTileRecSegment * (pos[s + 1] - pos[s]);
  name_len[s] = (int64_t)tile_key_len(start[s], tile_id[s], slice[s]);
}

__global__ void k_tilerec_names(const int64_t* start, const int64_t* tile_id, const int32_t* slice,
                                const int64_t* name_off, int64_t n_slices, uint8_t* names) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slices) return;
  tile_key_put(start[s], tile_id[s], slice[s], names + name_off[s]);
}

// A thread per output dword (every record is 4 + 40*count bytes, so the buffer is 4-byte
// aligned throughout): lane-consecutive stores, no LDS.  The block finds the record of its
// first dword once (the search is block-uniform) and every thread walks on from there.
constexpr int kTileRecEmit = 256;
__global__ __launch_bounds__(kTileRecEmit) void k_tilerec_emit(const otr_tile_row* rows, const double* t0,
                                                               const double* t1, const int32_t* idx,
                                                               const int64_t* pos, const int64_t* rec_off,
                                                               int64_t n_slices, int64_t n_words, uint32_t* out) {
  const int64_t w0 = (int64_t)blockIdx.x * kTileRecEmit;
  const int64_t w = w0 + threadIdx.x;
  // the last record starting at or before byte 4 * w0
  int64_t lo = 0, hi = n_slices - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (rec_off[mid] <= 4 * w0) lo = mid; else hi = mid - 1;
  }
  if (w >= n_words) return;
  int64_t r = lo;
  while (r + 1 < n_slices && rec_off[r + 1] <= 4 * w) ++r;
  const int64_t k = w - rec_off[r] / 4;  // the dword within the record
  if (k == 0) {
    out[w] = tr_bswap32((uint32_t)(pos[r + 1] - pos[r]));
    return;
  }
  const int64_t seg = (k - 1) / 10;
  const int32_t field = (int32_t)((k - 1) % 10);
  const int64_t i = idx[pos[r] + seg];
  TileSegment s;
  s.id = rows[i].id;
  s.next_id = rows[i].next_id;
  s.t0 = t0[i];
  s.t1 = t1[i];
  s.length = rows[i].length;
  s.queue = rows[i].queue_length;
  out[w] = tile_rec_segment_word(s, field);
}

// ---- restore --------------------------------------------------------------------------------
enum { TRC_ROWS = 0, TRC_SLICES, TRC_UNREF_ROWS, TRC_UNREF_SLICES, TRC_NAMED, TRC_WORDS };
constexpr unsigned long long kTileRecNone = ~0ull;

__device__ inline void tilerec_verdict(unsigned long long* verdict, int64_t index, int reason) {
  atomicMin(verdict, ((unsigned long long)index << 8) | (unsigned long long)reason);
}

struct TileRecIn {
  int64_t n_slices, n_bytes, q;
  int32_t slice_size;
  const int64_t* start;
  const int64_t* tile_id;
  const int32_t* slice;
  const int64_t* rec_off;
  const uint8_t* bytes;
};

// Pass 1, a wave per record: the header and the key once (every lane computes the same), the
// lanes cover the segments.  Writes the record's count (0 where the layout or the count is
// refused), whether its key is valid, its sort keys, and the verdict.  No lane waits on another
// except in the closing reduction.
__global__ __launch_bounds__(256) void k_tilerec_validate(TileRecIn a, int32_t* count_out, int32_t* key_ok,
                                                          unsigned long long* file_key,
                                                          unsigned long long* slice_key, int32_t* idx,
                                                          unsigned long long* verdict) {
  const int64_t i = (int64_t)blockIdx.x * (256 / OTR_WAVE) + threadIdx.x / OTR_WAVE;
  if (i >= a.n_slices) return;  // wave-uniform
  const int64_t b = a.rec_off[i], e = a.rec_off[i + 1];
  const int64_t st = a.start[i], tid = a.tile_id[i];
  const int32_t sl = a.slice[i];
  int32_t count;
  const bool layout = tile_rec_layout_ok(a.bytes, a.n_bytes, b, e, &count);
  const bool kok = tile_rec_key_ok(st, tid, sl, a.q);
  int reason = !layout ? OTR_TILE_RESTORE_E_LAYOUT : !kok ? OTR_TILE_RESTORE_E_KEY
               : (count < 1 || count > a.slice_size) ? OTR_TILE_RESTORE_E_COUNT : 0;
  if (reason == 0) {
    const int64_t bucket = st / a.q;
    bool bad = false;
    for (int32_t k = lane_id(); k < count; k += OTR_WAVE)
      if (!tile_rec_segment_ok(tile_rec_segment_get(a.bytes + b, k), tid, bucket, a.q)) bad = true;
    if (__any(bad)) reason = OTR_TILE_RESTORE_E_SEGMENT;
  }
  if (lane_id() == 0) {
    count_out[i] = (layout && count >= 1 && count <= a.slice_size) ? count : 0;
    key_ok[i] = kok ? 1 : 0;
    file_key[i] = kok ? tile_rec_file(st / a.q, tid) : 0ull;
    slice_key[i] = (unsigned long long)(uint32_t)sl;
    idx[i] = (int32_t)i;
    if (reason) tilerec_verdict(verdict, i, reason);
  }
}

// the second key of the two-pass sort, in the order the first pass left
__global__ void k_tilerec_gather(const unsigned long long* file_key, const int32_t* order, int64_t n,
                                 unsigned long long* out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) out[j] = file_key[order[j]];
}

// sorted by (file, slice), stable: among equal valid keys all but the first are duplicates
__global__ void k_tilerec_duplicates(const unsigned long long* file_sorted, const int32_t* order,
                                     const unsigned long long* slice_key, const int32_t* key_ok, int64_t n,
                                     unsigned long long* verdict) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < 1 || j >= n) return;
  const int32_t i = order[j], p = order[j - 1];
  if (key_ok[i] && key_ok[p] && file_sorted[j] == file_sorted[j - 1] && slice_key[i] == slice_key[p])
    tilerec_verdict(verdict, i, OTR_TILE_RESTORE_E_DUPLICATE);
}

// the map's entries: their sort key, and the entries refused on their own
__global__ void k_tilerec_map_keys(const uint8_t* map_bytes, int64_t n_tiles, int64_t q, unsigned long long* file_key,
                                   int32_t* idx, int32_t* value, int32_t* ok, unsigned long long* map_verdict,
                                   unsigned long long* counters) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tiles) return;
  int64_t st, tid;
  int32_t v;
  tile_map_get(map_bytes + kTileMapEntry * t, &st, &tid, &v);
  const bool kok = tile_rec_key_ok(st, tid, 0, q);
  file_key[t] = kok ? tile_rec_file(st / q, tid) : 0ull;
  idx[t] = (int32_t)t;
  value[t] = v;
  ok[t] = kok ? 1 : 0;
  if (!kok || v < 0) atomicMin(map_verdict, (unsigned long long)t);
  else atomicAdd(&counters[TRC_NAMED], (unsigned long long)v + 1ull);
}

__global__ void k_tilerec_map_duplicates(const unsigned long long* file_sorted, const int32_t* order,
                                         const int32_t* ok, int64_t n_tiles, unsigned long long* map_verdict) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < 1 || j >= n_tiles) return;
  const int32_t t = order[j], p = order[j - 1];
  if (ok[t] && ok[p] && file_sorted[j] == file_sorted[j - 1]) atomicMin(map_verdict, (unsigned long long)t);
}

// Sorted record j's rows to restore: its count where the map names it (no map: always), else 0
// and counted as unreferenced.  Run only on an input without a refused record or map entry, so
// every key is valid and the map's sorted keys are distinct.
__global__ void k_tilerec_join(const unsigned long long* file_sorted, const int32_t* order, const unsigned long long* slice_key,
                               const int32_t* count, int64_t n, const unsigned long long* map_sorted,
                               const int32_t* map_order, const int32_t* map_value, int64_t n_tiles, int64_t* ref_cnt,
                               unsigned long long* counters) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int32_t i = order[j];
  bool ref = true;
  if (n_tiles >= 0) {
    const unsigned long long f = file_sorted[j];
    int64_t lo = 0, hi = n_tiles;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (map_sorted[mid] < f) lo = mid + 1; else hi = mid;
    }
    ref = lo < n_tiles && map_sorted[lo] == f && (int64_t)slice_key[i] <= (int64_t)map_value[map_order[lo]];
  }
  const unsigned long long c = (unsigned long long)count[i];
  ref_cnt[j] = ref ? (int64_t)c : 0;
  atomicAdd(&counters[ref ? TRC_ROWS : TRC_UNREF_ROWS], c);
  atomicAdd(&counters[ref ? TRC_SLICES : TRC_UNREF_SLICES], 1ull);
}

// Pass 2, a wave per sorted record: every referenced segment's row (and times) whole from one
// lane, at the end of the held rows.
__global__ __launch_bounds__(256) void k_tilerec_write(TileRecIn a, const int32_t* order, const int64_t* ref_cnt,
                                                       const int64_t* row_off, otr_tile_row* rows, double* t0,
                                                       double* t1) {
  const int64_t j = (int64_t)blockIdx.x * (256 / OTR_WAVE) + threadIdx.x / OTR_WAVE;
  if (j >= a.n_slices) return;  // wave-uniform
  const int64_t cnt = ref_cnt[j];
  if (cnt == 0) return;
  const int32_t i = order[j];
  const uint8_t* rec = a.bytes + a.rec_off[i];
  const int64_t bucket = a.start[i] / a.q, base = row_off[j];
  for (int64_t k = lane_id(); k < cnt; k += OTR_WAVE) {
    const TileSegment s = tile_rec_segment_get(rec, (int32_t)k);
    BucketSpan sp;
    stream_span(s.t0, s.t1, s.length, s.queue, a.q, &sp);
    rows[base + k] = tile_row_of(bucket, s.id, s.next_id, sp, s.length, s.queue, tile_speed_bin(s.length, s.t0, s.t1));
    if (t0) {
      t0[base + k] = s.t0;
      t1[base + k] = s.t1;
    }
  }
}

// ---- restore in the store's own layout --------------------------------------------------------
// row i must be the row an add derives from its own (bucket, id, next_id, t0, t1, length, queue)
__global__ void k_tilerec_check_rows(const otr_tile_row* rows, const double* t0, const double* t1, int64_t n,
                                     int64_t q, unsigned long long* verdict) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const otr_tile_row r = rows[i];
  const double a = t0[i], b = t1[i];
  BucketSpan sp;
  bool ok = b < 4611686018427387904.0 && stream_span(a, b, r.length, r.queue_length, q, &sp);  // 2^62, as E_SEGMENT
  if (ok) {
    const int64_t bucket = (int64_t)(r.file >> 25);
    const otr_tile_row w = tile_row_of(bucket, r.id, r.next_id, sp, r.length, r.queue_length,
                                       tile_speed_bin(r.length, a, b));
    ok = bucket >= sp.min_bucket && bucket <= sp.max_bucket && w.file == r.file && w.id == r.id &&
         w.next_id == r.next_id && w.start == r.start && w.end == r.end && w.duration == r.duration &&
         w.length == r.length && w.queue_length == r.queue_length && w.speed_bin == r.speed_bin;
  }
  if (!ok) atomicMin(verdict, (unsigned long long)i);
}

}  // namespace otr
#endif  // __HIPCC__
