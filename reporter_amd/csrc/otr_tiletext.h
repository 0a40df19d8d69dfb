// otr_tiletext.h — K19: the texts and names of tile files written from otr_tile_row records
// (include/otr.h otr_tiles_text / otr_tile_store_flush_text).  The
// per-row and per-file rules are __host__ __device__ so that tools/tiletextcheck.cpp runs the
// very same functions on the CPU (under sanitizers) that the kernels below run on the device;
// they use no libc and no std::string.  A row's bytes are those otr_tiles_format (otr_api.cpp)
// appends for it: Segment.appendToStringBuffer (Segment.java:59-74) under
// OTR_TILE_RULES_STREAM, simple_reporter.py:188-196 under OTR_TILE_RULES_SIMPLE.
#pragma once
#include <stdint.h>

#include "../../include/otr.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OTR_TT_HD __host__ __device__ inline
#else
#define OTR_TT_HD inline
#endif

namespace otr {

constexpr int kTileTextTagPart = 255;                    // longest source, longest mode
constexpr int kTileTextTagMax = 2 * kTileTextTagPart + 3;  // ",source,MODE" and simple's "\n"
constexpr int kTileTextHeader = 117;                    // bytes of Segment.columnLayout()

// Segment.columnLayout() (Segment.java:55-57) = simple_reporter.py:252's column line
OTR_TT_HD const char* tile_text_header() {
  return "segment_id,next_segment_id,duration,count,length,queue_length,minimum_timestamp,maximum_timestamp,source,"
         "vehicle_type";
}

// ---- decimals ---------------------------------------------------------------------------
OTR_TT_HD int tt_len_u64(uint64_t v) {
  int n = 1;
  while (v >= 10ull) {
    v /= 10ull;
    ++n;
  }
  return n;
}
OTR_TT_HD uint64_t tt_mag_i64(int64_t v) { return v < 0 ? 0ull - (uint64_t)v : (uint64_t)v; }  // INT64_MIN: 2^63
OTR_TT_HD int tt_len_i64(int64_t v) { return tt_len_u64(tt_mag_i64(v)) + (v < 0 ? 1 : 0); }
OTR_TT_HD int tt_len_i32(int32_t v) { return tt_len_i64((int64_t)v); }

// A sink takes byte c at position pos of the text being written: set(pos, c).  The plain one
// writes through a pointer; the emit kernel's writes into its LDS window and drops the rest.
struct TtPtrSink {
  uint8_t* p;
  OTR_TT_HD void set(int64_t pos, uint8_t c) const { p[pos] = c; }
};

// the digits of v at pos, most significant first (written from the last digit back);
// returns the position behind them
template <class Sink>
OTR_TT_HD int64_t tt_put_u64(const Sink& s, int64_t pos, uint64_t v) {
  const int n = tt_len_u64(v);
  for (int k = n - 1; k >= 0; --k) {
    const uint64_t q = v / 10ull;
    s.set(pos + k, (uint8_t)('0' + (int)(v - q * 10ull)));
    v = q;
  }
  return pos + n;
}
template <class Sink>
OTR_TT_HD int64_t tt_put_i64(const Sink& s, int64_t pos, int64_t v) {
  if (v < 0) s.set(pos++, (uint8_t)'-');
  return tt_put_u64(s, pos, tt_mag_i64(v));
}
template <class Sink>
OTR_TT_HD int64_t tt_put_i32(const Sink& s, int64_t pos, int32_t v) {
  return tt_put_i64(s, pos, (int64_t)v);
}

// ---- a row ------------------------------------------------------------------------------
OTR_TT_HD bool tile_text_rules_ok(int32_t rules) {
  return rules == OTR_TILE_RULES_SIMPLE || rules == OTR_TILE_RULES_STREAM;
}
// the next id is left out only by the stream rules, for OTR_INVALID_SEGMENT_ID
OTR_TT_HD bool tile_text_has_next(const otr_tile_row& r, int32_t rules) {
  return rules != OTR_TILE_RULES_STREAM || r.next_id != OTR_INVALID_SEGMENT_ID;
}

// tag: the prepared ",source,MODE" (+ "\n" under the simple rules), tag_len bytes
OTR_TT_HD int32_t tile_text_row_len(const otr_tile_row& r, int32_t rules, int32_t tag_len) {
  return (rules == OTR_TILE_RULES_STREAM ? 1 : 0) + tt_len_u64(r.id) + 1 +
         (tile_text_has_next(r, rules) ? tt_len_u64(r.next_id) : 0) + 1 + tt_len_i32(r.duration) + 3 +
         tt_len_i32(r.length) + 1 + tt_len_i32(r.queue_length) + 1 + tt_len_i64(r.start) + 1 + tt_len_i64(r.end) +
         tag_len;
}

// the row's bytes from position pos on; returns the position behind them
template <class Sink>
OTR_TT_HD int64_t tile_text_row_emit(const otr_tile_row& r, int32_t rules, const uint8_t* tag, int32_t tag_len,
                                     const Sink& s, int64_t pos) {
  if (rules == OTR_TILE_RULES_STREAM) s.set(pos++, (uint8_t)'\n');
  pos = tt_put_u64(s, pos, r.id);
  s.set(pos++, (uint8_t)',');
  if (tile_text_has_next(r, rules)) pos = tt_put_u64(s, pos, r.next_id);
  s.set(pos++, (uint8_t)',');
  pos = tt_put_i32(s, pos, r.duration);
  s.set(pos++, (uint8_t)',');
  s.set(pos++, (uint8_t)'1');
  s.set(pos++, (uint8_t)',');
  pos = tt_put_i32(s, pos, r.length);
  s.set(pos++, (uint8_t)',');
  pos = tt_put_i32(s, pos, r.queue_length);
  s.set(pos++, (uint8_t)',');
  pos = tt_put_i64(s, pos, r.start);
  s.set(pos++, (uint8_t)',');
  pos = tt_put_i64(s, pos, r.end);
  for (int32_t k = 0; k < tag_len; ++k) s.set(pos++, tag[k]);
  return pos;
}

// the row's tile_text_row_len bytes at out; returns their number
OTR_TT_HD int32_t tile_text_row_put(const otr_tile_row& r, int32_t rules, const uint8_t* tag, int32_t tag_len,
                                    uint8_t* out) {
  return (int32_t)tile_text_row_emit(r, rules, tag, tag_len, TtPtrSink{out}, 0);
}

// ---- a file -----------------------------------------------------------------------------
// what precedes a file's first row: the column line, closed by "\n" under the simple rules
// (under the stream rules every row opens with its own)
OTR_TT_HD int32_t tile_text_header_len(int32_t rules) {
  return kTileTextHeader + (rules == OTR_TILE_RULES_STREAM ? 0 : 1);
}
template <class Sink>
OTR_TT_HD int64_t tile_text_header_emit(int32_t rules, const Sink& s, int64_t pos) {
  const char* h = tile_text_header();
  for (int k = 0; k < kTileTextHeader; ++k) s.set(pos++, (uint8_t)h[k]);
  if (rules != OTR_TILE_RULES_STREAM) s.set(pos++, (uint8_t)'\n');
  return pos;
}

// "{b*q}_{(b+1)*q-1}/{level}/{tile}" (simple_reporter.file_key): both products in uint64
// modulo 2^64, printed unsigned
struct TtName {
  uint64_t lo, hi;
  int32_t level, tile;
};
OTR_TT_HD TtName tile_text_name_parts(uint64_t file, int64_t quantisation) {
  const uint64_t b = file >> 25, q = (uint64_t)quantisation;
  TtName p;
  p.lo = b * q;
  p.hi = (b + 1ull) * q - 1ull;
  p.level = (int32_t)((file >> 22) & 7ull);
  p.tile = (int32_t)(file & 0x3fffffull);
  return p;
}
OTR_TT_HD int32_t tile_text_name_len(uint64_t file, int64_t quantisation) {
  const TtName p = tile_text_name_parts(file, quantisation);
  return tt_len_u64(p.lo) + 1 + tt_len_u64(p.hi) + 1 + 1 + 1 + tt_len_u64((uint64_t)p.tile);
}
OTR_TT_HD int32_t tile_text_name_put(uint64_t file, int64_t quantisation, uint8_t* out) {
  const TtName p = tile_text_name_parts(file, quantisation);
  const TtPtrSink s{out};
  int64_t pos = tt_put_u64(s, 0, p.lo);
  s.set(pos++, (uint8_t)'_');
  pos = tt_put_u64(s, pos, p.hi);
  s.set(pos++, (uint8_t)'/');
  s.set(pos++, (uint8_t)('0' + p.level));
  s.set(pos++, (uint8_t)'/');
  pos = tt_put_u64(s, pos, (uint64_t)p.tile);
  return (int32_t)pos;
}

// the tag of a call: ",source,MODE" with MODE's ASCII a-z upper-cased, "\n" appended under
// the simple rules.  source / mode: src_len / mode_len bytes (each <= kTileTextTagPart); out
// holds kTileTextTagMax bytes.  Returns the tag's length.
OTR_TT_HD int32_t tile_text_tag_put(const uint8_t* source, int32_t src_len, const uint8_t* mode, int32_t mode_len,
                                    int32_t rules, uint8_t* out) {
  int32_t n = 0;
  out[n++] = (uint8_t)',';
  for (int32_t k = 0; k < src_len; ++k) out[n++] = source[k];
  out[n++] = (uint8_t)',';
  for (int32_t k = 0; k < mode_len; ++k) {
    const uint8_t c = mode[k];
    out[n++] = (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c;
  }
  if (rules != OTR_TILE_RULES_STREAM) out[n++] = (uint8_t)'\n';
  return n;
}

#if defined(__HIPCC__)
// ---- the kernels --------------------------------------------------------------------------
// Input: n rows in HBM in which the rows of one file are adjacent, so a row opens a file where
// its `file` differs from the row before.  Passes are ordered by kernel boundaries only.

__device__ inline bool tile_text_file_head(const otr_tile_row* rows, int64_t i) {
  return i == 0 || rows[i].file != rows[i - 1].file;
}

// row i's bytes, the header's included where it opens a file
__global__ void k_tile_text_len(const otr_tile_row* rows, int64_t n, int32_t rules, int32_t tag_len, int64_t* len) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  len[i] = (int64_t)tile_text_row_len(rows[i], rules, tag_len) +
           (tile_text_file_head(rows, i) ? (int64_t)tile_text_header_len(rules) : 0);
}

// the file table of rows without one: file f starts at start[f]
__global__ void k_tile_text_table(const otr_tile_row* rows, const int64_t* start, int64_t n_files, int64_t n,
                                  unsigned long long* file, int64_t* row_off) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f > n_files) return;
  if (f == n_files) {
    row_off[f] = n;
    return;
  }
  file[f] = rows[start[f]].file;
  row_off[f] = start[f];
}

// per file f <= n_files: where its text starts (off: the rows' exclusive byte offsets,
// n + 1 of them; row_off[n_files] == n), and for f < n_files its name's length
__global__ void k_tile_text_files(const unsigned long long* file, const int64_t* row_off, const int64_t* off,
                                  int64_t n_files, int64_t quantisation, int64_t* text_off, int64_t* name_len) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f > n_files) return;
  text_off[f] = off[row_off[f]];
  if (f < n_files) name_len[f] = (int64_t)tile_text_name_len(file[f], quantisation);
}

__global__ void k_tile_text_names(const unsigned long long* file, const int64_t* name_off, int64_t n_files,
                                  int64_t quantisation, uint8_t* names) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_files) return;
  tile_text_name_put(file[f], quantisation, names + name_off[f]);
}

// The emit kernel's staging window in LDS: 96 bytes a row, above the common 75 to 85 of a
// row plus the share of a header, so that a block usually needs one window, and small enough
// for 6 blocks on a CU's 160 KB.
constexpr int kTtRows = 256;             // rows (threads) per block
constexpr int kTtStage = kTtRows * 96;   // bytes, a multiple of 16
// the kernel's dynamic LDS: the window, then the tag (it has no static LDS, so the dynamic
// region starts at the 16-byte aligned base and the window's uint4 reads are aligned)
constexpr int kTtLds = kTtStage + ((kTileTextTagMax + 15) & ~15);

// bytes at positions of the block's span; only those inside the current window land in LDS
struct TtWindowSink {
  uint8_t* lds;
  int32_t w0;  // the window's first position
  __device__ void set(int64_t pos, uint8_t c) const {
    const uint32_t d = (uint32_t)((int32_t)pos - w0);
    if (d < (uint32_t)kTtStage) lds[d] = c;
  }
};

// A block owns kTtRows consecutive rows; their texts and the headers of the files that begin
// among them are the contiguous span [off[r0], off[r1]) of the output.  Positions count from
// the 16-byte boundary at or below the span's start, so that position p and output byte
// base + p agree modulo 16: the block formats one window of kTtStage positions at a time
// into LDS (a row that crosses a window border is formatted once for each side) and copies
// the window's part of the span out, whole 16-byte groups as lane-consecutive uint4 stores
// and the span's unaligned first and last group as bytes.  The neighbouring blocks write the
// other bytes of those two groups, also as bytes, so no byte is written twice.
__global__ __launch_bounds__(kTtRows) void k_tile_text_emit(const otr_tile_row* rows, int64_t n, int32_t rules,
                                                            const uint8_t* tag, int32_t tag_len, const int64_t* off,
                                                            uint8_t* text) {
  extern __shared__ __attribute__((aligned(16))) uint8_t tt_lds[];
  uint8_t* const lds = tt_lds;
  uint8_t* const s_tag = tt_lds + kTtStage;
  const int64_t r0 = (int64_t)blockIdx.x * kTtRows;
  const int64_t r1 = r0 + kTtRows < n ? r0 + kTtRows : n;
  const int64_t i = r0 + threadIdx.x;
  const int64_t g0 = off[r0], g1 = off[r1];
  const int64_t base = g0 & ~(int64_t)15;            // output offset of position 0
  const int32_t p0 = (int32_t)(g0 - base);           // the span in positions: [p0, p1)
  const int32_t p1 = (int32_t)(g1 - base);
  for (int k = threadIdx.x; k < tag_len; k += kTtRows) s_tag[k] = tag[k];
  otr_tile_row r{};
  int32_t a = 0, b = 0;  // the thread's own positions [a, b), header first
  bool head = false;
  if (i < r1) {
    r = rows[i];
    head = tile_text_file_head(rows, i);
    a = (int32_t)(off[i] - base);
    b = (int32_t)(off[i + 1] - base);
  }
  for (int32_t w0 = 0; w0 < p1; w0 += kTtStage) {  // block-uniform
    __syncthreads();  // the tag is in place; the previous window has been copied out
    if (a < w0 + kTtStage && b > w0) {
      const TtWindowSink s{lds, w0};
      int64_t pos = a;
      if (head) pos = tile_text_header_emit(rules, s, pos);
      tile_text_row_emit(r, rules, s_tag, tag_len, s, pos);
    }
    __syncthreads();
    const int32_t lo = p0 > w0 ? p0 : w0;                                // the span's part of the window
    const int32_t hi = p1 < w0 + kTtStage ? p1 : w0 + kTtStage;
    const int32_t lo16 = (lo + 15) & ~15, hi16 = hi & ~15;               // its whole groups
    if (lo16 <= hi16) {
      for (int32_t p = lo16 + (int32_t)threadIdx.x * 16; p < hi16; p += kTtRows * 16)
        *(uint4*)(text + base + p) = *(const uint4*)(lds + (p - w0));
      for (int32_t p = lo + (int32_t)threadIdx.x; p < lo16; p += kTtRows) text[base + p] = lds[p - w0];
      for (int32_t p = hi16 + (int32_t)threadIdx.x; p < hi; p += kTtRows) text[base + p] = lds[p - w0];
    } else {  // the part lies inside one group
      for (int32_t p = lo + (int32_t)threadIdx.x; p < hi; p += kTtRows) text[base + p] = lds[p - w0];
    }
  }
}
#endif  // __HIPCC__

}  // namespace otr
