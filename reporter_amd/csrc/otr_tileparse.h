// otr_tileparse.h — K21: tile file texts read back into otr_tile_row records (include/otr.h
// otr_tiles_parse), the inverse of K19 (otr_tiletext.h).  The per-line and
// per-name rules and the line table's arithmetic are __host__ __device__ so that
// tools/tileparsecheck.cpp runs the very same functions on the CPU (under sanitizers) that the
// kernels below run on the device; they use no libc.
//
// THE RULE: a line becomes a row iff K19's tile_text_row_emit of that row, under the same rules
// and tag, reproduces the line's bytes.  The emitter writes every number as its canonical decimal
// (tt_put_*), so a numeric field is accepted iff it is digits (behind one '-' where the member is
// signed), its value fits the member and it is exactly as long as K19's length of that value
// (tt_len_*): a digit string of the canonical length has no leading zero.  "-0" has the length of
// no value and is refused by name.
#pragma once
#include <stdint.h>

#include "otr_tiletext.h"

#if defined(__HIPCC__)
#include "otr_ingest.h"  // k_nl_count / k_nl_write: the newline positions
#endif

namespace otr {

constexpr int kTileParseFields = 10;

// ---- decimals ---------------------------------------------------------------------------
// "-"? (where sign) then digits, s[b, e): the magnitude, or false (empty, another byte, or more
// than 2^64 - 1).  Leading zeros pass here; the length comparison of the callers refuses them.
OTR_TT_HD bool tp_read(const uint8_t* s, int64_t b, int64_t e, bool sign, uint64_t& mag, bool& neg) {
  mag = 0;
  neg = false;
  if (sign && b < e && s[b] == '-') {
    neg = true;
    ++b;
  }
  if (b >= e) return false;
  for (; b < e; ++b) {
    const uint8_t c = s[b];
    if (c < '0' || c > '9') return false;
    const uint64_t d = (uint64_t)(c - '0');
    if (mag > (~0ull - d) / 10ull) return false;
    mag = mag * 10ull + d;
  }
  return true;
}
OTR_TT_HD bool tp_u64(const uint8_t* s, int64_t b, int64_t e, uint64_t& out) {
  uint64_t mag;
  bool neg;
  if (!tp_read(s, b, e, false, mag, neg) || e - b != (int64_t)tt_len_u64(mag)) return false;
  out = mag;
  return true;
}
OTR_TT_HD bool tp_i64(const uint8_t* s, int64_t b, int64_t e, int64_t& out) {
  uint64_t mag;
  bool neg;
  if (!tp_read(s, b, e, true, mag, neg) || (neg && mag == 0)) return false;
  if (mag > (neg ? 1ull << 63 : (1ull << 63) - 1ull)) return false;
  const int64_t v = neg ? (int64_t)(0ull - mag) : (int64_t)mag;  // 2^63 negated: INT64_MIN
  if (e - b != (int64_t)tt_len_i64(v)) return false;
  out = v;
  return true;
}
OTR_TT_HD bool tp_i32(const uint8_t* s, int64_t b, int64_t e, int32_t& out) {
  int64_t v;
  if (!tp_i64(s, b, e, v) || v < -2147483647ll - 1ll || v > 2147483647ll) return false;
  out = (int32_t)v;
  return true;
}

// ---- a line -----------------------------------------------------------------------------
OTR_TT_HD bool tile_parse_is_header(const uint8_t* s, int64_t b, int64_t e) {
  if (e - b != kTileTextHeader) return false;
  const char* h = tile_text_header();
  for (int k = 0; k < kTileTextHeader; ++k)
    if (s[b + k] != (uint8_t)h[k]) return false;
  return true;
}

// The status (OTR_TILE_LINE_*) of the piece s[b, e) of a file whose name was accepted as `file`.
// first: it is its file's p0; terminated: a '\n' follows it.  tag: tile_text_tag_put's of the call
// (",source,MODE", "\n" behind it under the simple rules).  *row is written only for
// OTR_TILE_LINE_ROW.
OTR_TT_HD int32_t tile_parse_line(const uint8_t* s, int64_t b, int64_t e, bool first, bool terminated, int32_t rules,
                                  const uint8_t* tag, int32_t tag_len, uint64_t file, otr_tile_row* row) {
  const bool stream = rules == OTR_TILE_RULES_STREAM;
  const bool is_h = tile_parse_is_header(s, b, e);
  if (first && is_h) return OTR_TILE_LINE_HEADER;
  // field k is s[fb[k], fe[k]); the tenth runs to the line's end
  int64_t fb[kTileParseFields], fe[kTileParseFields];
  int32_t nf = 0;
  int64_t st = b;
  for (int64_t p = b; p <= e; ++p) {
    if (p == e || s[p] == ',') {
      if (nf < kTileParseFields) {
        fb[nf] = st;
        fe[nf] = p;
      }
      ++nf;
      st = p + 1;
    }
  }
  if (nf < 2) return OTR_TILE_LINE_E_FIELDS;
  if (!stream && !terminated) return OTR_TILE_LINE_U_END;
  if (is_h || (stream && first)) return OTR_TILE_LINE_U_HEADER;
  if (nf != kTileParseFields) return OTR_TILE_LINE_U_FIELDS;
  otr_tile_row r;
  r.file = file;
  r.speed_bin = -1;
  const bool no_next = fb[1] == fe[1];
  r.next_id = OTR_INVALID_SEGMENT_ID;
  if (!tp_u64(s, fb[0], fe[0], r.id) || (!no_next && !tp_u64(s, fb[1], fe[1], r.next_id)) ||
      !tp_i32(s, fb[2], fe[2], r.duration) || !tp_i32(s, fb[4], fe[4], r.length) ||
      !tp_i32(s, fb[5], fe[5], r.queue_length) || !tp_i64(s, fb[6], fe[6], r.start) ||
      !tp_i64(s, fb[7], fe[7], r.end))
    return OTR_TILE_LINE_U_NUMBER;
  // what K19 would not have written: no next id under the simple rules, the invalid one spelled
  // under the stream rules
  if (no_next ? !stream : (stream && r.next_id == OTR_INVALID_SEGMENT_ID)) return OTR_TILE_LINE_U_NEXT;
  if (fe[3] - fb[3] != 1 || s[fb[3]] != '1') return OTR_TILE_LINE_U_COUNT;
  // "source,MODE": the tag without its comma and without the simple rules' newline
  const int32_t want = tag_len - 1 - (stream ? 0 : 1);
  if (e - fb[8] != (int64_t)want) return OTR_TILE_LINE_U_TAG;
  for (int32_t k = 0; k < want; ++k)
    if (s[fb[8] + k] != tag[1 + k]) return OTR_TILE_LINE_U_TAG;
  *row = r;
  return OTR_TILE_LINE_ROW;
}

// ---- a name -----------------------------------------------------------------------------
// "{a}_{b}/{level}/{tile}" = s[b, e) at the quantisation q >= 1: the file value, or false.  With
// a % q == 0, b == a + q - 1 (in uint64, no wrap), a / q < 2^39, level <= 7 and tile < 2^22 the name
// is tile_text_name_put's of that value, digit for digit.
OTR_TT_HD bool tile_parse_name(const uint8_t* s, int64_t b, int64_t e, int64_t q, uint64_t& file) {
  int64_t cut[3];  // the '_' and the two '/'
  const uint8_t sep[3] = {'_', '/', '/'};
  int n = 0;
  for (int64_t p = b; p < e; ++p) {
    const uint8_t c = s[p];
    if (c >= '0' && c <= '9') continue;
    if (n == 3 || c != sep[n]) return false;
    cut[n++] = p;
  }
  if (n != 3) return false;
  uint64_t lo, hi, level, tile;
  if (!tp_u64(s, b, cut[0], lo) || !tp_u64(s, cut[0] + 1, cut[1], hi) || !tp_u64(s, cut[1] + 1, cut[2], level) ||
      !tp_u64(s, cut[2] + 1, e, tile))
    return false;
  const uint64_t uq = (uint64_t)q;
  if (lo % uq != 0 || lo > ~0ull - (uq - 1ull) || hi != lo + (uq - 1ull)) return false;
  const uint64_t bucket = lo / uq;
  if (bucket >= (1ull << 39) || level > 7ull || tile >= (1ull << 22)) return false;
  file = (bucket << 25) | (level << 22) | tile;
  return true;
}

// ---- the line table ---------------------------------------------------------------------
// first index of the ascending a[0, n) whose value is >= x (n: none)
OTR_TT_HD int64_t tp_lower_bound(const int64_t* a, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (a[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The lines of the file text[t0, t1) that holds the newlines nl[lo, hi) (lo, hi: tp_lower_bound
// of t0 and t1 in the newline positions): hi - lo + 1 pieces; the last one is no line under the
// simple rules when it is empty, and an empty text has no line at all.
OTR_TT_HD int64_t tile_parse_file_lines(const int64_t* nl, int64_t lo, int64_t hi, int64_t t0, int64_t t1,
                                        int32_t rules) {
  if (t1 <= t0) return 0;
  if (rules == OTR_TILE_RULES_STREAM) return hi - lo + 1;
  return hi - lo + ((hi > lo && nl[hi - 1] == t1 - 1) ? 0 : 1);
}

// the file of line i: the first f of [0, n_files) with file_line_off[f + 1] > i
// (0 <= i < file_line_off[n_files]; files without lines are stepped over)
OTR_TT_HD int64_t tile_parse_file_of(const int64_t* file_line_off, int64_t n_files, int64_t i) {
  int64_t lo = 0, hi = n_files - 1;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (file_line_off[mid + 1] <= i) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// piece j of the file text[t0, t1) whose newlines are nl[lo, hi): its bytes [*b, *e) and whether
// a '\n' follows (0 <= j <= hi - lo)
OTR_TT_HD bool tile_parse_piece(const int64_t* nl, int64_t lo, int64_t hi, int64_t t0, int64_t t1, int64_t j,
                                int64_t* b, int64_t* e) {
  *b = j == 0 ? t0 : nl[lo + j - 1] + 1;
  const bool terminated = j < hi - lo;
  *e = terminated ? nl[lo + j] : t1;
  return terminated;
}

#if defined(__HIPCC__)
// ---- the kernels --------------------------------------------------------------------------
// Passes are ordered by kernel boundaries only.  No result goes through an atomic but the
// first-bad word, as in K11.

struct TileParseIn {
  const uint8_t* text;      // the padded copy
  const int64_t* text_off;  // n_files + 1
  const uint8_t* names;
  const int64_t* name_off;  // n_files + 1
  int64_t n_files;
  const int64_t* nl;  // positions of '\n' in text, n_nl of them
  int64_t n_nl;
  int32_t rules;
  int64_t quantisation;
};

// one thread per file f <= n_files: nl_lo[f], the number of newlines before the file's text
// (nl_lo[n_files]: all of them), and for f < n_files the file's line count
__global__ void k_tile_parse_files(TileParseIn in, int64_t* nl_lo, int64_t* line_cnt) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f > in.n_files) return;
  const int64_t t0 = in.text_off[f];
  const int64_t lo = tp_lower_bound(in.nl, in.n_nl, t0);
  nl_lo[f] = lo;
  if (f == in.n_files) return;
  const int64_t t1 = in.text_off[f + 1];
  const int64_t hi = tp_lower_bound(in.nl, in.n_nl, t1);
  line_cnt[f] = tile_parse_file_lines(in.nl, lo, hi, t0, t1, in.rules);
}

// one thread per file f <= n_files: file_line_off[f] from the inclusive scan of the line counts,
// and for f < n_files the name's verdict
__global__ void k_tile_parse_names(TileParseIn in, const int64_t* line_incl, int64_t* file_line_off,
                                   unsigned long long* file, uint8_t* file_status) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f > in.n_files) return;
  file_line_off[f] = f > 0 ? line_incl[f - 1] : 0;
  if (f == in.n_files) return;
  uint64_t v = OTR_NO_ID;
  const bool ok = tile_parse_name(in.names, in.name_off[f], in.name_off[f + 1], in.quantisation, v);
  file[f] = ok ? v : OTR_NO_ID;
  file_status[f] = ok ? 0 : 1;
}

// One thread per line, as k_ingest_parse: the file by a binary search in file_line_off, the
// piece from the newline list, then the bytes one at a time (they come from L2: neighbouring
// threads read neighbouring lines).  Writes the line's status and, for a row, its slot.
__global__ void k_tile_parse(TileParseIn in, const int64_t* nl_lo, const int64_t* file_line_off,
                             const unsigned long long* file, const uint8_t* file_status, const uint8_t* tag,
                             int32_t tag_len, int64_t n_lines, uint8_t* line_status, otr_tile_row* slot,
                             unsigned long long* bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_lines) return;
  const int64_t f = tile_parse_file_of(file_line_off, in.n_files, i);
  int32_t st = OTR_TILE_LINE_U_NAME;
  if (!file_status[f]) {
    const int64_t j = i - file_line_off[f];
    int64_t b, e;
    const bool terminated = tile_parse_piece(in.nl, nl_lo[f], nl_lo[f + 1], in.text_off[f], in.text_off[f + 1], j, &b, &e);
    otr_tile_row r;
    st = tile_parse_line(in.text, b, e, j == 0, terminated, in.rules, tag, tag_len, file[f], &r);
    if (st == OTR_TILE_LINE_ROW) slot[i] = r;
  }
  line_status[i] = (uint8_t)st;
  if (st >= OTR_TILE_LINE_E_FIELDS) atomicMin(bad, ((unsigned long long)i << 8) | (unsigned)st);
}

// the three columns scanned together over the line statuses (otr_devscan.h tuple_sums): rows,
// headers, refused lines
struct TileParseColumns {
  const uint8_t* status;
  __host__ __device__ int64_t operator()(int q, int64_t i) const {
    const uint8_t s = status[i];
    return q == 0 ? s == OTR_TILE_LINE_ROW : (q == 1 ? s == OTR_TILE_LINE_HEADER : s >= OTR_TILE_LINE_E_FIELDS);
  }
};

// the rows densely in line order (row_incl: the inclusive count of rows along the lines), and
// per file f <= n_files its first row (n_lines may be 0: then row_incl is not read)
__global__ void k_tile_parse_compact(const uint8_t* line_status, const otr_tile_row* slot, const int64_t* row_incl,
                                     int64_t n_lines, const int64_t* file_line_off, int64_t n_files,
                                     otr_tile_row* rows, int64_t* row_off) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_lines && line_status[i] == OTR_TILE_LINE_ROW) rows[row_incl[i] - 1] = slot[i];
  if (i <= n_files) {
    const int64_t l = file_line_off[i];
    row_off[i] = l > 0 ? row_incl[l - 1] : 0;
  }
}
#endif  // __HIPCC__

}  // namespace otr
