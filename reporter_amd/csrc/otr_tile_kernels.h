// otr_tile_kernels.h — the kernels of the tile sort and privacy cull (K10) and the string-order
// keys the keyed histogram shares with them.  Included by otr_tiles.hip alone: its __global__
// functions are not templates, so they have one home in the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/otr.h"

namespace otr {

// Line order of simple_reporter.py:218 (segments.sort() over whole text lines).  Every
// field before the constant tail is a non-negative decimal integer followed by ',',
// and ',' sorts below every digit, so the string order is the field-by-field
// lexicographic order of the digit strings (a proper prefix sorts first).
__host__ __device__ inline int dec_digits(unsigned long long v) {
  int n = 1;
  while (v >= 10ull) {
    v /= 10ull;
    ++n;
  }
  return n;
}
__host__ __device__ inline int dec_cmp(unsigned long long a, unsigned long long b) {
  if (a == b) return 0;
  const int na = dec_digits(a), nb = dec_digits(b);
  unsigned long long pa = a, pb = b;
  for (int k = nb; k < na; ++k) pa /= 10ull;  // leading min(na, nb) digits
  for (int k = na; k < nb; ++k) pb /= 10ull;
  if (pa != pb) return pa < pb ? -1 : 1;
  return na < nb ? -1 : 1;
}
struct TileLineLess {
  __host__ __device__ bool operator()(const otr_tile_row& x, const otr_tile_row& y) const {
    if (x.file != y.file) return x.file < y.file;  // files are independent: any fixed order
    int c = dec_cmp(x.id, y.id);
    if (!c) c = dec_cmp(x.next_id, y.next_id);
    if (!c) c = dec_cmp((unsigned long long)x.duration, (unsigned long long)y.duration);
    if (!c) c = dec_cmp((unsigned long long)x.length, (unsigned long long)y.length);
    if (!c) c = dec_cmp((unsigned long long)x.queue_length, (unsigned long long)y.queue_length);
    if (!c) c = dec_cmp((unsigned long long)x.start, (unsigned long long)y.start);
    if (!c) c = dec_cmp((unsigned long long)x.end, (unsigned long long)y.end);
    return c < 0;
  }
};

// Radix keys for the line order: a non-negative integer's decimal string, left-aligned
// in 18 base-11 digits (digit d → d + 1, padding → 0), is an integer whose numeric
// order is the string order of the decimal strings (a proper prefix sorts first).
// 11^18 < 2^63.  Fields are stable-sorted least significant first (LSD over fields).
// Digits are taken least significant first by constant divisions (multiply-high), the
// weight of the last digit being 11^(18 - n); a number of more than 18 digits keys on its
// leading 18.
__host__ __device__ inline unsigned long long dec_key(unsigned long long v) {
  int n = dec_digits(v);
  for (; n > 18; --n) v /= 10ull;
  unsigned long long m = 1, key = 0;
  for (int k = n; k < 18; ++k) m *= 11ull;
  for (int k = 0; k < n; ++k) {
    key += (v % 10ull + 1ull) * m;
    v /= 10ull;
    m *= 11ull;
  }
  return key;
}
enum TileField { TF_FILE = 0, TF_ID, TF_NEXT, TF_DURATION, TF_LENGTH, TF_QUEUE, TF_START, TF_END, TF_COUNT };
// Segment.compareTo (Segment.java:50-53): numeric (id, next_id), stable
// (Collections.sort keeps arrival order within equal keys)
__global__ void k_pair_key(const otr_tile_row* rows, const int32_t* perm, int64_t n, int field,
                           unsigned long long* key) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const otr_tile_row& r = rows[perm[i]];
  key[i] = field == TF_FILE ? r.file : (field == TF_ID ? r.id : r.next_id);
}
__global__ void k_line_key(const otr_tile_row* rows, const int32_t* perm, int64_t n, int field,
                           unsigned long long* key) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const otr_tile_row& r = rows[perm[i]];
  unsigned long long v;
  switch (field) {
    case TF_FILE: key[i] = r.file; return;
    case TF_ID: v = r.id; break;
    case TF_NEXT: v = r.next_id; break;
    case TF_DURATION: v = (unsigned long long)(uint32_t)r.duration; break;
    case TF_LENGTH: v = (unsigned long long)(uint32_t)r.length; break;
    case TF_QUEUE: v = (unsigned long long)(uint32_t)r.queue_length; break;
    case TF_START: v = (unsigned long long)r.start; break;
    default: v = (unsigned long long)r.end; break;
  }
  key[i] = dec_key(v);
}
__global__ void k_gather_rows(const otr_tile_row* in, const int32_t* idx, int64_t n, otr_tile_row* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[idx[i]];
}

// K10: privacy cull (simple_reporter.py:221-239), one thread per file over its sorted
// rows.  Runs of equal (id, next_id) are kept iff at least `privacy` long — except that
// a trailing run of length 1 is judged together with the run before it (the loop
// reaches the last line while its range still starts at the previous run).
// Run-parallel form: rows → runs of equal (file, id, next_id) (head flags, scan,
// scatter of run starts); one thread per run decides from its own length and its
// neighbours' whether it is kept; rows inherit their run's decision.
__global__ void k_run_heads(const otr_tile_row* r, int64_t n, int64_t* head) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    head[i] = (i == 0 || r[i].file != r[i - 1].file || r[i].id != r[i - 1].id || r[i].next_id != r[i - 1].next_id)
                  ? 1 : 0;
}

__global__ void k_cull_runs(const otr_tile_row* r, int64_t n, const int64_t* run_start, int64_t n_runs,
                            int32_t privacy, uint8_t* run_keep) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_runs) return;
  auto len = [&](int64_t q) { return (q + 1 < n_runs ? run_start[q + 1] : n) - run_start[q]; };
  auto same_file = [&](int64_t p, int64_t q) { return r[run_start[p]].file == r[run_start[q]].file; };
  const bool last = k + 1 == n_runs || !same_file(k, k + 1);
  const int64_t L = len(k);
  bool keep;
  if (last) {
    // the final run of a file: a singleton after another run is judged with it
    keep = (L == 1 && k > 0 && same_file(k - 1, k)) ? len(k - 1) + 1 >= privacy : L >= privacy;
  } else {
    const bool next_last = k + 2 == n_runs || !same_file(k + 1, k + 2);
    keep = (next_last && len(k + 1) == 1) ? L + 1 >= privacy : L >= privacy;
  }
  run_keep[k] = keep ? 1 : 0;
}

// row keep flag from its run (run index = inclusive scan of run heads - 1)
__global__ void k_row_keep(const int64_t* run_pos, const uint8_t* run_keep, int64_t n, int64_t* keep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keep[i] = run_keep[run_pos[i] - 1];
}

}  // namespace otr
