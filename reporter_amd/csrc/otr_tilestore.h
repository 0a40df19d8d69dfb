// otr_tilestore.h — K15: the tile store's device code (include/otr.h otr_tile_store_*,
// DESIGN.md §3 item 14).  k_store_rows turns the reports of an add into
// OTR_TILE_RULES_STREAM rows at the end of the store's row buffer, in the reference's forward
// order; the small kernels below build the flush's per-file table from the sorted and the
// kept rows.  Passes are ordered by kernel boundaries only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/otr.h"
#include "otr_device.h"
#include "otr_tilerow.h"

namespace otr {

constexpr int kStoreWaves = 4;  // windows (waves) per 256-thread block
// a report's bucket count is counted up to here: beyond any max_rows (1 << 27), so such an
// add is refused before anything is written, and the window sums stay far from 2^63
constexpr unsigned long long kStoreBucketClamp = 1ull << 28;
// words of the add's counters
enum { TST_VALID = 0, TST_BAD_OFF, TST_WORDS };

struct StoreArgs {
  int64_t n_windows;
  const int32_t* order;  // the window at position p of the arrival order; nullptr: p itself
  const int64_t* rep_off;
  const unsigned long long* id;
  const unsigned long long* next_id;
  const double* t0;
  const double* t1;
  const int32_t* length;
  const int32_t* queue;
  int64_t quantisation;
  int64_t* row_cnt;             // pass 1 output, by position
  unsigned long long* counters;  // pass 1 output: TST_*
  const int64_t* row_off;       // pass 2 input: exclusive offsets, by position
  otr_tile_row* rows;           // pass 2 output: the first free row of the store
  double* row_t0;               // a store with the times (TIMES): the report's t0 and t1 beside
  double* row_t1;               // every row, from the first free row on
};

// the sort key of add_session's window order: triggers ascending; an eviction's windows
// (trigger -1 - rank) by rank
__global__ void k_store_order_key(const int64_t* trigger, int64_t n, unsigned long long* key, int32_t* idx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t t = trigger[i];
  key[i] = (unsigned long long)(t >= 0 ? t : -1 - t);
  idx[i] = (int32_t)i;
}

// One wave per window, a lane per report, 64 reports at a time: a report's rows are
// contiguous (buckets ascending), the reports of a chunk are placed by a wave prefix sum
// and the chunks by the running base, so a window's rows come out in report order and the
// windows at their scanned offsets.  WRITE false counts (row_cnt, the valid reports and
// whether rep_off runs backwards), WRITE true writes every row whole from one lane.  TIMES
// (OTR_TILE_STORE_TIMES) is a template parameter so that the plain store's instance stays the
// instruction stream it was.
template <bool WRITE, bool TIMES = false>
__global__ __launch_bounds__(256) void k_store_rows(StoreArgs a) {
  const int64_t p = (int64_t)blockIdx.x * kStoreWaves + threadIdx.x / OTR_WAVE;
  if (p >= a.n_windows) return;  // wave-uniform
  const int64_t w = a.order ? (int64_t)a.order[p] : p;
  const int64_t lo = a.rep_off[w], hi = a.rep_off[w + 1];
  int64_t base = WRITE ? a.row_off[p] : 0;
  unsigned long long valid = 0;
  for (int64_t r0 = lo; r0 < hi; r0 += OTR_WAVE) {
    const int64_t r = r0 + lane_id();
    BucketSpan sp;
    bool keep = false;
    double t0 = 0, t1 = 0;
    int32_t len = 0, qu = 0;
    if (r < hi) {
      t0 = a.t0[r];
      t1 = a.t1[r];
      len = a.length[r];
      qu = a.queue[r];
      keep = stream_span(t0, t1, len, qu, a.quantisation, &sp);
    }
    unsigned long long nb = keep ? (unsigned long long)(sp.max_bucket - sp.min_bucket + 1) : 0ull;
    if (nb > kStoreBucketClamp) nb = kStoreBucketClamp;
    const unsigned long long incl = wave_incl_scan_u64(nb);
    if (WRITE && keep) {
      const unsigned long long id = a.id[r], nx = a.next_id[r];
      const int speed_bin = tile_speed_bin(len, t0, t1);
      int64_t k = base + (int64_t)(incl - nb);
      for (int64_t bk = sp.min_bucket; bk <= sp.max_bucket; ++bk, ++k) {
        a.rows[k] = tile_row_of(bk, id, nx, sp, len, qu, speed_bin);
        if (TIMES) {
          a.row_t0[k] = t0;
          a.row_t1[k] = t1;
        }
      }
    }
    base += (int64_t)__shfl(incl, OTR_WAVE - 1);
    valid += keep ? 1ull : 0ull;
  }
  if (!WRITE) {
    for (int o = OTR_WAVE / 2; o > 0; o >>= 1) valid += __shfl_xor(valid, o);
    if (lane_id() == 0) {
      a.row_cnt[p] = base;
      if (valid) atomicAdd(&a.counters[TST_VALID], valid);
      if (lo < 0 || hi < lo || (w == 0 && lo != 0)) atomicAdd(&a.counters[TST_BAD_OFF], 1ull);
    }
  }
}

// ---- the flush's per-file table ---------------------------------------------------------
__global__ void k_store_file_heads(const otr_tile_row* r, int64_t n, int64_t* head) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) head[i] = (i == 0 || r[i].file != r[i - 1].file) ? 1 : 0;
}

// file f of the sorted rows starts at start[f] (head_incl: inclusive scan of the heads)
__global__ void k_store_file_starts(const int64_t* head, const int64_t* head_incl, int64_t n, int64_t* start) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && head[i]) start[head_incl[i] - 1] = i;
}

// rows of sorted file f that the clean kept: before[f] kept rows precede it
__device__ inline int64_t store_file_kept(const int64_t* start, int64_t n_files, int64_t n, const int64_t* kept_incl,
                                          int64_t f, int64_t* before, int64_t* rows_in) {
  const int64_t s0 = start[f], s1 = f + 1 < n_files ? start[f + 1] : n;
  *before = s0 > 0 ? kept_incl[s0 - 1] : 0;
  *rows_in = s1 - s0;
  return kept_incl[s1 - 1] - *before;
}

__global__ void k_store_file_listed(const int64_t* start, int64_t n_files, int64_t n, const int64_t* kept_incl,
                                    int64_t* listed) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_files) return;
  int64_t before, rows_in;
  listed[f] = store_file_kept(start, n_files, n, kept_incl, f, &before, &rows_in) > 0 ? 1 : 0;
}

// the listed files in order: file, first kept row, rows before clean; row_off's last
// element is the number of kept rows
__global__ void k_store_file_table(const otr_tile_row* sorted, const int64_t* start, int64_t n_files, int64_t n,
                                   const int64_t* kept_incl, const int64_t* listed, const int64_t* listed_incl,
                                   unsigned long long* file, int64_t* row_off, int64_t* n_unclean) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_files) return;
  if (f == n_files - 1) row_off[listed_incl[f]] = kept_incl[n - 1];
  if (!listed[f]) return;
  int64_t before, rows_in;
  store_file_kept(start, n_files, n, kept_incl, f, &before, &rows_in);
  const int64_t l = listed_incl[f] - 1;
  file[l] = sorted[start[f]].file;
  row_off[l] = before;
  n_unclean[l] = rows_in;
}

}  // namespace otr
