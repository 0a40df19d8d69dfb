// otr_tiles.hip — the tile stages behind the matching pipeline, on the matcher's stream and
// workspace slots (otr_slots.h): the tile sort and privacy cull (K10: tiles_cull, and cull_device
// for rows already in HBM) and the keyed speed histogram (otr_hist_reduce).  Kernels:
// otr_tile_kernels.h and below.  Nothing here reads the route tiers' build macros.
#include <cstring>
#include <utility>
#include <vector>

#include "otr_devscan.h"
#include "otr_engine.h"
#include "otr_slots.h"
#include "otr_tile_kernels.h"
#include "otr_util_kernels.h"

namespace otr {

// Tile stage: sort rows into simple_reporter's line order per file, then cull
// (K10).  Result rows are copied to host (matcher-owned).
int Matcher::tiles_cull(const otr_tile_row* rows, int64_t n, int memory, int privacy, int rules,
                        const otr_tile_row** out, int64_t* n_out, std::string* err) {
  return guarded(stream, err, [&]() -> int {
    GraphState& gs = graph_state();
    HIPCHK(hipSetDevice(gs.device));
    if (!stream) HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    *n_out = 0;
    *out = nullptr;
    h_tile_rows.clear();
    if (n <= 0) return OTR_OK;
    if (n >= (int64_t)INT32_MAX) {
      if (err) *err = "too many tile rows for one call";
      return OTR_BAD_REQUEST;
    }
    // staging: a copy of the caller's rows
    otr_tile_row* d_in = need<otr_tile_row>(S_ROWS_IN, n);
    HIPCHK(hipMemcpyAsync(d_in, rows, sizeof(otr_tile_row) * n,
                          memory == OTR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    CulledRows c;
    const int rc = cull_device(d_in, n, privacy, rules, &c, err);
    if (rc != OTR_OK) return rc;
    const int64_t nk = c.n_kept;
    h_tile_rows.resize(nk > 0 ? nk : 1);
    if (nk > 0) HIPCHK(hipMemcpy(h_tile_rows.data(), c.kept, sizeof(otr_tile_row) * nk, hipMemcpyDeviceToHost));
    HIPCHK(hipGetLastError());
    *out = h_tile_rows.data();
    *n_out = nk;
    return OTR_OK;
  });
}

// The sort, run split, k_cull_runs and compaction over 0 < n < 2^31 rows in HBM (d_in: any
// device memory but the cull slots below; it is only read).  Leaves the sorted rows, the
// kept rows and the inclusive scan of the sorted rows' keep flags in the matcher's cull
// slots, with the stream drained.
int Matcher::cull_device(const otr_tile_row* d_in, int64_t n, int privacy, int rules, CulledRows* out,
                         std::string* err) {
  return guarded(stream, err, [&]() -> int {
    // staging: sorted, kept; permutation + radix keys
    otr_tile_row* d = need<otr_tile_row>(S_ROWS_OUT, n);
    otr_tile_row* d_kept = need<otr_tile_row>(S_ROWS_KEPT, n);
    int32_t* perm_a = need<int32_t>(S_IDX_A, n);
    int32_t* perm_b = need<int32_t>(S_IDX_B, n);
    unsigned long long* key_a = need<unsigned long long>(S_KEY_A, n);
    unsigned long long* key_b = need<unsigned long long>(S_KEY_B, n);
    int64_t* head = need<int64_t>(S_FILE_HEAD, n);
    int64_t* keep = need<int64_t>(S_KEEP, n);
    int64_t* pos = need<int64_t>(S_POS_SCAN, n);
    int64_t* fstart = need<int64_t>(S_FILE_START, n);
    const int ni = (int)n;
    // one workspace for every sort and scan of the call, sized before the first launch
    int rc;
    Workspace tmp;
    if ((rc = scan_sort_bytes(head, pos, key_a, key_b, perm_a, perm_b, ni, &tmp.bytes, stream, err))) return rc;
    tmp.p = need<char>(S_SORT_TMP, tmp.bytes);
    // LSD over the sort fields: stable radix passes, least significant field first (the
    // identity start keeps arrival order within equal keys)
    k_iota<int32_t><<<grid_ceil(n, 256), 256, 0, stream>>>(perm_a, n);
    const bool pair_order = rules == OTR_TILE_RULES_STREAM;
    for (int f = pair_order ? TF_NEXT : TF_COUNT - 1; f >= 0; --f) {
      if (pair_order) k_pair_key<<<grid_ceil(n, 256), 256, 0, stream>>>(d_in, perm_a, n, f, key_a);
      else k_line_key<<<grid_ceil(n, 256), 256, 0, stream>>>(d_in, perm_a, n, f, key_a);
      const int end_bit = (f == TF_FILE || pair_order) ? 64 : 63;
      if ((rc = sort_pairs(tmp, key_a, key_b, perm_a, perm_b, ni, 0, end_bit, stream, err))) return rc;
      std::swap(perm_a, perm_b);
    }
    k_gather_rows<<<grid_ceil(n, 256), 256, 0, stream>>>(d_in, perm_a, n, d);
    // runs of equal (file, id, next_id): heads → scan → run starts; per-run decision
    k_run_heads<<<grid_ceil(n, 256), 256, 0, stream>>>(d, n, head);
    if ((rc = inclusive_sum(tmp, head, pos, ni, stream, err))) return rc;
    k_scatter_index<int64_t><<<grid_ceil(n, 256), 256, 0, stream>>>(head, pos, n, fstart);
    int64_t nr = 0;
    if ((rc = read_back(stream, err, fetch(&nr, pos + (n - 1))))) return rc;
    if (nr < 1 || nr > n) {
      if (err) *err = "tile run split failed";
      return OTR_DEVICE_ERROR;
    }
    uint8_t* run_keep = need<uint8_t>(S_RUN_KEEP, nr);
    k_cull_runs<<<grid_ceil(nr, 256), 256, 0, stream>>>(d, n, fstart, nr, privacy, run_keep);
    k_row_keep<<<grid_ceil(n, 256), 256, 0, stream>>>(pos, run_keep, n, keep);
    if ((rc = inclusive_sum(tmp, keep, head, ni, stream, err))) return rc;  // head: reused as positions
    std::swap(pos, head);
    k_scatter_flagged<otr_tile_row><<<grid_ceil(n, 256), 256, 0, stream>>>(d, keep, pos, n, d_kept);
    int64_t nk = 0;
    if ((rc = read_back(stream, err, fetch(&nk, pos + (n - 1))))) return rc;
    if (nk < 0 || nk > n) {
      if (err) *err = "tile cull compaction failed";
      return OTR_DEVICE_ERROR;
    }
    out->sorted = d;
    out->kept = d_kept;
    out->kept_incl = pos;
    out->n_kept = nk;
    return OTR_OK;
  });
}

// ---- keyed speed histogram (include/otr.h otr_hist_reduce) -----------------
struct EntryRange;
__device__ inline void entry_range_init(EntryRange* rng);
// (the first thread also starts the key ranges k_entry_range folds into, the next launch)
__global__ void k_rows_to_entries(const otr_tile_row* r, int64_t n, otr_hist_entry* e, EntryRange* rng) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) entry_range_init(rng);
  if (i >= n) return;
  otr_hist_entry x;
  x.file = r[i].file;
  x.id = r[i].id;
  x.next_id = r[i].next_id;
  x.speed_bin = (uint32_t)r[i].speed_bin;
  x.count = 1u;
  e[i] = x;
}
// key ranges of the entries, for the fewest radix-sort bits: OR of the ids and next ids
// (their widths), min / max hour bucket, and whether every file is the one K9 derives
// from its id (bucket << 25 | level << 22 | tile: then (file, id) order is (bucket,
// level, tile, index) order, one packed key)
struct EntryRange {
  unsigned long long id_or, next_or, file_or, bmin, bmax, foreign;
};
__device__ inline void entry_range_init(EntryRange* rng) { *rng = EntryRange{0ull, 0ull, 0ull, ~0ull, 0ull, 0ull}; }
// entries given as such: no conversion kernel to start the ranges in
__global__ void k_entry_range_init(EntryRange* rng) { entry_range_init(rng); }
// a fixed grid (kRangeBlocks x 1024) strides over the entries; one set of atomics per
// block (one per wave queued ~23K atomics on a single line: 263 us for 244K entries)
constexpr int kRangeBlocks = 128;
__global__ __launch_bounds__(1024) void k_entry_range(const otr_hist_entry* e, int64_t n, EntryRange* r) {
  unsigned long long v[6] = {0ull, 0ull, 0ull, ~0ull, 0ull, 0ull};  // id, next, file OR; bmin; bmax; foreign
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const otr_hist_entry x = e[i];
    v[0] |= x.id;
    v[1] |= x.next_id;
    v[2] |= x.file;
    const unsigned long long b = x.file >> 25;
    v[3] = b < v[3] ? b : v[3];
    v[4] = b > v[4] ? b : v[4];
    v[5] |= (x.file & 0x1FFFFFFull) != (((x.id & 7ull) << 22) | ((x.id >> 3) & 0x3FFFFFull)) ? 1ull : 0ull;
  }
  for (int o = OTR_WAVE / 2; o > 0; o >>= 1) {
    for (int q : {0, 1, 2, 5}) v[q] |= __shfl_xor(v[q], o);
    const unsigned long long a = __shfl_xor(v[3], o), b = __shfl_xor(v[4], o);
    v[3] = a < v[3] ? a : v[3];
    v[4] = b > v[4] ? b : v[4];
  }
  __shared__ unsigned long long part[1024 / OTR_WAVE][6];
  if (lane_id() == 0)
    for (int q = 0; q < 6; ++q) part[threadIdx.x / OTR_WAVE][q] = v[q];
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(blockDim.x / OTR_WAVE); ++w) {
      for (int q : {0, 1, 2, 5}) v[q] |= part[w][q];
      v[3] = part[w][3] < v[3] ? part[w][3] : v[3];
      v[4] = part[w][4] > v[4] ? part[w][4] : v[4];
    }
    atomicOr(&r->id_or, v[0]);
    atomicOr(&r->next_or, v[1]);
    atomicOr(&r->file_or, v[2]);
    atomicMin(&r->bmin, v[3]);
    atomicMax(&r->bmax, v[4]);
    atomicOr(&r->foreign, v[5]);
  }
}
static int bit_width(unsigned long long v) { return v ? 64 - __builtin_clzll(v) : 0; }
// sort key of one LSD pass: 0 file, 1 id, 2 next id, 3 speed bin, 4 next id << 3 | bin,
// 5 (bucket - bmin) << 46 | level << 43 | tile << 21 | index (K9 files, 46-bit ids)
// (iota non-null: the first pass, over the entries as they came; it also writes that identity
// permutation, the values of the first sort)
__global__ void k_entry_key(const otr_hist_entry* e, const int32_t* perm, int64_t n, int field,
                            unsigned long long bmin, unsigned long long* key, int32_t* iota) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (iota) iota[i] = (int32_t)i;
  const otr_hist_entry& x = e[iota ? i : perm[i]];
  unsigned long long k;
  switch (field) {
    case 0: k = x.file; break;
    case 1: k = x.id; break;
    case 2: k = x.next_id; break;
    case 3: k = x.speed_bin; break;
    case 4: k = (x.next_id << 3) | (x.speed_bin & 7u); break;
    default:
      k = (((x.file >> 25) - bmin) << 46) | ((x.id & 7ull) << 43) | (((x.id >> 3) & 0x3FFFFFull) << 21) |
          ((x.id >> 25) & 0x1FFFFFull);
  }
  key[i] = k;
}
// the entries in sorted order, and their run heads by the full key (k_entry_heads' pair = 0)
__global__ void k_gather_entries(const otr_hist_entry* in, const int32_t* idx, int64_t n, otr_hist_entry* out,
                                 int64_t* head) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const otr_hist_entry b = in[idx[i]];
  out[i] = b;
  bool h = i == 0;
  if (!h) {
    const otr_hist_entry& a = in[idx[i - 1]];
    h = a.file != b.file || a.id != b.id || a.next_id != b.next_id || a.speed_bin != b.speed_bin;
  }
  head[i] = h ? 1 : 0;
}
// run heads over sorted entries: pair = 0 the full key, 1 the (file, id, next_id) pair
__global__ void k_entry_heads(const otr_hist_entry* e, int64_t n, int pair, int64_t* head) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool h = i == 0;
  if (!h) {
    const otr_hist_entry &a = e[i - 1], &b = e[i];
    h = a.file != b.file || a.id != b.id || a.next_id != b.next_id || (!pair && a.speed_bin != b.speed_bin);
  }
  head[i] = h ? 1 : 0;
}
// the two columns scanned together over sorted entries (otr_devscan.h tuple_sums): the run head
// flags and the entries' counts, read from the entries themselves
struct HeadCountColumns {
  const int64_t* head;
  const otr_hist_entry* e;
  __host__ __device__ int64_t operator()(int q, int64_t i) const { return q == 0 ? head[i] : (int64_t)e[i].count; }
};
// the last entry of every run carries its run's count sum: csum = inclusive scan of counts,
// run r spans [start_r, next start); out[r] = entry at start_r with count = the sum
__global__ void k_entry_reduce(const otr_hist_entry* e, int64_t n, const int64_t* run_start, int64_t n_runs,
                               const int64_t* csum, otr_hist_entry* out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_runs) return;
  const int64_t s = run_start[r], t = r + 1 < n_runs ? run_start[r + 1] : n;
  otr_hist_entry x = e[s];
  const int64_t tot = csum[t - 1] - (s > 0 ? csum[s - 1] : 0);
  x.count = (uint32_t)(tot < 0xFFFFFFFFll ? tot : 0xFFFFFFFFll);
  out[r] = x;
}
// The owner's privacy cull of simple_reporter.py:218-239 on keyed entries.  A pair's run
// length in its file is its total count over the speed bins (one line per tile row); the
// reference sorts a file's lines as strings, so its runs are in the string order of
// (id, next_id) (dec_key), and the loop judges every run alone (kept iff >= privacy)
// except that a trailing run of ONE line is judged together with the run before it (both
// kept iff that run's length + 1 >= privacy).  Per file (files are
// contiguous in the numeric entry order), one block finds the string-last and the
// string-second pair (a top-2 reduction), then every entry gets its keep flag.
struct PairFile {
  unsigned long long s1, n1, s2, n2;  // dec_key of (id, next id): the string-last pair, the one before it
  int64_t t1, t2;                     // their totals
};
__device__ inline bool pf_after(unsigned long long as, unsigned long long an, unsigned long long bs,
                                unsigned long long bn) {
  return as > bs || (as == bs && an > bn);
}
__device__ inline void pf_add(PairFile& T, unsigned long long s, unsigned long long n, int64_t t) {
  if (pf_after(s, n, T.s1, T.n1)) {
    T.s2 = T.s1;
    T.n2 = T.n1;
    T.t2 = T.t1;
    T.s1 = s;
    T.n1 = n;
    T.t1 = t;
  } else if (pf_after(s, n, T.s2, T.n2)) {
    T.s2 = s;
    T.n2 = n;
    T.t2 = t;
  }
}
// (the number of pairs is still on the device, *n_pairs <= n_max: the launch covers n_max and
// writes zeros behind the pairs, so the scan over n_max ends at the number of files and both
// counts reach the host with one wait)
__global__ void k_pair_file_heads(const otr_hist_entry* e, const int64_t* pair_start, const int64_t* n_pairs,
                                  int64_t n_max, int64_t* head) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_max) return;
  head[p] = p < *n_pairs && (p == 0 || e[pair_start[p]].file != e[pair_start[p - 1]].file) ? 1 : 0;
}
// every pair's string-order keys (dec_key of id and next id) and total, one thread per
// pair: the per-file reduction below then only compares
struct PairKey {
  unsigned long long s, n;
  int64_t t;
};
__global__ void k_pair_keys(const otr_hist_entry* e, const int64_t* pair_start, int64_t n_pairs, int64_t n,
                            const int64_t* csum, PairKey* K) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const int64_t s = pair_start[p], t = p + 1 < n_pairs ? pair_start[p + 1] : n;
  const otr_hist_entry& x = e[s];
  K[p] = PairKey{dec_key(x.id), dec_key(x.next_id), csum[t - 1] - (s > 0 ? csum[s - 1] : 0)};
}
// one 1024-thread block per file over its pairs [ffirst[f], ffirst[f + 1]): the top two pairs
// by (dec_key(id), dec_key(next_id)) and their totals (dec_key > 0: 0 marks "none")
__global__ __launch_bounds__(1024) void k_pair_file_top2(const PairKey* K, int64_t n_pairs, const int64_t* ffirst,
                                                        int64_t nf, PairFile* F) {
  const int64_t f = blockIdx.x;
  const int64_t p0 = ffirst[f], p1 = f + 1 < nf ? ffirst[f + 1] : n_pairs;
  PairFile T{0ull, 0ull, 0ull, 0ull, 0, 0};
  for (int64_t p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
    const PairKey k = K[p];
    pf_add(T, k.s, k.n, k.t);
  }
  __shared__ PairFile sh[1024];
  sh[threadIdx.x] = T;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const PairFile U = sh[threadIdx.x + w];
      if (U.s1) pf_add(T, U.s1, U.n1, U.t1);
      if (U.s2) pf_add(T, U.s2, U.n2, U.t2);
      sh[threadIdx.x] = T;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) F[f] = T;
}
__global__ void k_entry_keep(const int64_t* pair_pos, int64_t n, const PairKey* K, const int64_t* fidx,
                             const PairFile* F, int32_t privacy, int64_t* keep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t p = pair_pos[i] - 1;
  const PairKey pk = K[p];
  bool k = pk.t >= (int64_t)privacy;
  const PairFile& f = F[fidx[p] - 1];
  if (f.s2 != 0ull && f.t1 == 1) {  // the file's string-last run is one line: judged with the run before it
    if ((pk.s == f.s1 && pk.n == f.n1) || (pk.s == f.s2 && pk.n == f.n2)) k = f.t2 + 1 >= (int64_t)privacy;
  }
  keep[i] = k ? 1 : 0;
}

int Matcher::copy_out(void* dst, const void* src, size_t bytes, int dst_memory, std::string* err) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, dst_memory == OTR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                        stream));
  HIPCHK(hipStreamSynchronize(stream));
  return OTR_OK;
}

int Matcher::hist_reduce(const void* in, int64_t n, int memory, int rows_in, int privacy, const otr_hist_entry** out,
                         int64_t* n_out, std::string* err) {
  return guarded(stream, err, [&]() -> int {
    GraphState& gs = graph_state();
    HIPCHK(hipSetDevice(gs.device));
    if (!stream) HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    *out = nullptr;
    *n_out = 0;
    if (n <= 0) return OTR_OK;
    if (n >= (int64_t)INT32_MAX) {
      if (err) *err = "too many histogram entries for one call";
      return OTR_BAD_REQUEST;
    }
    otr_hist_entry* e_in = need<otr_hist_entry>(S_HE_IN, n);
    otr_hist_entry* e_sorted = need<otr_hist_entry>(S_HE_SORTED, n);
    otr_hist_entry* e_red = need<otr_hist_entry>(S_HE_RED, n);
    otr_hist_entry* e_out = need<otr_hist_entry>(S_HE_OUT, n);
    int32_t* perm_a = need<int32_t>(S_IDX_A, n);
    int32_t* perm_b = need<int32_t>(S_IDX_B, n);
    unsigned long long* key_a = need<unsigned long long>(S_KEY_A, n);
    unsigned long long* key_b = need<unsigned long long>(S_KEY_B, n);
    int64_t* head = need<int64_t>(S_FILE_HEAD, n);
    int64_t* pos = need<int64_t>(S_POS_SCAN, n);
    int64_t* rstart = need<int64_t>(S_FILE_START, n);
    int64_t* csum = need<int64_t>(S_KEEP, n);
    EntryRange* rng = need<EntryRange>(S_HE_RANGE, 1);
    const int ni = (int)n;
    // one workspace for every sort and scan of the call, sized before the first launch
    int rc;
    Workspace tmp;
    if ((rc = scan_sort_bytes(head, pos, key_a, key_b, perm_a, perm_b, ni, &tmp.bytes, stream, err))) return rc;
    {
      Workspace q;
      int64_t* const two[2] = {pos, csum};
      if ((rc = tuple_sums<2>(&q, HeadCountColumns{head, e_sorted}, two, ni, stream, err))) return rc;
      tmp.bytes = std::max(tmp.bytes, q.bytes);
    }
    tmp.p = need<char>(S_SORT_TMP, tmp.bytes);
    const hipMemcpyKind kind = memory == OTR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (rows_in) {
      // rows already in device memory are read where they are (once, and only read)
      const otr_tile_row* rows = (const otr_tile_row*)in;
      if (memory != OTR_MEM_DEVICE) {
        otr_tile_row* staged = need<otr_tile_row>(S_ROWS_IN, n);
        HIPCHK(hipMemcpyAsync(staged, in, sizeof(otr_tile_row) * n, kind, stream));
        rows = staged;
      }
      k_rows_to_entries<<<grid_ceil(n, 256), 256, 0, stream>>>(rows, n, e_in, rng);
    } else {
      HIPCHK(hipMemcpyAsync(e_in, in, sizeof(otr_hist_entry) * n, kind, stream));
      k_entry_range_init<<<1, 1, 0, stream>>>(rng);
    }
    // LSD over (file, id, next_id, speed_bin), stable passes over a permutation, each only
    // as wide as the keys' range: typically two passes of ~49 bits (next id and bin) and
    // ~47 bits (hour offset and the id in file order), instead of 3 + 3 x 64 bits.  (At ~250K
    // pairs hipcub sorts each pass with a block sort and merge levels, 17 launches; rocprim's
    // one-sweep radix passes, 9 launches, and one merge sort of the 32-byte entries under their
    // full key were both measured slower: DESIGN.md §6u2.)
    // (the host reads of this call, the ranges and the four counts, come through the matcher's
    // pinned mailbox: otr_engine.h)
    static_assert(sizeof(EntryRange) == 6 * 8, "six mailbox words");
    k_entry_range<<<(unsigned)std::min<int64_t>(kRangeBlocks, (n + 1023) / 1024), 1024, 0, stream>>>(e_in, n, rng);
    if ((rc = post_wait({MailRun{rng, 6}}, err))) return rc;
    EntryRange hr;
    memcpy(&hr, mail, sizeof(hr));
    std::vector<std::pair<int, int>> passes;  // (field, end bit), least significant first
    const int wn = bit_width(hr.next_or), wi = bit_width(hr.id_or), ws = bit_width(hr.bmax - hr.bmin);
    if (wn + 3 <= 64) passes.push_back({4, wn + 3});
    else passes.insert(passes.end(), {{3, 3}, {2, wn}});
    if (!hr.foreign && wi <= 46 && ws + 46 <= 64) passes.push_back({5, std::max(46 + ws, 1)});
    else passes.insert(passes.end(), {{1, std::max(wi, 1)}, {0, std::max(bit_width(hr.file_or), 1)}});
    bool first = true;
    for (const auto& ps : passes) {
      k_entry_key<<<grid_ceil(n, 256), 256, 0, stream>>>(e_in, perm_a, n, ps.first, hr.bmin, key_a,
                                                         first ? perm_a : nullptr);
      first = false;
      if ((rc = sort_pairs(tmp, key_a, key_b, perm_a, perm_b, ni, 0, ps.second, stream, err))) return rc;
      std::swap(perm_a, perm_b);
    }
    // runs of equal keys -> one entry each, counts summed: the sorted entries with their run
    // heads, then the head positions and the count sums in one scan
    k_gather_entries<<<grid_ceil(n, 256), 256, 0, stream>>>(e_in, perm_a, n, e_sorted, head);
    {
      int64_t* const two[2] = {pos, csum};
      if ((rc = tuple_sums<2>(&tmp, HeadCountColumns{head, e_sorted}, two, ni, stream, err))) return rc;
    }
    k_scatter_index<int64_t><<<grid_ceil(n, 256), 256, 0, stream>>>(head, pos, n, rstart);
    if ((rc = post_wait({MailRun{pos + (n - 1), 1}}, err))) return rc;
    const int64_t nr = (int64_t)mail[0];
    if (nr < 1 || nr > n) {
      if (err) *err = "histogram run split failed";
      return OTR_DEVICE_ERROR;
    }
    k_entry_reduce<<<grid_ceil(nr, 256), 256, 0, stream>>>(e_sorted, n, rstart, nr, csum, e_red);
    otr_hist_entry* result = e_red;
    int64_t nres = nr;
    if (privacy > 1) {
      // pairs over the reduced entries: heads, totals, keep flags, compaction
      const int nri = (int)nr;
      k_entry_heads<<<grid_ceil(nr, 256), 256, 0, stream>>>(e_red, nr, 1, head);
      {
        int64_t* const two[2] = {pos, csum};
        if ((rc = tuple_sums<2>(&tmp, HeadCountColumns{head, e_red}, two, nri, stream, err))) return rc;
      }
      k_scatter_index<int64_t><<<grid_ceil(nr, 256), 256, 0, stream>>>(head, pos, nr, rstart);
      // per file: the string-last and string-second pairs (the reference loop's trailing run).
      // The file heads and their scan run over nr >= np slots, so np needs no wait of its own:
      // it comes back with nf.
      int64_t* fidx = need<int64_t>(S_HE_FIDX, nr);
      int64_t* fhead = need<int64_t>(S_HE_FHEAD, nr);
      k_pair_file_heads<<<grid_ceil(nr, 256), 256, 0, stream>>>(e_red, rstart, pos + (nr - 1), nr, fhead);
      if ((rc = inclusive_sum(tmp, fhead, fidx, nri, stream, err))) return rc;
      if ((rc = post_wait({MailRun{pos + (nr - 1), 1}, MailRun{fidx + (nr - 1), 1}}, err))) return rc;
      const int64_t np = (int64_t)mail[0], nf = (int64_t)mail[1];
      if (np < 1 || np > nr || nf < 1 || nf > np) {
        if (err) *err = "histogram pair split failed";
        return OTR_DEVICE_ERROR;
      }
      PairFile* pf = need<PairFile>(S_HE_PFILE, std::max<int64_t>(nf, 1));
      int64_t* ffirst = need<int64_t>(S_HE_FFIRST, std::max<int64_t>(nf, 1));
      PairKey* pkey = need<PairKey>(S_HE_PKEY, std::max<int64_t>(np, 1));
      k_scatter_index<int64_t><<<grid_ceil(np, 256), 256, 0, stream>>>(fhead, fidx, np, ffirst);
      k_pair_keys<<<grid_ceil(np, 256), 256, 0, stream>>>(e_red, rstart, np, nr, csum, pkey);
      k_pair_file_top2<<<(unsigned)nf, 1024, 0, stream>>>(pkey, np, ffirst, nf, pf);
      int64_t* keep = head;  // the pair heads are no longer needed
      k_entry_keep<<<grid_ceil(nr, 256), 256, 0, stream>>>(pos, nr, pkey, fidx, pf, privacy, keep);
      int64_t* kpos = rstart;  // pair starts no longer needed after k_entry_keep
      if ((rc = inclusive_sum(tmp, keep, kpos, nri, stream, err))) return rc;
      k_scatter_flagged<otr_hist_entry><<<grid_ceil(nr, 256), 256, 0, stream>>>(e_red, keep, kpos, nr, e_out);
      if ((rc = post_wait({MailRun{kpos + (nr - 1), 1}}, err))) return rc;
      nres = (int64_t)mail[0];
      result = e_out;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    *out = result;
    *n_out = nres;
    return OTR_OK;
  });
}

}  // namespace otr
