// otr_traversals.h — K13: the edge traversals of the matched route
// and the per-edge speed entries made of the complete ones.  Runs after k_segments, only
// for batches that ask for it (OTR_BATCH_EDGE_TRAVERSALS); reads the edge portions K7 left
// at the traces' capacity offsets and writes eleven dense arrays.  Times and fractions in
// binary64, no FMA contraction (the library's build).
#pragma once
#include "otr_kernels.h"

namespace otr {

struct TravArgs {
  BatchDev b;
  const int64_t* trace_state_off;
  const int64_t* state_probe;
  const int32_t* cand_count;
  const uint32_t* cand_edge;
  const double* cand_p;
  const int32_t* winner;
  // what K7 left: per active ordinal (from trace_state_off[t]) and at capacity offsets
  const int64_t* act;
  const int64_t* pos;
  const int32_t* subb;
  const uint32_t* por_e;  const int64_t* por_s0;  const int64_t* por_s1;  const int32_t* por_sa;
  const int64_t* cap_off;
  const uint32_t* route;  const int64_t* route_n;
  // per trace: the number of traversals, then their offsets
  int64_t* count;
  const int64_t* trav_off;
  // per traversal
  uint32_t* edge;  uint32_t* way;  unsigned long long* seg_id;  int64_t* first_state;
  double* f0;  double* f1;  int64_t* s0_mm;  int64_t* s1_mm;  double* t_enter;  double* t_exit;
};

// One wave per trace (k_segments' XCD map): a trace has as many traversals as its route has
// entries that are no separator.  The route's length is taken from route_n, cut to the
// trace's capacity, so the count stays inside the trace's share of the portion arrays
// whatever state a trace beyond every search tier was left in.
__global__ __launch_bounds__(64) void k_trav_count(TravArgs a) {
  const int lane = threadIdx.x;
  const int64_t t = xcd_remap(blockIdx.x, (a.b.n_traces + 7) / 8);
  if (t >= a.b.n_traces) return;
  const int64_t co = a.cap_off[t], cap = a.cap_off[t + 1] - co;
  int64_t n = a.route_n[t];
  if (n > cap) n = cap;
  int64_t c = 0;
  for (int64_t base = 0; base < n; base += OTR_WAVE) {
    const int64_t q = base + lane;
    c += __popcll(__ballot(q < n && a.route[co + q] != 0xFFFFFFFFu));
  }
  if (lane == 0) a.count[t] = c;
}

// time at route position x of the sub-path with active ordinals sa..sb (sb > sa): linear
// between the states around it (K7's time_at, restated)
__device__ inline double trav_time_at(const TravArgs& a, const int64_t* act, const int64_t* pos, int32_t sa,
                                      int32_t sb, int64_t x) {
  int32_t lo_i = sa + 1, hi_i = sb + 1;  // first ordinal m in [sa+1, sb] with pos[m] >= x
  while (lo_i < hi_i) {
    const int32_t mid = (lo_i + hi_i) >> 1;
    if (pos[mid] >= x) hi_i = mid;
    else lo_i = mid + 1;
  }
  const int32_t kk = (lo_i > sb ? sb : lo_i) - 1;
  const double t0 = (double)a.b.time[a.state_probe[act[kk]]];
  const double t1 = (double)a.b.time[a.state_probe[act[kk + 1]]];
  const int64_t p0 = pos[kk], p1 = pos[kk + 1];
  if (p1 > p0) return t0 + (t1 - t0) * ((double)(x - p0) / (double)(p1 - p0));
  return t0;
}

// One wave per trace, a lane per traversal (= K7 portion), 64 at a time.  A portion is the
// first of its sub-path when its predecessor has another por_sa, the last when its
// successor has: the first starts at the fraction of the sub-path's first winner, the last
// ends at the fraction of its last winner, every other end is an end of the edge.
__global__ __launch_bounds__(64) void k_edge_traversals(DevGraph g, TravArgs a) {
  const int lane = threadIdx.x;
  const int64_t t = xcd_remap(blockIdx.x, (a.b.n_traces + 7) / 8);
  if (t >= a.b.n_traces) return;
  const int64_t o = a.trav_off[t], n = a.trav_off[t + 1] - o;
  if (n <= 0) return;
  const int64_t so = a.trace_state_off[t], eo = a.trace_state_off[t + 1];
  const int64_t co = a.cap_off[t];
  int na = 0;
  for (int64_t base = so; base < eo; base += OTR_WAVE) {
    const int64_t s = base + lane;
    na += __popcll(__ballot(s < eo && a.cand_count[s] > 0));
  }
  const int64_t* act = a.act + so;
  const int64_t* pos = a.pos + so;
  const int32_t* subb = a.subb + so;
  for (int64_t j = lane; j < n; j += OTR_WAVE) {
    const int64_t q = co + j, w = o + j;
    const uint32_t e = a.por_e[q];
    const int32_t sa = a.por_sa[q];
    const int64_t s0 = a.por_s0[q], s1 = a.por_s1[q];
    const int32_t sb = (sa >= 0 && sa < na) ? subb[sa] : -1;
    // (only a trace beyond every search tier can fail this: its entries are not to be read)
    if (!(sb > sa && sb < na) || e >= g.n_edges) {
      a.edge[w] = e;
      a.way[w] = 0u;
      a.seg_id[w] = OTR_NO_ID_U64;
      a.first_state[w] = -1;
      a.f0[w] = 0.0;
      a.f1[w] = 0.0;
      a.s0_mm[w] = s0;
      a.s1_mm[w] = s1;
      a.t_enter[w] = 0.0;
      a.t_exit[w] = 0.0;
      continue;
    }
    const bool first = j == 0 || a.por_sa[q - 1] != sa;
    const bool last = j == n - 1 || a.por_sa[q + 1] != sa;
    const int64_t st_a = act[sa], st_b = act[sb];
    const uint32_t key = g.edge_seg[e];
    a.edge[w] = e;
    a.way[w] = g.edge_way[e];
    a.seg_id[w] = key != OTR_NO_SEGMENT ? g.seg_id[key] : OTR_NO_ID_U64;
    a.first_state[w] = st_a;
    a.f0[w] = first ? a.cand_p[st_a * OTR_KMAX + a.winner[st_a]] : 0.0;
    a.f1[w] = last ? a.cand_p[st_b * OTR_KMAX + a.winner[st_b]] : 1.0;
    a.s0_mm[w] = s0;
    a.s1_mm[w] = s1;
    a.t_enter[w] = trav_time_at(a, act, pos, sa, sb, s0);
    a.t_exit[w] = trav_time_at(a, act, pos, sa, sb, s1);
  }
}

// ---- per-edge speed entries of the complete traversals -----------------------------------
struct TravObsArgs {
  int64_t n;
  const uint32_t* edge;  const int64_t* first_state;
  const double* f0;  const double* f1;  const int64_t* s0_mm;  const int64_t* s1_mm;
  const double* t_enter;  const double* t_exit;
  int64_t quantisation;
  int64_t* keep;           // 1: the traversal yields an entry
  const int64_t* keep_off;  // keep's scan: [0] = 0, [j + 1] inclusive
  otr_hist_entry* entries;
};

constexpr unsigned kTravObsGrid = 2048;  // blocks of the grid strides over the traversals

// complete (fraction 0 to 1) and longer than half a second (OTR_TILE_RULES_SIMPLE's floor)
__global__ void k_trav_obs_keep(TravObsArgs a) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.n; j += (int64_t)gridDim.x * blockDim.x) {
    const double dt = a.t_exit[j] - a.t_enter[j];
    a.keep[j] = (a.f0[j] == 0.0 && a.f1[j] == 1.0 && dt > 0.5) ? 1 : 0;
  }
}

__global__ void k_trav_obs_fill(DevGraph g, TravObsArgs a) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.n; j += (int64_t)gridDim.x * blockDim.x) {
    if (a.keep[j] == 0) continue;
    const uint32_t e = a.edge[j];
    const double te = a.t_enter[j];
    const double dt = a.t_exit[j] - te;
    const int64_t hour = (int64_t)floor(te) / a.quantisation;
    const double kph20 = (double)(a.s1_mm[j] - a.s0_mm[j]) / 1000.0 / dt * 3.6 / 20.0;
    const int bin = (int)kph20;
    otr_hist_entry h;
    h.file = ((uint64_t)hour << 25) | ((uint64_t)OTR_ATTR_LEVEL(g.edge_attr[e]) << 22);
    h.id = e;
    h.next_id = (j + 1 < a.n && a.first_state[j + 1] == a.first_state[j]) ? (uint64_t)a.edge[j + 1]
                                                                           : (uint64_t)OTR_INVALID_SEGMENT_ID;
    h.speed_bin = (uint32_t)(bin < 7 ? bin : 7);
    h.count = 1u;
    a.entries[a.keep_off[j]] = h;
  }
}

}  // namespace otr
