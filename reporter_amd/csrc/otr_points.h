// otr_points.h — K12 k_matched_points: where on the road every probe ended up
// (DESIGN.md §3 item 11).  Runs after k_segments, only for batches that ask for it
// (OTR_BATCH_MATCHED_POINTS); reads what the earlier stages left in HBM and writes eight
// per-probe arrays.  Every decision in binary64, no FMA contraction (the library's build).
#pragma once
#include "otr_kernels.h"

namespace otr {

struct PointArgs {
  BatchDev b;
  const int64_t* trace_state_off;
  const int64_t* state_probe;
  const int32_t* cand_count;
  const uint32_t* cand_edge;
  const double* cand_p;
  const int32_t* winner;
  const uint8_t* brk;
  const int64_t* path_off;
  const int32_t* path_len;
  const uint32_t* path;
  const int64_t* act;  // K7's compact active state list and positions (by active ordinal)
  const int64_t* pos;
  // per probe
  uint8_t* kind;
  uint32_t* edge;
  double* frac;
  double* lat;
  double* lon;
  double* dist;
  int64_t* state;
  int64_t* pos_mm;
};

constexpr uint8_t kPointUnmatched = 0, kPointState = 1, kPointInterpolated = 2;

__device__ inline void point_unmatched(const PointArgs& a, int64_t i) {
  a.kind[i] = kPointUnmatched;
  a.edge[i] = 0xFFFFFFFFu;
  a.frac[i] = 0.0;
  a.lat[i] = 0.0;
  a.lon[i] = 0.0;
  a.dist[i] = 0.0;
  a.state[i] = -1;
  a.pos_mm[i] = -1;
}

// project(e, probe): K1's projection onto the whole polyline of edge e in the probe-local
// metric (project_edge's arithmetic and order; no radius, mode or cell test)
__device__ inline void point_project(const DevGraph& g, uint32_t e, double plat, double plon, double mpl, double* d2_out,
                                     double* frac_out) {
  double best = __builtin_huge_val(), best_along = 0.0, acc = 0.0;
  const uint32_t k0 = g.edge_shape[e], k1 = g.edge_shape[e + 1];
  int2 pa = k0 < k1 ? g.shape_ll[k0] : make_int2(0, 0);
  for (uint32_t k = k0; k + 1 < k1; ++k) {
    const int2 pb = g.shape_ll[k + 1];
    const double ax = (e6(pa.y) - plon) * mpl;
    const double ay = (e6(pa.x) - plat) * kMetersPerDeg;
    const double bx = (e6(pb.y) - plon) * mpl;
    const double by = (e6(pb.x) - plat) * kMetersPerDeg;
    const double dx = bx - ax, dy = by - ay;
    const double l2 = dx * dx + dy * dy;
    double t = 0.0;
    if (l2 > 0.0) {
      t = -(ax * dx + ay * dy) / l2;
      if (t < 0.0) t = 0.0;
      if (t > 1.0) t = 1.0;
    }
    const double qx = ax + t * dx, qy = ay + t * dy;
    const double d2 = qx * qx + qy * qy;
    const double sl = sqrt(l2);
    if (d2 < best) {
      best = d2;
      best_along = acc + t * sl;
    }
    acc = acc + sl;
    pa = pb;
  }
  *d2_out = best;
  *frac_out = acc > 0.0 ? best_along / acc : 0.0;
}

// length of shape segment k -> k + 1 as K1 computes it
__device__ inline double point_seg_len(int2 pa, int2 pb, double plat, double plon, double mpl) {
  const double ax = (e6(pa.y) - plon) * mpl;
  const double ay = (e6(pa.x) - plat) * kMetersPerDeg;
  const double bx = (e6(pb.y) - plon) * mpl;
  const double by = (e6(pb.x) - plat) * kMetersPerDeg;
  const double dx = bx - ax, dy = by - ay;
  return sqrt(dx * dx + dy * dy);
}

// point_at(e, f): the coordinate at fraction f of edge e's length in the same metric
__device__ inline void point_at(const DevGraph& g, uint32_t e, double f, double plat, double plon, double mpl,
                                double* lat_out, double* lon_out) {
  const uint32_t k0 = g.edge_shape[e], k1 = g.edge_shape[e + 1];
  if (k0 + 1 >= k1) {  // (no shape segment: never in a valid graph file)
    const int2 p = k0 < k1 ? g.shape_ll[k0] : make_int2(0, 0);
    *lat_out = e6(p.x);
    *lon_out = e6(p.y);
    return;
  }
  double acc = 0.0;
  int2 pa = g.shape_ll[k0];
  for (uint32_t k = k0; k + 1 < k1; ++k) {
    const int2 pb = g.shape_ll[k + 1];
    acc = acc + point_seg_len(pa, pb, plat, plon, mpl);
    pa = pb;
  }
  const double target = f * acc;
  double cum = 0.0, sl = 0.0;
  pa = g.shape_ll[k0];
  int2 pb = pa;
  for (uint32_t k = k0; k + 1 < k1; ++k) {
    pb = g.shape_ll[k + 1];
    sl = point_seg_len(pa, pb, plat, plon, mpl);
    if (cum + sl >= target || k + 2 >= k1) break;  // the first segment reaching target, else the last
    cum = cum + sl;
    pa = pb;
  }
  double u = sl > 0.0 ? (target - cum) / sl : 0.0;
  if (u < 0.0) u = 0.0;
  if (u > 1.0) u = 1.0;
  const double la = e6(pa.x), lo = e6(pa.y);
  *lat_out = la + u * (e6(pb.x) - la);
  *lon_out = lo + u * (e6(pb.y) - lo);
}

__device__ inline void point_write(const DevGraph& g, const PointArgs& a, int64_t i, uint8_t kind, uint32_t e, double f,
                                   double plat, double plon, double mpl, int64_t state, int64_t pos_mm) {
  double la, lo;
  point_at(g, e, f, plat, plon, mpl, &la, &lo);
  a.kind[i] = kind;
  a.edge[i] = e;
  a.frac[i] = f;
  a.lat[i] = la;
  a.lon[i] = lo;
  a.dist[i] = gc_dist(plat, plon, la, lo);
  a.state[i] = state;
  a.pos_mm[i] = pos_mm;
}

// One wave per trace (k_segments' XCD map), a lane per active state a: the lane writes a's
// own probe (kind 1) and every probe up to the next active state b — interpolated along
// the pieces of the winner route a -> b with the gap's cursor when b continues a's
// sub-path, unmatched otherwise.  Lane 0's first state also takes the probes before it,
// the last state the probes after it, so every probe of the trace is written exactly once.
// A gap is serial by definition (the cursor) and its lane walks it alone: polylines,
// gaps and piece lists of any length are loops, not wave-sized chunks.
__global__ __launch_bounds__(64) void k_matched_points(DevGraph g, PointArgs a) {
  const int lane = threadIdx.x;
  const int64_t t = xcd_remap(blockIdx.x, (a.b.n_traces + 7) / 8);
  if (t >= a.b.n_traces) return;
  const int64_t so = a.trace_state_off[t], eo = a.trace_state_off[t + 1];
  const int64_t lo = a.b.trace_off[t], hi = a.b.trace_off[t + 1];
  int na = 0;
  for (int64_t base = so; base < eo; base += OTR_WAVE) {
    const int64_t s = base + lane;
    na += __popcll(__ballot(s < eo && a.cand_count[s] > 0));
  }
  if (na == 0) {
    for (int64_t i = lo + lane; i < hi; i += OTR_WAVE) point_unmatched(a, i);
    return;
  }
  const int64_t* act = a.act + so;
  const int64_t* pos = a.pos + so;
  for (int k = lane; k < na; k += OTR_WAVE) {
    const int64_t sa = act[k];
    const int64_t ia = a.state_probe[sa];
    const int wa = a.winner[sa];
    const uint32_t ea = a.cand_edge[sa * OTR_KMAX + wa];
    const double pa = a.cand_p[sa * OTR_KMAX + wa];
    const int64_t pos_a = pos[k];
    if (k == 0)
      for (int64_t i = lo; i < ia; ++i) point_unmatched(a, i);
    {
      const double plat = a.b.lat[ia], plon = a.b.lon[ia];
      point_write(g, a, ia, kPointState, ea, pa, plat, plon, kMetersPerDeg * cos_deg(plat), sa, pos_a);
    }
    const bool has_next = k + 1 < na;
    const int64_t sb = has_next ? act[k + 1] : 0;
    const int64_t ib = has_next ? a.state_probe[sb] : hi;
    if (!has_next || a.brk[sb] != 0) {
      for (int64_t i = ia + 1; i < ib; ++i) point_unmatched(a, i);
      continue;
    }
    if (ia + 1 >= ib) continue;
    // ---- the gap a -> b
    const int wb = a.winner[sb];
    const uint32_t eb = a.cand_edge[sb * OTR_KMAX + wb];
    const double pb = a.cand_p[sb * OTR_KMAX + wb];
    const int64_t pos_b = pos[k + 1];
    const bool same = eb == ea && pb >= pa;
    const int pl = same ? 0 : a.path_len[sb];
    const uint32_t* path = a.path + (same ? 0 : a.path_off[sb]);
    const int np = same ? 1 : pl + 2;  // pieces: (ea, [pa, pb]) | (ea, [pa, 1]), the path's edges, (eb, [0, pb])
    int c = 0;                         // the cursor (c, fc) and the route length before piece c
    double fc = pa;
    int64_t before = 0;
    for (int64_t i = ia + 1; i < ib; ++i) {
      const double plat = a.b.lat[i], plon = a.b.lon[i];
      const double mpl = kMetersPerDeg * cos_deg(plat);
      int bq = c;
      double bd2 = 0.0, bf = 0.0;
      for (int q = c; q < np; ++q) {
        const uint32_t e = q == 0 ? ea : (q == np - 1 ? eb : path[q - 1]);
        double d2, f;
        point_project(g, e, plat, plon, mpl, &d2, &f);
        if (q == c || d2 < bd2) {
          bd2 = d2;
          bf = f;
          bq = q;
        }
      }
      const double f_lo = bq == 0 ? pa : 0.0;
      const double f_hi = same ? pb : (bq == np - 1 ? pb : 1.0);
      double f = bf;
      if (f < f_lo) f = f_lo;
      if (f > f_hi) f = f_hi;
      if (bq == c && f < fc) f = fc;
      for (; c < bq; ++c)
        before += c == 0 ? part_mm(1.0 - pa, g.len_mm[ea]) : (int64_t)g.len_mm[path[c - 1]];
      fc = f;
      const uint32_t e = bq == 0 ? ea : (bq == np - 1 ? eb : path[bq - 1]);
      int64_t pm = pos_a + (bq == 0 ? part_mm(f - pa, g.len_mm[ea]) : before + part_mm(f, g.len_mm[e]));
      if (pm > pos_b) pm = pos_b;
      point_write(g, a, i, kPointInterpolated, e, f, plat, plon, mpl, sa, pm);
    }
  }
}

// every probe of the traces whose search outgrew the largest table (trace_status not OK,
// known on the host after the batch drained) is unmatched
__global__ void k_points_failed(PointArgs a, const int32_t* status) {
  for (int64_t t = blockIdx.x; t < a.b.n_traces; t += gridDim.x) {
    if (status[t] == 0) continue;
    for (int64_t i = a.b.trace_off[t] + threadIdx.x; i < a.b.trace_off[t + 1]; i += blockDim.x) point_unmatched(a, i);
  }
}

}  // namespace otr
