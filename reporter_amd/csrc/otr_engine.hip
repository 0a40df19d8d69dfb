// otr_engine.hip — graph upload (flattened CSR + grid → HBM), the matcher's workspace and the
// batched matching pipeline on one HIP stream (Batch, K0..K9, K12, K13), the edge observations of
// K13's traversals and report_lists_device.  Kernels: otr_kernels.h.  The tile stages are in
// otr_tiles.hip, probe ingest and the stream formatter in otr_text.hip.
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "otr_devscan.h"
#include "otr_engine.h"
#include "otr_kernels.h"
#include "otr_edge.h"
#include "otr_edge1.h"
#include "otr_launch.h"
#include "otr_points.h"
#include "otr_slots.h"
#include "otr_traversals.h"
#include "otr_util_kernels.h"

namespace otr {
static_assert(kTraceWaves == 4, "grid_trace_rows (otr_launch.h) assumes 4 traces per block");

void finalize_params(MatchParams* p) {
  p->inv2s2 = 1.0 / (p->sigma_z * p->sigma_z * 2.0);
  p->inv_beta = 1.0 / p->beta;
  if (p->kmax > OTR_KMAX) p->kmax = OTR_KMAX;
  if (p->kmax < 1) p->kmax = 1;
}

// values the engine cannot honour are refused by name (400), never silently changed
const char* check_params(const MatchParams& p) {
  if (!(p.breakage_distance >= 0.0 && p.breakage_distance <= kMaxBreakage))
    return "breakage_distance must be within [0, 30000] m";
  if (!(p.max_route_distance_factor >= 0.0) || !(p.max_route_distance_factor < 1e6))
    return "max_route_distance_factor must be >= 0";
  if (!(p.max_route_time_factor >= 0.0) || !(p.max_route_time_factor < 1e6)) return "max_route_time_factor must be >= 0";
  if (!(p.turn_penalty_factor >= 0.0) || !(p.turn_penalty_factor <= 1e6)) return "turn_penalty_factor must be within [0, 1e6]";
  if (!(p.sigma_z > 0.0)) return "sigma_z must be > 0";
  if (!(p.beta > 0.0)) return "beta must be > 0";
  if (!(p.search_radius >= 0.0) || !(p.max_search_radius >= 0.0)) return "search_radius must be >= 0";
  if (!(p.interpolation_distance >= 0.0)) return "interpolation_distance must be >= 0";
  if (!(p.speed_kph >= 0.0) || !(p.queue_kph >= 0.0)) return "speed_kph and queue_kph must be >= 0";
  return nullptr;
}

ModeParams default_mode_params() {
  ModeParams mp{};
  for (int m = 0; m < OTR_MODES; ++m) {
    MatchParams& p = mp.m[m];
    p.sigma_z = 4.07;                   // Dockerfile:14
    p.beta = 3.0;                       // Dockerfile:15
    p.max_route_distance_factor = 5.0;  // Dockerfile:16
    p.max_route_time_factor = 2.0;      // Dockerfile:17,48 (MATCHER_TIME_FACTOR)
    p.breakage_distance = 2000.0;
    p.interpolation_distance = 10.0;
    p.search_radius = 50.0;
    p.max_search_radius = 100.0;
    p.gps_accuracy = 5.0;
    p.kmax = 32;
    p.queue_kph = 10.0;
  }
  // valhalla_build_config per-mode meili sections; mode speeds and queue
  // thresholds of DESIGN.md §3.5/3.8
  mp.m[0].turn_penalty_factor = 200.0;
  mp.m[1].turn_penalty_factor = 140.0;
  mp.m[1].speed_kph = 18.0;
  mp.m[1].queue_kph = 5.0;
  mp.m[2].turn_penalty_factor = 100.0;
  mp.m[2].speed_kph = 5.1;
  mp.m[2].queue_kph = 2.0;
  for (int m = 0; m < OTR_MODES; ++m) finalize_params(&mp.m[m]);
  mp.delta = 60.0;  // round width (m): search order only; C2 39.3M -> 39.7M, C4 4.35M -> ~4.4M single stream vs 100
  return mp;
}

// route time of an edge at the mode's speed, 0.1 s (oracle edge_time_ds)
static uint32_t edge_time_ds(uint32_t attr, uint32_t len_mm, double speed_cap) {
  double kph = (double)OTR_ATTR_SPEED(attr);
  if (!(kph > 0.0)) kph = 30.0;  // unknown speed
  if (speed_cap > 0.0 && speed_cap < kph) kph = speed_cap;
  const double v = (double)len_mm * 0.036 / kph;
  return v < 2.0e9 ? (uint32_t)llround(v) : 2000000000u;
}

// heading of the shape segment a -> b, integer degrees clockwise from north, -1 when
// degenerate (oracle seg_heading)
static int seg_heading(const int32_t* a, const int32_t* b) {
  const double la1 = (double)a[0] * 1e-6, lo1 = (double)a[1] * 1e-6;
  const double la2 = (double)b[0] * 1e-6, lo2 = (double)b[1] * 1e-6;
  const double m = 20037581.187 / 180.0;  // metres per degree, Batch.java:36
  const double x = (lo2 - lo1) * m * cos_deg(0.5 * (la1 + la2));
  const double y = (la2 - la1) * m;
  if (x == 0.0 && y == 0.0) return -1;
  double deg = atan2(x, y) * (180.0 / 3.14159265358979323846);
  if (deg < 0.0) deg = deg + 360.0;
  return (int)(llround(deg) % 360);
}

void turn_table(double factor, int32_t* tab) {
  const double x = -1.0 / 45.0;  // e^(-1/45) by its Taylor series, then powers
  double r = 1.0, term = 1.0;
  for (int k = 1; k <= 20; ++k) {
    term = term * x / (double)k;
    r = r + term;
  }
  double f = 1.0;
  for (int i = 0; i <= 180; ++i) {
    const double v = 1000.0 * factor * f;
    tab[i] = factor > 0.0 ? (int32_t)llround(v) : 0;
    f = f * r;
  }
}

GraphState& graph_state() {
  static GraphState gs;
  return gs;
}

namespace {
struct Mapped {
  void* p = MAP_FAILED;
  size_t n = 0;
  ~Mapped() {
    if (p != MAP_FAILED) munmap(p, n);
  }
};
struct Staged {  // a graph replica being built; freed unless adopted
  std::vector<void*> allocs;
  bool adopted = false;
  ~Staged() {
    if (!adopted)
      for (void* q : allocs) (void)hipFree(q);
  }
};
}  // namespace

int engine_configure(const Config& cfg, std::string* err) {
  for (int m = 0; m < OTR_MODES; ++m)
    if (const char* bad = check_params(cfg.mp.m[m])) {
      if (err) *err = std::string("config: ") + bad;
      return OTR_BAD_REQUEST;
    }
  int fd = open(cfg.graph_path.c_str(), O_RDONLY);
  if (fd < 0) {
    if (err) *err = "cannot open graph file " + cfg.graph_path + ": " + strerror(errno);
    return OTR_BAD_REQUEST;
  }
  struct stat st;
  fstat(fd, &st);
  Mapped mf;
  mf.n = (size_t)st.st_size;
  mf.p = mf.n >= sizeof(otr_graph_header) ? mmap(nullptr, mf.n, PROT_READ, MAP_PRIVATE, fd, 0) : MAP_FAILED;
  close(fd);
  if (mf.p == MAP_FAILED) {
    if (err) *err = "cannot map graph file " + cfg.graph_path;
    return OTR_BAD_REQUEST;
  }
  const char* base = (const char*)mf.p;
  otr_graph_header h;
  memcpy(&h, base, sizeof(h));
  if (memcmp(h.magic, OTR_GRAPH_MAGIC, 8) != 0 || h.version != OTR_GRAPH_VERSION ||
      h.array_offset[OTR_A_END] > (uint64_t)st.st_size) {
    if (err) *err = "not an OTR graph file: " + cfg.graph_path;
    return OTR_BAD_REQUEST;
  }
  if (h.n_nodes >= (1u << 28)) {  // adj packs dst in 28 bits
    if (err) *err = "graph has more than 2^28 nodes";
    return OTR_BAD_REQUEST;
  }
  if (h.n_edges >= (1u << 28)) {  // the edge-state records pack the out-edge id in 28 bits (erec)
    if (err) *err = "graph has more than 2^28 directed edges";
    return OTR_BAD_REQUEST;
  }
  const uint32_t* dst = (const uint32_t*)(base + h.array_offset[OTR_A_EDGE_DST]);
  const float* lenf = (const float*)(base + h.array_offset[OTR_A_EDGE_LEN]);
  const uint32_t* attr = (const uint32_t*)(base + h.array_offset[OTR_A_EDGE_ATTR]);
  const uint32_t* row = (const uint32_t*)(base + h.array_offset[OTR_A_NODE_ROW]);
  const int32_t* nll = (const int32_t*)(base + h.array_offset[OTR_A_NODE_LL]);
  const uint32_t* eshape = (const uint32_t*)(base + h.array_offset[OTR_A_EDGE_SHAPE]);
  const int32_t* sll = (const int32_t*)(base + h.array_offset[OTR_A_SHAPE_LL]);
  // ---- host-side validation and derived views (nothing on the device is touched yet)
  // len_mm = round(len * 1000), >= 1 mm: the integer routing length the oracle derives
  // the same way
  std::vector<uint32_t> len(h.n_edges + 1, 0u);
  for (uint32_t e = 0; e < h.n_edges; ++e) {
    const double mm = (double)lenf[e] * 1000.0;
    if (!(mm >= 0.0 && mm < 2.0e9)) {  // uint32 label arithmetic
      if (err) *err = "graph edge length outside [0, 2000 km)";
      return OTR_BAD_REQUEST;
    }
    len[e] = (uint32_t)std::max(1LL, (long long)llround(mm));
  }
  for (uint32_t u = 0; u < h.n_nodes; ++u)
    if (row[u + 1] < row[u] || row[u + 1] > h.n_edges) {
      if (err) *err = "graph CSR rows are not monotone";
      return OTR_BAD_REQUEST;
    }
  for (uint32_t e = 0; e < h.n_edges; ++e)
    if (dst[e] >= h.n_nodes || eshape[e + 1] < eshape[e] + 2 || eshape[e + 1] > h.n_shape) {
      if (err) *err = "graph edge " + std::to_string(e) + " has a bad end node or shape range";
      return OTR_BAD_REQUEST;
    }
  // minin(v): the shortest in-edge of every node (mm, any mode: a lower bound for each),
  // the IN criterion of the exact search rounds; 0xFFFFFFFF: no in-edge
  std::vector<uint32_t> minin(h.n_nodes + 1, 0xFFFFFFFFu);
  for (uint32_t e = 0; e < h.n_edges; ++e) minin[dst[e]] = std::min(minin[dst[e]], len[e]);
  std::vector<uint4> pack(h.n_edges + 1);
  for (uint32_t e = 0; e < h.n_edges; ++e) pack[e] = make_uint4(dst[e], len[e], attr[e], minin[dst[e]]);
  // per edge what k_prep needs of a candidate's edge in one 16-B gather: {len_mm, src,
  // minin(src), dst} (no dependent minin load; C5's country graph misses the L2 there)
  std::vector<uint4> eprep(h.n_edges + 1, make_uint4(0u, 0u, 0u, 0u));
  {
    const uint32_t* srcv = (const uint32_t*)(base + h.array_offset[OTR_A_EDGE_SRC]);
    for (uint32_t e = 0; e < h.n_edges; ++e) eprep[e] = make_uint4(len[e], srcv[e], minin[srcv[e]], dst[e]);
  }
  // per-node adjacency records: the first 4 out-edges of a node in one 64-B record,
  // {dst | access<<28 | more<<31, len_mm, minin(dst), 0} per edge
  std::vector<uint4> adj(4ull * h.n_nodes + 4, make_uint4(kAdjDstMask, 0u, 0u, 0u));
  for (uint32_t u = 0; u < h.n_nodes; ++u) {
    const uint32_t deg = row[u + 1] - row[u];
    for (uint32_t k = 0; k < deg && k < 4; ++k) {
      const uint32_t e = row[u] + k;
      adj[4ull * u + k] = make_uint4(dst[e] | ((attr[e] & OTR_ATTR_ACCESS_MASK) << 28), len[e], minin[dst[e]], 0u);
    }
    if (deg > 4) adj[4ull * u + 3].x |= kAdjMore;
  }
  // route times per mode (0.1 s) per edge and per adjacency slot
  std::vector<uint32_t> et[OTR_MODES], at[OTR_MODES];
  for (int m = 0; m < OTR_MODES; ++m) {
    et[m].assign(h.n_edges + 1, 0u);
    for (uint32_t e = 0; e < h.n_edges; ++e) et[m][e] = edge_time_ds(attr[e], len[e], cfg.mp.m[m].speed_kph);
    at[m].assign(4ull * h.n_nodes + 4, 0u);
    for (uint32_t u = 0; u < h.n_nodes; ++u)
      for (uint32_t k = 0; k < 4 && row[u] + k < row[u + 1]; ++k) at[m][4ull * u + k] = et[m][row[u] + k];
  }
  // edge headings: first / last non-degenerate shape segment (oracle orc_graph_load)
  std::vector<short2> head(h.n_edges + 1, make_short2(0, 0));
  for (uint32_t e = 0; e < h.n_edges; ++e) {
    const uint32_t k0 = eshape[e], k1 = eshape[e + 1];
    int hb = -1, he = -1;
    for (uint32_t k = k0; k + 1 < k1 && hb < 0; ++k) hb = seg_heading(sll + 2ull * k, sll + 2ull * k + 2);
    for (uint32_t k = k1 - 1; k > k0 && he < 0; --k) he = seg_heading(sll + 2ull * k - 2, sll + 2ull * k);
    head[e] = make_short2((short)(hb < 0 ? 0 : hb), (short)(he < 0 ? 0 : he));
  }
  // edge-state view of the adjacency slots (turn-cost searches, otr_edge.h): the slot's
  // edge id and its begin / end headings
  std::vector<uint2> adje(4ull * h.n_nodes + 4, make_uint2(0u, 0u));
  for (uint32_t u = 0; u < h.n_nodes; ++u)
    for (uint32_t k = 0; k < 4 && row[u] + k < row[u + 1]; ++k) {
      const uint32_t e = row[u] + k;
      adje[4ull * u + k] = make_uint2(e, (uint32_t)(uint16_t)head[e].x | ((uint32_t)(uint16_t)head[e].y << 16));
    }
  // edge-state view (otr_edge1.h): per edge state b (arrived at v = dst(b)) one 16-B record
  // per out-edge slot k < 4 of v: {e | access(e) << 28 | more << 31, len_mm(e), the turn
  // degree b -> e | b's end heading << 8, v}, and per mode the slot's route time in a
  // parallel array: a relaxation is one record load and one time load at the same index,
  // with the turn already resolved
  const size_t es = 4ull * h.n_edges + 4;
  std::vector<uint4> erec(es, make_uint4(kAdjDstMask, 0u, 0u, 0u));
  std::vector<uint32_t> erec_t(es * OTR_MODES, 0u);
  for (uint32_t b = 0; b < h.n_edges; ++b) {
    const uint32_t v = dst[b], deg = row[v + 1] - row[v];
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t hend = (uint32_t)(uint16_t)head[b].y << 8;  // b's end heading (target offers)
      if (k >= deg) {
        erec[4ull * b + k] = make_uint4(kAdjDstMask, 0u, hend, v);  // (access 0: never relaxed)
        continue;
      }
      const uint32_t e = row[v] + k;
      const uint32_t x = e | ((attr[e] & OTR_ATTR_ACCESS_MASK) << 28) | ((k == 3 && deg > 4) ? kAdjMore : 0u);
      erec[4ull * b + k] =
          make_uint4(x, len[e], (uint32_t)turn_degree((int)head[b].y, (int)head[e].x) | hend, v);
      for (int m = 0; m < OTR_MODES; ++m) erec_t[es * m + 4ull * b + k] = std::min(et[m][e], 0x1FFFFu);
    }
  }
  // candidate-search view: each grid-cell entry carries its edge's shape range and
  // attributes, 48 B per entry: {edge, shape begin, shape end, attr} + the first four shape points
  const uint32_t* cedge = (const uint32_t*)(base + h.array_offset[OTR_A_CELL_EDGE]);
  std::vector<uint4> crec(3 * ((size_t)h.n_cell_entries + 1), make_uint4(0u, 0u, 0u, 0u));
  for (uint64_t q = 0; q < h.n_cell_entries; ++q) {
    const uint32_t e = cedge[q];
    if (e >= h.n_edges) {
      if (err) *err = "graph cell index names a missing edge";
      return OTR_BAD_REQUEST;
    }
    const uint32_t k0 = eshape[e], k1 = eshape[e + 1];
    crec[3 * q] = make_uint4(e, k0, k1, attr[e]);
    uint32_t pt[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (uint32_t i = 0; i < 4 && k0 + i < k1; ++i) {
      pt[2 * i] = (uint32_t)sll[2ull * (k0 + i)];
      pt[2 * i + 1] = (uint32_t)sll[2ull * (k0 + i) + 1];
    }
    crec[3 * q + 1] = make_uint4(pt[0], pt[1], pt[2], pt[3]);
    crec[3 * q + 2] = make_uint4(pt[4], pt[5], pt[6], pt[7]);
  }
  // ---- upload into a staged replica
  HIPCHK(hipSetDevice(cfg.device));
  Staged sg;
  bool alloc_ok = true;
  auto upv = [&](const void* src, size_t bytes) -> void* {
    void* d = nullptr;
    if (hipMalloc(&d, bytes ? bytes : 16) != hipSuccess) {
      alloc_ok = false;
      return nullptr;
    }
    sg.allocs.push_back(d);
    if (bytes && hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) alloc_ok = false;
    return d;
  };
  auto up = [&](int a, size_t bytes) -> void* { return upv(base + h.array_offset[a], bytes); };
  DevGraph g{};
  g.node_row = (const uint32_t*)up(OTR_A_NODE_ROW, 4ull * (h.n_nodes + 1));
  g.rev_row = (const uint32_t*)up(OTR_A_REV_ROW, 4ull * (h.n_nodes + 1));
  g.node_ll = (const int2*)up(OTR_A_NODE_LL, 8ull * h.n_nodes);
  g.rev_edge = (const uint32_t*)up(OTR_A_REV_EDGE, 4ull * h.n_edges);
  g.edge_src = (const uint32_t*)up(OTR_A_EDGE_SRC, 4ull * h.n_edges);
  g.edge_dst = (const uint32_t*)up(OTR_A_EDGE_DST, 4ull * h.n_edges);
  g.edge_len = (const float*)up(OTR_A_EDGE_LEN, 4ull * h.n_edges);
  g.edge_attr = (const uint32_t*)up(OTR_A_EDGE_ATTR, 4ull * h.n_edges);
  g.edge_shape = (const uint32_t*)up(OTR_A_EDGE_SHAPE, 4ull * (h.n_edges + 1));
  g.edge_seg = (const uint32_t*)up(OTR_A_EDGE_SEG, 4ull * h.n_edges);
  g.edge_way = (const uint32_t*)up(OTR_A_EDGE_WAY, 4ull * h.n_edges);
  g.shape_ll = (const int2*)up(OTR_A_SHAPE_LL, 8ull * h.n_shape);
  g.seg_id = (const unsigned long long*)up(OTR_A_SEG_ID, 8ull * h.n_segments);
  g.seg_len = (const uint32_t*)up(OTR_A_SEG_LEN, 4ull * h.n_segments);
  g.cell_row = (const uint32_t*)up(OTR_A_CELL_ROW, 4ull * (h.n_cells + 1));
  g.cell_edge = (const uint32_t*)up(OTR_A_CELL_EDGE, 4ull * h.n_cell_entries);
  g.len_mm = (const uint32_t*)upv(len.data(), 4ull * len.size());
  g.edge_pack = (const uint4*)upv(pack.data(), sizeof(uint4) * pack.size());
  g.eprep = (const uint4*)upv(eprep.data(), sizeof(uint4) * eprep.size());
  g.adj = (const uint4*)upv(adj.data(), sizeof(uint4) * adj.size());
  g.node_minin = (const uint32_t*)upv(minin.data(), 4ull * minin.size());
  {
    std::vector<uint32_t> all_et, all_at;
    for (int m = 0; m < OTR_MODES; ++m) {
      all_et.insert(all_et.end(), et[m].begin(), et[m].end());
      all_at.insert(all_at.end(), at[m].begin(), at[m].end());
    }
    g.edge_t = (const uint32_t*)upv(all_et.data(), 4ull * all_et.size());
    g.adj_t = (const uint32_t*)upv(all_at.data(), 4ull * all_at.size());
    g.edge_t_stride = (uint32_t)et[0].size();
    g.adj_t_stride = (uint32_t)at[0].size();
  }
  g.edge_head = (const short2*)upv(head.data(), sizeof(short2) * head.size());
  g.adj_e = (const uint2*)upv(adje.data(), sizeof(uint2) * adje.size());
  g.erec = (const uint4*)upv(erec.data(), sizeof(uint4) * erec.size());
  g.erec_t = (const uint32_t*)upv(erec_t.data(), 4ull * erec_t.size());
  g.erec_stride = es;
  g.cell_rec = (const uint4*)upv(crec.data(), sizeof(uint4) * crec.size());
  if (!alloc_ok) {
    if (err) *err = "device allocation for the graph failed";
    return OTR_DEVICE_ERROR;  // the previous graph (if any) stays configured
  }
  g.n_nodes = h.n_nodes;
  g.n_edges = h.n_edges;
  g.n_segments = h.n_segments;
  g.grid_rows = h.grid_rows;
  g.grid_cols = h.grid_cols;
  g.grid_min_lat = h.grid_min_lat;
  g.grid_min_lon = h.grid_min_lon;
  g.grid_cell_deg = h.grid_cell_deg;
  std::vector<unsigned long long> sid((const unsigned long long*)(base + h.array_offset[OTR_A_SEG_ID]),
                                      (const unsigned long long*)(base + h.array_offset[OTR_A_SEG_ID]) + h.n_segments);
  // ---- swap in: batches in flight hold the shared lock, so the old arrays are unused
  GraphState& gs = graph_state();
  std::vector<void*> old;
  {
    std::unique_lock<std::shared_mutex> lk(gs.mu);
    old.swap(gs.allocs);
    gs.allocs = sg.allocs;
    sg.adopted = true;
    gs.dg = g;
    gs.n_nodes = h.n_nodes;
    gs.n_edges = h.n_edges;
    gs.n_segments = h.n_segments;
    gs.seg_id.swap(sid);
    gs.defaults = cfg.mp;
    gs.device = cfg.device;
    gs.ready = true;
  }
  for (void* q : old) (void)hipFree(q);
  return OTR_OK;
}

// ---------------------------------------------------------------------------------
// workspace slots
// ---------------------------------------------------------------------------------

// (the slots, need() and want(): otr_slots.h)

bool Matcher::release_optional() {
  if (opt_busy) return false;
  bool any = false;
  for (int s = 0; s < (int)pool.b.size(); ++s)
    if (optional_slot(s) && pool.held(s, 0)) {
      if (!any && stream) (void)hipStreamSynchronize(stream);  // (no queued kernel still reads it)
      any = true;
      pool.drop(s);
    }
  return any;
}

Matcher::~Matcher() {
  if (ses) sessions_destroy(ses);
  if (tst) tile_store_destroy(tst);
  if (ttx) tile_text_destroy(ttx);
  if (tpx) tile_parse_destroy(tpx);
  pool.release();
  if (mail) (void)hipHostFree(mail);
  if (h_drain) (void)hipHostFree(h_drain);
  for (auto& sl : gslab)
    for (void* q : {(void*)sl.key, (void*)sl.lab, (void*)sl.qmark, (void*)sl.fr, (void*)sl.touched})
      if (q) (void)hipFree(q);
  if (ev_init)
    for (auto& e : ev) (void)hipEventDestroy(e);
  if (stream) (void)hipStreamDestroy(stream);
}

// the runs gathered by one k_post launch into dst (the mailbox when null)
int Matcher::post(std::initializer_list<MailRun> runs, unsigned long long* dst, std::string* err) {
  if (!mail) HIPCHK(hipHostMalloc((void**)&mail, 8 * kMailWords, hipHostMallocMapped | hipHostMallocCoherent));
  PostArgs a{};
  int q = 0, words = 0;
  for (const MailRun& r : runs) {
    if (q >= kPostRuns || r.words < 0 || (!dst && words + r.words > kMailWords)) {
      if (err) *err = "mailbox record too large";
      return OTR_DEVICE_ERROR;
    }
    a.src[q] = (const unsigned long long*)r.src;
    a.n[q] = r.words;
    words += r.words;
    ++q;
  }
  a.dst = dst;
  if (!dst) HIPCHK(hipHostGetDevicePointer((void**)&a.dst, mail, 0));
  k_post<<<1, 64, 0, stream>>>(a);
  return OTR_OK;
}

int Matcher::post_wait(std::initializer_list<MailRun> runs, std::string* err) {
  if (int rc = post(runs, nullptr, err)) return rc;
  HIPCHK(hipStreamSynchronize(stream));
  return OTR_OK;
}

// per-trace output capacity: route/segment/way/report slots
__global__ void k_capacity(int32_t n_traces, const int64_t* trace_state_off, const int32_t* cand_count,
                           const int32_t* path_len, int64_t* cap) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_traces) return;
  int64_t c = 2;
  for (int64_t s = trace_state_off[t]; s < trace_state_off[t + 1]; ++s) {
    if (cand_count[s] <= 0) continue;
    c += 3;
    if (path_len[s] > 0) c += path_len[s];
  }
  cap[t] = c;
}

__global__ void k_fill_i32(int32_t* p, int64_t n, int32_t v) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// Append `value` to an unordered list, one global atomic per block (a single counter
// takes ~3 ns per same-address atomic: per-wave appends of ~1M items cost ~0.5 ms).
__device__ inline void block_append(bool hit, int64_t value, int64_t* list, unsigned long long* count) {
  __shared__ unsigned int s_n;
  __shared__ unsigned long long s_base;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  unsigned int my = 0;
  if (hit) my = atomicAdd(&s_n, 1u);
  __syncthreads();
  if (threadIdx.x == 0) s_base = s_n ? atomicAdd(count, (unsigned long long)s_n) : 0ull;
  __syncthreads();
  if (hit) list[s_base + my] = value;
}

// every task the first route tier flagged (overflow or general): the superset of what the
// later tiers collect, so their collects scan this short list instead of every task.  It reads
// every flag (55 MB at C2) and keeps few, so it runs at memory speed: four flags per thread in
// one 16-byte load (flag: 16-byte aligned, a pool buffer), an ordered count inside the block
// (wave scans of the threads' hit counts, then the 16 wave totals) and one global atomic per
// block that has a hit.  A block's tasks stay in task order in the list (the retry tiers'
// locality); the blocks' order is arbitrary, as it always was.
constexpr int kFlagsPerThread = 4, kFlaggedBlock = 1024;
__global__ __launch_bounds__(kFlaggedBlock) void k_collect_flagged(int64_t n, const int32_t* flag, int64_t* list,
                                                                  unsigned long long* count) {
  __shared__ unsigned int s_wave[kFlaggedBlock / OTR_WAVE];
  __shared__ unsigned long long s_base;
  const int64_t i0 = ((int64_t)blockIdx.x * kFlaggedBlock + threadIdx.x) * kFlagsPerThread;
  int4 f = make_int4(0, 0, 0, 0);
  if (i0 + 3 < n) {
    f = *reinterpret_cast<const int4*>(flag + i0);
  } else if (i0 < n) {  // (the last tasks, fewer than four)
    f.x = flag[i0];
    if (i0 + 1 < n) f.y = flag[i0 + 1];
    if (i0 + 2 < n) f.z = flag[i0 + 2];
  }
  const unsigned int c = (f.x != 0) + (f.y != 0) + (f.z != 0) + (f.w != 0);
  const int lane = (int)(threadIdx.x % OTR_WAVE), w = (int)(threadIdx.x / OTR_WAVE);
  unsigned int incl = c;
  for (int o = 1; o < OTR_WAVE; o <<= 1) {
    const unsigned int v = (unsigned int)__shfl_up((int)incl, o);
    if (lane >= o) incl += v;
  }
  if (lane == OTR_WAVE - 1) s_wave[w] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int t = 0;
    for (int k = 0; k < kFlaggedBlock / OTR_WAVE; ++k) {
      const unsigned int x = s_wave[k];
      s_wave[k] = t;
      t += x;
    }
    s_base = t ? atomicAdd(count, (unsigned long long)t) : 0ull;
  }
  __syncthreads();
  if (c == 0) return;
  int64_t o = (int64_t)s_base + s_wave[w] + (incl - c);
  if (f.x != 0) list[o++] = i0;
  if (f.y != 0) list[o++] = i0 + 1;
  if (f.z != 0) list[o++] = i0 + 2;
  if (f.w != 0) list[o++] = i0 + 3;
}

// A retry tier's collect over the device-counted list of flagged tasks cand[0..*n_cand): it
// takes the tasks whose flag is in the bit set `want` (bit f = flag value f: otr_tiers.h
// flag_bit) and clears their flags; tasks flagged for a later tier keep theirs.  The list
// length stays on the device: the next kernel reads it there.  A fixed grid strides over
// the list (block-uniform trip count: block_append synchronises the block)
__global__ void k_collect_tier_from(const int64_t* cand, const unsigned long long* n_cand, int32_t* flag,
                                    uint32_t want, int64_t* list, unsigned long long* count) {
  const int64_t n = (int64_t)*n_cand;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = base + threadIdx.x;
    const int64_t task = i < n ? cand[i] : 0;
    const int f = i < n ? flag[task] : 0;
    const bool sel = f != 0 && ((want >> f) & 1u);
    if (sel) flag[task] = 0;
    block_append(sel, task, list, count);
  }
}

// Spatial order of a retry list (the edge-state tier's 15.7M tasks at C2, deployed): a
// counting sort by the root's id >> shift (4,096 buckets; graph ids are spatially ordered,
// so a bucket is a small patch of the map).  The list tiers split their list into 8
// contiguous ranges, one per XCD (XcdQueue): sorted, each XCD's waves search one band of
// the map and its 4 MB L2 holds that band's records instead of the whole graph's.  Pass 1
// counts (LDS histogram per block, then one global add per non-empty bucket), pass 2 scans
// the 4,096 counts, pass 3 places each task (local rank by LDS atomic + the block's range
// reserved per bucket).  Order inside a bucket is arbitrary: tasks are independent.
constexpr int kSortBuckets = 4096;
__global__ __launch_bounds__(1024) void k_sort_hist(const int64_t* list, const unsigned long long* n_in,
                                                    const uint4* rec, int shift, uint32_t* hist) {
  __shared__ uint32_t h[kSortBuckets];
  const int64_t n = (int64_t)*n_in, i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if ((int64_t)blockIdx.x * blockDim.x >= n) return;  // (block-uniform)
  for (int b = threadIdx.x; b < kSortBuckets; b += blockDim.x) h[b] = 0;
  __syncthreads();
  if (i < n) atomicAdd(&h[min(rec[3 * list[i]].z >> shift, (uint32_t)kSortBuckets - 1u)], 1u);
  __syncthreads();
  for (int b = threadIdx.x; b < kSortBuckets; b += blockDim.x)
    if (h[b]) atomicAdd(&hist[b], h[b]);
}
__global__ __launch_bounds__(1024) void k_sort_scan(uint32_t* hist) {  // one block: exclusive scan in place
  __shared__ uint32_t part[1024];
  constexpr int per = kSortBuckets / 1024;
  uint32_t v[per], t = 0;
  for (int q = 0; q < per; ++q) t += (v[q] = hist[threadIdx.x * per + q]);
  part[threadIdx.x] = t;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan of the block sums
    const uint32_t x = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0u;
    __syncthreads();
    part[threadIdx.x] += x;
    __syncthreads();
  }
  uint32_t base = part[threadIdx.x] - t;
  for (int q = 0; q < per; ++q) {
    hist[threadIdx.x * per + q] = base;
    base += v[q];
  }
}
__global__ __launch_bounds__(1024) void k_sort_place(const int64_t* list, const unsigned long long* n_in,
                                                     const uint4* rec, int shift, uint32_t* cursor, int64_t* out) {
  __shared__ uint32_t h[kSortBuckets];
  const int64_t n = (int64_t)*n_in, i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if ((int64_t)blockIdx.x * blockDim.x >= n) return;
  for (int b = threadIdx.x; b < kSortBuckets; b += blockDim.x) h[b] = 0;
  __syncthreads();
  int64_t task = 0;
  uint32_t key = 0, r = 0;
  if (i < n) {
    task = list[i];
    key = min(rec[3 * task].z >> shift, (uint32_t)kSortBuckets - 1u);
    r = atomicAdd(&h[key], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kSortBuckets; b += blockDim.x)
    if (h[b]) h[b] = atomicAdd(&cursor[b], h[b]);  // this block's range of bucket b
  __syncthreads();
  if (i < n) out[h[key] + r] = task;
}

// the same over a device-counted list (steps of the path stage): entries list_in[0..*n_in)
__global__ void k_collect_tier_list(const unsigned long long* n_in, int32_t* flag, uint32_t want, int64_t* list,
                                    unsigned long long* count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int f = i < (int64_t)*n_in ? flag[i] : 0;
  const bool sel = f != 0 && ((want >> f) & 1u);
  if (sel) flag[i] = 0;
  block_append(sel, i, list, count);
}

// states that need a path: a step inside a sub-path.  The step flags ovf[0, n_states] (one per
// list position, fewer than states) are zeroed here, so the path stage's first attempt fills nothing.
__global__ void k_step_list(int64_t n_states, const int64_t* prev, const uint8_t* brk, const int32_t* cand_count,
                            int64_t* list, unsigned long long* count, int32_t* ovf) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n_states) ovf[s] = 0;
  if (s == 0) ovf[n_states] = 0;
  block_append(s < n_states && cand_count[s] > 0 && prev[s] >= 0 && !brk[s], s, list, count);
}

// the same steps in two lists within list[0, n_states): the small-search path tier's from
// the front (count_front), the rest from the back (count_back); *n_all = n_states (the
// retry collects scan the whole index range, whose gap keeps its zero flags)
__global__ void k_step_lists(int64_t n_states, const int64_t* prev, const uint8_t* brk, const int32_t* cand_count,
                             PathClass pc, int64_t* list, unsigned long long* count_front,
                             unsigned long long* count_back, unsigned long long* n_all, int32_t* ovf) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s == 0) *n_all = (unsigned long long)n_states;
  // (the step flags of every index, the gap between the two lists included: k_step_list)
  if (s < n_states) ovf[s] = 0;
  if (s == 0) ovf[n_states] = 0;
  const bool hit = s < n_states && cand_count[s] > 0 && prev[s] >= 0 && !brk[s];
  bool small = false;
  if (hit) {
    const int64_t sp = prev[s];
    const int md = pc.mode[pc.state_trace[s]] < OTR_MODES ? pc.mode[pc.state_trace[s]] : 0;
    const uint32_t r = pc.trans[pc.trans_off[s] + (int64_t)pc.winner[sp] * cand_count[s] + pc.winner[s]];
    const double b = fmin(floor(pc.bound[s] * 1000.0), (double)r) * 1e-3;  // (k_paths' bound, m)
    small = !((pc.turn_modes >> md) & 1u) && pc.est4 * (float)(b * b) <= pc.small_keys;
  }
  // one atomic per wave and list
  const unsigned long long mf = __ballot(hit && small), mb = __ballot(hit && !small);
  const int lane = (int)(threadIdx.x % OTR_WAVE);
  unsigned long long bf = 0, bb = 0;
  if (lane == 0) {
    if (mf) bf = atomicAdd(count_front, (unsigned long long)__popcll(mf));
    if (mb) bb = atomicAdd(count_back, (unsigned long long)__popcll(mb));
  }
  bf = __shfl(bf, 0);
  bb = __shfl(bb, 0);
  const unsigned long long below = (1ull << lane) - 1ull;
  if (hit && small) list[bf + __popcll(mf & below)] = s;
  if (hit && !small) list[n_states - 1 - (int64_t)(bb + __popcll(mb & below))] = s;
}

// work counters: fold the kCShards shards of every (bank, kind) into one value before the
// copy-out (one block of kCShards threads per pair)
__global__ __launch_bounds__(kCShards) void k_ctr_fold(const unsigned long long* in, unsigned long long* out) {
  __shared__ unsigned long long part[kCShards / OTR_WAVE];
  unsigned long long v = in[(size_t)blockIdx.x * kCShards + threadIdx.x];
  for (int o = OTR_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if (lane_id() == 0) part[threadIdx.x / OTR_WAVE] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < kCShards / OTR_WAVE; ++w) t += part[w];
    out[blockIdx.x] = t;
  }
}

// the small-search tier's default size limit (keys of k_ntask's estimate; OTR_SMALL_KEYS)
constexpr double kSmallKeys = 24.0;
// the tiny-search tier's (eight searches per wave, at most 8 targets; OTR_TINY_KEYS)
constexpr double kTinyKeys = 12.0;
// the small-search path tier's (keys of k_step_lists' estimate; OTR_SMALL_PATH_KEYS)
constexpr double kSmallPathKeys = 16.0;

// the node retry tiers of this process (otr_tiers.h; OTR_TIERS: A/B knob)
static const std::vector<int>& route_tiers() {
  static const std::vector<int> t = parse_route_tiers(getenv("OTR_TIERS"));
  return t;
}

// a persistent grid (work queues or a grid stride over a device-side list) of at most
// `full` blocks, but never more than the list can hold (`units`, known on the host: tasks
// or steps): a small batch does not launch thousands of workgroups that find nothing
static unsigned pgrid(unsigned full, int64_t units) {
  const int64_t u = std::max<int64_t>(8, (units + 7) / 8 * 8);
  return (unsigned)std::min<int64_t>((int64_t)full, u);
}

constexpr unsigned kCollectGrid = 512;  // blocks of a collect over the flagged tasks (a grid stride)

// words rounded up to whole 256 B lines (the parts of a batch's control block)
static constexpr size_t line(size_t words) { return (words + 31) / 32 * 32; }

// One batch on its way through the pipeline: what the stages share, and the stages in the
// order Matcher::run calls them.  A stage returns OTR_OK or the code the batch ends with.
struct Batch {
  Matcher& mat;
  const otr_trace_batch* in;
  const ModeParams& mp;
  otr_batch_result* out;
  std::string* err;
  const DevGraph& g;
  hipStream_t stream;
  bool timing;
  bool used[10] = {false};
  // traces, probes, states, tasks (NT: every task; [0, NT8) the tiny tier's, [NT8, NT8 + NT4)
  // the small tier's), transition entries, the capacity layout's entries
  int32_t T = 0;
  int64_t N = 0, S = 0, NT = 0, NT4 = 0, NT8 = 0, NTR = 0, C = 0;
  BatchDev b{};
  CandBuf cb{};
  StepBuf sb{};
  PrepArgs pr{};
  RouteArgs ra{};
  GenArgs ga{};
  ViterbiArgs va{};
  SegArgs sa{};
  HistArgs ha{};
  PointArgs pta{};  // K12, with OTR_BATCH_MATCHED_POINTS
  bool want_points = false;
  TravArgs tva{};  // K13, with OTR_BATCH_EDGE_TRAVERSALS
  bool want_traversals = false;
  int64_t n_trav = 0;
  size_t hist_len = 0, scan_bytes = 0;
  int64_t *trace_state_off = nullptr, *state_probe = nullptr, *trans_off = nullptr, *path_off = nullptr,
          *cap_off = nullptr;
  int32_t *state_trace = nullptr, *path_len = nullptr;
  uint32_t turn_modes = 0;  // modes whose searches carry turn costs (edge-based, k_general)
  bool k32 = true;          // no mode keeps more than 32 candidates (K <= 32 lanes)
  int vit_variant = 0;      // the k_viterbi instance viterbi() launched (otr.h: OTR_VITERBI_VARIANT)
  // the first tiers' size estimate (link())
  int route_g = 2, n_est_tiers = 0;
  float est_k = 0.f, est_v[OTR_MODES] = {};
  uint32_t est_tier_keys[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  double tiny_keys = 0.0;
  // work counters (kBanks banks of OTR_COUNTERS kinds x kCShards, folded at the end into
  // n_ctr values behind them) and list counters (otr_tiers.h CntWord)
  static constexpr size_t bank = (size_t)OTR_COUNTERS * kCShards;
  static constexpr size_t n_ctr = kBanks * (size_t)OTR_COUNTERS;
  // The batch's control block, one buffer zeroed by ONE fill at batch start (upload()): the work
  // counter banks, their folded values, the list counters and path cursors (cnt), the route
  // tiers' work queues and the path tiers' (pq); each part starts on a 256 B line.  Only a
  // repeated path attempt clears its own words again (paths_attempt).
  static constexpr int kPQWords = 16 * 8;
  static constexpr size_t kCntAt = line(kBanks * bank + n_ctr);
  static constexpr size_t kQueuesAt = kCntAt + line(C_CURSORS + kShards);
  static constexpr size_t kPQAt = kQueuesAt + line((size_t)kQueues * kQueueWords);
  static constexpr size_t kControlWords = kPQAt + line(kPathQueues * kPQWords);
  unsigned long long *d_counters = nullptr, *cnt = nullptr, *pq = nullptr;
  int64_t *list = nullptr, *fail_tasks = nullptr, *flagged = nullptr;
  int32_t *task_ovf = nullptr, *d_turn = nullptr;
  uint32_t *trans = nullptr, *trans_tc = nullptr;
  uint4* task_rec = nullptr;
  // the route stages
  unsigned long long *rwork = nullptr, *queues = nullptr;
  int32_t* task_dump = nullptr;
  bool node_tasks = true, turns = false, nresume = true, eresume = true;
  // the path stage's step lists: the list's length (the back list's with two lists: small_paths), the
  // front list's, the retry collects' index range; the (front, back) lengths on the host
  int64_t* steps = nullptr;
  unsigned long long *nsteps_d = nullptr, *nsteps4_d = nullptr, h_nsteps[2] = {0ull, 0ull};
  const unsigned long long* nscan_d = nullptr;
  int32_t* step_ovf = nullptr;
  bool small_paths = false;
  int64_t* cap = nullptr;  // per-trace output capacity (k_capacity, queued behind every path attempt)
  int path_attempts = 0;
  // what drain() brought back (the matcher's pinned drain buffer)
  const unsigned long long* hc = nullptr;
  unsigned long long h_fail[2] = {0ull, 0ull};  // route tasks / paths beyond every search tier
  const int64_t *route_n = nullptr, *seg_n = nullptr, *way_n = nullptr, *rep_n = nullptr;

  // the stages, in order
  int upload(), check_probes(), states(), candidates(), link(), route_first(), route_retry(), route_edge(), route_global(), viterbi();
  int paths(), paths_attempt(int64_t capacity, bool again), segments(), points(), traversals(), drain(), debug_fail(),
      name_failed();
  void fold_counters();
  int copy_out(), points_out(), traversals_out();

  template <class X> X* need(int slot, size_t n) { return mat.need<X>(slot, n); }
  template <class X> X* want(int slot, size_t n) { return mat.want<X>(slot, n); }
  // stage k's event pair (OTR_BATCH_TIMING)
  void tb(int k) {
    if (timing) (void)hipEventRecord(mat.ev[2 * k], stream);
  }
  void te(int k) {
    if (timing) (void)hipEventRecord(mat.ev[2 * k + 1], stream), used[k] = true;
  }
  // a route tier's event pair, counter bank (when counting was asked for), list counter and queue
  void tier_begin(int slot) {
    if (timing) (void)hipEventRecord(mat.ev[route_event(slot)], stream);
  }
  void tier_end(int slot) {
    if (timing) (void)hipEventRecord(mat.ev[route_event(slot) + 1], stream);
  }
  unsigned long long* tier_bank(int slot) const { return d_counters + kRouteTiers[slot].bank * bank; }
  unsigned long long* tier_work(int slot) const { return rwork ? tier_bank(slot) : nullptr; }
  unsigned long long* tier_list(int slot) const { return cnt + kRouteTiers[slot].list; }
  unsigned long long* tier_queue(int slot) const { return queues + kRouteTiers[slot].queue * kQueueWords; }
  unsigned long long ctr(int bank_, int k) const { return hc[(size_t)bank_ * OTR_COUNTERS + (size_t)k]; }

  int scan(const int64_t* src, int64_t* dst_np1, int64_t n);
  int read_i64(const int64_t* p, int64_t* v);
  template <class... R>
  int post_wait(R... runs) {
    return mat.post_wait({runs...}, err);
  }
  int slabs(int tier, GSlabs* out);
  // A retry tier's collect: the items whose flag is in `take` (otr_tiers.h: a tier's take
  // column) go to `dst`, their number to list counter `word`, and their flags are cleared.
  // Route tasks are looked for among the flagged ones, path steps among all of them.
  enum class Chain { Route, Path };
  void collect(Chain chain, uint32_t take, int word, int64_t* dst) {
    if (chain == Chain::Route)
      k_collect_tier_from<<<kCollectGrid, 1024, 0, stream>>>(flagged, cnt + C_FLAGGED, task_ovf, take, dst, cnt + word);
    else
      k_collect_tier_list<<<grid_ceil(S, 1024), 1024, 0, stream>>>(nscan_d, step_ovf, take, dst, cnt + word);
  }
  // a route list tier's turn: its collect, and the arguments of its launch
  RouteArgs take_list(int slot) {
    collect(Chain::Route, kRouteTiers[slot].take, kRouteTiers[slot].list, list);
    RouteArgs rb = ra;
    rb.task_list = list;
    rb.list_count = tier_list(slot);
    rb.queue = tier_queue(slot);
    return rb;
  }
  template <class V>
  int dl(V& vec, const void* src, size_t n) {
    vec.resize(n ? n : 1);
    if (n) HIPCHK(hipMemcpyAsync(vec.data(), src, n * sizeof(vec[0]), hipMemcpyDeviceToHost, stream));
    return OTR_OK;
  }
  template <int CAP, int G, bool LIST>
  void launch_route(unsigned grid, const RouteArgs& args, unsigned long long* ctr_bank);
  void first_tier(int slot, int cap, int g_, int64_t n_tasks, int64_t task_base, int64_t units);
  int retry_tier(int code, const RouteArgs& rb, unsigned long long* ctr_bank);
};

int Matcher::run(const otr_trace_batch* in, const ModeParams& mp, otr_batch_result* out, std::string* err) {
  pts_have = false;  // (points() sets it once this batch's points exist)
  pts = otr_point_result{};
  trv_have = false;
  trv = otr_traversal_result{};
  const int rc = guarded(stream, err, [&]() -> int {
    GraphState& gs = graph_state();
    std::shared_lock<std::shared_mutex> graph_lock(gs.mu);  // a reconfigure waits for this batch
    if (!gs.ready) {
      if (err) *err = "otr_configure has not been called";
      return OTR_NOT_CONFIGURED;
    }
    HIPCHK(hipSetDevice(gs.device));
    if (!stream) HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    if (!ev_init) {
      for (auto& e : ev) HIPCHK(hipEventCreate(&e));
      ev_init = true;
    }
    memset(out, 0, sizeof(*out));
    out->n_traces = in->n_traces;
    if (in->n_traces <= 0) {
      pts_have = (in->flags & OTR_BATCH_MATCHED_POINTS) != 0;  // (no probe, no point)
      if (in->flags & OTR_BATCH_EDGE_TRAVERSALS) {  // (no trace, no traversal: a trace_off of one zero)
        trv.d_trace_off = need<int64_t>(S_TR_OFF, 1);
        HIPCHK(hipMemsetAsync(trv.d_trace_off, 0, 8, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (in->flags & OTR_BATCH_COPY_OUT) {
          h_tr_off.assign(1, 0);
          trv.trace_off = h_tr_off.data();
        }
        trv_have = true;
      }
      return OTR_OK;
    }
    Batch c{*this, in, mp, out, err, gs.dg, stream, (in->flags & OTR_BATCH_TIMING) != 0};
    c.T = in->n_traces;
    c.want_points = (in->flags & OTR_BATCH_MATCHED_POINTS) != 0;
    c.want_traversals = (in->flags & OTR_BATCH_EDGE_TRAVERSALS) != 0;
    int rc;
    if ((rc = c.upload()) || (rc = c.states()) || (rc = c.candidates()) || (rc = c.link()) || (rc = c.route_first()) ||
        (rc = c.route_retry()) || (rc = c.route_edge()) || (rc = c.route_global()) || (rc = c.viterbi()) ||
        (rc = c.paths()) || (rc = c.segments()) || (rc = c.points()) || (rc = c.traversals()) || (rc = c.drain()) ||
        (rc = c.debug_fail()) || (rc = c.name_failed()))
      return rc;
    c.fold_counters();
    if ((rc = c.copy_out()) || (rc = c.points_out())) return rc;
    return c.traversals_out();
  });
  opt_busy = false;  // (on both paths: an allocation failure inside ends at the guard)
  return rc;
}

// input upload (host batches), the batch-size check, the work counters
int Batch::upload() {
  b.n_traces = T;
  if (in->memory == OTR_MEM_HOST) {
    N = in->trace_offsets[T];
    int64_t* d_off = need<int64_t>(S_TRACE_OFF, T + 1);
    double* d_lat = need<double>(S_LAT, N);
    double* d_lon = need<double>(S_LON, N);
    int64_t* d_time = need<int64_t>(S_TIME, N);
    uint8_t* d_mode = need<uint8_t>(S_MODE, T);
    float* d_acc = in->accuracy ? need<float>(S_ACC, N) : nullptr;
    HIPCHK(hipMemcpyAsync(d_off, in->trace_offsets, 8 * (T + 1), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_lat, in->lat, 8 * N, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_lon, in->lon, 8 * N, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_time, in->time, 8 * N, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_mode, in->mode, T, hipMemcpyHostToDevice, stream));
    if (d_acc) HIPCHK(hipMemcpyAsync(d_acc, in->accuracy, 4 * N, hipMemcpyHostToDevice, stream));
    b.trace_off = d_off;
    b.lat = d_lat;
    b.lon = d_lon;
    b.time = d_time;
    b.mode = d_mode;
    b.acc = d_acc;
  } else {
    // (N, the last trace offset, is still on the device: it comes back with S, states())
    b.trace_off = in->trace_offsets;
    b.lat = in->lat;
    b.lon = in->lon;
    b.time = in->time;
    b.mode = in->mode;
    b.acc = in->accuracy;
  }
  mat.h_trace_status.assign(T, OTR_OK);
  d_counters = need<unsigned long long>(S_COUNTERS, kControlWords);
  cnt = d_counters + kCntAt;
  queues = d_counters + kQueuesAt;
  pq = d_counters + kPQAt;
  HIPCHK(hipMemsetAsync(d_counters, 0, kControlWords * 8, stream));
  return in->memory == OTR_MEM_HOST ? check_probes() : OTR_OK;
}

// the batch-size check, once N is known (a device batch: after K0's first pass, which launches
// by traces and reads no N)
int Batch::check_probes() {
  out->n_probes = N;
  // one wave per state / trace in the per-state and per-trace kernels: a dispatch counts
  // its work-items in 32 bits, so a batch holds at most kMaxBatchProbes = 2^26 - 64 probes
  // (otr_launch.h: the widest launch of such a batch, k_candidates at states = probes,
  // stays below 2^32; callers split larger inputs, the JSON service batches at 16M)
  if (N > kMaxBatchProbes || max_launch_items(N, N, 1) > kMaxDispatchItems) {
    if (err)
      *err = "batch of " + std::to_string(N) + " probes: at most " + std::to_string(kMaxBatchProbes) +
             " per otr_match_batch call";
    return OTR_BAD_REQUEST;
  }
  return OTR_OK;
}

// dst[0] = 0, dst[1..n] = inclusive prefix sums: one inclusive sum over the n + 1 values
// 0, src[0], .., src[n - 1] (otr_devscan.h shifted_input), so the leading zero needs no fill
int Batch::scan(const int64_t* src, int64_t* dst_np1, int64_t n) {
  const auto in0 = shifted_input(src);
  Workspace tmp;
  if (int rc = otr::scan_bytes(in0, dst_np1, (int)n + 1, &tmp.bytes, stream, err)) return rc;
  scan_bytes = std::max(scan_bytes, tmp.bytes);  // (the slot keeps the batch's largest)
  tmp.p = need<char>(S_SCAN_TMP, scan_bytes);
  return inclusive_sum(tmp, in0, dst_np1, (int)n + 1, stream, err);
}

// one word through the mailbox
int Batch::read_i64(const int64_t* p, int64_t* v) {
  if (int rc = post_wait(Matcher::MailRun{p, 1})) return rc;
  *v = (int64_t)mat.mail[0];
  return OTR_OK;
}

// ---- K0: states
int Batch::states() {
  int rc;
  int64_t* state_cnt = need<int64_t>(S_STATE_CNT, T);
  trace_state_off = need<int64_t>(S_TRACE_STATE_OFF, T + 1);
  tb(OTR_STAGE_STATES);
  k_select_states<<<grid_ceil(T, 256), 256, 0, stream>>>(b, mp, state_cnt, nullptr, nullptr, nullptr);
  te(OTR_STAGE_STATES);
  if ((rc = scan(state_cnt, trace_state_off, T))) return rc;
  if (in->memory == OTR_MEM_HOST) {
    if ((rc = read_i64(trace_state_off + T, &S))) return rc;
  } else {  // a device batch: its probe count rides along
    if ((rc = post_wait(Matcher::MailRun{trace_state_off + T, 1}, Matcher::MailRun{in->trace_offsets + T, 1}))) return rc;
    S = (int64_t)mat.mail[0];
    N = (int64_t)mat.mail[1];
    if ((rc = check_probes())) return rc;
  }
  out->n_states = S;
  state_probe = need<int64_t>(S_STATE_PROBE, S);
  state_trace = need<int32_t>(S_STATE_TRACE, S);
  k_select_states<<<grid_ceil(T, 256), 256, 0, stream>>>(b, mp, state_cnt, trace_state_off, state_probe,
                                                         state_trace);
  return OTR_OK;
}

// ---- K1: candidates
int Batch::candidates() {
  cb.edge = need<uint32_t>(S_CAND_EDGE, (size_t)S * OTR_KMAX);
  cb.p = need<double>(S_CAND_P, (size_t)S * OTR_KMAX);
  cb.sqd = need<double>(S_CAND_SQD, (size_t)S * OTR_KMAX);
  cb.count = need<int32_t>(S_CAND_COUNT, S);
  cb.radius = need<double>(S_CAND_RADIUS, S);
  if (S > 0) {
    tb(OTR_STAGE_CANDIDATES);
    // two states per wave when no mode keeps more than 32 candidates (lane groups of 32) and
    // no search radius can exceed 100 m (windows of a few cells: C2 1.86 -> 1.72 ms, C5 16.1
    // -> 11.8 ms; C4's 200 m windows take 15.9 -> 22.1 ms with half the lanes each, so they
    // keep a wave per state).  A probe's radius is min(max_search_radius, max(search_radius,
    // accuracy)): without per-probe accuracies the mode's gps_accuracy stands for it.
    bool kc32 = true;
    for (int m = 0; m < OTR_MODES; ++m) {
      const MatchParams& q = mp.m[m];
      const double rmax = b.acc ? q.max_search_radius
                                : std::min(q.max_search_radius, std::max(q.search_radius, q.gps_accuracy));
      kc32 = kc32 && q.kmax <= 32 && rmax <= 100.0;
    }
    static const int cand_g = getenv("OTR_CAND_G") ? atoi(getenv("OTR_CAND_G")) : 2;  // A/B knob
    if (kc32 && cand_g == 2)
      k_candidates<2><<<(unsigned)grid_candidates((S + 1) / 2).blocks, 64, 0, stream>>>(g, b, mp, S, state_probe,
                                                                                       state_trace, cb, d_counters);
    else
      k_candidates<1><<<(unsigned)grid_candidates(S).blocks, 64, 0, stream>>>(g, b, mp, S, state_probe, state_trace, cb,
                                                                        d_counters);
    te(OTR_STAGE_CANDIDATES);
  }
  return OTR_OK;
}

// ---- K_link + task map: link, per-state search inputs, the first tiers' size estimate, task
// counts and records (K_link, K2b, K2, K2c)
int Batch::link() {
  int rc;
  for (int m = 0; m < OTR_MODES; ++m)
    if (mp.m[m].turn_penalty_factor > 0.0) turn_modes |= 1u << m;
  sb.prev = need<int64_t>(S_PREV, S);
  sb.g = need<double>(S_G, S);
  sb.bound = need<double>(S_BOUND, S);
  sb.forced = need<uint8_t>(S_FORCED, S);
  sb.bt = need<int32_t>(S_BT, S);
  sb.ntask = need<int64_t>(S_NTASK, S);
  sb.ntrans = need<int64_t>(S_NTRANS, S);
  int64_t* task_off = need<int64_t>(S_TASK_OFF, S + 1);
  trans_off = need<int64_t>(S_TRANS_OFF, S + 1);
  tb(OTR_STAGE_LINK);  // (K_link, the search inputs and the task records: through k_tasks)
  k_link<<<(unsigned)grid_link(T).blocks, 256, 0, stream>>>(b, mp, trace_state_off, state_probe, cb.count, sb);
  // K2b: per-state search inputs
  pr.n_states = S;
  pr.prev = sb.prev;
  pr.bound = sb.bound;
  pr.cand_count = cb.count;
  pr.cand_edge = cb.edge;
  pr.cand_p = cb.p;
  pr.state_trace = state_trace;
  pr.mode = b.mode;
  pr.cprep = need<uint4>(S_CPREP, (size_t)S * OTR_KMAX);
  pr.cprep_t = need<uint2>(S_CPREP_T, (size_t)S * OTR_KMAX);
  pr.clen = need<uint2>(S_CLEN, (size_t)S * OTR_KMAX);
  pr.nroot = need<int32_t>(S_CAND_NROOT, S);
  pr.turn_modes = turn_modes;
  // two states per wave when no mode keeps more than 32 candidates (K <= 32 lanes)
  for (int m = 0; m < OTR_MODES; ++m) k32 = k32 && mp.m[m].kmax <= 32;
  if (S > 0) {
    if (k32) k_prep<2><<<(unsigned)grid_per_state_waves(S, 2).blocks, 256, 0, stream>>>(g, pr);
    else k_prep<1><<<(unsigned)grid_per_state_waves(S, 1).blocks, 256, 0, stream>>>(g, pr);
  }
  // the first tier's size estimate (k_ntask, k_tasks, for route_unit): an exact search runs
  // to its bounds unless its targets resolve first, so its keys grow with the area it can
  // reach, est = c * density * reach^2, reach = min(length bound, time bound x 50 km/h
  // capped by the mode's speed).  A search whose estimate exceeds the first tier's table
  // starts in the retry tier that holds it: k_tasks flags it and the first tier passes it
  // on without loading its step.  c = 0.5 (C4's 60 s steps reach ~1.7 km and start in the
  // 1024-slot tier: C4 1.69M -> 2.47M probes/s; c = 1.7, the full-exhaustion fit of C2,
  // sent them to the 4096 tier, 1.07M; C2's 15 s steps stay in the first tier either way,
  // profiles/r03_est_*).  OTR_EST_K scales c (A/B knob; 0 = every search starts in the
  // first tier).  A step whose estimate is at most OTR_SMALL_KEYS keys (and has at most
  // 16 targets) goes to the small-search tier, four searches per wave (k_ntask).
  static const int route_g_env = getenv("OTR_ROUTE_G") ? atoi(getenv("OTR_ROUTE_G")) : 2;  // A/B knob
  route_g = route_g_env;
  {
    static const double est_scale = getenv("OTR_EST_K") ? atof(getenv("OTR_EST_K")) : 1.0;
    const double mlat = g.grid_min_lat + 0.5 * g.grid_rows * g.grid_cell_deg;
    const double area = (g.grid_rows * g.grid_cell_deg * kMetersPerDeg) *
                        (g.grid_cols * g.grid_cell_deg * kMetersPerDeg * cos_deg(fmin(fabs(mlat), 89.0)));
    est_k = (float)(est_scale * 0.5 * (area > 0.0 ? (double)g.n_nodes / area : 0.0));
    for (int m = 0; m < OTR_MODES; ++m) {
      const double kph = mp.m[m].speed_kph > 0.0 && mp.m[m].speed_kph < 50.0 ? mp.m[m].speed_kph : 50.0;
      est_v[m] = (float)(kph / 3.6);
    }
    const std::vector<int>& tl = route_tiers();
    n_est_tiers = (int)std::min<size_t>(tl.size(), 8);
    for (int t = 0; t < n_est_tiers; ++t) est_tier_keys[t] = (uint32_t)((tl[t] / 10) * 7 / 8);
  }
  static const double small_keys = getenv("OTR_SMALL_KEYS") ? atof(getenv("OTR_SMALL_KEYS")) : kSmallKeys;  // A/B knob
  static const double tiny_keys_env = getenv("OTR_TINY_KEYS") ? atof(getenv("OTR_TINY_KEYS")) : kTinyKeys;  // A/B knob
  tiny_keys = tiny_keys_env;
  const bool small_tier = route_g == 2 && k32 && small_keys > 0.0 && est_k > 0.f;
  const bool tiny_tier = small_tier && tiny_keys > 0.0;
  int64_t* ntask4 = small_tier ? need<int64_t>(S_NTASK4, S) : nullptr;
  int64_t* task4_off = small_tier ? need<int64_t>(S_TASK4_OFF, S + 1) : nullptr;
  int64_t* ntask8 = tiny_tier ? need<int64_t>(S_NTASK8, S) : nullptr;
  int64_t* task8_off = tiny_tier ? need<int64_t>(S_TASK8_OFF, S + 1) : nullptr;
  // the step's task count: the distinct roots (k_prep) of the previous state's candidates
  if (S > 0) {
    SmallArgs sm{};
    sm.ntask4 = ntask4;
    sm.ntask8 = ntask8;
    sm.tiny_keys = (float)tiny_keys;
    sm.bound = sb.bound;
    sm.bt = sb.bt;
    sm.forced = sb.forced;
    sm.cand_count = cb.count;
    sm.state_trace = state_trace;
    sm.mode = b.mode;
    sm.turn_modes = turn_modes;
    sm.est_k = est_k;
    for (int m = 0; m < OTR_MODES; ++m) sm.est_v[m] = est_v[m];
    sm.small_keys = (float)small_keys;
    k_ntask<<<grid_ceil(S, 256), 256, 0, stream>>>(S, sb.prev, pr.nroot, sb.ntask, sm);
  }
  // the four offset arrays in one scan over the 4-tuple (otr_devscan.h tuple_sums), each
  // behind its leading zero: S + 1 tuples, the totals in element S
  {
    const ArrayColumns<4, true> cols{{sb.ntask, sb.ntrans, ntask4, ntask8}};
    int64_t* const offs[4] = {task_off, trans_off, task4_off, task8_off};
    Workspace tmp;
    if ((rc = tuple_sums<4>(&tmp, cols, offs, (int)S + 1, stream, err))) return rc;
    scan_bytes = std::max(scan_bytes, tmp.bytes);
    tmp.p = need<char>(S_SCAN_TMP, scan_bytes);
    if ((rc = tuple_sums<4>(&tmp, cols, offs, (int)S + 1, stream, err))) return rc;
  }
  // the four totals in one mailbox record (a tier that is off: no word, its count stays 0)
  if ((rc = post_wait(Matcher::MailRun{task_off + S, 1}, Matcher::MailRun{trans_off + S, 1},
                      Matcher::MailRun{small_tier ? task4_off + S : nullptr, small_tier ? 1 : 0},
                      Matcher::MailRun{tiny_tier ? task8_off + S : nullptr, tiny_tier ? 1 : 0})))
    return rc;
  NT = (int64_t)mat.mail[0];
  NTR = (int64_t)mat.mail[1];
  if (small_tier) NT4 = (int64_t)mat.mail[2];
  if (tiny_tier) NT8 = (int64_t)mat.mail[3];  // (the tiny tier needs the small one: word 3)
  NT += NT4 + NT8;
  task_ovf = need<int32_t>(S_TASK_OVF, NT);
  trans = need<uint32_t>(S_TRANS, NTR);
  trans_tc = need<uint32_t>(S_TRANS_TC, turn_modes ? NTR : 1);  // read for turn modes only
  task_rec = need<uint4>(S_TASK_REC, 3 * (size_t)std::max<int64_t>(NT, 1));
  if (S > 0) {  // tasks and their records (K2 + K2c)
    TaskArgs ta{};
    ta.n_states = S;
    ta.prev = sb.prev;
    ta.cand_count = cb.count;
    ta.cand_edge = cb.edge;
    ta.edge_dst = g.edge_dst;
    ta.task_off = task_off;
    ta.bound = sb.bound;
    ta.forced = sb.forced;
    ta.bt = sb.bt;
    ta.state_trace = state_trace;
    ta.mode = b.mode;
    ta.cprep = pr.cprep;
    ta.cprep_t = pr.cprep_t;
    ta.trans_off = trans_off;
    ta.turn_modes = turn_modes;
    ta.rec = task_rec;
    ta.ntask4 = ntask4;
    ta.task4_off = task4_off;
    ta.nt4 = NT4;
    ta.ntask8 = ntask8;
    ta.task8_off = task8_off;
    ta.nt8 = NT8;
    ta.flag_turn = task_ovf;  // turn-mode tasks start in the first edge-state tier (RF_EDGE_FIRST)
    // the two-search first tier's table: a step expected beyond it is flagged here
    ta.est_first_keys = route_g == 2 ? (OTR_CAP1 * OTR_LOAD1) / 8 : 0;
    ta.est_k = est_k;
    for (int m = 0; m < OTR_MODES; ++m) ta.est_v[m] = est_v[m];
    ta.n_tiers = n_est_tiers;
    for (int t = 0; t < n_est_tiers; ++t) ta.tier_keys[t] = est_tier_keys[t];
    // (no fill of task_ovf: every task's representative stores its flag, 0 or 5, with its
    // record.  OTR_DEBUG_TASKS checks that on the host: a pattern no flag takes goes in first
    // and none of it may be left)
    static const bool debug_tasks = getenv("OTR_DEBUG_TASKS") != nullptr;
    if (debug_tasks && NT > 0) HIPCHK(hipMemsetAsync(task_ovf, 0x7F, 4 * NT, stream));
    if (k32) k_tasks<2><<<(unsigned)grid_per_state_waves(S, 2).blocks, 256, 0, stream>>>(ta);
    else k_tasks<1><<<(unsigned)grid_per_state_waves(S, 1).blocks, 256, 0, stream>>>(ta);
    if (debug_tasks && NT > 0) {
      std::vector<int32_t> h((size_t)NT);
      HIPCHK(hipMemcpyAsync(h.data(), task_ovf, 4 * NT, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      const int64_t written = NT - std::count(h.begin(), h.end(), 0x7F7F7F7F);
      if (written != NT) {
        if (err) *err = "k_tasks wrote " + std::to_string(written) + " of " + std::to_string(NT) + " task flags";
        return OTR_DEVICE_ERROR;
      }
    }
  }
  te(OTR_STAGE_LINK);
  return OTR_OK;
}

// general (global-memory) search slabs: allocated on first use, cleared once
int Batch::slabs(int tier, GSlabs* out) {
  GSlab& sl = mat.gslab[tier];
  const uint32_t cap = (uint32_t)kRouteTiers[SLOT_GLOBAL + tier].cap;
  const uint32_t n = tier == 0 ? 1024u : 8u;
  if (!sl.key) {
    // all five arrays or none: a partial set is freed and the batch fails with
    // OTR_DEVICE_ERROR (a later batch never sees a half-allocated slab)
    const size_t c = (size_t)cap * n;
    void* p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t bytes[5] = {4 * c, 8 * c, 4 * c, 8 * c, 4 * c};
    bool good = true;
    for (int attempt = 0; attempt < 2; ++attempt) {
      good = true;
      for (int q = 0; q < 5 && good; ++q) good = hipMalloc(&p[q], bytes[q]) == hipSuccess;
      if (good) break;
      (void)hipGetLastError();
      for (void*& q : p)
        if (q) (void)hipFree(q), q = nullptr;
      if (attempt > 0 || !mat.release_optional()) break;  // (the optional workspace gone: once more)
    }
    if (good)
      good = hipMemsetAsync(p[0], 0xFF, 4 * c, stream) == hipSuccess &&
             hipMemsetAsync(p[1], 0xFF, 8 * c, stream) == hipSuccess &&
             hipMemsetAsync(p[2], 0, 4 * c, stream) == hipSuccess;
    if (!good) {
      (void)hipGetLastError();
      for (void* q : p)
        if (q) (void)hipFree(q);
      throw DeviceOom{PoolOwner::matcher, nullptr, S_NUM + tier, 28 * c};  // (the global-search slabs of this tier)
    }
    sl.key = (uint32_t*)p[0];
    sl.lab = (unsigned long long*)p[1];
    sl.qmark = (uint32_t*)p[2];
    sl.fr = (uint32_t*)p[3];
    sl.touched = (uint32_t*)p[4];
  }
  out->key = sl.key;
  out->lab = sl.lab;
  out->qmark = sl.qmark;
  out->fr = sl.fr;
  out->touched = sl.touched;
  out->cap = cap;
  out->n = n;
  return OTR_OK;
}

// the LDS route kernels: with the work counters (CNT) only when counting was asked for
template <int CAP, int G, bool LIST>
void Batch::launch_route(unsigned grid, const RouteArgs& args, unsigned long long* ctr_bank) {
  if (ctr_bank) k_route<CAP, G, LIST, false, true><<<grid, 64, 0, stream>>>(g, args, ctr_bank);
  else k_route<CAP, G, LIST, false, false><<<grid, 64, 0, stream>>>(g, args, nullptr);
}

// One of the first tiers (tiny, small, two-search): tasks [task_base, n_tasks) in `units` of
// g searches, one unit per block, in launches of at most 2^25 blocks: a dispatch's grid size
// counts work-items in 32 bits (178M tasks at 12.5M probes would wrap).
// (a block per unit: a persistent grid over per-XCD queues was slower, C5 26.5 -> 35.6 ms,
// DESIGN.md §6)
void Batch::first_tier(int slot, int cap, int g_, int64_t n_tasks, int64_t task_base, int64_t units) {
  constexpr int64_t kMaxUnits = 1ll << 25;
  unsigned long long* ctr_bank = tier_work(slot);
  // (the two-search tier's time is the route stage's less the other two tiers')
  if (slot != SLOT_FIRST) tier_begin(slot);
  for (int64_t base = 0; base < units; base += kMaxUnits) {
    RouteArgs rf = ra;
    rf.n_tasks = n_tasks;
    rf.task_base = task_base;
    rf.unit_base = base;
    const int64_t u = std::min<int64_t>(kMaxUnits, units - base);
    const unsigned grid = (unsigned)(8 * ((u + 7) / 8));
    if (slot == SLOT_TINY) launch_route<OTR_CAP8, 8, false>(grid, rf, ctr_bank);
    else if (slot == SLOT_SMALL) launch_route<OTR_CAP4, 4, false>(grid, rf, ctr_bank);
    else if (g_ == 2) launch_route<OTR_CAP1, 2, false>(grid, rf, ctr_bank);
    else launch_route<256, 1, false>(grid, rf, ctr_bank);
  }
  if (slot != SLOT_FIRST) tier_end(slot);
  out->route_tier_code[slot] = route_tier_code(slot, cap, g_);
}

// f(std::integral_constant<int, i>) for the row i of a table of N rows: how a tier picks the
// kernel instance of its row (a table size is a template argument); false: no such row
template <int N, int I = 0, class F>
static bool with_row(int i, F&& f) {
  if constexpr (I < N) {
    if (i == I) {
      f(std::integral_constant<int, I>{});
      return true;
    }
    return with_row<N, I + 1>(i, f);
  } else {
    return false;
  }
}

// a node retry tier's kernel by its code (otr_tiers.h kRetryShapes: every code OTR_TIERS
// accepts has its kernel here)
int Batch::retry_tier(int code, const RouteArgs& rb, unsigned long long* ctr_bank) {
  int row = 0;
  while (row < kRetryShapeN && kRetryShapes[row].code() != code) ++row;
  const bool known = with_row<kRetryShapeN>(row, [&](auto i) {
    constexpr int cap = kRetryShapes[decltype(i)::value].cap, gw = kRetryShapes[decltype(i)::value].g;
    // persistent grids over per-XCD queues: about twice a tier's resident waves (256 CUs x
    // 4 SIMDs x 8 waves for the small tables, fewer for the big ones, whose LDS admits
    // fewer); a block that finds its queue drained exits at once
    launch_route<cap, gw, true>(pgrid(cap <= 512 ? 16384u : 16384u * 512u / cap, (NT + gw - 1) / gw), rb, ctr_bank);
  });
  if (!known) {
    if (err) *err = "no route kernel for retry tier " + std::to_string(code);
    return OTR_DEVICE_ERROR;
  }
  return OTR_OK;
}

// ---- K3/K4: routing + transition costs, the first tiers
int Batch::route_first() {
  // turn cost tables of this batch's parameters (oracle orc_turn_table)
  // (uploaded only when the parameters or the buffer changed since this matcher's last batch:
  // the copy is queued from mat.h_turn, which no later batch touches unless it differs)
  d_turn = need<int32_t>(S_TURN, 181 * OTR_MODES);
  {
    int32_t tab[181 * OTR_MODES];
    for (int m = 0; m < OTR_MODES; ++m) turn_table(mp.m[m].turn_penalty_factor, tab + 181 * m);
    if (mat.turn_dev != d_turn || mat.h_turn.size() != (size_t)(181 * OTR_MODES) ||
        memcmp(mat.h_turn.data(), tab, sizeof(tab)) != 0) {
      mat.turn_dev = nullptr;  // (until the copy is queued)
      HIPCHK(hipStreamSynchronize(stream));  // (an earlier copy may still read h_turn)
      mat.h_turn.assign(tab, tab + 181 * OTR_MODES);
      HIPCHK(hipMemcpyAsync(d_turn, mat.h_turn.data(), sizeof(tab), hipMemcpyHostToDevice, stream));
      mat.turn_dev = d_turn;
    }
  }
  ra.task_list = nullptr;
  ra.n_tasks = NT;
  ra.prev = sb.prev;
  ra.g = sb.g;
  ra.bound = sb.bound;
  ra.forced = sb.forced;
  ra.trans_off = trans_off;
  ra.trans = trans;
  ra.cand_count = cb.count;
  ra.cand_edge = cb.edge;
  ra.cand_p = cb.p;
  ra.state_trace = state_trace;
  ra.mode = b.mode;
  ra.bt = sb.bt;
  ra.turn = d_turn;
  ra.trans_tc = trans_tc;
  ra.cprep = pr.cprep;
  ra.cprep_t = pr.cprep_t;
  ra.clen = pr.clen;
  ra.rec = task_rec;
  for (int m = 0; m < OTR_MODES; ++m) ra.inv_beta[m] = mp.m[m].inv_beta;
  ra.overflow_flag = task_ovf;
  ra.stamps = d_counters;
  ra.est_k = est_k;
  for (int m = 0; m < OTR_MODES; ++m) ra.est_v[m] = est_v[m];
  ra.n_tiers = n_est_tiers;
  for (int t = 0; t < n_est_tiers; ++t) ra.tier_keys[t] = est_tier_keys[t];
  // (the device-side counters of the retry lists, otr_tiers.h CntWord, and the path bump
  // cursors behind them: cnt, in the control block, zero since upload())
  list = need<int64_t>(S_LIST, std::max<int64_t>(NT, S));
  fail_tasks = need<int64_t>(S_GFLAG, std::max<int64_t>(NT, 1));
  flagged = need<int64_t>(S_FLAGGED, std::max<int64_t>(NT, 1));
  ga.prev = sb.prev;
  ga.g = sb.g;
  ga.bt = sb.bt;
  ga.bound = sb.bound;
  ga.cand_count = cb.count;
  ga.cand_edge = cb.edge;
  ga.cand_p = cb.p;
  ga.cprep = pr.cprep;
  ga.cprep_t = pr.cprep_t;
  ga.state_trace = state_trace;
  ga.mode_of_trace = b.mode;
  ga.turn_modes = turn_modes;
  ga.turn = d_turn;
  ga.rec = task_rec;
  ga.trans_off = trans_off;
  ga.trans = trans;
  ga.trans_tc = trans_tc;
  ga.counters = d_counters;
  ga.n_overflow = cnt + C_GEN_OVERFLOW;
  if (NT == 0) return OTR_OK;
  // the LDS tiers count their work only when asked (OTR_BATCH_ROUTE_WORK): the end-of-
  // wave counter atomics cost ~7% of the first tier (tools/ab_libs.sh)
  rwork = (in->flags & OTR_BATCH_ROUTE_WORK) ? d_counters : nullptr;
  // turn-mode (edge-state) tasks belong to the edge-state tiers below: the node
  // tiers pass them on unflagged, and when every mode has turn costs (the deployed
  // configuration) no node task exists and the first node tier is not launched at all
  turns = turn_modes != 0u;
#ifdef OTR_FORCE_GENERAL
  node_tasks = true;  // (test build: the first tier flags every task for k_general)
#else
  node_tasks = turn_modes != (1u << OTR_MODES) - 1u;
#endif
#ifdef OTR_FORCE_RETRY
  {  // test build: OTR_FORCE_EDGE bits force the edge-state tiers to fail (tests/test_gpu_tiers.py)
    const char* fe = getenv("OTR_FORCE_EDGE");
    ra.force_edge = fe ? atoi(fe) : 0;
  }
#endif
  // (the list tiers' work queues, XcdQueue: 8 counters per launch, 128 B apart, in the control
  // block, zero since upload())
  // retry-tier dumps (search_run NDump, otr_edge1.h): per task, the dump slot its search
  // left for the next tier; every tier that fails a task writes it (-1: restart), so the
  // first node tier, which flags every task a retry tier will see, initialises it
  static const bool nresume_env = !getenv("OTR_NRESUME") || atoi(getenv("OTR_NRESUME")) != 0;  // A/B knob
  static const bool eresume_env = !getenv("OTR_E1RESUME") || atoi(getenv("OTR_E1RESUME")) != 0;  // A/B knob
  nresume = nresume_env;
  eresume = eresume_env;
  // (optional: without it outgrown searches restart, same results)
  if ((nresume && node_tasks) || (eresume && turns)) task_dump = want<int32_t>(S_TASK_DUMP, NT);
  mat.opt_busy = true;  // the optional workspace stays until the route stage's kernels are queued
  ra.task_dump = task_dump;
  tb(OTR_STAGE_ROUTE);
  if (node_tasks) {
    // The tiny tier (eight searches per wave, tasks [0, NT8)) first, only in batches that
    // are mostly tiny steps (C5); elsewhere its few tasks join the small tier's range (they
    // are adjacent), which saves a launch (C1: 18k tiny tasks cost 2 %).  Then the small
    // tier (four searches per wave), then the two-search tier (CAP 160 tables) over the
    // rest; wider steps and overflows retry in route_retry()
    const bool tiny_run = NT8 > 0 && (2 * NT8 >= NT || tiny_keys >= 1e8);  // (1e8: tests force it)
    const int64_t small_lo = tiny_run ? NT8 : 0;
    if (tiny_run) first_tier(SLOT_TINY, OTR_CAP8, 8, NT8, 0, (NT8 + 7) / 8);
    if (NT8 + NT4 - small_lo > 0)
      first_tier(SLOT_SMALL, OTR_CAP4, 4, NT8 + NT4, small_lo, (NT8 + NT4 - small_lo + 3) / 4);
    if (route_g == 2) first_tier(SLOT_FIRST, OTR_CAP1, 2, NT, NT8 + NT4, (NT - NT8 - NT4 + 1) / 2);
    else first_tier(SLOT_FIRST, 256, 1, NT, NT8 + NT4, NT);
  }
  te(OTR_STAGE_ROUTE);
  return OTR_OK;
}

// ---- the route retry tiers on LDS tables: the node retry tiers, then the 64-bit tier
int Batch::route_retry() {
  if (NT == 0) return OTR_OK;
  int rc;
  // overflow retries with larger LDS tables (same results, fewer resident waves): each
  // tier takes its list on the device and runs a fixed grid over it — no host round
  // trip between tiers.  Tier t takes the previous tier's overflows and the first-tier tasks
  // whose size estimate starts them in a tier <= t (otr_tiers.h node_tier_mask); OTR_TIERS
  // (A/B knob) lists the retry kernels.
  tb(OTR_STAGE_ROUTE_BIG);
  const std::vector<int>& tiers = route_tiers();
  const int ntier = (int)tiers.size();
  // the first tier's flagged tasks, once; every later collect scans only them
  k_collect_flagged<<<grid_ceil(NT, kFlaggedBlock * kFlagsPerThread), kFlaggedBlock, 0, stream>>>(
      NT, task_ovf, flagged, cnt + C_FLAGGED);
  // node dump slots: tier t writes buffer t % 2 and tier t + 1 resumes from it; slots for a
  // quarter of the tasks, at most OTR_NDUMP_GB (4) GB per buffer (C4: 4 % of the 1024-slot
  // searches outgrow it, 10 KB each); beyond them, or without the memory, searches restart
  unsigned long long* ndump[2] = {nullptr, nullptr};
  uint32_t nslots[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  // (tables compiled with the resume / dump code, otr_kernels.h OTR_ND_IN_MIN / OTR_ND_OUT_MIN)
  auto nd_in = [&](int t) { return t > 0 && t < ntier && tiers[t] / 10 >= OTR_ND_IN_MIN; };
  auto nd_out = [&](int t) { return t + 1 < ntier && tiers[t] / 10 >= OTR_ND_OUT_MIN && nd_in(t + 1); };
  if (nresume && node_tasks && task_dump && ntier > 1) {
    static const double gb = getenv("OTR_NDUMP_GB") ? atof(getenv("OTR_NDUMP_GB")) : 4.0;
    const int64_t cap_bytes = (int64_t)(gb * (double)(1ll << 30));
    size_t words[2] = {0, 0};
    for (int t = 0; t + 1 < ntier && t < 8; ++t) {
      if (!nd_out(t)) continue;
      const uint32_t w = nd_words(tiers[t] / 10);
      nslots[t] = (uint32_t)std::min<int64_t>(std::max<int64_t>(NT / 4, 1024), cap_bytes / (8 * (int64_t)w));
      words[t & 1] = std::max<size_t>(words[t & 1], (size_t)nslots[t] * w);
    }
    for (int q = 0; q < 2; ++q)
      if (words[q]) ndump[q] = want<unsigned long long>(q == 0 ? S_NDUMP0 : S_NDUMP1, words[q]);
    if ((words[0] && !ndump[0]) || (words[1] && !ndump[1])) ndump[0] = ndump[1] = nullptr;
  }
  for (int tier = 0; tier < (node_tasks ? ntier : 0); ++tier) {  // (no node task: no node tier)
    const int slot = SLOT_NODE + tier;
    RouteArgs rb = take_list(slot);
    const bool din = nd_in(tier) && nd_out(tier - 1) && ndump[(tier + 1) & 1] != nullptr;
    const bool dout = nd_out(tier) && ndump[tier & 1] != nullptr;
    rb.dump_in = din ? ndump[(tier + 1) & 1] : nullptr;
    rb.dump_in_words = din ? nd_words(tiers[tier - 1] / 10) : 0u;
    rb.dump_out = dout ? ndump[tier & 1] : nullptr;
    rb.dump_ctr = queues + dump_ctr_word(slot);  // (its queue was zeroed with the others; one line per tier)
    rb.dump_out_words = dout ? nd_words(tiers[tier] / 10) : 0u;
    rb.dump_out_slots = dout ? nslots[tier] : 0u;
    out->route_tier_code[slot] = tiers[tier];
    tier_begin(slot);
    if ((rc = retry_tier(tiers[tier], rb, tier_work(slot)))) return rc;
    tier_end(slot);
  }
#ifndef OTR_FORCE_GENERAL  // (test build: every search in k_general)
  // the node-mode tasks whose (length << sh | time) words need more than 32 bits
  // (RF_GENERAL: long gaps between states) run in an LDS table of 64-bit words (same labels,
  // DESIGN.md §3.5); what outgrows it is flagged RF_GENERAL again.  It runs ahead of the
  // edge-state tiers for a reason: otr_tiers.h kRouteOrder
  {
    constexpr RouteTier w = kRouteTiers[SLOT_WIDE64];
    const RouteArgs rb = take_list(SLOT_WIDE64);
    out->route_tier_code[SLOT_WIDE64] = route_tier_code(SLOT_WIDE64, w.cap, 1);
    tier_begin(SLOT_WIDE64);
    if (rwork) k_route<w.cap, 1, true, true, true><<<pgrid(w.grid, NT), 64, 0, stream>>>(g, rb, tier_bank(SLOT_WIDE64));
    else k_route<w.cap, 1, true, true, false><<<pgrid(w.grid, NT), 64, 0, stream>>>(g, rb, nullptr);
    tier_end(SLOT_WIDE64);
  }
#endif
  return OTR_OK;
}

// the table of edge-state tier et (kEdgeSlots): the first one's is a build knob
static constexpr int edge_cap(int et) { return kRouteTiers[kEdgeSlots[et]].cap ? kRouteTiers[kEdgeSlots[et]].cap : OTR_E1CAP; }

// edge-state tiers (turn-cost modes, otr_edge1.h), in the order of kEdgeSlots: OTR_E1CAP (360)
// states, 512, 1024, each taking what the one before outgrew; what outgrows those goes on to
// the global-memory tiers (otr_tiers.h edge_overflow_flag)
int Batch::route_edge() {
  if (NT == 0) return OTR_OK;
  if (turns) {
    // dump slots of the first two edge tiers: a search they outgrow between two rounds
    // resumes in the next table (otr_edge1.h e1_dump / e1_restore) instead of starting
    // over; slots for 1/16 of the tasks (C2, deployed: 4.4 % outgrow the first table),
    // at most 4 GB / 1 GB — searches beyond them, or when the memory is not there,
    // restart in the next table (same results)
    unsigned long long* dump[2] = {nullptr, nullptr};
    uint32_t dslots[2] = {0u, 0u};
    const uint32_t dwords[2] = {e1_dump_words(edge_cap(0)), e1_dump_words(edge_cap(1))};
    if (eresume && task_dump) {
      const int64_t cap_bytes[2] = {4ll << 30, 1ll << 30};
      const int64_t wanted[2] = {std::max<int64_t>(NT / 16, 4096), std::max<int64_t>(NT / 64, 1024)};
      for (int q = 0; q < 2; ++q) {  // (no dumps beyond what was allocated: those searches restart)
        const int64_t n = std::min<int64_t>(wanted[q], cap_bytes[q] / (8 * (int64_t)dwords[q]));
        dump[q] = want<unsigned long long>(q == 0 ? S_E1DUMP0 : S_E1DUMP1, (size_t)n * dwords[q]);
        dslots[q] = dump[q] ? (uint32_t)n : 0u;
      }
      if (!dump[0]) dump[1] = nullptr, dslots[1] = 0u;
    }
    for (int et = 0; et < 3; ++et) {
      const int slot = kEdgeSlots[et];
      out->route_tier_code[slot] = route_tier_code(slot, edge_cap(et), 1);
      RouteArgs rb = take_list(slot);
      const unsigned long long* c = rb.list_count;
      // the first edge tier's list in spatial order (k_sort_*: one band of the map per XCD)
      static const bool esort = !getenv("OTR_SORT") || atoi(getenv("OTR_SORT")) != 0;  // A/B knob
      int64_t* list2 = nullptr;
      uint32_t* hist = nullptr;
      if (et == 0 && esort && NT >= 65536) {
        list2 = want<int64_t>(S_SORT_LIST, NT);  // (no memory for the copy: the list stays in task order)
        hist = list2 ? want<uint32_t>(S_SORT_HIST, kSortBuckets) : nullptr;
      }
      if (list2 && hist) {
        int bits = 0;
        while (bits < 32 && (g.n_edges >> bits) > 0u) ++bits;
        const int shift = bits > 12 ? bits - 12 : 0;
        HIPCHK(hipMemsetAsync(hist, 0, 4 * kSortBuckets, stream));
        k_sort_hist<<<grid_ceil(NT, 1024), 1024, 0, stream>>>(list, c, task_rec, shift, hist);
        k_sort_scan<<<1, 1024, 0, stream>>>(hist);
        k_sort_place<<<grid_ceil(NT, 1024), 1024, 0, stream>>>(list, c, task_rec, shift, hist, list2);
        rb.task_list = list2;
      }
      rb.dump_in = et > 0 ? dump[et - 1] : nullptr;
      rb.dump_in_words = et > 0 ? dwords[et - 1] : 0u;
      rb.dump_in_cap = et == 1 ? edge_cap(0) : edge_cap(1);
      rb.dump_out = et < 2 ? dump[et] : nullptr;  // (the last tier never dumps: otr_tiers.h)
      rb.dump_ctr = queues + dump_ctr_word(slot);
      rb.dump_out_words = et < 2 ? dwords[et] : 0u;
      rb.dump_out_slots = et < 2 ? dslots[et] : 0u;
      rb.task_dump = task_dump;
      unsigned long long* rcn = tier_work(slot);
      tier_begin(slot);
      // persistent grids of at least every resident wave (16 per CU at 384 states, 13 at
      // 512, 6 at 1024) claiming tasks from per-XCD queues; steps with more than 32
      // targets (modes keeping > 32 candidates) pass the lean tiers (their TG = 32) on to
      // k_general
      with_row<3>(et, [&](auto i) {
        k_route_e1<edge_cap(decltype(i)::value)><<<pgrid(kRouteTiers[slot].grid, NT), 64, 0, stream>>>(g, rb, rcn);
      });
      tier_end(slot);
    }
  }
  mat.opt_busy = false;  // (every user of the optional workspace is queued)
  return OTR_OK;
}

// everything left — tasks whose labels need 64 bits, overflows of the largest LDS tables
// (node and edge-state) — runs in the global-memory search: first on 32K-slot slabs, then
// what outgrew those on 1M-slot slabs
int Batch::route_global() {
  if (NT == 0) return OTR_OK;
  int rc;
  for (int gt = 0; gt < 2; ++gt) {
    const int slot = SLOT_GLOBAL + gt;
    collect(Chain::Route, kRouteTiers[slot].take, kRouteTiers[slot].list, list);
    GSlabs gs2;
    if ((rc = slabs(gt, &gs2))) return rc;
    ga.mode = 0;
    ga.list = list;
    ga.list_count = tier_list(slot);
    ga.flag = task_ovf;
    ga.counters = tier_bank(slot);
    out->route_tier_code[slot] = route_tier_code(slot, (int)gs2.cap, 0);
    tier_begin(slot);
    k_general<<<pgrid(gs2.n, NT), kGenThreads, 0, stream>>>(g, ga, gs2);
    tier_end(slot);
  }
  // tasks still flagged (beyond a 1M-state slab): their traces get OTR_MATCH_ERROR
  collect(Chain::Route, kTasksLeft.take, kTasksLeft.list, fail_tasks);
  te(OTR_STAGE_ROUTE_BIG);
  return OTR_OK;
}

// ---- K5: Viterbi
int Batch::viterbi() {
  va.n_traces = T;
  va.trace_state_off = trace_state_off;
  va.cand_count = cb.count;
  va.cand_sqd = cb.sqd;
  va.prev = sb.prev;
  va.trans_off = trans_off;
  va.trans = trans;
  va.trans_tc = trans_tc;
  va.turn_modes = turn_modes;
  va.g = sb.g;
  va.mode = b.mode;
  for (int m = 0; m < OTR_MODES; ++m) va.inv2s2[m] = mp.m[m].inv2s2;
  for (int m = 0; m < OTR_MODES; ++m) va.inv_beta[m] = mp.m[m].inv_beta;
  va.bp = need<int8_t>(S_BP, (size_t)S * OTR_KMAX);
  va.brk = need<uint8_t>(S_BRK, S);
  va.end_win = need<int32_t>(S_END_WIN, S);
  va.winner = need<int32_t>(S_WINNER, S);
  va.subpath = need<int32_t>(S_SUBPATH, S);
  tb(OTR_STAGE_VITERBI);
  {
    // two traces per wave when no mode keeps more than 32 candidates (K <= 32 lanes); a
    // batch too small to fill the GPU that way (fewer than 8,192 traces: C1's 1,000) runs
    // one trace per wave with each step's predecessor scan split over the two halves
    static const int64_t split_below = getenv("OTR_VIT_SPLIT") ? atoll(getenv("OTR_VIT_SPLIT")) : 8192;  // A/B knob
    if (k32 && T < split_below) {
      vit_variant = 11;
      k_viterbi<1, true><<<(unsigned)(T < 1048576 ? T : 1048576), 64, 0, stream>>>(va, d_counters);
    } else if (k32) {
      vit_variant = 20;
      const int64_t w = (T + 1) / 2;
      k_viterbi<2><<<(unsigned)(w < 1048576 ? w : 1048576), 64, 0, stream>>>(va, d_counters);
    } else {
      vit_variant = 10;
      k_viterbi<1><<<(unsigned)(T < 1048576 ? T : 1048576), 64, 0, stream>>>(va, d_counters);
    }
  }
  te(OTR_STAGE_VITERBI);
  return OTR_OK;
}

// ---- K6: winner paths (step list, tiers and general fallback counted on the device); a
// path buffer that proves too small grows and the stage runs again
int Batch::paths() {
  int rc;
  path_off = need<int64_t>(S_PATH_OFF, S);
  path_len = need<int32_t>(S_PATH_LEN, S);
  if (S > 0) k_fill_i32<<<grid_ceil(S, 256), 256, 0, stream>>>(path_len, S, 0);
  {
    steps = need<int64_t>(S_LIST2, std::max<int64_t>(S, 1));
    step_ovf = need<int32_t>(S_STEP_OVF, S + 1);  // (zeroed by the step-list kernel)
    nsteps_d = cnt + C_STEPS;
    // the small-search path tier (four searches per wave): steps whose winning route
    // bounds a search of at most OTR_SMALL_PATH_KEYS keys (estimate: 4 x the node density
    // x r^2, the diamond of road distance r around the root and its frontier); the
    // two-search tier takes the rest.  Both lists' lengths come back to the host (one
    // synchronisation) so each tier launches the blocks its list needs and no more (a grid
    // sized for every step costs a dispatch per empty block: C5 paths 13.2 -> 18.8 ms
    // instead of 8.3).  Only in batches whose route tasks went mostly to the small route
    // tier (C5, C1): at C2 (3 % small) the synchronisation cost more than the tier saved.
    static const double small_path_keys =
        getenv("OTR_SMALL_PATH_KEYS") ? atof(getenv("OTR_SMALL_PATH_KEYS")) : kSmallPathKeys;  // A/B knob
    small_paths = small_path_keys > 0.0 && est_k > 0.f && (small_path_keys >= 1e8 || 2 * (NT4 + NT8) >= NT);
    nsteps4_d = cnt + C_STEPS_FRONT;                          // (the front list's count)
    unsigned long long* nall_d = cnt + C_STEPS_ALL;           // (S: the collects' index range)
    if (S > 0 && small_paths) {
      PathClass pc{};
      pc.winner = va.winner;
      pc.trans_off = trans_off;
      pc.trans = trans;
      pc.bound = sb.bound;
      pc.state_trace = state_trace;
      pc.mode = b.mode;
      pc.turn_modes = turn_modes;
      pc.est4 = 8.f * est_k;  // (est_k = half the node density)
      pc.small_keys = (float)small_path_keys;
      // (both counts are zero since upload(): the control block)
      k_step_lists<<<grid_ceil(S, 256), 256, 0, stream>>>(S, sb.prev, va.brk, cb.count, pc, steps, nsteps4_d, nsteps_d,
                                                          nall_d, step_ovf);
      if ((rc = post_wait(Matcher::MailRun{nsteps4_d, 1}, Matcher::MailRun{nsteps_d, 1}))) return rc;
      h_nsteps[0] = mat.mail[0];
      h_nsteps[1] = mat.mail[1];
    } else if (S > 0) {
      k_step_list<<<grid_ceil(S, 1024), 1024, 0, stream>>>(S, sb.prev, va.brk, cb.count, steps, nsteps_d, step_ovf);
    }
    // the retry collects' index range: every step index (front and back lists), or the list
    nscan_d = small_paths ? nall_d : nsteps_d;
    // OTR_PATH_CAP0 (test knob, read once per process): the first attempt's capacity in entries
    static const int64_t cap0 = getenv("OTR_PATH_CAP0") ? atoll(getenv("OTR_PATH_CAP0")) : 0;
    int64_t capacity = cap0 > 0 ? kShards * ((cap0 + kShards - 1) / kShards)
                                : kShards * ((int64_t)S * 24 / kShards + 1024);
    // The per-trace output capacities (K7's layout) are queued behind every attempt without
    // waiting for its cap flag, so the flag, the cursors and the layout's total C come back in
    // ONE mailbox record and one host wait.  A set flag (never seen outside the tests) grows
    // the buffer and runs the path kernels, k_capacity and its scan again; the capacities of
    // the failed attempt are simply overwritten.
    cap = need<int64_t>(S_CAP, T);
    cap_off = need<int64_t>(S_CAP_OFF, T + 1);
    bool paths_fit = false;
    for (int attempt = 0; attempt < 8; ++attempt) {
      path_attempts = attempt + 1;
      if (S > 0 && (rc = paths_attempt(capacity, attempt > 0))) return rc;
      k_capacity<<<grid_ceil(T, 256), 256, 0, stream>>>(T, trace_state_off, cb.count, path_len, cap);
      if ((rc = scan(cap, cap_off, T))) return rc;
      if ((rc = post_wait(Matcher::MailRun{cnt + C_CAP_FLAG, 1}, Matcher::MailRun{cap_off + T, 1},
                          Matcher::MailRun{cnt + C_CURSORS, kShards})))
        return rc;
      if ((mat.mail[0] & 0xFFFFFFFFu) == 0) {  // every path fitted its region (no state: no path, no flag)
        C = (int64_t)mat.mail[1];
        paths_fit = true;
        break;
      }
      unsigned long long mx = 0;
      for (int q = 0; q < kShards; ++q) mx = std::max(mx, mat.mail[2 + q]);
      capacity = kShards * ((int64_t)mx + (int64_t)mx / 2 + 1024);  // grow and redo
    }
    if (!paths_fit) {  // (the capacity grows 1.5x past the largest shard: never seen)
      if (err) *err = "winner paths did not fit the path buffer after 8 attempts";
      return OTR_DEVICE_ERROR;
    }
    if (path_attempts > 1 && getenv("OTR_DEBUG_FAIL"))
      fprintf(stderr, "otr: winner paths regrown: %d attempts, %lld entries\n", path_attempts, (long long)capacity);
  }
  return OTR_OK;
}

// one run of the path kernels into a buffer of `capacity` entries: the first tiers over the
// step lists, the retry tiers, the edge-state tiers and the global-memory search
int Batch::paths_attempt(int64_t capacity, bool again) {
  int rc;
  uint32_t* path = need<uint32_t>(S_PATH, capacity);
  if (again) {  // (the first attempt finds its words zero: the control block, upload(); the step-list kernel)
    HIPCHK(hipMemsetAsync(step_ovf, 0, 4 * (S + 1), stream));
    // path tier counts .. cap flag (the words between are the path stage's too)
    HIPCHK(hipMemsetAsync(cnt + C_PATH_TIER, 0, 8 * (C_CAP_FLAG + 1 - C_PATH_TIER), stream));
    HIPCHK(hipMemsetAsync(cnt + C_EDGE_PATH, 0, 8 * 2, stream));  // edge-state path tier counts
    HIPCHK(hipMemsetAsync(cnt + C_CURSORS, 0, 8 * kShards, stream));
    HIPCHK(hipMemsetAsync(pq, 0, 8 * kPathQueues * kPQWords, stream));  // the path retry tiers' work queues
  }
  PathArgs pa{};
  pa.steps = steps;
  pa.n_steps = S;
  pa.n_steps_dev = nsteps_d;
  pa.prev = sb.prev;
  pa.bound = sb.bound;
  pa.brk = va.brk;
  pa.winner = va.winner;
  pa.cand_edge = cb.edge;
  pa.cand_p = cb.p;
  pa.state_trace = state_trace;
  pa.mode = b.mode;
  pa.cprep = ra.cprep;
  pa.cprep_t = ra.cprep_t;
  pa.bt = sb.bt;
  pa.turn_modes = turn_modes;
  pa.path_off = path_off;
  pa.path_len = path_len;
  pa.path = path;
  pa.cursor = cnt + C_CURSORS;
  pa.capacity = capacity;
  pa.overflow_flag = step_ovf;
  pa.cap_flag = (int32_t*)(cnt + C_CAP_FLAG);
  pa.cand_count = cb.count;
  pa.trans_off = trans_off;
  pa.trans = trans;
  pa.force_edge = ra.force_edge;
  // (the path retry tiers' work queues, XcdQueue: pq, in the control block)
  tb(OTR_STAGE_PATHS);
  if (small_paths) {
    // the front list four searches per wave, the back list two, each grid sized by its
    // list's length (blocks past a list's end exit at once, but cost a dispatch each)
    if (h_nsteps[0] > 0) {
      PathArgs p4 = pa;
      p4.n_steps_dev = nsteps4_d;
      k_paths<OTR_CAP4, 4><<<(unsigned)grid_paths((int64_t)(h_nsteps[0] + 1) / 2).blocks, 64, 0, stream>>>(
          g, p4, nullptr, nullptr);
    }
    if (h_nsteps[1] > 0) {
      PathArgs p2 = pa;
      p2.from_back = true;
      k_paths<OTR_CAP1, 2><<<(unsigned)grid_paths((int64_t)h_nsteps[1]).blocks, 64, 0, stream>>>(g, p2, nullptr,
                                                                                                 nullptr);
    }
  } else {
    // (steps <= states: two searches per wave)
    k_paths<OTR_CAP1, 2><<<(unsigned)grid_paths(S).blocks, 64, 0, stream>>>(g, pa, nullptr, nullptr);
  }
  te(OTR_STAGE_PATHS);
  tb(OTR_STAGE_PATHS_BIG);
  // The retry tiers in the order of kPathTiers (otr_tiers.h), on device-side lists: larger
  // node tables for table overflows, the edge-state LDS search for turn-cost winners, then
  // k_general for 64-bit labels, the largest-table overflows and what the edge tiers left.
  // Each LDS launch's waves claim steps from its own per-XCD queue (XcdQueue).
  ga.steps = steps;
  ga.winner = va.winner;
  ga.path_off = path_off;
  ga.path_len = path_len;
  ga.path = path;
  ga.cursor = cnt + C_CURSORS;
  ga.capacity = capacity;
  ga.cap_flag = (int32_t*)(cnt + C_CAP_FLAG);
  int gt = 0;  // the next global-memory tier's slabs
  for (int t = 0; t < kPathTierN; ++t) {
    const PathTier& pt = kPathTiers[t];
    if (pt.kind == PathKind::EdgeState && turn_modes == 0u) continue;
    unsigned long long* c = cnt + pt.list;
    collect(Chain::Path, pt.take, pt.list, list);
    if (pt.kind == PathKind::Global) {
      GSlabs gs2;
      if ((rc = slabs(gt++, &gs2))) return rc;
      ga.mode = 1;
      ga.list = list;
      ga.list_count = c;
      ga.flag = step_ovf;
      ga.counters = nullptr;
      k_general<<<pgrid(gs2.n, S), kGenThreads, 0, stream>>>(g, ga, gs2);
      continue;
    }
    PathArgs pb = pa;
    pb.queue = pq + pt.queue * kPQWords;
    with_row<kPathTierN>(t, [&](auto i) {
      constexpr PathTier row = kPathTiers[decltype(i)::value];
      if constexpr (row.kind == PathKind::Node)
        k_paths<row.cap, 1><<<pgrid(row.grid, S), 64, 0, stream>>>(g, pb, list, c);
      else if constexpr (row.kind == PathKind::EdgeState)
        k_paths_edge<row.cap><<<pgrid(row.grid, S), 64, 0, stream>>>(g, pb, d_turn, list, c, row.overflow);
    });
  }
  // steps still flagged (beyond a 1M-state slab): named after the final sync
  collect(Chain::Path, kPathsLeft.take, kPathsLeft.list, list);
  te(OTR_STAGE_PATHS_BIG);
  return OTR_OK;
}

// ---- K7..K9: stitching, segments, report(); hour buckets -> histogram; tile rows
int Batch::segments() {
  int rc;
  // (the capacity layout cap_off and its total C: paths(), with the path stage's host wait)
  sa.b = b;
  sa.trace_state_off = trace_state_off;
  sa.state_probe = state_probe;
  sa.cand_count = cb.count;
  sa.cand_edge = cb.edge;
  sa.cand_p = cb.p;
  sa.prev = sb.prev;
  sa.brk = va.brk;
  sa.winner = va.winner;
  sa.path_off = path_off;
  sa.path_len = path_len;
  sa.path = (const uint32_t*)need<uint32_t>(S_PATH, 1);
  sa.pos = need<int64_t>(S_POS, S);
  sa.act = need<int64_t>(S_ACT, S);
  sa.ent = need<int64_t>(S_ENT, S);
  sa.suba = need<int32_t>(S_SUBA, S);
  sa.subb = need<int32_t>(S_SUBB, S);
  sa.por_e = need<uint32_t>(S_POR_E, C);
  sa.por_s0 = need<int64_t>(S_POR_S0, C);
  sa.por_s1 = need<int64_t>(S_POR_S1, C);
  sa.por_sa = need<int32_t>(S_POR_SA, C);
  sa.gstart = need<int32_t>(S_GSTART, C);
  sa.cap_off = cap_off;
  sa.route = need<uint32_t>(S_ROUTE, C);
  // the four per-trace output counts in one slab, the folded counters and the two fail
  // counts behind them: drain() brings it over with one copy
  int64_t* counts = need<int64_t>(S_ROUTE_N, 4 * (size_t)T + n_ctr + 2);
  sa.route_n = counts;
  sa.seg_id = need<unsigned long long>(S_SEG_ID, C);
  sa.seg_start = need<double>(S_SEG_START, C);
  sa.seg_end = need<double>(S_SEG_END, C);
  sa.seg_length = need<int32_t>(S_SEG_LEN, C);
  sa.seg_queue = need<int32_t>(S_SEG_QUEUE, C);
  sa.seg_internal = need<uint8_t>(S_SEG_INTERNAL, C);
  sa.seg_bshape = need<int32_t>(S_SEG_BSHAPE, C);
  sa.seg_eshape = need<int32_t>(S_SEG_ESHAPE, C);
  sa.seg_index = need<uint32_t>(S_SEG_INDEX, C);
  sa.seg_n = counts + T;
  sa.seg_way_n = need<int64_t>(S_SEG_WAY_N, C);
  sa.seg_way = need<uint32_t>(S_SEG_WAY, C);
  sa.way_n = counts + 3 * (size_t)T;
  sa.rep_id = need<unsigned long long>(S_REP_ID, C);
  sa.rep_next = need<unsigned long long>(S_REP_NEXT, C);
  sa.rep_t0 = need<double>(S_REP_T0, C);
  sa.rep_t1 = need<double>(S_REP_T1, C);
  sa.rep_length = need<int32_t>(S_REP_LEN, C);
  sa.rep_queue = need<int32_t>(S_REP_QUEUE, C);
  sa.rep_seg = need<uint32_t>(S_REP_SEG, C);
  sa.rep_n = counts + 2 * (size_t)T;
  sa.shape_used = need<int32_t>(S_SHAPE_USED, T);
  sa.stats = need<int32_t>(S_STATS, 7 * (size_t)T);
  sa.stats_len = need<double>(S_STATS_LEN, 2 * (size_t)T);
  sa.threshold = (double)(in->threshold_sec >= 0 ? in->threshold_sec : 15);
  sa.report_levels = in->report_levels;
  sa.transition_levels = in->transition_levels;
  for (int m = 0; m < OTR_MODES; ++m) sa.queue_kph[m] = mp.m[m].queue_kph;
  tb(OTR_STAGE_SEGMENTS);
  k_segments<<<(unsigned)grid_segments(T).blocks, 64, 0, stream>>>(g, sa, d_counters);
  te(OTR_STAGE_SEGMENTS);
  // ---- K8: hour buckets → histogram
  ha.b = b;
  ha.cap_off = cap_off;
  ha.rep_n = sa.rep_n;
  ha.rep_id = sa.rep_id;
  ha.rep_t0 = sa.rep_t0;
  ha.rep_t1 = sa.rep_t1;
  ha.rep_length = sa.rep_length;
  ha.rep_queue = sa.rep_queue;
  ha.rep_seg = sa.rep_seg;
  ha.quantisation = in->quantisation > 0 ? in->quantisation : 3600;
  ha.base_time = in->hist_base_time;
  ha.hours = in->hist_hours;
  ha.n_segments = g.n_segments;
  ha.n_rows = d_counters + 8 * kCShards;
  hist_len = (size_t)(in->hist_hours > 0 ? in->hist_hours : 0) * g.n_segments * OTR_HIST_BINS;
  ha.hist = hist_len ? (in->hist_device ? in->hist_device : need<uint32_t>(S_HIST, hist_len)) : nullptr;
  if (hist_len) HIPCHK(hipMemsetAsync(ha.hist, 0, hist_len * 4, stream));
  tb(OTR_STAGE_HISTOGRAM);
  // K8 also counts the rows (n_rows) when K9 does not
  if (hist_len || !(in->flags & OTR_BATCH_TILE_ROWS))
    k_histogram<<<(unsigned)grid_trace_rows(T).blocks, 256, 0, stream>>>(ha);
  te(OTR_STAGE_HISTOGRAM);
  // ---- K9: simple_reporter tile rows (optional)
  if (in->flags & OTR_BATCH_TILE_ROWS) {
    TileArgs ta{};
    ta.b = b;
    ta.cap_off = cap_off;
    ta.rep_n = sa.rep_n;
    ta.rep_id = sa.rep_id;
    ta.rep_next = sa.rep_next;
    ta.rep_t0 = sa.rep_t0;
    ta.rep_t1 = sa.rep_t1;
    ta.rep_length = sa.rep_length;
    ta.rep_queue = sa.rep_queue;
    ta.quantisation = ha.quantisation;
    ta.rules = in->tile_rules;
    ta.row_cnt = need<int64_t>(S_ROW_CNT, T);
    k_tile_rows<<<(unsigned)grid_trace_rows(T).blocks, 256, 0, stream>>>(ta);
    int64_t* row_off = need<int64_t>(S_ROW_OFF, T + 1);
    if ((rc = scan(ta.row_cnt, row_off, T))) return rc;
    int64_t R = 0;
    if ((rc = read_i64(row_off + T, &R))) return rc;
    ta.row_off = row_off;
    ta.rows = need<otr_tile_row>(S_ROWS, R > 0 ? R : 1);
    if (R > 0) k_tile_rows<<<(unsigned)grid_trace_rows(T).blocks, 256, 0, stream>>>(ta);
    out->d_rows = ta.rows;
    out->n_rows = R;
  }
  HIPCHK(hipGetLastError());
  return OTR_OK;
}

// ---- K12: every probe's matched point (optional), 53 B per probe
int Batch::points() {
  if (!want_points) return OTR_OK;
  pta.b = b;
  pta.trace_state_off = trace_state_off;
  pta.state_probe = state_probe;
  pta.cand_count = cb.count;
  pta.cand_edge = cb.edge;
  pta.cand_p = cb.p;
  pta.winner = va.winner;
  pta.brk = va.brk;
  pta.path_off = path_off;
  pta.path_len = path_len;
  pta.path = sa.path;
  pta.act = sa.act;
  pta.pos = sa.pos;
  pta.kind = need<uint8_t>(S_PT_KIND, N);
  pta.edge = need<uint32_t>(S_PT_EDGE, N);
  pta.frac = need<double>(S_PT_FRAC, N);
  pta.lat = need<double>(S_PT_LAT, N);
  pta.lon = need<double>(S_PT_LON, N);
  pta.dist = need<double>(S_PT_DIST, N);
  pta.state = need<int64_t>(S_PT_STATE, N);
  pta.pos_mm = need<int64_t>(S_PT_POS, N);
  if (timing) (void)hipEventRecord(mat.ev[kPointsEvent], stream);
  k_matched_points<<<(unsigned)grid_segments(T).blocks, 64, 0, stream>>>(g, pta);
  if (timing) (void)hipEventRecord(mat.ev[kPointsEvent + 1], stream);
  HIPCHK(hipGetLastError());
  return OTR_OK;
}

// after the batch drained: the traces beyond every tier lose their points, the stage's
// time, the host copies (OTR_BATCH_COPY_OUT); the matcher remembers the result
int Batch::points_out() {
  int rc;
  if (!want_points) return OTR_OK;
  if (out->n_overflow_traces > 0) {
    int32_t* d_status = need<int32_t>(S_PT_STATUS, T);
    HIPCHK(hipMemcpyAsync(d_status, mat.h_trace_status.data(), 4 * (size_t)T, hipMemcpyHostToDevice, stream));
    k_points_failed<<<(unsigned)std::min<int64_t>(T, 1024), 64, 0, stream>>>(pta, d_status);
    HIPCHK(hipGetLastError());
  }
  otr_point_result& r = mat.pts;
  r.n_probes = N;
  if (timing) {
    (void)hipEventElapsedTime(&r.kernel_ms, mat.ev[kPointsEvent], mat.ev[kPointsEvent + 1]);
    (void)hipGetLastError();
  }
  r.d_kind = pta.kind;
  r.d_edge = pta.edge;
  r.d_frac = pta.frac;
  r.d_lat = pta.lat;
  r.d_lon = pta.lon;
  r.d_dist = pta.dist;
  r.d_state = pta.state;
  r.d_pos_mm = pta.pos_mm;
  if (in->flags & OTR_BATCH_COPY_OUT) {
    if ((rc = dl(mat.h_pt_kind, pta.kind, N)) || (rc = dl(mat.h_pt_edge, pta.edge, N)) ||
        (rc = dl(mat.h_pt_frac, pta.frac, N)) || (rc = dl(mat.h_pt_lat, pta.lat, N)) ||
        (rc = dl(mat.h_pt_lon, pta.lon, N)) || (rc = dl(mat.h_pt_dist, pta.dist, N)) ||
        (rc = dl(mat.h_pt_state, pta.state, N)) || (rc = dl(mat.h_pt_pos, pta.pos_mm, N)))
      return rc;
    r.kind = mat.h_pt_kind.data();
    r.edge = mat.h_pt_edge.data();
    r.frac = mat.h_pt_frac.data();
    r.lat = mat.h_pt_lat.data();
    r.lon = mat.h_pt_lon.data();
    r.dist = mat.h_pt_dist.data();
    r.state = mat.h_pt_state.data();
    r.pos_mm = mat.h_pt_pos.data();
  }
  HIPCHK(hipStreamSynchronize(stream));
  mat.pts_have = true;
  return OTR_OK;
}

int Matcher::matched_points(otr_point_result* out, std::string* err) const {
  if (!pts_have) {
    if (err)
      *err = "otr_matched_points: the matcher has run no batch, or its last otr_match_batch did not set "
             "OTR_BATCH_MATCHED_POINTS";
    return OTR_BAD_REQUEST;
  }
  *out = pts;
  return OTR_OK;
}

// ---- K13: the edge traversals of the matched route (optional), 76 B
// per traversal: count per trace, offsets (one more host read, for the arrays' size), fill
int Batch::traversals() {
  int rc;
  if (!want_traversals) return OTR_OK;
  tva.b = b;
  tva.trace_state_off = trace_state_off;
  tva.state_probe = state_probe;
  tva.cand_count = cb.count;
  tva.cand_edge = cb.edge;
  tva.cand_p = cb.p;
  tva.winner = va.winner;
  tva.act = sa.act;
  tva.pos = sa.pos;
  tva.subb = sa.subb;
  tva.por_e = sa.por_e;
  tva.por_s0 = sa.por_s0;
  tva.por_s1 = sa.por_s1;
  tva.por_sa = sa.por_sa;
  tva.cap_off = cap_off;
  tva.route = sa.route;
  tva.route_n = sa.route_n;
  tva.count = need<int64_t>(S_TR_CNT, T);
  int64_t* off = need<int64_t>(S_TR_OFF, T + 1);
  tva.trav_off = off;
  if (timing) (void)hipEventRecord(mat.ev[kTravEvent], stream);
  k_trav_count<<<(unsigned)grid_segments(T).blocks, 64, 0, stream>>>(tva);
  if ((rc = scan(tva.count, off, T))) return rc;
  if ((rc = read_i64(off + T, &n_trav))) return rc;
  const size_t n = (size_t)n_trav;
  tva.edge = need<uint32_t>(S_TR_EDGE, n);
  tva.way = need<uint32_t>(S_TR_WAY, n);
  tva.seg_id = need<unsigned long long>(S_TR_SEG, n);
  tva.first_state = need<int64_t>(S_TR_FIRST, n);
  tva.f0 = need<double>(S_TR_F0, n);
  tva.f1 = need<double>(S_TR_F1, n);
  tva.s0_mm = need<int64_t>(S_TR_S0, n);
  tva.s1_mm = need<int64_t>(S_TR_S1, n);
  tva.t_enter = need<double>(S_TR_T0, n);
  tva.t_exit = need<double>(S_TR_T1, n);
  if (n_trav > 0) k_edge_traversals<<<(unsigned)grid_segments(T).blocks, 64, 0, stream>>>(g, tva);
  if (timing) (void)hipEventRecord(mat.ev[kTravEvent + 1], stream);
  HIPCHK(hipGetLastError());
  return OTR_OK;
}

// after the batch drained: the stage's time, the host copies (OTR_BATCH_COPY_OUT); the
// matcher remembers the result
int Batch::traversals_out() {
  int rc;
  if (!want_traversals) return OTR_OK;
  otr_traversal_result& r = mat.trv;
  r.n_traversals = n_trav;
  r.n_traces = T;
  if (timing) {
    (void)hipEventElapsedTime(&r.kernel_ms, mat.ev[kTravEvent], mat.ev[kTravEvent + 1]);
    (void)hipGetLastError();
  }
  r.d_trace_off = const_cast<int64_t*>(tva.trav_off);
  r.d_edge = tva.edge;
  r.d_way = tva.way;
  r.d_seg_id = reinterpret_cast<uint64_t*>(tva.seg_id);
  r.d_first_state = tva.first_state;
  r.d_f0 = tva.f0;
  r.d_f1 = tva.f1;
  r.d_s0_mm = tva.s0_mm;
  r.d_s1_mm = tva.s1_mm;
  r.d_t_enter = tva.t_enter;
  r.d_t_exit = tva.t_exit;
  if (in->flags & OTR_BATCH_COPY_OUT) {
    const size_t n = (size_t)n_trav;
    if ((rc = dl(mat.h_tr_off, tva.trav_off, (size_t)T + 1)) || (rc = dl(mat.h_tr_edge, tva.edge, n)) ||
        (rc = dl(mat.h_tr_way, tva.way, n)) || (rc = dl(mat.h_tr_seg, tva.seg_id, n)) ||
        (rc = dl(mat.h_tr_first, tva.first_state, n)) || (rc = dl(mat.h_tr_f0, tva.f0, n)) ||
        (rc = dl(mat.h_tr_f1, tva.f1, n)) || (rc = dl(mat.h_tr_s0, tva.s0_mm, n)) ||
        (rc = dl(mat.h_tr_s1, tva.s1_mm, n)) || (rc = dl(mat.h_tr_t0, tva.t_enter, n)) ||
        (rc = dl(mat.h_tr_t1, tva.t_exit, n)))
      return rc;
    r.trace_off = mat.h_tr_off.data();
    r.edge = mat.h_tr_edge.data();
    r.way = mat.h_tr_way.data();
    r.seg_id = mat.h_tr_seg.data();
    r.first_state = mat.h_tr_first.data();
    r.f0 = mat.h_tr_f0.data();
    r.f1 = mat.h_tr_f1.data();
    r.s0_mm = mat.h_tr_s0.data();
    r.s1_mm = mat.h_tr_s1.data();
    r.t_enter = mat.h_tr_t0.data();
    r.t_exit = mat.h_tr_t1.data();
  }
  HIPCHK(hipStreamSynchronize(stream));
  mat.trv_have = true;
  return OTR_OK;
}

static const char kNoTraversals[] =
    ": the matcher has run no batch, or its last otr_match_batch did not set OTR_BATCH_EDGE_TRAVERSALS";

int Matcher::edge_traversals(otr_traversal_result* out, std::string* err) const {
  if (!trv_have) {
    if (err) *err = std::string("otr_edge_traversals") + kNoTraversals;
    return OTR_BAD_REQUEST;
  }
  *out = trv;
  return OTR_OK;
}

// the speed entries of the last batch's complete traversals: keep flags, their scan, fill
int Matcher::edge_observations(int quantisation, otr_hist_entry** d_entries, int64_t* n, std::string* err) {
  return guarded(stream, err, [&]() -> int {
    *d_entries = nullptr;
    *n = 0;
    if (!trv_have) {
      if (err) *err = std::string("otr_edge_observations") + kNoTraversals;
      return OTR_BAD_REQUEST;
    }
    const int64_t nt = trv.n_traversals;
    if (nt <= 0) return OTR_OK;
    if (nt >= (int64_t)INT32_MAX) {
      if (err) *err = "too many traversals for one call";
      return OTR_BAD_REQUEST;
    }
    GraphState& gs = graph_state();
    std::shared_lock<std::shared_mutex> graph_lock(gs.mu);
    HIPCHK(hipSetDevice(gs.device));
    TravObsArgs oa{};
    oa.n = nt;
    oa.edge = trv.d_edge;
    oa.first_state = trv.d_first_state;
    oa.f0 = trv.d_f0;
    oa.f1 = trv.d_f1;
    oa.s0_mm = trv.d_s0_mm;
    oa.s1_mm = trv.d_s1_mm;
    oa.t_enter = trv.d_t_enter;
    oa.t_exit = trv.d_t_exit;
    oa.quantisation = quantisation > 0 ? quantisation : 3600;
    oa.keep = need<int64_t>(S_TR_KEEP, (size_t)nt);
    int64_t* keep_off = need<int64_t>(S_TR_KEEP_OFF, (size_t)nt + 1);
    oa.keep_off = keep_off;
    int rc;
    Workspace tmp;  // (sized before the first launch)
    if ((rc = scan_bytes(oa.keep, keep_off + 1, (int)nt, &tmp.bytes, stream, err))) return rc;
    tmp.p = need<char>(S_TR_TMP, tmp.bytes);
    const unsigned grid = (unsigned)std::min<int64_t>(kTravObsGrid, (nt + 255) / 256);
    k_trav_obs_keep<<<grid, 256, 0, stream>>>(oa);
    HIPCHK(hipMemsetAsync(keep_off, 0, 8, stream));
    if ((rc = inclusive_sum(tmp, oa.keep, keep_off + 1, (int)nt, stream, err))) return rc;
    int64_t ne = 0;
    if ((rc = read_back(stream, err, fetch(&ne, keep_off + nt)))) return rc;
    if (ne < 0 || ne > nt) {
      if (err) *err = "edge observations: the keep scan failed";
      return OTR_DEVICE_ERROR;
    }
    oa.entries = need<otr_hist_entry>(S_TR_ENTRIES, (size_t)ne);
    if (ne > 0) k_trav_obs_fill<<<grid, 256, 0, stream>>>(gs.dg, oa);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    *d_entries = oa.entries;
    *n = ne;
    return OTR_OK;
  });
}

// the work counters folded, the counts of what no tier could search and the per-trace
// output counts: one host wait per batch for all of them
int Batch::drain() {
  // the slab of segments(): {route_n, seg_n, rep_n, way_n}[T], then the folded counters (k_ctr_fold
  // stores them there) and the two fail counts (k_post): one copy into the matcher's pinned buffer
  const size_t words = 4 * (size_t)T + n_ctr + 2;
  unsigned long long* slab = (unsigned long long*)sa.route_n;
  k_ctr_fold<<<(unsigned)n_ctr, kCShards, 0, stream>>>(d_counters, slab + 4 * (size_t)T);
  if (int rc = mat.post({Matcher::MailRun{cnt + C_TASKS_LEFT, 1}, Matcher::MailRun{cnt + C_PATHS_LEFT, 1}},
                        slab + 4 * (size_t)T + n_ctr, err))
    return rc;
  if (mat.h_drain_words < words) {
    if (mat.h_drain) (void)hipHostFree(mat.h_drain);
    mat.h_drain = nullptr;
    mat.h_drain_words = 0;
    HIPCHK(hipHostMalloc((void**)&mat.h_drain, 8 * (words + words / 4), hipHostMallocDefault));
    mat.h_drain_words = words + words / 4;
  }
  HIPCHK(hipMemcpyAsync(mat.h_drain, slab, 8 * words, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  const int64_t* h = (const int64_t*)mat.h_drain;
  route_n = h, seg_n = h + T, rep_n = h + 2 * (size_t)T, way_n = h + 3 * (size_t)T;
  hc = mat.h_drain + 4 * (size_t)T;
  h_fail[0] = hc[n_ctr];
  h_fail[1] = hc[n_ctr + 1];
  return OTR_OK;
}

// OTR_DEBUG_FAIL diagnostic: which stage left searches beyond every tier, which tiers saw them
int Batch::debug_fail() {
  if (h_fail[0] + h_fail[1] > 0 && getenv("OTR_DEBUG_FAIL")) {
    unsigned long long hc2[C_CURSORS];
    HIPCHK(hipMemcpy(hc2, cnt, 8 * C_CURSORS, hipMemcpyDeviceToHost));
    fprintf(stderr, "otr: %llu route tasks, %llu paths beyond every tier; tier lists:", h_fail[0], h_fail[1]);
    for (int k = 0; k < C_CURSORS; ++k) fprintf(stderr, " %llu", hc2[k]);
    fprintf(stderr, "\n");
    if (h_fail[1]) {  // the first failing winner paths: state, its step's bound and winning route
      const int64_t* steps_d = need<int64_t>(S_LIST2, 1);
      std::vector<int64_t> ks(std::min<unsigned long long>(h_fail[1], 6));
      HIPCHK(hipMemcpy(ks.data(), list, 8 * ks.size(), hipMemcpyDeviceToHost));
      for (int64_t k : ks) {
        int64_t s = 0, sp = 0, to = 0;
        int32_t wi = 0, wj = 0, K = 0;
        double bd = 0;
        HIPCHK(hipMemcpy(&s, steps_d + k, 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&sp, sb.prev + s, 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&wj, need<int32_t>(S_WINNER, 1) + s, 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&wi, need<int32_t>(S_WINNER, 1) + sp, 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&K, cb.count + s, 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&to, trans_off + s, 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&bd, sb.bound + s, 8, hipMemcpyDeviceToHost));
        uint32_t r = 0;
        HIPCHK(hipMemcpy(&r, trans + to + (int64_t)wi * K + wj, 4, hipMemcpyDeviceToHost));
        fprintf(stderr, "otr: step k %lld state %lld prev %lld winners %d/%d K %d trans_off %lld bound %.3f route %u\n",
                (long long)k, (long long)s, (long long)sp, wi, wj, K, (long long)to, bd, r);
      }
    }
  }
  return OTR_OK;
}

// tasks / steps beyond a 1M-state slab (never seen): name the traces (task/step -> state -> trace)
int Batch::name_failed() {
  if (h_fail[0] + h_fail[1] > 0) {
    for (int which = 0; which < 2; ++which) {
      const unsigned long long nf = h_fail[which];
      if (!nf) continue;
      std::vector<int64_t> idx(nf), st(nf);
      HIPCHK(hipMemcpy(idx.data(), which == 0 ? fail_tasks : list, 8 * nf, hipMemcpyDeviceToHost));
      const int64_t* src = need<int64_t>(S_LIST2, 1);  // (steps: the step list; tasks: their records)
      for (unsigned long long k = 0; k < nf; ++k) {
        int64_t sidx = 0;
        int32_t t = 0;
        if (which == 0) {
          uint32_t s32 = 0;
          HIPCHK(hipMemcpy(&s32, task_rec + 3 * idx[k], 4, hipMemcpyDeviceToHost));
          sidx = s32;
        } else {
          HIPCHK(hipMemcpy(&sidx, src + idx[k], 8, hipMemcpyDeviceToHost));
        }
        HIPCHK(hipMemcpy(&t, state_trace + sidx, 4, hipMemcpyDeviceToHost));
        if (t >= 0 && t < T && mat.h_trace_status[t] == OTR_OK) {
          mat.h_trace_status[t] = OTR_MATCH_ERROR;
          ++out->n_overflow_traces;
        }
      }
    }
  }
  return OTR_OK;
}

// the folded work counters into otr_batch_result's counters and route_tier_work (each tier
// from its bank, otr_tiers.h), and the stage and tier times
void Batch::fold_counters() {
  const int bank_first = kRouteTiers[SLOT_FIRST].bank;  // (also the batch's own counters)
  for (int k = 0; k < OTR_COUNTERS; ++k) out->counters[k] = ctr(bank_first, k);
  for (int k : {3, 4, 13, 14})  // (the first tier: every launch)
    out->counters[k] += ctr(kRouteTiers[SLOT_SMALL].bank, k) + ctr(kRouteTiers[SLOT_TINY].bank, k);
  out->counters[11] = out->counters[12] = 0;
  // per route kernel: searches, settled, relaxed, transition entries
  for (int t = 0; t < kRouteSlots; ++t) {
    const int tb_ = kRouteTiers[t].bank;
    const TierKind kind = kRouteTiers[t].kind;
    out->route_tier_work[t][0] = ctr(tb_, 6);
    out->route_tier_work[t][1] = ctr(tb_, 3);
    out->route_tier_work[t][2] = ctr(tb_, 4);
    out->route_tier_work[t][3] = ctr(tb_, 5);
    if (kind == TierKind::NodeRetry || kind == TierKind::Wide64) {  // the LDS retry tiers together (counters 9 / 10)
      out->counters[9] += ctr(tb_, 3);
      out->counters[10] += ctr(tb_, 4);
    }
    if (kind == TierKind::NodeRetry) {  // node searches resumed from / dumped to a retry tier's dump
      out->counters[11] += ctr(tb_, 11);
      out->counters[12] += ctr(tb_, 12);
    }
  }
  out->counters[5] = (uint64_t)NT;
  out->counters[6] = (uint64_t)NTR;
  // edge-state searches resumed from a dump (the 512- and 1024-state tiers) and dumped
  // (the first two edge tiers), with OTR_BATCH_ROUTE_WORK
  out->counters[22] = ctr(kRouteTiers[kEdgeSlots[1]].bank, 22) + ctr(kRouteTiers[kEdgeSlots[2]].bank, 22);
  out->counters[23] = ctr(kRouteTiers[kEdgeSlots[0]].bank, 23) + ctr(kRouteTiers[kEdgeSlots[1]].bank, 23);
  if (!(in->flags & OTR_BATCH_TILE_ROWS)) out->n_rows = (int64_t)out->counters[8];
  else out->counters[8] = (uint64_t)out->n_rows;  // K9 counted them (K8 may not have run)
  out->d_hist = ha.hist;
  out->hist_len = (int64_t)hist_len;
  out->kernel_ms[OTR_VITERBI_VARIANT] = (float)vit_variant;  // (a code, not a time: otr.h)
  if (timing) {
    for (int k = 0; k < 10; ++k)
      if (used[k]) (void)hipEventElapsedTime(&out->kernel_ms[k], mat.ev[2 * k], mat.ev[2 * k + 1]);
    for (int t = 0; t < kRouteSlots; ++t)
      if (t != SLOT_FIRST && out->route_tier_code[t] != 0)
        (void)hipEventElapsedTime(&out->route_tier_ms[t], mat.ev[route_event(t)], mat.ev[route_event(t) + 1]);
    // (the route stage holds the tiny and small tiers' launches, then the two-search tier's)
    out->route_tier_ms[SLOT_FIRST] =
        out->kernel_ms[OTR_STAGE_ROUTE] - out->route_tier_ms[SLOT_SMALL] - out->route_tier_ms[SLOT_TINY];
    (void)hipGetLastError();  // an unrecorded pair must not leave a sticky error for the next call
  }
}

// ---- copy-out (tests / JSON path), compacting the capacity layout
int Batch::copy_out() {
  int rc;
  int64_t nroute = 0, nseg = 0, nrep = 0;
  for (int t = 0; t < T; ++t) {
    nroute += route_n[t];
    nseg += seg_n[t];
    nrep += rep_n[t];
  }
  out->n_route = nroute;
  out->n_seg = nseg;
  out->n_rep = nrep;
  out->status = out->n_overflow_traces ? OTR_MATCH_ERROR : OTR_OK;
  const bool full = (in->flags & OTR_BATCH_COPY_OUT) != 0;
  if (!full && !(in->flags & OTR_BATCH_COPY_REPORTS)) return OTR_OK;
  out->trace_status = mat.h_trace_status.data();
  if (full) {
    if ((rc = dl(mat.h_trace_state_off, trace_state_off, T + 1))) return rc;
    if ((rc = dl(mat.h_state_probe, state_probe, S))) return rc;
    if ((rc = dl(mat.h_cand_count, cb.count, S))) return rc;
    if ((rc = dl(mat.h_cand_edge, cb.edge, (size_t)S * OTR_KMAX))) return rc;
    if ((rc = dl(mat.h_cand_p, cb.p, (size_t)S * OTR_KMAX))) return rc;
    if ((rc = dl(mat.h_cand_sqd, cb.sqd, (size_t)S * OTR_KMAX))) return rc;
    if ((rc = dl(mat.h_winner, va.winner, S))) return rc;
    if ((rc = dl(mat.h_subpath, va.subpath, S))) return rc;
  }
  if ((rc = dl(mat.h_shape_used, sa.shape_used, T))) return rc;
  if ((rc = dl(mat.h_stats, sa.stats, 7 * (size_t)T))) return rc;
  if ((rc = dl(mat.h_stats_len, sa.stats_len, 2 * (size_t)T))) return rc;
  // dense layout on device (k_compact), then only the used entries cross PCIe
  int64_t nway = 0;
  for (int t = 0; t < T; ++t) nway += way_n[t];
  CompactArgs ca{};
  ca.n_traces = T;
  ca.cap_off = cap_off;
  int64_t* route_off = need<int64_t>(S_C_ROUTE_OFF, T + 1);
  int64_t* seg_off = need<int64_t>(S_C_SEG_OFF, T + 1);
  int64_t* way_off = need<int64_t>(S_C_WAY_OFF, T + 1);
  int64_t* rep_off = need<int64_t>(S_C_REP_OFF, T + 1);
  if ((rc = scan(sa.seg_n, seg_off, T)) || (rc = scan(sa.way_n, way_off, T)) || (rc = scan(sa.rep_n, rep_off, T)))
    return rc;
  if (full && (rc = scan(sa.route_n, route_off, T))) return rc;
  ca.route_off = full ? route_off : nullptr;
  ca.seg_off = seg_off;
  ca.way_off = way_off;
  ca.rep_off = rep_off;
  // K7's arguments for k_compact: uploaded from pinned memory (the mailbox: the stream is idle
  // since drain()), and only when they or their buffer changed since this matcher's last upload
  SegArgs* d_sa = need<SegArgs>(S_C_ARGS, 1);
  static_assert(sizeof(SegArgs) <= 8 * Matcher::kMailWords, "SegArgs goes through the mailbox");
  if (mat.seg_args_dev != d_sa || mat.seg_args.size() != sizeof(SegArgs) ||
      memcmp(mat.seg_args.data(), &sa, sizeof(SegArgs)) != 0) {
    mat.seg_args_dev = nullptr;
    mat.seg_args.assign((const char*)&sa, (const char*)&sa + sizeof(SegArgs));
    memcpy(mat.mail, &sa, sizeof(SegArgs));
    HIPCHK(hipMemcpyAsync(d_sa, mat.mail, sizeof(SegArgs), hipMemcpyHostToDevice, stream));
    mat.seg_args_dev = d_sa;
  }
  ca.s = d_sa;
  auto n1 = [](int64_t n) { return (size_t)(n > 0 ? n : 1); };
  ca.route = need<uint32_t>(S_C_ROUTE, n1(nroute));
  ca.seg_id = need<unsigned long long>(S_C_SEG_ID, n1(nseg));
  ca.seg_start = need<double>(S_C_SEG_START, n1(nseg));
  ca.seg_end = need<double>(S_C_SEG_END, n1(nseg));
  ca.seg_length = need<int32_t>(S_C_SEG_LEN, n1(nseg));
  ca.seg_queue = need<int32_t>(S_C_SEG_QUEUE, n1(nseg));
  ca.seg_internal = need<uint8_t>(S_C_SEG_INTERNAL, n1(nseg));
  ca.seg_bshape = need<int32_t>(S_C_SEG_BSHAPE, n1(nseg));
  ca.seg_eshape = need<int32_t>(S_C_SEG_ESHAPE, n1(nseg));
  ca.seg_way_n = need<int64_t>(S_C_SEG_WAY_N, n1(nseg));
  ca.seg_way = need<uint32_t>(S_C_SEG_WAY, n1(nway));
  ca.rep_id = need<unsigned long long>(S_C_REP_ID, n1(nrep));
  ca.rep_next = need<unsigned long long>(S_C_REP_NEXT, n1(nrep));
  ca.rep_t0 = need<double>(S_C_REP_T0, n1(nrep));
  ca.rep_t1 = need<double>(S_C_REP_T1, n1(nrep));
  ca.rep_length = need<int32_t>(S_C_REP_LEN, n1(nrep));
  ca.rep_queue = need<int32_t>(S_C_REP_QUEUE, n1(nrep));
  k_compact<<<(unsigned)grid_compact(T).blocks, 64, 0, stream>>>(ca);
  int64_t* seg_way_off = need<int64_t>(S_C_SEG_WAY_OFF, (size_t)nseg + 1);
  if ((rc = scan(ca.seg_way_n, seg_way_off, nseg))) return rc;
  HIPCHK(hipGetLastError());
  if (full && (rc = dl(mat.h_route_edge, ca.route, nroute))) return rc;
  if (!full) mat.h_route_edge.clear();
  if ((rc = dl(mat.h_seg_id, ca.seg_id, nseg)) || (rc = dl(mat.h_seg_start, ca.seg_start, nseg)) ||
      (rc = dl(mat.h_seg_end, ca.seg_end, nseg)) || (rc = dl(mat.h_seg_length, ca.seg_length, nseg)) ||
      (rc = dl(mat.h_seg_queue, ca.seg_queue, nseg)) || (rc = dl(mat.h_seg_internal, ca.seg_internal, nseg)) ||
      (rc = dl(mat.h_seg_bshape, ca.seg_bshape, nseg)) || (rc = dl(mat.h_seg_eshape, ca.seg_eshape, nseg)) ||
      (rc = dl(mat.h_seg_way_off, seg_way_off, (size_t)nseg + 1)) || (rc = dl(mat.h_seg_way, ca.seg_way, nway)) ||
      (rc = dl(mat.h_rep_id, ca.rep_id, nrep)) || (rc = dl(mat.h_rep_next, ca.rep_next, nrep)) ||
      (rc = dl(mat.h_rep_t0, ca.rep_t0, nrep)) || (rc = dl(mat.h_rep_t1, ca.rep_t1, nrep)) ||
      (rc = dl(mat.h_rep_length, ca.rep_length, nrep)) || (rc = dl(mat.h_rep_queue, ca.rep_queue, nrep)))
    return rc;
  HIPCHK(hipStreamSynchronize(stream));
  mat.h_trace_route_off.assign(T + 1, 0);
  mat.h_trace_seg_off.assign(T + 1, 0);
  mat.h_trace_rep_off.assign(T + 1, 0);
  for (int t = 0; t < T; ++t) {
    mat.h_trace_route_off[t + 1] = mat.h_trace_route_off[t] + route_n[t];
    mat.h_trace_seg_off[t + 1] = mat.h_trace_seg_off[t] + seg_n[t];
    mat.h_trace_rep_off[t + 1] = mat.h_trace_rep_off[t] + rep_n[t];
  }
  auto P = [](auto& v) { return v.empty() ? nullptr : v.data(); };
  if (full) {
    out->trace_state_off = P(mat.h_trace_state_off);
    out->state_probe = P(mat.h_state_probe);
    out->cand_count = P(mat.h_cand_count);
    out->cand_edge = P(mat.h_cand_edge);
    out->cand_p = P(mat.h_cand_p);
    out->cand_sqd = P(mat.h_cand_sqd);
    out->winner = P(mat.h_winner);
    out->subpath = P(mat.h_subpath);
    out->trace_route_off = P(mat.h_trace_route_off);
    out->route_edge = P(mat.h_route_edge);
  }
  out->trace_seg_off = P(mat.h_trace_seg_off);
  out->seg_id = (uint64_t*)P(mat.h_seg_id);
  out->seg_start = P(mat.h_seg_start);
  out->seg_end = P(mat.h_seg_end);
  out->seg_length = P(mat.h_seg_length);
  out->seg_queue = P(mat.h_seg_queue);
  out->seg_internal = P(mat.h_seg_internal);
  out->seg_begin_shape = P(mat.h_seg_bshape);
  out->seg_end_shape = P(mat.h_seg_eshape);
  out->seg_way_off = P(mat.h_seg_way_off);
  out->seg_way = P(mat.h_seg_way);
  out->trace_rep_off = P(mat.h_trace_rep_off);
  out->rep_id = (uint64_t*)P(mat.h_rep_id);
  out->rep_next = (uint64_t*)P(mat.h_rep_next);
  out->rep_t0 = P(mat.h_rep_t0);
  out->rep_t1 = P(mat.h_rep_t1);
  out->rep_length = P(mat.h_rep_length);
  out->rep_queue = P(mat.h_rep_queue);
  out->shape_used = P(mat.h_shape_used);
  out->stats = P(mat.h_stats);
  out->stats_len = P(mat.h_stats_len);
  return OTR_OK;
}

// report() over many segment lists on the device (include/otr.h otr_report_lists_device):
// one thread per list runs the report_segments K7 runs.
__global__ void k_report_lists(ReportLists a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.n) return;
  const int64_t o = a.seg_off[c];
  ReportStats rs;
  report_segments((int32_t)(a.seg_off[c + 1] - o), a.seg_id + o, a.start + o, a.end + o, a.internal + o, a.queue + o,
                  a.has_length + o, a.length + o, a.begin_shape + o, nullptr, a.end_time[c], a.threshold[c], a.rl[c],
                  a.tl[c], a.rep_id + o, a.rep_next + o, a.rep_t0 + o, a.rep_t1 + o, a.rep_length + o, a.rep_queue + o,
                  nullptr, &rs);
  a.n_rep[c] = rs.n_rep;
  a.shape_used[c] = rs.shape_used;
  for (int k = 0; k < 6; ++k) a.counts[6 * c + k] = rs.counts[k];
  for (int k = 0; k < 2; ++k) {
    a.lengths[2 * c + k] = rs.lengths[k];
    a.length_set[2 * c + k] = rs.length_set[k];
  }
}

int report_lists_device(const ReportLists& h, std::string* err) {
  GraphState& gs = graph_state();
  HIPCHK(hipSetDevice(gs.device));
  const int32_t n = h.n;
  if (n <= 0) return OTR_OK;
  const int64_t S = h.seg_off[n];
  std::vector<void*> mem;
  bool ok = true;
  auto put = [&](const void* src, size_t bytes) -> void* {
    void* d = nullptr;
    if (hipMalloc(&d, bytes ? bytes : 16) != hipSuccess) ok = false;
    mem.push_back(d);
    if (ok && bytes && src && hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) ok = false;
    return d;
  };
  ReportLists d = h;
  d.seg_off = (const int64_t*)put(h.seg_off, 8ull * (n + 1));
  d.seg_id = (const unsigned long long*)put(h.seg_id, 8ull * S);
  d.start = (const double*)put(h.start, 8ull * S);
  d.end = (const double*)put(h.end, 8ull * S);
  d.internal = (const uint8_t*)put(h.internal, (size_t)S);
  d.queue = (const int32_t*)put(h.queue, 4ull * S);
  d.has_length = (const uint8_t*)put(h.has_length, (size_t)S);
  d.length = (const int32_t*)put(h.length, 4ull * S);
  d.begin_shape = (const int32_t*)put(h.begin_shape, 4ull * S);
  d.end_time = (const int64_t*)put(h.end_time, 8ull * n);
  d.threshold = (const double*)put(h.threshold, 8ull * n);
  d.rl = (const uint32_t*)put(h.rl, 4ull * n);
  d.tl = (const uint32_t*)put(h.tl, 4ull * n);
  d.rep_id = (unsigned long long*)put(nullptr, 8ull * S);
  d.rep_next = (unsigned long long*)put(nullptr, 8ull * S);
  d.rep_t0 = (double*)put(nullptr, 8ull * S);
  d.rep_t1 = (double*)put(nullptr, 8ull * S);
  d.rep_length = (int32_t*)put(nullptr, 4ull * S);
  d.rep_queue = (int32_t*)put(nullptr, 4ull * S);
  d.n_rep = (int32_t*)put(nullptr, 4ull * n);
  d.shape_used = (int32_t*)put(nullptr, 4ull * n);
  d.counts = (int32_t*)put(nullptr, 24ull * n);
  d.lengths = (double*)put(nullptr, 16ull * n);
  d.length_set = (int32_t*)put(nullptr, 8ull * n);
  auto release = [&] {
    for (void* q : mem)
      if (q) (void)hipFree(q);
  };
  if (!ok) {
    release();
    if (err) *err = "device allocation failed (report lists)";
    return OTR_DEVICE_ERROR;
  }
  k_report_lists<<<grid_ceil(n, 128), 128>>>(d);
  hipError_t e = hipDeviceSynchronize();
  auto get = [&](void* dst, const void* src, size_t bytes) {
    if (e == hipSuccess && bytes) e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
  };
  get(h.rep_id, d.rep_id, 8ull * S);
  get(h.rep_next, d.rep_next, 8ull * S);
  get(h.rep_t0, d.rep_t0, 8ull * S);
  get(h.rep_t1, d.rep_t1, 8ull * S);
  get(h.rep_length, d.rep_length, 4ull * S);
  get(h.rep_queue, d.rep_queue, 4ull * S);
  get(h.n_rep, d.n_rep, 4ull * n);
  get(h.shape_used, d.shape_used, 4ull * n);
  get(h.counts, d.counts, 24ull * n);
  get(h.lengths, d.lengths, 16ull * n);
  get(h.length_set, d.length_set, 8ull * n);
  release();
  if (e != hipSuccess) {
    if (err) *err = std::string("HIP error: ") + hipGetErrorString(e);
    return OTR_DEVICE_ERROR;
  }
  return OTR_OK;
}

}  // namespace otr
