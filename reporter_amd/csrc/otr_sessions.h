// otr_sessions.h — K14: the streaming reporter's per-key sessions in HBM (include/otr.h
// otr_sessions_*): an open-addressing table of 64-bit keys, per session
// {n, max_sep, last_update} and SoA points, the report gate, the shape_used trim and the
// eviction of quiet sessions.  The passes are ordered by kernel boundaries only: no lane
// ever waits on another lane's store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/otr.h"
#include "otr_device.h"
#include "otr_session_names.h"
#include "otr_session_records.h"

namespace otr {

constexpr unsigned long long kSesEmpty = OTR_NO_ID;  // the table's empty mark (refused as a key)
constexpr int32_t kSesNew = -1;                       // entry without a session yet (and every empty entry)
constexpr int32_t kSesDead = -2;                      // entry of a deleted key
// counter words of the store
enum { SES_NFREE = 0, SES_DEAD, SES_FORCED, SES_DROPPED, SES_FLAGS, SES_WORDS };
constexpr int32_t kSesFlagNoId = 1, kSesFlagFull = 2;

struct SesTable {
  unsigned long long* key;  // [cap]
  int32_t* slot;            // [cap]: session index, kSesNew or kSesDead
  uint32_t cap;
};

struct SesStore {
  int32_t* n;                // [max_sessions] points held; 0: no session
  float* max_sep;            // Batch.java max_separation (float)
  int64_t* last;             // last_update
  unsigned long long* skey;  // the session's key
  int32_t* entry;            // its table entry
  float *lat, *lon;          // [max_sessions * max_points]
  int32_t* acc;
  int64_t* time;
  int32_t max_sessions, max_points;
};

struct SesChunk {
  int64_t n;
  const unsigned long long* key;
  const float *lat, *lon;
  const int32_t* acc;
  const int64_t *time, *ts;
};

struct SesGate {
  float dist;
  int32_t count;
  int64_t time;
};

__host__ __device__ inline uint32_t ses_hash(unsigned long long k, uint32_t cap) {
  k ^= k >> 30;
  k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27;
  k *= 0x94d049bb133111ebull;
  k ^= k >> 31;
  return (uint32_t)(k % cap);
}

// Batch.java:37-41 with Point's float fields: the differences and the mid latitude in
// binary32, the rest in binary64, one operation at a time (the build has no contraction)
__host__ __device__ inline double ses_dist(float alat, float alon, float blat, float blon) {
  const float dlon = alon - blon;
  const float mid = 0.5f * (alat + blat);
  const float dlat = alat - blat;
  const double x = ((double)dlon * kMetersPerDeg) * cos_deg((double)mid);
  const double y = (double)dlat * kMetersPerDeg;
  return sqrt(x * x + y * y);
}

// what Point.Serder.put_json's "###.######" text parses back to: rint(f * 1e6) / 1e6
// ((double)f * 1e6 is exact: 24 bits times 15625 * 2^6)
__host__ __device__ inline double ses_widen(float f) { return rint((double)f * 1e6) / 1e6; }

// one lane per point: find the key's entry or claim an empty one.  Entries only go from
// empty to a key inside this kernel, and every lane of a key walks the same chain, so all
// of them end at one entry; the lane whose CAS claimed it is the key's creator.
__global__ void k_ses_insert(SesTable t, SesChunk c, int32_t* lane_entry, int32_t* is_new, int32_t* cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.n) return;
  const unsigned long long key = c.key[i];
  int32_t entry = -1, fresh = 0;
  if (key == kSesEmpty) {
    atomicOr(&cnt[SES_FLAGS], kSesFlagNoId);
  } else {
    uint32_t e = ses_hash(key, t.cap);
    for (uint32_t probe = 0; probe < t.cap; ++probe) {
      unsigned long long k = t.key[e];
      if (k == kSesEmpty) {
        k = atomicCAS(&t.key[e], kSesEmpty, key);
        if (k == kSesEmpty) {
          entry = (int32_t)e;
          fresh = 1;
          break;
        }
      }
      if (k == key && t.slot[e] != kSesDead) {
        entry = (int32_t)e;
        break;
      }
      e = e + 1 == t.cap ? 0 : e + 1;
    }
    if (entry < 0) atomicOr(&cnt[SES_FLAGS], kSesFlagFull);
  }
  lane_entry[i] = entry;
  is_new[i] = fresh;
}

// a refused chunk: the claimed entries are empty again (they were before)
__global__ void k_ses_rollback(SesTable t, int64_t n, const int32_t* lane_entry, const int32_t* is_new) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && is_new[i]) t.key[lane_entry[i]] = kSesEmpty;
}

// creators take a session from the top of the free stack, by their rank among the creators
__global__ void k_ses_assign(SesTable t, SesStore s, SesChunk c, const int32_t* lane_entry, const int32_t* is_new,
                             const int32_t* rank_incl, const int32_t* free_list, int32_t n_free) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.n || !is_new[i]) return;
  const int32_t slot = free_list[n_free - rank_incl[i]];
  const int32_t e = lane_entry[i];
  t.slot[e] = slot;
  s.n[slot] = 0;
  s.max_sep[slot] = 0.f;
  s.last[slot] = 0;
  s.skey[slot] = c.key[i];
  s.entry[slot] = e;
}

__global__ void k_ses_add(int32_t* word, int32_t v) { *word += v; }

__global__ void k_ses_lane_slot(SesTable t, int64_t n, const int32_t* lane_entry, uint32_t* lane_slot, int32_t* idx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  lane_slot[i] = (uint32_t)t.slot[lane_entry[i]];
  idx[i] = (int32_t)i;
}

__global__ void k_ses_heads(const uint32_t* sorted_slot, int64_t n, int32_t* head) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) head[i] = (i == 0 || sorted_slot[i] != sorted_slot[i - 1]) ? 1 : 0;
}

// segment g (a key's points of the chunk, in arrival order): its session and [cur, end)
__global__ void k_ses_segments(const uint32_t* sorted_slot, const int32_t* seg_incl, int64_t n, int32_t* seg_slot,
                               int32_t* seg_cur, int32_t* seg_end) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t g = seg_incl[i] - 1;
  if (i == 0 || sorted_slot[i] != sorted_slot[i - 1]) {
    seg_slot[g] = (int32_t)sorted_slot[i];
    seg_cur[g] = (int32_t)i;
  }
  if (i == n - 1 || sorted_slot[i] != sorted_slot[i + 1]) seg_end[g] = (int32_t)i + 1;
}

// one lane per key with unconsumed points: BatchingProcessor.process point by point until
// the gate passes (trip_at[arrival index] = 1) or the points run out.  Serial by definition.
__global__ void k_ses_advance(int32_t n_seg, const int32_t* seg_slot, int32_t* seg_cur, const int32_t* seg_end,
                              const int32_t* sorted_idx, SesChunk c, SesStore s, SesGate gate, int32_t* trip_at,
                              int32_t* cnt) {
  const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_seg) return;
  int32_t pos = seg_cur[g];
  const int32_t end = seg_end[g];
  if (pos >= end) return;
  const int32_t slot = seg_slot[g];
  const size_t base = (size_t)slot * (size_t)s.max_points;
  int32_t n = s.n[slot];
  float ms = s.max_sep[slot];
  float lat0 = 0.f, lon0 = 0.f;
  int64_t t0 = 0, last = 0;
  if (n > 0) {
    lat0 = s.lat[base];
    lon0 = s.lon[base];
    t0 = s.time[base];
  }
  while (pos < end) {
    const int32_t i = sorted_idx[pos];
    ++pos;
    const float la = c.lat[i], lo = c.lon[i];
    const int64_t tm = c.time[i];
    last = c.ts[i];
    s.lat[base + n] = la;
    s.lon[base + n] = lo;
    s.acc[base + n] = c.acc[i];
    s.time[base + n] = tm;
    if (n == 0) {  // no session: it becomes [p]
      lat0 = la;
      lon0 = lo;
      t0 = tm;
      ms = 0.f;
      n = 1;
      continue;
    }
    const double d = ses_dist(la, lo, lat0, lon0);
    ms = (float)(d > (double)ms ? d : (double)ms);
    ++n;
    bool report = !(ms < gate.dist || n < gate.count || tm - t0 < gate.time);
    if (!report && n == s.max_points) {  // the cap: reported as at eviction, or cleared
      if (tm - t0 >= 0) {
        report = true;
        atomicAdd(&cnt[SES_FORCED], 1);
      } else {
        atomicAdd(&cnt[SES_DROPPED], 1);
        n = 0;
        continue;
      }
    }
    if (report) {
      trip_at[i] = 1;
      break;
    }
  }
  s.n[slot] = n;
  s.max_sep[slot] = ms;
  s.last[slot] = last;
  seg_cur[g] = pos;
}

// the tripped keys in ascending trigger order
__global__ void k_ses_windows(int64_t n, int32_t* trip_at, const int32_t* trip_incl, const uint32_t* lane_slot,
                              SesStore s, int32_t* win_slot, int64_t* win_trig, int64_t* win_n,
                              unsigned long long* win_key) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !trip_at[i]) return;
  trip_at[i] = 0;
  const int32_t w = trip_incl[i] - 1;
  const int32_t slot = (int32_t)lane_slot[i];
  win_slot[w] = slot;
  win_trig[w] = i;
  win_n[w] = s.n[slot];
  win_key[w] = s.skey[slot];
}

// one wave per window: its points into the batch (coordinates as the matcher's JSON caller
// would read them) or, RAW, as they are stored (the snapshot)
template <bool RAW>
__global__ __launch_bounds__(64) void k_ses_gather(int32_t n_win, const int32_t* win_slot, const int64_t* off,
                                                   SesStore s, double* lat, double* lon, int64_t* time, float* acc,
                                                   uint8_t* mode, uint8_t mode_value, float* rlat, float* rlon,
                                                   int32_t* racc) {
  const int32_t w = blockIdx.x;
  if (w >= n_win) return;
  const int32_t slot = win_slot[w];
  const size_t base = (size_t)slot * (size_t)s.max_points;
  const int64_t o = off[w];
  const int32_t n = (int32_t)(off[w + 1] - o);
  for (int32_t k = threadIdx.x; k < n; k += 64) {
    time[o + k] = s.time[base + k];
    if (RAW) {
      rlat[o + k] = s.lat[base + k];
      rlon[o + k] = s.lon[base + k];
      racc[o + k] = s.acc[base + k];
    } else {
      lat[o + k] = ses_widen(s.lat[base + k]);
      lon[o + k] = ses_widen(s.lon[base + k]);
      acc[o + k] = (float)s.acc[base + k];
    }
  }
  if (!RAW && threadIdx.x == 0) mode[w] = mode_value;
}

// one wave per window: Batch.java:73-80.  The kept points move to the front in blocks of 64,
// upwards; a block is read completely (one load instruction of the wave) before it is
// written, and block b writes below everything the later blocks still read.
__global__ __launch_bounds__(64) void k_ses_commit(int32_t n_win, const int32_t* win_slot, const int32_t* shape_used,
                                                   const int32_t* status, SesStore s, int32_t* win_su,
                                                   int32_t* win_trim) {
  const int32_t w = blockIdx.x;
  if (w >= n_win) return;
  const int32_t slot = win_slot[w];
  const size_t base = (size_t)slot * (size_t)s.max_points;
  const int32_t n = s.n[slot];
  const int32_t su = (status[w] == OTR_OK && shape_used[w] > 0) ? shape_used[w] : -1;
  const int32_t trim = su > 0 && su < n ? su : n;
  const int32_t kept = n - trim;
  float ms = 0.f;
  if (kept > 0) {
    const float lat0 = s.lat[base + trim], lon0 = s.lon[base + trim];
    for (int32_t b = 0; b < kept; b += 64) {
      const int32_t k = b + (int32_t)threadIdx.x;
      const bool on = k < kept;
      float la = 0.f, lo = 0.f;
      int32_t ac = 0;
      int64_t tm = 0;
      if (on) {
        la = s.lat[base + trim + k];
        lo = s.lon[base + trim + k];
        ac = s.acc[base + trim + k];
        tm = s.time[base + trim + k];
      }
      __builtin_amdgcn_wave_barrier();
      if (on) {
        s.lat[base + k] = la;
        s.lon[base + k] = lo;
        s.acc[base + k] = ac;
        s.time[base + k] = tm;
        if (k > 0) {
          const float d = (float)ses_dist(la, lo, lat0, lon0);
          ms = d > ms ? d : ms;
        }
      }
    }
    for (int sh = 32; sh > 0; sh >>= 1) {
      const float o = __shfl_xor(ms, sh, 64);
      ms = o > ms ? o : ms;
    }
  }
  if (threadIdx.x == 0) {
    s.n[slot] = kept;
    s.max_sep[slot] = ms;
    win_su[w] = su;
    win_trim[w] = trim;
  }
}

// sessions left empty are deleted: the entry is dead, the session back on the free stack
__global__ void k_ses_release(int32_t n_list, const int32_t* list, SesTable t, SesStore s, int32_t* free_list,
                              int32_t* cnt) {
  const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_list) return;
  const int32_t slot = list[g];
  if (s.n[slot] != 0) return;
  t.slot[s.entry[slot]] = kSesDead;
  s.skey[slot] = kSesEmpty;
  free_list[atomicAdd(&cnt[SES_NFREE], 1)] = slot;
  atomicAdd(&cnt[SES_DEAD], 1);
}

__global__ void k_ses_clear(int32_t n_list, const int32_t* list, SesStore s) {
  const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n_list) s.n[list[g]] = 0;
}

// the live sessions into a fresh table (keys are distinct: every CAS on an empty entry wins
// or meets another key)
__global__ void k_ses_rebuild(SesTable from, SesTable to, SesStore s) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= from.cap) return;
  const int32_t slot = from.slot[e];
  if (slot < 0) return;
  const unsigned long long key = from.key[e];
  uint32_t q = ses_hash(key, to.cap);
  for (uint32_t probe = 0; probe < to.cap; ++probe) {
    if (to.key[q] == kSesEmpty && atomicCAS(&to.key[q], kSesEmpty, key) == kSesEmpty) {
      to.slot[q] = slot;
      s.entry[slot] = (int32_t)q;
      return;
    }
    q = q + 1 == to.cap ? 0 : q + 1;
  }
}

// live sessions (stale_only 0) or the ones quiet for more than `gap` at `ts`
__global__ void k_ses_flag(SesStore s, int32_t stale_only, int64_t ts, int64_t gap, int32_t* flag) {
  const int32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= s.max_sessions) return;
  flag[slot] = (s.n[slot] > 0 && (!stale_only || ts - s.last[slot] > gap)) ? 1 : 0;
}

__global__ void k_ses_list(SesStore s, const int32_t* flag, const int32_t* incl, unsigned long long* key,
                           int32_t* slot_out) {
  const int32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= s.max_sessions || !flag[slot]) return;
  key[incl[slot] - 1] = s.skey[slot];
  slot_out[incl[slot] - 1] = slot;
}

// evicted sessions in key order: which report (gates 0, 2, 0), and every one's size
__global__ void k_ses_evict_gate(int32_t n_list, const int32_t* list, SesStore s, int32_t* rep, int64_t* cnt_n) {
  const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_list) return;
  const int32_t slot = list[g];
  const size_t base = (size_t)slot * (size_t)s.max_points;
  const int32_t n = s.n[slot];
  rep[g] = (n >= 2 && s.time[base + n - 1] - s.time[base] >= 0) ? 1 : 0;
  cnt_n[g] = n;
}

__global__ void k_ses_evict_windows(int32_t n_list, const int32_t* list, const unsigned long long* key,
                                    const int32_t* rep, const int32_t* rep_incl, const int64_t* cnt_n,
                                    int32_t* win_slot, int64_t* win_trig, int64_t* win_n, unsigned long long* win_key) {
  const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_list || !rep[g]) return;
  const int32_t w = rep_incl[g] - 1;
  win_slot[w] = list[g];
  win_trig[w] = -1 - (int64_t)g;
  win_n[w] = cnt_n[g];
  win_key[w] = key[g];
}

// ---- K17: restore, export and move (include/otr.h otr_sessions_restore ...) ----------------

// sessions given to a restore: SoA (off counts points, `total` is n_points) or records (off
// counts bytes, `total` is n_bytes)
struct SesGiven {
  int64_t n, total;
  const unsigned long long* key;
  const int64_t* off;  // [n + 1]
  const float *max_sep, *lat, *lon;
  const int64_t *last, *time;
  const int32_t* acc;
  const uint8_t* bytes;
};

constexpr unsigned long long kSesNoBad = ~0ull;
constexpr int32_t kSesNoLane = 0x7F7F7F7F;  // the scratch array's fill: above every lane index

__device__ inline void ses_refuse(unsigned long long* bad, int64_t i, int32_t reason) {
  atomicMin(bad, ((unsigned long long)i << 8) | (unsigned long long)reason);
}

// one lane per given session: layout, key and count, then the table walk of k_ses_insert.  A
// live key is refused; so is every occurrence of a key but its first.  The lanes of one key
// end at one entry and leave the lowest of their indices in first[entry]: a lane that finds a
// lower one there refuses itself, a lane that replaces a higher one refuses that one, so
// every occurrence but the first is refused whichever lane claimed the entry, and no lane
// waits.  bad: the lowest (index << 8 | reason), reasons in the order of their precedence.
template <bool REC>
__global__ void k_ses_restore_check(SesTable t, SesGiven g, int32_t max_points, int32_t* first, int32_t* lane_entry,
                                    int32_t* is_new, unsigned long long* bad, int32_t* cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.n) return;
  lane_entry[i] = -1;
  is_new[i] = 0;
  const int64_t b = g.off[i], e = g.off[i + 1];
  int64_t count;
  bool layout;
  if (REC) {
    int32_t c32;
    layout = rec_layout_ok(g.bytes, g.total, b, e, &c32);
    count = c32;
  } else {
    layout = !(e < b || (i == 0 && b != 0) || (i == g.n - 1 && e != g.total));
    count = e - b;
  }
  const unsigned long long key = g.key[i];
  if (!layout) return ses_refuse(bad, i, OTR_RESTORE_E_LAYOUT);
  if (key == kSesEmpty) return ses_refuse(bad, i, OTR_RESTORE_E_KEY);
  if (count < 1 || count > (int64_t)max_points - 1) return ses_refuse(bad, i, OTR_RESTORE_E_COUNT);
  uint32_t q = ses_hash(key, t.cap);
  for (uint32_t probe = 0; probe < t.cap; ++probe) {
    unsigned long long k = t.key[q];
    bool mine = false;
    if (k == kSesEmpty) {
      k = atomicCAS(&t.key[q], kSesEmpty, key);
      mine = k == kSesEmpty;
    }
    if (mine || k == key) {
      const int32_t slot = mine ? kSesNew : t.slot[q];
      if (slot >= 0) return ses_refuse(bad, i, OTR_RESTORE_E_LIVE);
      if (slot == kSesNew) {  // claimed in this call, by this lane or by another of its key
        lane_entry[i] = (int32_t)q;
        is_new[i] = mine ? 1 : 0;
        const int32_t old = atomicMin(&first[q], (int32_t)i);
        if (old < (int32_t)i) ses_refuse(bad, i, OTR_RESTORE_E_DUPLICATE);
        else if (old != kSesNoLane) ses_refuse(bad, old, OTR_RESTORE_E_DUPLICATE);
        return;
      }
      // (a dead entry of this key: the walk goes on to a new one)
    }
    q = q + 1 == t.cap ? 0 : q + 1;
  }
  atomicOr(&cnt[SES_FLAGS], kSesFlagFull);
}

// one wave per given session (none was refused, so each claimed its entry): the session from
// the free stack by its index, the points strided over the lanes; records are decoded on the
// way, byte by byte, so that neither the buffer nor a record needs any alignment
template <bool REC>
__global__ __launch_bounds__(64) void k_ses_restore_copy(SesTable t, SesStore s, SesGiven g, const int32_t* lane_entry,
                                                         const int32_t* free_list, int32_t n_free) {
  const int64_t i = blockIdx.x;
  if (i >= g.n) return;
  const int32_t slot = free_list[n_free - 1 - (int32_t)i];
  const size_t base = (size_t)slot * (size_t)s.max_points;
  const int64_t b = g.off[i];
  int32_t n;
  float ms;
  int64_t last;
  if (REC) {
    rec_header_get(g.bytes + b, &n, &ms, &last);
  } else {
    n = (int32_t)(g.off[i + 1] - b);
    ms = g.max_sep[i];
    last = g.last[i];
  }
  for (int32_t k = threadIdx.x; k < n; k += 64) {
    float la, lo;
    int32_t ac;
    int64_t tm;
    if (REC) {
      rec_point_get(g.bytes + b, k, &la, &lo, &ac, &tm);
    } else {
      la = g.lat[b + k];
      lo = g.lon[b + k];
      ac = g.acc[b + k];
      tm = g.time[b + k];
    }
    s.lat[base + k] = la;
    s.lon[base + k] = lo;
    s.acc[base + k] = ac;
    s.time[base + k] = tm;
  }
  if (threadIdx.x == 0) {
    const int32_t e = lane_entry[i];
    t.slot[e] = slot;
    s.n[slot] = n;
    s.max_sep[slot] = ms;
    s.last[slot] = last;
    s.skey[slot] = g.key[i];
    s.entry[slot] = e;
  }
}

// listed sessions: the length of each one's record
__global__ void k_ses_record_len(int32_t n_list, const int32_t* list, SesStore s, int64_t* len) {
  const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n_list) len[g] = kRecHeader + kRecPoint * (int64_t)s.n[list[g]];
}

// one wave per listed session: lane 0 writes the header, the lanes the points
__global__ __launch_bounds__(64) void k_ses_encode(int32_t n_list, const int32_t* list, const int64_t* rec_off,
                                                   SesStore s, uint8_t* bytes) {
  const int32_t g = blockIdx.x;
  if (g >= n_list) return;
  const int32_t slot = list[g];
  const size_t base = (size_t)slot * (size_t)s.max_points;
  uint8_t* rec = bytes + rec_off[g];
  const int32_t n = (int32_t)((rec_off[g + 1] - rec_off[g] - kRecHeader) / kRecPoint);
  if (threadIdx.x == 0) rec_header_put(rec, n, s.max_sep[slot], s.last[slot]);
  for (int32_t k = threadIdx.x; k < n; k += 64)
    rec_point_put(rec, k, s.lat[base + k], s.lon[base + k], s.acc[base + k], s.time[base + k]);
}

// the live sessions of one part: key % n_parts == part (the keys are mixed hashes already)
__global__ void k_ses_flag_part(SesStore s, uint32_t n_parts, uint32_t part, int32_t* flag) {
  const int32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= s.max_sessions) return;
  flag[slot] = (s.n[slot] > 0 && s.skey[slot] % n_parts == part) ? 1 : 0;
}

// ---- K18: the uuid directory (include/otr.h otr_sessions_open_named ...) ---------------------
// The name of every live session, by session slot (a table rebuild does not move it).  The
// per-name rules are otr_session_names.h's.

struct SesDir {
  uint8_t* bytes;  // [max_sessions * row]: 16-byte aligned rows, zero-filled beyond the length
  int32_t* len;    // [max_sessions]
  int32_t row, uuid_bytes;
};

// the names that come with a chunk's points or a restore's sessions (device arrays)
struct SesNamesIn {
  const uint8_t* bytes;
  int64_t n_bytes;
  const int64_t* off;
  const int32_t* len;
};

// after k_ses_insert: the first-arriving point of every key that is new in the chunk (K17's
// atomicMin into a scratch word of the entry; first[] is kSesNoLane everywhere between calls)
__global__ void k_ses_name_first(SesTable t, int64_t n, const int32_t* lane_entry, int32_t* first) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t e = lane_entry[i];
  if (e >= 0 && t.slot[e] == kSesNew) atomicMin(&first[e], (int32_t)i);
}

// one lane per point, a kernel boundary after k_ses_name_first and before anything is
// committed: the name's own faults, then the compare with the live session's row or with the
// name of the key's first-arriving point.  A first arrival with a fault of its own is refused
// at its lower index, so its name is not read.  bad: the lowest (index << 8 | reason).
__global__ void k_ses_name_check(SesTable t, SesDir d, SesNamesIn nm, int64_t n, const int32_t* lane_entry,
                                 const int32_t* first, unsigned long long* bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t e = lane_entry[i];
  if (e < 0) return;  // (the chunk is refused for its keys)
  const int64_t off = nm.off[i];
  const int32_t len = nm.len[i];
  const int32_t slot = t.slot[e];
  const uint8_t* row = nullptr;
  int32_t row_len = 0, flen = 0;
  int64_t foff = 0;
  bool has_first = false;
  if (slot >= 0) {
    row = d.bytes + (size_t)slot * (size_t)d.row;
    row_len = d.len[slot];
  } else {
    const int32_t f = first[e];
    if (f >= 0 && (int64_t)f < i) {
      has_first = true;
      foff = nm.off[f];
      flen = nm.len[f];
    }
  }
  const int32_t why = name_reason(nm.bytes, nm.n_bytes, d.uuid_bytes, off, len, row, row_len, has_first, foff, flen);
  if (why) ses_refuse(bad, i, why);
}

// an accepted chunk, after k_ses_assign: the creator lane of every new key writes the name of
// the key's first-arriving point into the session's row and clears the scratch word
__global__ void k_ses_name_write(SesTable t, SesDir d, SesNamesIn nm, int64_t n, const int32_t* lane_entry,
                                 const int32_t* is_new, int32_t* first) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !is_new[i]) return;
  const int32_t e = lane_entry[i];
  const int32_t f = first[e];
  first[e] = kSesNoLane;
  const int32_t slot = t.slot[e];
  if (f < 0 || (int64_t)f >= n || slot < 0) return;
  const int32_t len = nm.len[f];
  name_write_row(d.bytes + (size_t)slot * (size_t)d.row, d.row, nm.bytes, nm.off[f], len);
  d.len[slot] = len;
}

// a refused chunk: the scratch words are kSesNoLane again
__global__ void k_ses_name_unmark(int64_t n, const int32_t* lane_entry, const int32_t* is_new, int32_t* first) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && is_new[i]) first[lane_entry[i]] = kSesNoLane;
}

// restore: the name of every given session (keys are checked by k_ses_restore_check: none is
// live, none comes twice, so there is nothing to compare with)
__global__ void k_ses_restore_name_check(SesDir d, SesNamesIn nm, int64_t n, unsigned long long* bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && name_own_reason(nm.off[i], nm.len[i], nm.n_bytes, d.uuid_bytes)) ses_refuse(bad, i, OTR_RESTORE_E_NAME);
}

// beside k_ses_restore_copy: session i took free_list[n_free - 1 - i]
__global__ void k_ses_restore_name_copy(SesDir d, SesNamesIn nm, int64_t n, const int32_t* free_list, int32_t n_free) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t slot = free_list[n_free - 1 - (int32_t)i];
  const int32_t len = nm.len[i];
  name_write_row(d.bytes + (size_t)slot * (size_t)d.row, d.row, nm.bytes, nm.off[i], len);
  d.len[slot] = len;
}

// listed sessions: the length of each one's name, then the names packed at their offsets
__global__ void k_ses_name_len(int32_t n_list, const int32_t* list, SesDir d, int64_t* len) {
  const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n_list) len[g] = d.len[list[g]];
}

__global__ void k_ses_name_gather(int32_t n_list, const int32_t* list, const int64_t* off, SesDir d, uint8_t* bytes) {
  const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_list) return;
  const uint8_t* row = d.bytes + (size_t)list[g] * (size_t)d.row;
  const int64_t o = off[g];
  const int32_t len = (int32_t)(off[g + 1] - o);
  for (int32_t k = 0; k < len; ++k) bytes[o + k] = row[k];
}

// evictions in name order: stable LSD passes over a permutation of the key-ordered list.  The
// key of pass w is sort word w of the row, or the name's length (w < 0).
__global__ void k_ses_iota(int32_t n, int32_t* perm) {
  const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n) perm[g] = g;
}

__global__ void k_ses_name_sort_key(int32_t n_list, const int32_t* list, const int32_t* perm, SesDir d, int32_t w,
                                    unsigned long long* key) {
  const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_list) return;
  const int32_t slot = list[perm[g]];
  key[g] = w < 0 ? (unsigned long long)d.len[slot] : name_sort_word(d.bytes + (size_t)slot * (size_t)d.row, w);
}

__global__ void k_ses_permute(int32_t n_list, const int32_t* perm, const int32_t* list_in,
                              const unsigned long long* key_in, int32_t* list_out, unsigned long long* key_out) {
  const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_list) return;
  list_out[g] = list_in[perm[g]];
  key_out[g] = key_in[perm[g]];
}

}  // namespace otr
