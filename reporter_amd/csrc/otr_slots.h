// otr_slots.h — the matcher's workspace slots: ONE enum on ONE pool (Matcher::pool) for every
// unit that takes matcher buffers (otr_engine.hip, otr_tiles.hip, otr_text.hip), and need() /
// want() over it.  Stages share slots on purpose: the tile cull and the keyed histogram the
// S_IDX_*, S_KEY_*, S_FILE_HEAD, S_KEEP, S_POS_SCAN and S_SORT_TMP slots, probe ingest and the
// stream formatter the S_IN_* slots.  Host code only.
#pragma once
#include <cstdlib>

#include "otr_engine.h"

namespace otr {

enum Slot {
  S_TRACE_OFF, S_LAT, S_LON, S_TIME, S_ACC, S_MODE,
  S_STATE_CNT, S_TRACE_STATE_OFF, S_STATE_PROBE, S_STATE_TRACE,
  S_CAND_EDGE, S_CAND_P, S_CAND_SQD, S_CAND_COUNT, S_CAND_RADIUS,
  S_PREV, S_G, S_BOUND, S_FORCED, S_NTASK, S_NTRANS, S_TASK_OFF, S_TRANS_OFF, S_NTASK4, S_TASK4_OFF, S_NTASK8, S_TASK8_OFF, S_UNIT,
  S_TASK_STATE, S_TASK_MASK, S_TASK_OVF, S_TRANS,
  S_BP, S_BRK, S_END_WIN, S_WINNER, S_SUBPATH,
  S_PATH_OFF, S_PATH_LEN, S_PATH, S_STEP_OVF,
  S_CAP, S_CAP_OFF, S_POS, S_ACT, S_ENT, S_SUBA, S_SUBB, S_POR_E, S_POR_S0, S_POR_S1, S_POR_SA, S_GSTART,
  S_ROUTE, S_ROUTE_N, S_SEG_ID, S_SEG_START, S_SEG_END, S_SEG_LEN, S_SEG_QUEUE, S_SEG_INTERNAL,
  S_SEG_BSHAPE, S_SEG_ESHAPE, S_SEG_INDEX, S_SEG_N, S_SEG_WAY_N, S_SEG_WAY, S_WAY_N,
  S_REP_ID, S_REP_NEXT, S_REP_T0, S_REP_T1, S_REP_LEN, S_REP_QUEUE, S_REP_SEG, S_REP_N,
  S_SHAPE_USED, S_STATS, S_STATS_LEN, S_HIST, S_COUNTERS, S_SCAN_TMP, S_LIST, S_MISC,
  S_HEUR, S_CPREP, S_ROW_CNT, S_ROW_OFF, S_ROWS, S_ROWS_IN, S_ROWS_OUT, S_ROWS_KEPT, S_IDX_A, S_IDX_B, S_KEY_A, S_KEY_B, S_POS_SCAN, S_RUN_KEEP, S_KEEP, S_FILE_HEAD, S_FILE_START, S_NFILES, S_SORT_TMP,
  S_C_ROUTE_OFF, S_C_SEG_OFF, S_C_WAY_OFF, S_C_REP_OFF, S_C_ARGS, S_C_ROUTE, S_C_SEG_ID, S_C_SEG_START,
  S_C_SEG_END, S_C_SEG_LEN, S_C_SEG_QUEUE, S_C_SEG_INTERNAL, S_C_SEG_BSHAPE, S_C_SEG_ESHAPE, S_C_SEG_WAY_N,
  S_C_SEG_WAY, S_C_SEG_WAY_OFF, S_C_REP_ID, S_C_REP_NEXT, S_C_REP_T0, S_C_REP_T1, S_C_REP_LEN, S_C_REP_QUEUE,
  S_TASK_REC, S_BT, S_CPREP_T, S_TRANS_TC, S_TURN, S_LIST2, S_GFLAG, S_HE_IN, S_HE_SORTED, S_HE_RED, S_HE_OUT, S_HE_RANGE, S_IN_TEXT, S_IN_CNT, S_IN_CSCAN, S_IN_NL, S_IN_HASH, S_IN_UOFF, S_IN_ULEN, S_IN_TIME, S_IN_LAT, S_IN_LON,
  S_IN_ACC, S_IN_KEEP, S_IN_KPOS, S_IN_KIDX, S_IN_KEY_A, S_IN_KEY_B, S_IN_VAL_A, S_IN_VAL_B, S_IN_HEAD, S_IN_GID,
  S_IN_GFIRST, S_IN_GKEY, S_IN_WS, S_IN_KLEN, S_IN_KFLAG, S_IN_POFF, S_IN_TPOS, S_IN_BAD, S_IN_TMP,
  S_IN_T_OFF, S_IN_T_LAT, S_IN_T_LON, S_IN_T_TIME, S_IN_T_ACC, S_IN_T_MODE, S_IN_T_UOFF, S_IN_T_ULEN,
  S_CLEN, S_CAND_NROOT, S_FLAGGED, S_HE_FIDX, S_HE_FHEAD, S_HE_PFILE, S_HE_FFIRST, S_HE_PKEY, S_QUEUE, S_PQUEUE,
  S_E1DUMP0, S_E1DUMP1, S_TASK_DUMP, S_NDUMP0, S_NDUMP1, S_SORT_LIST, S_SORT_HIST,
  S_PT_KIND, S_PT_EDGE, S_PT_FRAC, S_PT_LAT, S_PT_LON, S_PT_DIST, S_PT_STATE, S_PT_POS, S_PT_STATUS,
  S_TR_CNT, S_TR_OFF, S_TR_EDGE, S_TR_WAY, S_TR_SEG, S_TR_FIRST, S_TR_F0, S_TR_F1, S_TR_S0, S_TR_S1, S_TR_T0, S_TR_T1,
  S_TR_KEEP, S_TR_KEEP_OFF, S_TR_ENTRIES, S_TR_TMP,
  S_FM_KEYS, S_FM_OFF, S_FM_TSIN, S_FM_WRONG, S_FM_STATUS, S_FM_P_LAT, S_FM_P_LON, S_FM_P_ACC, S_FM_FLAG,
  S_FM_KEY, S_FM_LAT, S_FM_LON, S_FM_ACC, S_FM_TIME, S_FM_TS, S_FM_MSG, S_FM_UOFF, S_FM_ULEN,
  S_NUM
};

inline bool optional_slot(int s) {
  return s == S_E1DUMP0 || s == S_E1DUMP1 || s == S_TASK_DUMP || s == S_NDUMP0 || s == S_NDUMP1 ||
         s == S_SORT_LIST || s == S_SORT_HIST;
}

// mandatory workspace: the buffer or DeviceOom, never nullptr.  On top of the pool's growth: a
// second attempt at the exact size, then, for a slot that is not itself optional, one more
// after the optional workspace is released.
template <class T>
T* Matcher::need(int slot, size_t n) {
  if ((int)pool.b.size() < S_NUM) pool.b.resize(S_NUM);
  return pool.get<T>(slot, n, true, [this](int s) { return !optional_slot(s) && release_optional(); });
}

// the free device memory an optional buffer must leave (OTR_OPT_RESERVE_GB, default 8 GB or
// an eighth of the device, whichever is more): the later stages' mandatory buffers
inline size_t opt_reserve() {
  static const double gb = getenv("OTR_OPT_RESERVE_GB") ? atof(getenv("OTR_OPT_RESERVE_GB")) : -1.0;
  if (gb >= 0) return (size_t)std::min(gb * (double)(1ll << 30), 1e18);
  size_t fr = 0, tot = 0;
  (void)hipMemGetInfo(&fr, &tot);
  return std::max<size_t>(8ull << 30, tot / 8);
}

template <class T>
T* Matcher::want(int slot, size_t n) {
  if ((int)pool.b.size() < S_NUM) pool.b.resize(S_NUM);
  const size_t bytes = (n ? n : 1) * sizeof(T);
  if (void* p = pool.held(slot, bytes)) return (T*)p;
  pool.drop(slot);
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < bytes || fr - bytes < opt_reserve()) {
    (void)hipGetLastError();
    return nullptr;
  }
  return (T*)pool.try_exact(slot, bytes);
}

}  // namespace otr
