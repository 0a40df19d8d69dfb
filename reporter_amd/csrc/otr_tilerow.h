// otr_tilerow.h — what one report becomes in the Java streaming path's tiles
// (OTR_TILE_RULES_STREAM), shared by K9 (k_tile_rows, otr_kernels.h: the reports of one
// batch) and K15 (k_store_rows, otr_tilestore.h: the tile store's adds), so that both write
// the same rows bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/otr.h"
#include "otr_device.h"
#include "otr_report.h"

namespace otr {

// inclusive prefix sum over the wave (lane order)
__device__ inline unsigned long long wave_incl_scan_u64(unsigned long long v) {
  const int l = lane_id();
  for (int o = 1; o < OTR_WAVE; o <<= 1) {
    const unsigned long long u = __shfl_up(v, o);
    if (l >= o) v += u;
  }
  return v;
}

// BatchingProcessor.java:119-126 (Segment.valid, Segment.java:38-40) and
// TimeQuantisedTile.getTiles (TimeQuantisedTile.java:26-35): buckets from the
// truncated times, no span limit; duration Math.round (ties up), Segment.java:65-71.
// false: the report is not forwarded (sp untouched)
__host__ __device__ inline bool stream_span(double t0, double t1, int32_t len, int32_t qu, int64_t q, BucketSpan* sp) {
  if (!(t0 > 0 && t1 > 0 && t1 > t0 && len > 0 && qu >= 0)) return false;
  sp->duration = py2_round_int(t1 - t0);
  sp->start = (int64_t)floor(t0);
  sp->end = (int64_t)ceil(t1);
  sp->min_bucket = (int64_t)t0 / q;
  sp->max_bucket = (int64_t)t1 / q;
  sp->ok = true;
  return true;
}

// the report's 20 km/h speed bin, as K8 bins it (oracle/tiles.py speed_bin)
__host__ __device__ inline int tile_speed_bin(int32_t len, double t0, double t1) {
  const double bq = (((double)len / (t1 - t0)) * 3.6) / 20.0;
  return bq >= (double)(OTR_HIST_BINS - 1) ? OTR_HIST_BINS - 1 : (bq < 0.0 ? 0 : (int)bq);
}

// the row of bucket bk (simple_reporter.py:188-195 / Segment.java:59-74 in binary form);
// nx OTR_NO_ID: no next segment
__host__ __device__ inline otr_tile_row tile_row_of(int64_t bk, unsigned long long id, unsigned long long nx,
                                                    const BucketSpan& sp, int32_t len, int32_t qu, int speed_bin) {
  otr_tile_row row;
  row.file = ((unsigned long long)bk << 25) | ((id & 7ull) << 22) | ((id >> 3) & 0x3FFFFFull);
  row.id = id;
  row.next_id = nx == OTR_NO_ID ? OTR_INVALID_SEGMENT_ID : nx;
  row.start = sp.start;
  row.end = sp.end;
  row.duration = (int32_t)sp.duration;
  row.length = len;
  row.queue_length = qu;
  row.speed_bin = speed_bin;
  return row;
}

}  // namespace otr
