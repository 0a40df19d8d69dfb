// otr_session_records.h — K17: the per-record rules of Batch.Serder's value bytes
// (Batch.java:110-116, Point.java:50-55; include/otr.h otr_session_records), big-endian:
//   int32 count, float max_separation, int64 last_update, count x (float lat, float lon,
//   int32 accuracy, int64 time): 16 + 20 * count bytes.
// Bytes are read and written one at a time: a record may start at any address.  The
// functions are __host__ __device__ so that tools/recordcheck.cpp runs the very same rules
// on the CPU (under sanitizers) that the kernels of otr_sessions.h run on the device.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OTR_REC_HD __host__ __device__ inline
#else
#define OTR_REC_HD inline
#endif

namespace otr {

constexpr int64_t kRecHeader = 16;  // count, max_separation, last_update
constexpr int64_t kRecPoint = 20;   // lat, lon, accuracy, time

OTR_REC_HD uint32_t rec_get32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

OTR_REC_HD uint64_t rec_get64(const uint8_t* p) { return ((uint64_t)rec_get32(p) << 32) | (uint64_t)rec_get32(p + 4); }

OTR_REC_HD void rec_put32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

OTR_REC_HD void rec_put64(uint8_t* p, uint64_t v) {
  rec_put32(p, (uint32_t)(v >> 32));
  rec_put32(p + 4, (uint32_t)v);
}

// floats travel by their bits (Float.intBitsToFloat / floatToRawIntBits: a NaN's payload too)
OTR_REC_HD float rec_bits_float(uint32_t u) { return __builtin_bit_cast(float, u); }
OTR_REC_HD uint32_t rec_float_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// Record [b, e) of a buffer of n_bytes: inside the buffer, at least a header, and as long as
// its count says, computed in 64 bits (a negative count or one near 2^31 cannot wrap).
// count is set once the header is readable.
OTR_REC_HD bool rec_layout_ok(const uint8_t* bytes, int64_t n_bytes, int64_t b, int64_t e, int32_t* count) {
  *count = 0;
  if (b < 0 || e < b || e > n_bytes || e - b < kRecHeader) return false;
  *count = (int32_t)rec_get32(bytes + b);
  return kRecHeader + kRecPoint * (int64_t)*count == e - b;
}

OTR_REC_HD void rec_header_get(const uint8_t* rec, int32_t* count, float* max_sep, int64_t* last) {
  *count = (int32_t)rec_get32(rec);
  *max_sep = rec_bits_float(rec_get32(rec + 4));
  *last = (int64_t)rec_get64(rec + 8);
}

OTR_REC_HD void rec_header_put(uint8_t* rec, int32_t count, float max_sep, int64_t last) {
  rec_put32(rec, (uint32_t)count);
  rec_put32(rec + 4, rec_float_bits(max_sep));
  rec_put64(rec + 8, (uint64_t)last);
}

OTR_REC_HD void rec_point_get(const uint8_t* rec, int32_t k, float* lat, float* lon, int32_t* acc, int64_t* time) {
  const uint8_t* p = rec + kRecHeader + kRecPoint * (int64_t)k;
  *lat = rec_bits_float(rec_get32(p));
  *lon = rec_bits_float(rec_get32(p + 4));
  *acc = (int32_t)rec_get32(p + 8);
  *time = (int64_t)rec_get64(p + 12);
}

OTR_REC_HD void rec_point_put(uint8_t* rec, int32_t k, float lat, float lon, int32_t acc, int64_t time) {
  uint8_t* p = rec + kRecHeader + kRecPoint * (int64_t)k;
  rec_put32(p, rec_float_bits(lat));
  rec_put32(p + 4, rec_float_bits(lon));
  rec_put32(p + 8, (uint32_t)acc);
  rec_put64(p + 12, (uint64_t)time);
}

}  // namespace otr
