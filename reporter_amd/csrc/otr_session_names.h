// otr_session_names.h — K18: the per-name rules of the session store's uuid directory
// (include/otr.h otr_sessions_open_named).  A directory row is the
// name's bytes, zero-filled to row_bytes = round_up(uuid_bytes, 16), at a 16-byte aligned
// address; a caller's name sits at any address and is read one byte at a time, never outside
// [off, off + len).  The functions are __host__ __device__ so that tools/namecheck.cpp runs the
// very same rules on the CPU (under sanitizers) that the kernels of otr_sessions.h run on the
// device.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OTR_NAME_HD __host__ __device__ inline
#else
#define OTR_NAME_HD inline
#endif

namespace otr {

// the refusal reasons of include/otr.h (OTR_NAME_E_*), for the host program that does not
// include it
constexpr int32_t kNameLong = 1, kNameCollision = 2, kNameLayout = 3;

OTR_NAME_HD int32_t name_row_bytes(int32_t uuid_bytes) { return (uuid_bytes + 15) & ~15; }
OTR_NAME_HD int32_t name_sort_words(int32_t uuid_bytes) { return (uuid_bytes + 7) / 8; }

// name [off, off + len) of a buffer of n_bytes (no sum that could wrap)
OTR_NAME_HD bool name_layout_ok(int64_t off, int32_t len, int64_t n_bytes) {
  return off >= 0 && len >= 0 && off <= n_bytes && (int64_t)len <= n_bytes - off;
}

// 0, or the lowest of the reasons the name has by itself: too long (the length as given, also
// where the layout is at fault) before layout
OTR_NAME_HD int32_t name_own_reason(int64_t off, int32_t len, int64_t n_bytes, int32_t uuid_bytes) {
  if (!name_layout_ok(off, len, n_bytes)) return len > uuid_bytes ? kNameLong : kNameLayout;
  return len > uuid_bytes ? kNameLong : 0;
}

// a well-formed name against a directory row: same length, same bytes
OTR_NAME_HD bool name_equals_row(const uint8_t* bytes, int64_t off, int32_t len, const uint8_t* row, int32_t row_len) {
  if (len != row_len) return false;
  for (int32_t k = 0; k < len; ++k)
    if (bytes[off + k] != row[k]) return false;
  return true;
}

// two well-formed names of one buffer
OTR_NAME_HD bool name_equals_name(const uint8_t* bytes, int64_t off_a, int32_t len_a, int64_t off_b, int32_t len_b) {
  if (len_a != len_b) return false;
  for (int32_t k = 0; k < len_a; ++k)
    if (bytes[off_a + k] != bytes[off_b + k]) return false;
  return true;
}

// The reason of a point's name, 0 when it has none: its own faults, else the compare with what
// its key meets: the row of the key's live session (row non-null), or the name of the key's
// first-arriving point of the chunk (has_first; a first arrival with a fault of its own is
// refused at its lower index and is not read).
OTR_NAME_HD int32_t name_reason(const uint8_t* bytes, int64_t n_bytes, int32_t uuid_bytes, int64_t off, int32_t len,
                                const uint8_t* row, int32_t row_len, bool has_first, int64_t first_off,
                                int32_t first_len) {
  const int32_t own = name_own_reason(off, len, n_bytes, uuid_bytes);
  if (own) return own;
  if (row) return name_equals_row(bytes, off, len, row, row_len) ? 0 : kNameCollision;
  if (has_first && !name_own_reason(first_off, first_len, n_bytes, uuid_bytes) &&
      !name_equals_name(bytes, off, len, first_off, first_len))
    return kNameCollision;
  return 0;
}

// a well-formed name of at most row_bytes into its row, zero-filled beyond its length (a slot
// taken from the free stack does not show the previous occupant's tail)
OTR_NAME_HD void name_write_row(uint8_t* row, int32_t row_bytes, const uint8_t* bytes, int64_t off, int32_t len) {
  for (int32_t k = 0; k < len; ++k) row[k] = bytes[off + k];
  for (int32_t k = len; k < row_bytes; ++k) row[k] = 0;
}

// sort word w of a row: bytes 8w .. 8w+7 big-endian, so that unsigned word order is byte order
// (8 * name_sort_words(uuid_bytes) <= row_bytes: the read stays inside the row)
OTR_NAME_HD uint64_t name_sort_word(const uint8_t* row, int32_t w) {
  uint64_t v = 0;
  for (int k = 0; k < 8; ++k) v = (v << 8) | (uint64_t)row[8 * w + k];
  return v;
}

}  // namespace otr
