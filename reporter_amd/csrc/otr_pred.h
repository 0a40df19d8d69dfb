// otr_pred.h — the per-round predicates of the node search (otr_kernels.h search_run) in
// 32-bit arithmetic, for the tables whose packed label words are 32 bits wide (label modes
// 0 and 1).  Lengths are u32 mm; kmin is the smallest pending length of the round
// (0xFFFFFFFF: nothing pending).  Host and device: tests/route_pred32_check.cpp compares
// them with the 64-bit expressions they replace.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace otr {

// IN criterion of a pending label of length d: final when d < kmin + gap.  Every pending
// entry has d >= kmin (kmin is the minimum over the pending list), so the difference
// neither wraps nor needs the 64-bit sum.
__host__ __device__ inline bool in_final32(uint32_t d, uint32_t kmin, uint32_t gap) { return d - kmin < gap; }

// Target test (target_resolved): `none` the target has no label yet, else d its length.
// next = kmin + gapT bounds every later offer from below; the target's label is final
// below it, and the target is unreachable when even min(label, next) + tpart breaks the
// relative bound pd.  The sum may pass 2^32 (kmin = 0xFFFFFFFF, or lengths near the top of
// the range): the carry stands for "next is above every u32".  tpart, pd < 2^31.
__host__ __device__ inline bool target_final32(bool none, uint32_t d, uint32_t kmin, uint32_t gapT, uint32_t tpart,
                                               uint32_t pd) {
  const uint32_t next = kmin + gapT;
  const bool carry = next < kmin;
  const bool below = !none & (carry | (d < next));  // label < next
  const uint32_t m = below ? d : next;                // min(label, next), when it fits 32 bits
  const bool unreach = (!below & carry) | (tpart > pd) | (m > pd - tpart);
  return below | unreach;
}

}  // namespace otr
