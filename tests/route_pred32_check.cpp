// Check behind the node search's 32-bit round predicates (reporter_amd/csrc/otr_pred.h):
// in_final32 and target_final32 against the 64-bit expressions they replaced in search_run
// and target_resolved (otr_kernels.h), over the edges of the u32 range and random tuples.
// Prints the mismatch count.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "otr_pred.h"

// the partition's IN criterion as search_run had it
static bool in_final64(uint32_t d, uint32_t kmin, uint32_t gap) { return (uint64_t)d < (uint64_t)kmin + gap; }

// target_resolved's arithmetic as it was: the label (none: far above every bound) below
// next = kmin + gapT, or min(label, next) + tpart beyond pd
static bool target_final64(bool none, uint32_t d, uint32_t kmin, uint32_t gapT, uint32_t tpart, uint32_t pd) {
  const int64_t lab = none ? INT64_MAX / 4 : (int64_t)d;
  const int64_t next = (int64_t)kmin + (int64_t)gapT;
  const bool unreach = (lab < next ? lab : next) + (int64_t)tpart > (int64_t)pd;
  return (lab < next) | unreach;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

static uint64_t bad = 0, checked = 0;

static void check(uint32_t d, uint32_t kmin, uint32_t gap, uint32_t tpart, uint32_t pd) {
  if (d >= kmin) {  // (every pending entry: kmin is the pending list's minimum)
    bad += otr::in_final32(d, kmin, gap) != in_final64(d, kmin, gap);
    ++checked;
  }
  for (int none = 0; none < 2; ++none) {  // the target's label is any length, or none
    bad += otr::target_final32(none != 0, d, kmin, gap, tpart, pd) != target_final64(none != 0, d, kmin, gap, tpart, pd);
    ++checked;
  }
}

int main() {
  const uint32_t gaps[] = {1u, 16u, 65535u * 16u};
  const uint32_t parts[] = {0u, 1u, 2u, 1000u, 0x3FFFFFFFu, 0x40000000u, 0x7FFFFFFEu, 0x7FFFFFFFu};
  for (uint32_t gap : gaps) {
    std::vector<uint32_t> v;
    const uint64_t centres[] = {0ull, 1ull, gap - 1ull, gap, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFEull, 0xFFFFFFFFull};
    for (uint64_t c : centres)
      for (int64_t o = -1; o <= 1; ++o) {
        const int64_t x = (int64_t)c + o;
        if (x >= 0 && x <= 0xFFFFFFFFll) v.push_back((uint32_t)x);
      }
    for (uint32_t d : v)
      for (uint32_t kmin : v)
        for (uint32_t tpart : parts)
          for (uint32_t pd : parts) check(d, kmin, gap, tpart, pd);
  }
  for (int it = 0; it < 4000000; ++it) {
    const uint64_t a = rnd(), b = rnd(), c = rnd();
    // lengths over the whole u32 range or close together, gaps up to the largest code's
    uint32_t kmin = (uint32_t)a, d = (uint32_t)(a >> 32);
    if (b & 1) d = kmin + (uint32_t)((b >> 8) % 3000000u);  // (may wrap: then d < kmin, the target test only)
    if (b & 2) kmin = 0xFFFFFFFFu;                          // nothing pending
    const uint32_t gap = (b & 4) ? gaps[(b >> 3) % 3] : 1u + (uint32_t)((b >> 5) % (65535u * 16u));
    check(d, kmin, gap, (uint32_t)c & 0x7FFFFFFFu, (uint32_t)(c >> 32) & 0x7FFFFFFFu);
    if (b & 64) check(d, kmin, gap, (uint32_t)c & 0xFFFFFu, (uint32_t)(c >> 32) & 0xFFFFFu);  // near each other
  }
  std::printf("%llu %llu\n", (unsigned long long)bad, (unsigned long long)checked);
  return 0;
}
