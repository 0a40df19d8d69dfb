// Host check of reporter_amd/csrc/otr_tiers.h (tests/test_route_tier_table.py): the route
// tier table against the numbering the engine had when it was written out in literals, and
// the OTR_TIERS parser against known answers.  Prints "<bad> <checked>".
#include <cstdio>
#include <vector>

#include "otr_tiers.h"

using namespace otr;

static int bad = 0, checked = 0;
static void eq(long a, long b, const char* what, int i) {
  ++checked;
  if (a != b) {
    ++bad;
    fprintf(stderr, "%s[%d]: %ld, expected %ld\n", what, i, a, b);
  }
}
static void tiers(const char* spec, std::vector<int> want) {
  const std::vector<int> got = parse_route_tiers(spec);
  eq((long)got.size(), (long)want.size(), spec ? spec : "(null)", -1);
  for (size_t k = 0; k < got.size() && k < want.size(); ++k) eq(got[k], want[k], spec ? spec : "(null)", (int)k);
}

int main() {
  // slot -> bank, list word, queue, dump-counter queue and line (-1: none)
  const int bank[14] = {0, 2, 3, 4, 5, 6, 8, 9, 7, 1, 10, 11, 12, 13};
  const int list[14] = {-1, 0, 1, 2, 3, 4, 8, 9, 7, 25, 23, 26, -1, -1};
  const int queue[14] = {-1, 0, 1, 2, 3, 4, -1, -1, 8, 10, 9, 11, -1, -1};
  const int dq[14] = {-1, 15, 15, 15, 15, 15, -1, -1, -1, 14, 13, 15, -1, -1};
  const int dl[14] = {0, 0, 1, 2, 3, 4, 0, 0, 0, 0, 0, 0, 0, 0};
  eq(kRouteSlots, 14, "kRouteSlots", 0);
  eq(kBanks, 14, "kBanks", 0);
  for (int s = 0; s < 14; ++s) {
    eq(kRouteTiers[s].bank, bank[s], "bank", s);
    eq(kRouteTiers[s].list, list[s], "list", s);
    eq(kRouteTiers[s].queue, queue[s], "queue", s);
    eq(kRouteTiers[s].dump_queue, dq[s], "dump_queue", s);
    eq(kRouteTiers[s].dump_line, dl[s], "dump_line", s);
    eq(route_event(s), 24 + 2 * s, "event", s);
    if (dq[s] >= 0) eq(dump_ctr_word(s), dq[s] * 128 + 16 * dl[s], "dump_ctr_word", s);
  }
  // the edge-state tiers run in the order first (slot 10), 512 (9), 1024 (11)
  eq(kEdgeSlots[0], 10, "edge", 0);
  eq(kEdgeSlots[1], 9, "edge", 1);
  eq(kEdgeSlots[2], 11, "edge", 2);
  // the other list counter words
  const int words[][2] = {{C_TASKS_LEFT, 10}, {C_STEPS, 11}, {C_PATH_TIER, 12}, {C_PATH_GLOBAL, 16}, {C_PATHS_LEFT, 18},
                          {C_GEN_OVERFLOW, 19}, {C_CAP_FLAG, 20}, {C_STEPS_FRONT, 21}, {C_STEPS_ALL, 22},
                          {C_FLAGGED, 24}, {C_EDGE_PATH, 27}, {C_CURSORS, 32}};
  for (int k = 0; k < (int)(sizeof(words) / sizeof(words[0])); ++k) eq(words[k][0], words[k][1], "word", k);
  // route_tier_code values
  eq(route_tier_code(SLOT_FIRST, 160, 2), 1602, "code", 0);
  eq(route_tier_code(SLOT_NODE + 1, 448, 2), 4482, "code", 2);
  eq(route_tier_code(SLOT_GLOBAL, kRouteTiers[6].cap, 0), -1, "code", 6);
  eq(route_tier_code(SLOT_GLOBAL + 1, kRouteTiers[7].cap, 0), -2, "code", 7);
  eq(route_tier_code(SLOT_WIDE64, kRouteTiers[8].cap, 1), 902048, "code", 8);
  eq(route_tier_code(SLOT_EDGE_512, kRouteTiers[9].cap, 1), 6051232, "code", 9);
  eq(route_tier_code(SLOT_EDGE_FIRST, 360, 1), 6036032, "code", 10);
  eq(route_tier_code(SLOT_EDGE_1024, kRouteTiers[11].cap, 1), 6102432, "code", 11);
  eq(route_tier_code(SLOT_SMALL, 80, 4), 804, "code", 12);
  eq(route_tier_code(SLOT_TINY, 40, 8), 408, "code", 13);
  // OTR_TIERS
  tiers(nullptr, {2561, 4482, 10241, 20481, 40961});
  tiers("256,512x2,1024,4096", {2561, 5122, 10241, 40961});
  tiers("384x2", {3842, 40961});
  tiers("300", {40961});
  tiers("512x3", {40961});
  tiers("", {40961});
  tiers("256,300,512x3,,1024", {2561, 10241, 40961});
  tiers("256,512,768,1024,2048,512x2", {2561, 5121, 7681, 10241, 40961});
  printf("%d %d\n", bad, checked);
  return 0;
}
