// Host check of reporter_amd/csrc/otr_tiers.h (tests/test_route_tier_table.py): the route
// tier table against the numbering the engine had when it was written out in literals, the
// retry protocol (flags, collect masks, run order, path tiers, force_edge bits, the task
// record word) against the literals the kernels and the engine had, and the OTR_TIERS parser
// against known answers.  Prints "<bad> <checked>".
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
  // ---- the retry protocol: the flag values the kernels wrote as literals
  eq(RF_NONE, 0, "route flag", 0);
  eq(RF_OVERFLOW, 1, "route flag", 1);
  eq(RF_GENERAL, 3, "route flag", 3);
  eq(RF_EDGE_FIRST, 5, "route flag", 5);
  eq(RF_EDGE_512, 6, "route flag", 6);
  eq(RF_EDGE_1024, 7, "route flag", 7);
  eq(RF_START_TIER, 16, "route flag", 16);
  for (int t = 0; t < 5; ++t) eq(route_start_flag(t), 16 + t, "start flag", t);
  eq(PF_NONE, 0, "path flag", 0);
  eq(PF_OVERFLOW, 1, "path flag", 1);
  eq(PF_GENERAL, 3, "path flag", 3);
  eq(PF_EDGE_FIRST, 5, "path flag", 5);
  eq(PF_EDGE_SECOND, 6, "path flag", 6);
  eq(kSlabOverflow, 1, "k_general's overflow", 0);
  eq(flag_bit(RF_GENERAL), 0x8, "flag_bit", 3);
  eq(flag_bit(PF_EDGE_SECOND), 0x40, "flag_bit", 6);
  // k_route_e1<CAP>'s CAP < 512 ? 6 : (CAP < 1024 ? 7 : 3); k_paths_edge's launch argument 6, then 3
  eq(edge_overflow_flag(360), 6, "edge_overflow_flag", 360);
  eq(edge_overflow_flag(512), 7, "edge_overflow_flag", 512);
  eq(edge_overflow_flag(1024), 3, "edge_overflow_flag", 1024);
  eq(path_edge_overflow_flag(384), 6, "path_edge_overflow_flag", 384);
  eq(path_edge_overflow_flag(2048), 3, "path_edge_overflow_flag", 2048);
  // the mask every route collect took, per slot (0: no collect), and the flag its overflow wrote
  const unsigned take[14] = {0, 0x2u | (1u << 16), 0x2u | (3u << 16), 0x2u | (7u << 16), 0x2u | (15u << 16),
                             0x2u | (31u << 16), 0x1Eu, 0x2u, 0x8u, 0x40u, 0x20u, 0x80u, 0, 0};
  const int over[14] = {1, 1, 1, 1, 1, 1, 1, 1, 3, 7, 6, 3, 1, 1};
  const unsigned grid[14] = {0, 0, 0, 0, 0, 0, 0, 0, 4096, 4096, 8192, 2048, 0, 0};
  for (int s = 0; s < 14; ++s) {
    eq(kRouteTiers[s].take, take[s], "take", s);
    eq(kRouteTiers[s].overflow, over[s], "overflow", s);
    eq(kRouteTiers[s].grid, grid[s], "grid", s);
  }
  for (int t = 0; t < 5; ++t) eq(node_tier_mask(t), 0x2u | (((2u << t) - 1u) << 16), "node_tier_mask", t);
  for (int et = 0; et < 3; ++et) eq(kRouteTiers[kEdgeSlots[et]].take, 0x20u << et, "edge take", et);
  eq(kTasksLeft.list, 10, "tasks left", 0);
  eq(kTasksLeft.take, 0x1Eu, "tasks left", 1);
  // the run order: tiny, small, first, the node tiers, the 64-bit table, the edge tiers, the slabs
  const int order[14] = {13, 12, 0, 1, 2, 3, 4, 5, 8, 10, 9, 11, 6, 7};
  for (int i = 0; i < 14; ++i) eq(kRouteOrder[i], order[i], "order", i);
  // the path tiers: kind, table size, list counter word, queue, grid, mask, overflow flag
  const long path[7][7] = {{0, 512, 12, 0, 16384, 0x2, 1}, {0, 1024, 13, 1, 8192, 0x2, 1},  {0, 4096, 14, 2, 4096, 0x2, 1},
                           {1, 384, 27, 3, 4096, 0x20, 6}, {1, 2048, 28, 4, 512, 0x40, 3},
                           {2, 1 << 15, 16, -1, 0, 0xA, 1}, {2, 1 << 20, 17, -1, 0, 0x2, 1}};
  eq(kPathTierN, 7, "kPathTierN", 0);
  for (int t = 0; t < 7 && t < kPathTierN; ++t) {
    const PathTier& p = kPathTiers[t];
    const long got[7] = {(long)p.kind, p.cap, p.list, p.queue, (long)p.grid, (long)p.take, p.overflow};
    for (int c = 0; c < 7; ++c) eq(got[c], path[t][c], "path tier", 10 * t + c);
  }
  eq(kPathsLeft.list, 18, "paths left", 0);
  eq(kPathsLeft.take, 0xAu, "paths left", 1);
  eq(kPathQueues, 8, "kPathQueues", 0);
  // the slab sizes are the route stage's
  eq(kPathTiers[5].cap, kRouteTiers[SLOT_GLOBAL].cap, "slab", 0);
  eq(kPathTiers[6].cap, kRouteTiers[SLOT_GLOBAL + 1].cap, "slab", 1);
  // OTR_FORCE_EDGE bits (the tests pass the numbers)
  const int fe[8] = {FE_FAIL_E1, FE_FAIL_E512, FE_FAIL_E1024, FE_FAIL_PATH_384, FE_FAIL_PATH_2048,
                     FE_STOP_E1, FE_STOP_E512, FE_STOP_NODE};
  for (int k = 0; k < 8; ++k) eq(fe[k], 1 << k, "force_edge", k);
  // the task record word: Kb | mode << 8 | forced << 10 | sh << 11 | general << 16 | turn << 17 | pre << 18 |
  // tier << 19, through pack and accessors at the field extremes
  eq(task_word(64, 3, 1, 31, 1, 1, task_start(kNodeTiers - 1)),
     64 | (3 << 8) | (1 << 10) | (31 << 11) | (1 << 16) | (1 << 17) | (1 << 18) | (4 << 19), "task_word", 0);
  eq(task_word(1, 0, 0, 0, 0, 0, 0), 1, "task_word", 1);
  for (int bits = 0; bits < 16; ++bits) {  // each single-bit field on and off
    const unsigned f = bits & 1, g = (bits >> 1) & 1, t = (bits >> 2) & 1, p = (bits >> 3) & 1;
    for (int ext = 0; ext < 2; ++ext) {  // the wide fields at their smallest and largest
      const unsigned Kb = ext ? 64 : 1, md = ext ? 3 : 0, sh = ext ? 31 : 0, tier = ext ? kNodeTiers - 1 : 0;
      const unsigned w = task_word(Kb, md, f, sh, g, t, p ? task_start(tier) : 0u);
      eq(tw_Kb(w), Kb, "tw_Kb", bits);
      eq(tw_mode(w), md, "tw_mode", bits);
      eq(tw_forced(w), f, "tw_forced", bits);
      eq(tw_sh(w), sh, "tw_sh", bits);
      eq(tw_general(w), g, "tw_general", bits);
      eq(tw_turn(w), t, "tw_turn", bits);
      eq(tw_pre(w), p, "tw_pre", bits);
      eq(tw_start_tier(w), p ? tier : 0u, "tw_start_tier", bits);
      eq(w >> 22, 0, "task_word's unused bits", bits);
    }
  }
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
