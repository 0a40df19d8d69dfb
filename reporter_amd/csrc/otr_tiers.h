// otr_tiers.h — the numbering of the route search tiers, in one place (host only).
//
// A route tier is known by its slot in otr_batch_result's route_tier_code / route_tier_ms /
// route_tier_work (public: bench.py and the tests read the slots by number).  Everything
// else the engine keeps per tier follows from the slot through kRouteTiers: the counter
// bank in the work counters, the word of the list counters (CntWord) that holds its retry
// list's length, its work queue, the line of its dump-slot counter and its event pair.
#pragma once
#include <cstdlib>
#include <string>
#include <vector>

namespace otr {

enum class TierKind { First, Tiny, Small, NodeRetry, Wide64, EdgeState, Global };

constexpr int kRouteSlots = 14;     // slots in use
constexpr int kRouteSlotsAbi = 16;  // otr_batch_result route_tier_*[16]
constexpr int kBanks = 14;          // counter banks of OTR_COUNTERS kinds x kCShards (bank 0: also the batch's)
constexpr int kQueues = 16;         // work queues (XcdQueue) of one batch
constexpr int kQueueWords = 16 * 8; // 8 counters per queue, 128 B apart
constexpr int kDumpLineWords = 16;  // a dump-slot counter has a 128 B line of a queue to itself
constexpr int kNodeTiers = 5;       // node retry tiers at most (OTR_TIERS: four and the 4096-slot one)
constexpr int kStageEvents = 24;    // events 0..19 the batch stages, 20..23 ingest
constexpr int kEvents = 58;         // Matcher::ev
constexpr int kPointsEvent = 54;    // 54, 55: the matched-points stage (K12), after the route tier slots' pairs
constexpr int kTravEvent = 56;      // 56, 57: the edge-traversals stage (K13)

// the words of the device-side list counters (one allocation, cleared per batch)
enum CntWord {
  C_NODE_TIER = 0,      // ..4: the node retry tiers' lists (5, 6 unused)
  C_WIDE64 = 7,         // the 64-bit LDS tier's list
  C_GLOBAL = 8,         // 8, 9: the global-memory tiers' lists
  C_TASKS_LEFT = 10,    // route tasks beyond every tier
  C_STEPS = 11,         // winner path steps (the back list with two step lists)
  C_PATH_TIER = 12,     // ..14: the path retry tiers' lists (15 unused)
  C_PATH_GLOBAL = 16,   // 16, 17: the path stage's global-memory lists
  C_PATHS_LEFT = 18,    // paths beyond every tier
  C_GEN_OVERFLOW = 19,  // k_general's overflow count
  C_CAP_FLAG = 20,      // a path did not fit its region
  C_STEPS_FRONT = 21,   // the small-search path tier's step list
  C_STEPS_ALL = 22,     // the index range of the path collects with two step lists
  C_EDGE_FIRST = 23,    // the first edge-state tier's list
  C_FLAGGED = 24,       // tasks the first tiers flagged
  C_EDGE_512 = 25,      // the 512- and 1024-state edge tiers' lists
  C_EDGE_1024 = 26,
  C_EDGE_PATH = 27,     // 27, 28: the edge-state path tiers' lists
  C_CURSORS = 32,       // ..32 + kShards: path bump cursors
};

struct RouteTier {
  TierKind kind;
  int cap;         // table capacity; 0: a build knob (OTR_CAP1/4/8, OTR_E1CAP) or OTR_TIERS
  int g;           // searches per wave; 0: OTR_TIERS (node retry) or not wave-based
  int bank;        // counter bank
  int list;        // CntWord of its retry list's length, -1: no list
  int queue;       // work queue, -1: none
  int dump_queue;  // queue whose line dump_line holds its dump-slot counter, -1: never dumps
  int dump_line;
};

enum RouteSlot {
  SLOT_FIRST = 0,    // two searches per wave (or 256x1, OTR_ROUTE_G=1)
  SLOT_NODE = 1,     // ..5: node retry tier t = slot - 1
  SLOT_GLOBAL = 6,   // 6, 7: global-memory search on 32K- / 1M-slot slabs
  SLOT_WIDE64 = 8,   // LDS table of 64-bit label words
  SLOT_EDGE_512 = 9,
  SLOT_EDGE_FIRST = 10,
  SLOT_EDGE_1024 = 11,
  SLOT_SMALL = 12,   // four searches per wave
  SLOT_TINY = 13,    // eight searches per wave
};

constexpr RouteTier kRouteTiers[kRouteSlots] = {
    //  kind               cap      g  bank list          queue dump queue, line
    {TierKind::First,      0,       2, 0,  -1,            -1,   -1, 0},
    {TierKind::NodeRetry,  0,       0, 2,  C_NODE_TIER+0, 0,    15, 0},
    {TierKind::NodeRetry,  0,       0, 3,  C_NODE_TIER+1, 1,    15, 1},
    {TierKind::NodeRetry,  0,       0, 4,  C_NODE_TIER+2, 2,    15, 2},
    {TierKind::NodeRetry,  0,       0, 5,  C_NODE_TIER+3, 3,    15, 3},
    {TierKind::NodeRetry,  0,       0, 6,  C_NODE_TIER+4, 4,    15, 4},
    {TierKind::Global,     1 << 15, 0, 8,  C_GLOBAL+0,    -1,   -1, 0},
    {TierKind::Global,     1 << 20, 0, 9,  C_GLOBAL+1,    -1,   -1, 0},
    {TierKind::Wide64,     2048,    1, 7,  C_WIDE64,      8,    -1, 0},
    {TierKind::EdgeState,  512,     1, 1,  C_EDGE_512,    10,   14, 0},
    {TierKind::EdgeState,  0,       1, 10, C_EDGE_FIRST,  9,    13, 0},
    {TierKind::EdgeState,  1024,    1, 11, C_EDGE_1024,   11,   15, 0},  // (never dumps: see below)
    {TierKind::Small,      0,       4, 12, -1,            -1,   -1, 0},
    {TierKind::Tiny,       0,       8, 13, -1,            -1,   -1, 0},
};
// the edge-state tiers in the order they run
constexpr int kEdgeSlots[3] = {SLOT_EDGE_FIRST, SLOT_EDGE_512, SLOT_EDGE_1024};

// route_tier_code of a slot whose table has `cap` slots and runs `g` searches per wave
constexpr int route_tier_code(int slot, int cap, int g) {
  switch (kRouteTiers[slot].kind) {
    case TierKind::Wide64: return 900000 + cap;
    case TierKind::EdgeState: return 6000000 + cap * 100 + 32;
    case TierKind::Global: return -1 - (slot - SLOT_GLOBAL);
    default: return cap * 10 + g;
  }
}
constexpr int route_event(int slot) { return kStageEvents + 2 * slot; }  // (and + 1: its end)
constexpr int dump_ctr_word(int slot) {
  return kRouteTiers[slot].dump_queue * kQueueWords + kDumpLineWords * kRouteTiers[slot].dump_line;
}

// The node retry tables there are kernels for (capacity, searches per wave).  OTR_TIERS
// accepts every one but the last, which always ends the list (its overflows go on to the
// global-memory tiers); the engine's launcher walks the same list, so a code cannot be
// accepted without a kernel behind it.
struct TierShape {
  int cap, g;
  constexpr int code() const { return cap * 10 + g; }
};
constexpr TierShape kRetryShapes[] = {{256, 1},  {512, 1}, {768, 1}, {1024, 1}, {2048, 1},
                                      {384, 2},  {448, 2}, {512, 2}, {4096, 1}};
constexpr int kRetryShapeN = (int)(sizeof(kRetryShapes) / sizeof(kRetryShapes[0]));

// Retry tiers of the route search after the first (160-slot, 2 per wave) tier, as
// capacity * 10 + searches per wave.  512x2 (two 512-slot searches per wave) takes the
// long-bound overflows: C4 route 117 -> 112 ms against a 1024-slot G = 1 tier; a 2048-slot
// tier before the 4096 one (2.5x its occupancy): C4 4.57M -> 4.79M probes/s.  The last tier
// is always the 4096-slot one.  `spec` (OTR_TIERS, null: the default) overrides the list for
// A/B runs, e.g. "256,512x2,1024,4096"; items that name no kernel are dropped.
inline std::vector<int> parse_route_tiers(const char* spec_or_null) {
  std::vector<int> t;
  const std::string spec = spec_or_null ? spec_or_null : "256,448x2,1024,2048";
  size_t i = 0;
  while (i < spec.size()) {
    size_t j = spec.find(',', i);
    if (j == std::string::npos) j = spec.size();
    const std::string item = spec.substr(i, j - i);
    const int cap = atoi(item.c_str());
    const int gw = item.find('x') != std::string::npos ? atoi(item.c_str() + item.find('x') + 1) : 1;
    for (int k = 0; k + 1 < kRetryShapeN; ++k)
      if (cap * 10 + gw == kRetryShapes[k].code()) t.push_back(kRetryShapes[k].code());
    i = j + 1;
  }
  if (t.size() > (size_t)kNodeTiers - 1) t.resize(kNodeTiers - 1);
  t.push_back(kRetryShapes[kRetryShapeN - 1].code());
  return t;
}

// ---- the numbering holds together
namespace tier_check {
constexpr bool in_range() {
  for (int s = 0; s < kRouteSlots; ++s) {
    const RouteTier& t = kRouteTiers[s];
    if (t.bank < 0 || t.bank >= kBanks || t.list >= C_CURSORS || t.queue >= kQueues || t.dump_queue >= kQueues ||
        (t.dump_line + 1) * kDumpLineWords > kQueueWords)
      return false;
  }
  return true;
}
// the list counter words that are not a tier's list
constexpr int kOtherWords[] = {C_TASKS_LEFT,   C_STEPS,    C_PATH_TIER,   C_PATH_TIER + 1, C_PATH_TIER + 2,
                               C_PATH_GLOBAL,  C_PATH_GLOBAL + 1, C_PATHS_LEFT,  C_GEN_OVERFLOW,  C_CAP_FLAG,
                               C_STEPS_FRONT,  C_STEPS_ALL, C_FLAGGED,    C_EDGE_PATH,     C_EDGE_PATH + 1};
constexpr bool distinct() {
  for (int a = 0; a < kRouteSlots; ++a) {
    const RouteTier& x = kRouteTiers[a];
    for (int w : kOtherWords)
      if (x.list == w) return false;
    for (int b = 0; b < kRouteSlots; ++b) {
      const RouteTier& y = kRouteTiers[b];
      if (x.dump_queue >= 0 && x.dump_queue == y.queue) return false;  // a dump line inside a work queue
      if (b <= a) continue;
      if (x.bank == y.bank) return false;
      if (x.list >= 0 && x.list == y.list) return false;
      if (x.queue >= 0 && x.queue == y.queue) return false;
      // One shared dump-counter line: the last edge-state tier's is the first node retry
      // tier's.  The last edge tier never dumps (nothing resumes after it: its dump_out is
      // null, so k_route_e1 never claims a slot), and the line stays the node tier's alone.
      const bool last_edge_exception = (a == SLOT_NODE && b == SLOT_EDGE_1024) || (a == SLOT_EDGE_1024 && b == SLOT_NODE);
      if (x.dump_queue >= 0 && x.dump_queue == y.dump_queue && x.dump_line == y.dump_line && !last_edge_exception)
        return false;
    }
  }
  return true;
}
}  // namespace tier_check
static_assert(kRouteSlots <= kRouteSlotsAbi, "route tier slots: otr_batch_result has 16");
static_assert(SLOT_NODE + kNodeTiers == SLOT_GLOBAL && kEdgeSlots[2] == SLOT_EDGE_1024, "slot ranges");
static_assert(route_event(kRouteSlots - 1) + 1 < kEvents, "every slot's event pair lies inside Matcher::ev");
static_assert(route_event(kRouteSlots - 1) + 1 < kPointsEvent && kPointsEvent + 1 < kEvents, "K12's event pair");
static_assert(kTravEvent == kPointsEvent + 2 && kTravEvent + 1 < kEvents, "K13's event pair");
static_assert(tier_check::in_range(), "banks < kBanks, list words < 32, queues and dump lines < 16 queues");
static_assert(tier_check::distinct(), "banks, list words, queues and dump lines are distinct among the tiers");

}  // namespace otr
