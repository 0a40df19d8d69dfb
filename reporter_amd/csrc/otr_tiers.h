// otr_tiers.h — the numbering of the route and path search tiers and the protocol that
// chains them, in one place.  The kernels (otr_kernels.h) read the flags, the task record
// word and the force_edge bits from here; the tables, the parser and the checks are the host's.
//
// A route tier is known by its slot in otr_batch_result's route_tier_code / route_tier_ms /
// route_tier_work (public: bench.py and the tests read the slots by number).  Everything
// else the engine keeps per tier follows from the slot through kRouteTiers: the counter
// bank in the work counters, the word of the list counters (CntWord) that holds its retry
// list's length, its work queue, the line of its dump-slot counter, its event pair, the
// flags its collect takes and the flag its own overflow writes.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

namespace otr {

// ---- the retry protocol.  A search that its tier cannot finish is handed on through a per
// item int32 flag: route tasks in RouteArgs::overflow_flag (one per task), winner-path steps
// in PathArgs::overflow_flag (one per step index).  A kernel writes the flag, the next
// tier's collect takes every item whose flag's bit is in its mask (flag_bit) and clears it.
// The two arrays are separate and so are the two sets of values: distinct types.
enum RouteFlag : int32_t {
  RF_NONE = 0,
  RF_OVERFLOW = 1,     // the table overflowed: the next larger node table, then the slabs
  RF_GENERAL = 3,      // labels of 64 bits: the 64-bit LDS table, then the global-memory search
  RF_EDGE_FIRST = 5,   // a turn-mode task (k_tasks): the first edge-state table
  RF_EDGE_512 = 6,     // outgrew that: the 512-state table
  RF_EDGE_1024 = 7,    // the 1024-state table
  RF_START_TIER = 16,  // + t: a first-tier task whose size estimate starts it in node retry tier t
};
enum PathFlag : int32_t {
  PF_NONE = 0,
  PF_OVERFLOW = 1,     // the table overflowed: the next larger node table, then the slabs
  PF_GENERAL = 3,      // labels of 64 bits, or beyond the edge-state tables: the global-memory search
  PF_EDGE_FIRST = 5,   // a turn-mode step: the 384-state edge table
  PF_EDGE_SECOND = 6,  // outgrew that: the 2048-state table
};
// What a kernel calls from here is inlined ahead of every optimisation, so the kernel compiles
// to exactly what it did with the numbers and shifts written out.
#define OTR_FOLD [[gnu::always_inline]] constexpr
constexpr uint32_t flag_bit(RouteFlag f) { return 1u << f; }
constexpr uint32_t flag_bit(PathFlag f) { return 1u << f; }

constexpr int kNodeTiers = 5;  // node retry tiers at most (OTR_TIERS: four and the 4096-slot one)
OTR_FOLD RouteFlag route_start_flag(int tier) { return (RouteFlag)(RF_START_TIER + tier); }
// what node retry tier t takes: the tier before's overflows and the tasks that start in a tier <= t
constexpr uint32_t node_tier_mask(int t) { return flag_bit(RF_OVERFLOW) | (((2u << t) - 1u) << RF_START_TIER); }
// what k_route_e1 / k_paths_edge write for a search their table of `cap` states cannot finish
OTR_FOLD RouteFlag edge_overflow_flag(int cap) { return cap < 512 ? RF_EDGE_512 : (cap < 1024 ? RF_EDGE_1024 : RF_GENERAL); }
constexpr PathFlag path_edge_overflow_flag(int cap) { return cap < 2048 ? PF_EDGE_SECOND : PF_GENERAL; }
// k_general serves both stages and writes one value into either array when a slab overflows
constexpr int32_t kSlabOverflow = RF_OVERFLOW;
static_assert(kSlabOverflow == (int32_t)PF_OVERFLOW && (int32_t)RF_NONE == (int32_t)PF_NONE,
              "k_general writes the same flags in both stages");
// Bits 2 and 4 of the masks the global-memory route tier and the left-over collect take: no
// kernel writes flag 2 or 4.  Kept bit for bit; dropping them is a change of its own.
constexpr uint32_t kUnusedRouteBits = (1u << 2) | (1u << 4);

// ---- the task record word rec[3t+1].y (the layout: the record comment above k_tasks).
// `start`: 0, or task_start(t) for a step whose size estimate starts it in node retry tier t.
// The fields go in and come out as plain uint32 values (OTR_FOLD, above).
enum TaskWordShift { TW_MODE = 8, TW_FORCED = 10, TW_SH = 11, TW_GENERAL = 16, TW_TURN = 17, TW_START = 18 };
OTR_FOLD uint32_t task_start(uint32_t tier) { return 1u | (tier << 1); }
OTR_FOLD uint32_t task_word(uint32_t Kb, uint32_t mode, uint32_t forced, uint32_t sh, uint32_t general, uint32_t turn,
                            uint32_t start) {
  return Kb | (mode << TW_MODE) | (forced << TW_FORCED) | (sh << TW_SH) | (general << TW_GENERAL) | (turn << TW_TURN) |
         (start << TW_START);
}
OTR_FOLD uint32_t tw_Kb(uint32_t w) { return w & 0xFFu; }            // candidates of the step's state, <= OTR_KMAX
OTR_FOLD uint32_t tw_mode(uint32_t w) { return (w >> TW_MODE) & 3u; }
OTR_FOLD uint32_t tw_forced(uint32_t w) { return (w >> TW_FORCED) & 1u; }
OTR_FOLD uint32_t tw_sh(uint32_t w) { return (w >> TW_SH) & 31u; }
OTR_FOLD uint32_t tw_general(uint32_t w) { return (w >> TW_GENERAL) & 1u; }
OTR_FOLD uint32_t tw_turn(uint32_t w) { return (w >> TW_TURN) & 1u; }
OTR_FOLD uint32_t tw_pre(uint32_t w) { return (w >> TW_START) & 1u; }        // bit 0 of `start`
OTR_FOLD uint32_t tw_start_tier(uint32_t w) { return (w >> (TW_START + 1)) & 7u; }  // the rest of it
static_assert(kNodeTiers - 1 <= 7, "the record's start-tier field (3 bits) holds the last node tier");
static_assert(RF_START_TIER + kNodeTiers <= 32, "the start-tier flags fit a collect's 32 mask bits");
static_assert(RF_EDGE_1024 < RF_START_TIER && PF_EDGE_SECOND < 32, "every flag has its own mask bit");

// ---- RouteArgs::force_edge (test build OTR_FORCE_RETRY; the tests pass the number in OTR_FORCE_EDGE)
enum ForceEdge : int {
  FE_FAIL_E1 = 1,          // fail every OTR_E1CAP (360) / 512 / 1024-state edge-state route search:
  FE_FAIL_E512 = 2,        // the next tier takes it
  FE_FAIL_E1024 = 4,
  FE_FAIL_PATH_384 = 8,    // fail every 384 / 2048-state winner path
  FE_FAIL_PATH_2048 = 16,
  FE_STOP_E1 = 32,         // stop every OTR_E1CAP / 512-state search after 2 / 4 rounds: resumed in
  FE_STOP_E512 = 64,       // the next table (otr_edge1.h e1_dump / e1_restore)
  FE_STOP_NODE = 128,      // stop every node retry-tier search that has dump slots after 2 rounds
                           // (search_run, NDump): resumed tier after tier to the last
};

enum class TierKind { First, Tiny, Small, NodeRetry, Wide64, EdgeState, Global };

constexpr int kRouteSlots = 14;     // slots in use
constexpr int kRouteSlotsAbi = 16;  // otr_batch_result route_tier_*[16]
constexpr int kBanks = 14;          // counter banks of OTR_COUNTERS kinds x kCShards (bank 0: also the batch's)
constexpr int kQueues = 16;         // work queues (XcdQueue) of one batch
constexpr int kQueueWords = 16 * 8; // 8 counters per queue, 128 B apart
constexpr int kDumpLineWords = 16;  // a dump-slot counter has a 128 B line of a queue to itself
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
  unsigned grid;   // blocks of its persistent grid at most (pgrid); 0: sized by its launcher
  uint32_t take;   // the flags its collect takes (a mask of flag_bit), 0: no collect
  RouteFlag overflow;  // the flag it leaves on a task it cannot finish (the first tiers: kFirstWrites)
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
    //  kind               cap      g  bank list          queue dump queue, line  grid  take               overflow
    {TierKind::First,      0,       2, 0,  -1,            -1,   -1, 0,  0,    0u,                RF_OVERFLOW},
    {TierKind::NodeRetry,  0,       0, 2,  C_NODE_TIER+0, 0,    15, 0,  0,    node_tier_mask(0), RF_OVERFLOW},
    {TierKind::NodeRetry,  0,       0, 3,  C_NODE_TIER+1, 1,    15, 1,  0,    node_tier_mask(1), RF_OVERFLOW},
    {TierKind::NodeRetry,  0,       0, 4,  C_NODE_TIER+2, 2,    15, 2,  0,    node_tier_mask(2), RF_OVERFLOW},
    {TierKind::NodeRetry,  0,       0, 5,  C_NODE_TIER+3, 3,    15, 3,  0,    node_tier_mask(3), RF_OVERFLOW},
    {TierKind::NodeRetry,  0,       0, 6,  C_NODE_TIER+4, 4,    15, 4,  0,    node_tier_mask(4), RF_OVERFLOW},
    {TierKind::Global,     1 << 15, 0, 8,  C_GLOBAL+0,    -1,   -1, 0,  0,
     flag_bit(RF_OVERFLOW) | flag_bit(RF_GENERAL) | kUnusedRouteBits,                            RF_OVERFLOW},
    {TierKind::Global,     1 << 20, 0, 9,  C_GLOBAL+1,    -1,   -1, 0,  0,    flag_bit(RF_OVERFLOW), RF_OVERFLOW},
    {TierKind::Wide64,     2048,    1, 7,  C_WIDE64,      8,    -1, 0,  4096, flag_bit(RF_GENERAL), RF_GENERAL},
    {TierKind::EdgeState,  512,     1, 1,  C_EDGE_512,    10,   14, 0,  4096, flag_bit(RF_EDGE_512), edge_overflow_flag(512)},
    {TierKind::EdgeState,  0,       1, 10, C_EDGE_FIRST,  9,    13, 0,  8192, flag_bit(RF_EDGE_FIRST), edge_overflow_flag(0)},
    {TierKind::EdgeState,  1024,    1, 11, C_EDGE_1024,   11,   15, 0,  2048, flag_bit(RF_EDGE_1024), edge_overflow_flag(1024)},  // (never dumps: see below)
    {TierKind::Small,      0,       4, 12, -1,            -1,   -1, 0,  0,    0u,                RF_OVERFLOW},
    {TierKind::Tiny,       0,       8, 13, -1,            -1,   -1, 0,  0,    0u,                RF_OVERFLOW},
};
// the edge-state tiers in the order they run
constexpr int kEdgeSlots[3] = {SLOT_EDGE_FIRST, SLOT_EDGE_512, SLOT_EDGE_1024};
// Every flag a first tier (tiny, small, two-search) leaves, k_tasks' RF_EDGE_FIRST on the
// turn-mode tasks before them included: overflow, general, and a start in any node retry tier
constexpr uint32_t kFirstWrites = flag_bit(RF_OVERFLOW) | flag_bit(RF_GENERAL) | flag_bit(RF_EDGE_FIRST) |
                                  (((1u << kNodeTiers) - 1u) << RF_START_TIER);
// The order the route chain runs in.  The 64-bit table takes RF_GENERAL BEFORE the edge-state
// tiers run: the RF_GENERAL that the last edge-state table writes is therefore taken by the
// global-memory search (which knows edge states), never by the 64-bit node table (which does
// not).  tier_check::wide64_first() holds that.
constexpr int kRouteOrder[kRouteSlots] = {SLOT_TINY,     SLOT_SMALL,    SLOT_FIRST,      SLOT_NODE + 0,  SLOT_NODE + 1,
                                          SLOT_NODE + 2, SLOT_NODE + 3, SLOT_NODE + 4,   SLOT_WIDE64,    SLOT_EDGE_FIRST,
                                          SLOT_EDGE_512, SLOT_EDGE_1024, SLOT_GLOBAL + 0, SLOT_GLOBAL + 1};
// a stage's left-over collect: what is still flagged after its last tier (OTR_MATCH_ERROR)
struct LeftOver {
  int list;
  uint32_t take;
};
constexpr LeftOver kTasksLeft = {C_TASKS_LEFT, flag_bit(RF_OVERFLOW) | flag_bit(RF_GENERAL) | kUnusedRouteBits};

// ---- the winner-path stage's retry tiers, in the order they run (paths_attempt).  Before
// them the first tiers (k_paths over the step lists) leave kPathFirstWrites.
enum class PathKind { Node, EdgeState, Global };
struct PathTier {
  PathKind kind;
  int cap;         // table size (states), or slots of a global-memory slab
  int list;        // CntWord of its list's length
  int queue;       // work queue of the path stage (Batch::pq), -1: none
  unsigned grid;   // blocks of its persistent grid at most; 0: one per slab (Batch::slabs)
  uint32_t take;
  PathFlag overflow;
};
constexpr PathTier kPathTiers[] = {
    {PathKind::Node,      512,     C_PATH_TIER + 0,   0,  16384, flag_bit(PF_OVERFLOW),    PF_OVERFLOW},
    {PathKind::Node,      1024,    C_PATH_TIER + 1,   1,  8192,  flag_bit(PF_OVERFLOW),    PF_OVERFLOW},
    {PathKind::Node,      4096,    C_PATH_TIER + 2,   2,  4096,  flag_bit(PF_OVERFLOW),    PF_OVERFLOW},
    {PathKind::EdgeState, 384,     C_EDGE_PATH + 0,   3,  4096,  flag_bit(PF_EDGE_FIRST),  path_edge_overflow_flag(384)},
    {PathKind::EdgeState, 2048,    C_EDGE_PATH + 1,   4,  512,   flag_bit(PF_EDGE_SECOND), path_edge_overflow_flag(2048)},
    {PathKind::Global,    1 << 15, C_PATH_GLOBAL + 0, -1, 0,     flag_bit(PF_OVERFLOW) | flag_bit(PF_GENERAL), PF_OVERFLOW},
    {PathKind::Global,    1 << 20, C_PATH_GLOBAL + 1, -1, 0,     flag_bit(PF_OVERFLOW),    PF_OVERFLOW},
};
constexpr int kPathQueues = 8;  // work queues of the path stage (Batch::pq)
constexpr int kPathTierN = (int)(sizeof(kPathTiers) / sizeof(kPathTiers[0]));
constexpr uint32_t kPathFirstWrites = flag_bit(PF_OVERFLOW) | flag_bit(PF_GENERAL) | flag_bit(PF_EDGE_FIRST);
constexpr LeftOver kPathsLeft = {C_PATHS_LEFT, flag_bit(PF_OVERFLOW) | flag_bit(PF_GENERAL)};

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
// the place of a slot in the run order, -1: not in it
constexpr int order_of(int slot) {
  for (int i = 0; i < kRouteSlots; ++i)
    if (kRouteOrder[i] == slot) return i;
  return -1;
}
constexpr bool first_kind(TierKind k) { return k == TierKind::First || k == TierKind::Small || k == TierKind::Tiny; }
constexpr uint32_t route_writes(int slot) {
  return first_kind(kRouteTiers[slot].kind) ? kFirstWrites : flag_bit(kRouteTiers[slot].overflow);
}
// every flag a tier leaves is taken by a tier that runs later, or by the left-over collect
constexpr bool route_chain() {
  for (int i = 0; i < kRouteSlots; ++i) {
    if (order_of(i) < 0) return false;  // (every slot runs)
    uint32_t later = kTasksLeft.take;
    for (int j = i + 1; j < kRouteSlots; ++j) later |= kRouteTiers[kRouteOrder[j]].take;
    if (route_writes(kRouteOrder[i]) & ~later) return false;
  }
  return true;
}
constexpr bool path_chain() {
  for (int i = 0; i < kPathTierN; ++i)
    if (kPathTiers[i].queue >= kPathQueues || kPathTiers[i].list >= C_CURSORS) return false;
  for (int i = -1; i < kPathTierN; ++i) {  // (-1: the first tiers)
    uint32_t later = kPathsLeft.take;
    for (int j = i + 1; j < kPathTierN; ++j) later |= kPathTiers[j].take;
    if ((i < 0 ? kPathFirstWrites : flag_bit(kPathTiers[i].overflow)) & ~later) return false;
  }
  return true;
}
// only the first tiers write RF_GENERAL ahead of the 64-bit table (kRouteOrder's comment)
constexpr bool wide64_first() {
  for (int i = 0; i < order_of(SLOT_WIDE64); ++i) {
    const RouteTier& t = kRouteTiers[kRouteOrder[i]];
    if (!first_kind(t.kind) && t.overflow == RF_GENERAL) return false;
  }
  return kRouteTiers[SLOT_WIDE64].take == flag_bit(RF_GENERAL);
}
constexpr uint32_t global_takes(bool paths) {
  uint32_t m = 0;
  for (int s = 0; s < kRouteSlots; ++s)
    if (!paths && kRouteTiers[s].kind == TierKind::Global) m |= kRouteTiers[s].take;
  for (int t = 0; t < kPathTierN; ++t)
    if (paths && kPathTiers[t].kind == PathKind::Global) m |= kPathTiers[t].take;
  return m;
}
}  // namespace tier_check
static_assert(tier_check::route_chain(), "a route flag that no later tier and no left-over collect takes");
static_assert(tier_check::path_chain(), "a path flag that no later tier and no left-over collect takes, or a queue or list word out of range");
static_assert(tier_check::wide64_first(), "the 64-bit table must take RF_GENERAL before a retry tier writes it");
static_assert(kTasksLeft.take == tier_check::global_takes(false) && kPathsLeft.take == tier_check::global_takes(true),
              "a left-over collect takes what the stage's global-memory tiers take");
static_assert(kRouteOrder[9] == kEdgeSlots[0] && kRouteOrder[10] == kEdgeSlots[1] && kRouteOrder[11] == kEdgeSlots[2],
              "kEdgeSlots is the run order's edge-state part");
static_assert(kRouteSlots <= kRouteSlotsAbi, "route tier slots: otr_batch_result has 16");
static_assert(SLOT_NODE + kNodeTiers == SLOT_GLOBAL && kEdgeSlots[2] == SLOT_EDGE_1024, "slot ranges");
static_assert(route_event(kRouteSlots - 1) + 1 < kEvents, "every slot's event pair lies inside Matcher::ev");
static_assert(route_event(kRouteSlots - 1) + 1 < kPointsEvent && kPointsEvent + 1 < kEvents, "K12's event pair");
static_assert(kTravEvent == kPointsEvent + 2 && kTravEvent + 1 < kEvents, "K13's event pair");
static_assert(tier_check::in_range(), "banks < kBanks, list words < 32, queues and dump lines < 16 queues");
static_assert(tier_check::distinct(), "banks, list words, queues and dump lines are distinct among the tiers");

#undef OTR_FOLD
}  // namespace otr
