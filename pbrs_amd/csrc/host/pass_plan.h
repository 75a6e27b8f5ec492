// host/pass_plan.h — what the pass driver of pbrs_gpu.hip (ensure_work, pass_size, run_pass, render_common) decides before it allocates
// or launches: plain C++, no HIP header and no pbrs_ctx, so that tests/pass_plan_check.cpp runs every decision on a CPU under
// AddressSanitizer.
//
//   path_layout       where each per-path column of a pass set lies in its one allocation, from one table (kPathColumns)
//   kCounters         where each region of a pass set's counter block lies
//   samples_per_pass  the pass size of a render, from the memory it is told is free
//   bounce_count, pass_shape, bounce_plan   the bounces of a pass, its grids, and what each bounce launches
// pbrs_gpu.hip allocates, turns offsets into pointers and launches: every value of a launch that is not a pointer comes from here.
#pragma once
#include <cstddef>
#include <cstdint>
#include <optional>

#include "arg_checks.h"     // kMaxDepth
#include "kernel_choice.h"  // IntegratorChoice; device/scene.h: kBlock, PBRS_SORT_TILE, PBRS_WORK_*, PBRS_PERSISTENT_BLOCKS, PBRS_QSPLIT_*

namespace pbrs {

// ---- the path state of a pass set ----
// The columns of a pass set, in the order they lie in its allocation (kernels.h, PathState, says what each holds; the nee queue, the slow
// list and rng_hi0 are arguments of the kernels that use them, pbrs_ctx::PassSet).
enum PathColumn : uint32_t {
    COL_Q,                  // q[half][k] at COL_Q + 3 * half + k
    COL_HIT = COL_Q + 6,
    COL_L,
    COL_NEE,                // nee[k] at COL_NEE + k
    COL_SR = COL_NEE + 3,   // sr[k] at COL_SR + k
    COL_OCC = COL_SR + 3,   // occ[0]; occ[1] follows it at + n_slots
    COL_NEEQ,
    COL_PERM,
    COL_CLS,
    COL_SLOW,
    COL_TILE_HIST,
    COL_CLASS_RANGE,
    COL_RNG_HI0,
    N_PATH_COLUMNS
};
// A column holds per_slot * n_slots + per_tile * n_tiles + fixed elements of `elem` bytes (n_tiles: path_tiles).  Its region is
// rounded up to kPathAlign bytes — in `parts` equal parts, each rounded on its own (sr[k]: one aligned half per shadow ray of a path).
struct PathColumnRow {
    const char* name;
    uint32_t elem, per_slot, per_tile, fixed, parts;
};
constexpr size_t kPathAlign = 256;
constexpr PathColumnRow kPathColumns[N_PATH_COLUMNS] = {
    {"q[0][0]", 16, 1, 0, 0, 1}, {"q[0][1]", 16, 1, 0, 0, 1}, {"q[0][2]", 16, 1, 0, 0, 1},
    {"q[1][0]", 16, 1, 0, 0, 1}, {"q[1][1]", 16, 1, 0, 0, 1}, {"q[1][2]", 16, 1, 0, 0, 1},
    {"hit", 16, 1, 0, 0, 1},
    {"L", 16, 1, 0, 0, 1},
    {"nee[0]", 16, 1, 0, 0, 1}, {"nee[1]", 16, 1, 0, 0, 1}, {"nee[2]", 16, 1, 0, 0, 1},
    {"sr[0]", 16, 2, 0, 0, 2}, {"sr[1]", 16, 2, 0, 0, 2}, {"sr[2]", 16, 2, 0, 0, 2},  // two shadow rays per path
    {"occ", 1, 2, 0, 0, 1},                                                             // one byte per shadow ray
    {"nee queue", 4, 1, 0, 0, 1},
    {"perm", 4, 1, 0, 0, 1},
    {"cls", 1, 1, 0, 0, 1},
    {"slow", 4, 2, 0, 0, 1},                                   // a slow-list entry per shadow ray
    {"tile_hist", 4, 0, PBRS_MAX_CLASSES, 0, 1},               // per sort tile and class
    {"class_range", 8, 0, 0, PBRS_MAX_CLASSES + 1, 1},         // a uint2 per class, and one for the classes before the last
    {"rng_hi0", 4, 1, 0, 0, 1},
};
// The bytes a path holds: what samples_per_pass budgets the free memory with (the sort tables and the alignment are not per path).
constexpr uint64_t path_bytes_per_slot() {
    uint64_t b = 0;
    for (const PathColumnRow& r : kPathColumns) b += (uint64_t)r.elem * r.per_slot;
    return b;
}
constexpr uint64_t kPathBytesPerSlot = path_bytes_per_slot();
static_assert(kPathBytesPerSlot == 295, "a column changed: every automatic pass size moves with it");

// Sort tiles the tile_hist column has room for.
constexpr size_t path_tiles(size_t n_slots) { return n_slots / PBRS_SORT_TILE + 1; }

struct PathLayout {
    size_t offset[N_PATH_COLUMNS];  // bytes from the start of the allocation; every one a multiple of kPathAlign
    size_t bytes[N_PATH_COLUMNS];   // the region: at least the column's elements
    size_t total;                   // the allocation: the end of the last region
};
PathLayout path_layout(size_t n_slots);

// ---- the counter block of a pass set ----
// Words (u32) of the block, zeroed at the start of every pass.  Per bounce b: act[b] paths entering bounce b (k_shade of bounce b counts
// into act[b + 1]); ns[b], one 64-bit word: low half = paths whose light estimate waits for visibility, high half = shadow rays; slows[b],
// k_shadow's slow-list length; and kHeadWords work-fetch heads each (one per queue segment, kernels.h) for k_extend, k_shadow and the
// binary-walk launch over k_shadow's slow list.
constexpr uint32_t kHeadWords = PBRS_WORK_HEADS * PBRS_WORK_HEAD_STRIDE;
struct CounterLayout {
    uint32_t act, ns, slows, xhead, shead, shead2;  // word offsets of the regions
    uint32_t words;                                 // the block
};
constexpr CounterLayout counter_layout(uint32_t max_depth, uint32_t head_words) {
    const uint32_t stride = max_depth + 2;  // act[b + 1] of the last bounce, and a word to spare
    CounterLayout l{};
    l.act = 0;
    l.ns = l.act + stride;
    l.slows = l.ns + 2 * stride;
    l.xhead = l.slows + stride;
    l.shead = l.xhead + stride * head_words;
    l.shead2 = l.shead + stride * head_words;
    l.words = l.shead2 + stride * head_words;
    return l;
}
constexpr CounterLayout kCounters = counter_layout(kMaxDepth, kHeadWords);
static_assert(kCounters.ns % 2 == 0, "ns is read as 64-bit words");

// ---- the pass size ----
// The samples per pass of a render of `tile_pixels` pixels at `spp` samples each.  `requested`: pbrs_render_params::samples_per_pass, 0 =
// automatic.  `with_direct`: every path carries a record of the D column as well (light passes).  `held_slots`: the slots the context's
// two pass sets hold; `held_direct_bytes`: the bytes its two D columns hold — what the context already holds for paths counts as
// available, so that the answer does not change between calls.  `free_bytes`: the device memory free now, empty where the query failed.
uint32_t samples_per_pass(uint64_t tile_pixels, uint64_t spp, uint32_t requested, bool with_direct, uint64_t held_slots, uint64_t held_direct_bytes,
                          std::optional<uint64_t> free_bytes);

// ---- a pass ----
// The bounces a pass runs: one k_extend, k_shade and k_shadow stage each.
uint32_t bounce_count(uint32_t integrator, uint32_t max_depth);

constexpr uint32_t kStreamGridCap = 4096;                        // blocks of k_nee_resolve, whose work is counted on the device (kernels.h)
constexpr uint32_t kPersistentBlocks = PBRS_PERSISTENT_BLOCKS;  // 256 CUs x up to 6 resident 256-thread blocks (VGPR/LDS permitting)
constexpr uint32_t kSlowGrid = 64;                               // blocks of a binary-walk launch over a slow list (empty in nearly every launch)
struct PassShape {
    uint32_t n_slots;    // P * kc
    uint32_t grid;       // a thread per slot
    uint32_t sgrid;      // ... capped at kStreamGridCap
    uint32_t pgrid;      // persistent traversal kernels: enough blocks to fill the chip, each pulls work until the queue is empty
    uint32_t slow_grid;  // ... of the launch over k_shadow's slow list
    uint32_t n_tiles;    // sort tiles of the queue
};
// A pass of kc sample indices for every one of P pixels (P * kc below 2^28: pass_size).
PassShape pass_shape(uint32_t P, uint32_t kc);

// What bounce `bounce` of a pass launches between k_extend and k_shadow.
struct BouncePlan {
    // PBRS_QSPLIT_* (device/scene.h), or 0: the path integrator on a scene with one shading class (no class sort) has k_extend split
    // its queue into the hits k_shade shades, the paths that only end (emitter hits, misses that see the environment) and the misses
    // nothing happens to
    uint32_t split;
    // the queue in the order the choice asks for; a queue k_extend split: class-major over its two classes, class 1 = the kept paths, last
    IntegratorChoice::Order order;
    uint32_t n_classes;     // CLASS_MAJOR: the k_class_count / k_class_scatter instantiation: PBRS_MAX_CLASSES, or 2 for a split queue
    uint32_t last;          // ... and the class k_class_scan puts last
    uint32_t zero_dropped;  // ... and whether the scatter stores L = 0 for the paths a split queue drops, which no k_shade lane visits (bounce 0)
    uint32_t sorted;        // k_shade reads its paths through the permutation
    uint32_t shade_range[2];  // per k_shade launch: the st.class_range entry it covers (a split queue: the kept paths, 1), 0: the whole queue
};
// `split_queue`: KernelChoice::split_queue.  `ic`: the integrator's choice.  `split_decision`: pbrs_ctx::split_decision (0 = not yet,
// 1 = split, 2 = do not).
BouncePlan bounce_plan(uint32_t integrator, bool split_queue, const IntegratorChoice& ic, int split_decision, uint32_t bounce);

}  // namespace pbrs
