// host/pass_plan.cpp — see pass_plan.h: plain C++, linked into libpbrs_gpu.so and into the CPU check of tests/pass_plan_check.cpp.
#include "pass_plan.h"

namespace pbrs {

PathLayout path_layout(size_t n_slots) {
    PathLayout l{};
    size_t at = 0;
    for (uint32_t i = 0; i < N_PATH_COLUMNS; ++i) {
        const PathColumnRow& r = kPathColumns[i];
        const size_t part = (r.per_slot * n_slots + r.per_tile * path_tiles(n_slots) + r.fixed) * r.elem / r.parts;
        l.offset[i] = at;
        l.bytes[i] = r.parts * ((part + kPathAlign - 1) / kPathAlign * kPathAlign);
        at += l.bytes[i];
    }
    l.total = at;
    return l;
}

uint32_t samples_per_pass(uint64_t tile_pixels, uint64_t spp, uint32_t requested, bool with_direct, uint64_t held_slots, uint64_t held_direct_bytes,
                          std::optional<uint64_t> free_bytes) {
    const uint64_t P = tile_pixels;
    uint64_t k = requested;
    if (k == 0) {
        // ~240M paths in flight (~67 GB of the 288 GB HBM for path, hit, radiance, shadow-ray and nee records), less when
        // that would exceed a quarter of the memory currently free.  Every bounce is a handful of launches and a persistent
        // traversal kernel ends with the latency of its longest walks (hundreds of dependent node fetches on a deep BLAS): the
        // fewer, larger launches a frame is cut into, the less of it is spent draining (C2, 256 spp: 617 / 629 / 637
        // Msamples/s at 32 / 64 / 128 samples per pass; C4: 921 / 939 at 64 / 115).  Stays under the 2^28 paths of check_params.
        uint64_t target = 240ull << 20;
        if (free_bytes) {
            // path, hit, radiance, shadow-ray and nee records; a render with light passes: and the D column (a float4)
            const uint64_t per_path = kPathBytesPerSlot + (with_direct ? 16u : 0u);
            // what the context already holds for paths counts as available
            // (... in both of its pass sets: a set may take a quarter of the memory, the two of them half)
            const uint64_t held_direct = with_direct ? held_direct_bytes : 0u;
            const uint64_t fit = (*free_bytes + held_slots * kPathBytesPerSlot + held_direct) / 4 / per_path;
            if (fit < target) target = fit < (4ull << 20) ? (4ull << 20) : fit;
        }
        k = P >= target ? 1 : target / P;
        if (k < 1) k = 1;
        if (k < spp) {  // passes of equal size: 256 spp at 240 per pass is 128 + 128, not 240 + 16
            const uint64_t passes = (spp + k - 1) / k;
            k = (spp + passes - 1) / passes;
        }
    }
    if (k > spp) k = spp;
    if (k < 1) k = 1;
    return (uint32_t)k;
}

uint32_t bounce_count(uint32_t integrator, uint32_t max_depth) {
    // the direct-lighting integrator is at most two rays deep whatever `depth` says (directlighting.rs:15-17, :36, :49)
    if (integrator == PBRS_INTEGRATOR_DIRECT) return max_depth ? 2u : 0u;
    if (integrator >= PBRS_INTEGRATOR_MATERIALS) return 1u;  // the visualisers: one cast, no lights
    return max_depth;
}

PassShape pass_shape(uint32_t P, uint32_t kc) {
    PassShape s{};
    s.n_slots = P * kc;
    s.grid = (s.n_slots + kBlock - 1) / kBlock;
    s.sgrid = s.grid < kStreamGridCap ? s.grid : kStreamGridCap;
    s.pgrid = s.grid < kPersistentBlocks ? s.grid : kPersistentBlocks;
    s.slow_grid = s.pgrid < kSlowGrid ? s.pgrid : kSlowGrid;
    s.n_tiles = (s.n_slots + PBRS_SORT_TILE - 1) / PBRS_SORT_TILE;
    return s;
}

BouncePlan bounce_plan(uint32_t integrator, bool split_queue, const IntegratorChoice& ic, int split_decision, uint32_t bounce) {
    BouncePlan b{};
    const bool split = integrator == PBRS_INTEGRATOR_PATH && split_queue && split_decision != 2;
    b.split = split ? (PBRS_QSPLIT_ON | (bounce == 0 ? PBRS_QSPLIT_ENV : 0u)) : 0u;
    b.order = split ? IntegratorChoice::CLASS_MAJOR : ic.order;
    b.n_classes = split ? 2u : PBRS_MAX_CLASSES;
    b.last = split ? 1u : ic.last_class;
    b.zero_dropped = (split && bounce == 0) ? 1u : 0u;
    b.sorted = b.order != IntegratorChoice::NO_ORDER ? 1u : 0u;
    // one class range of a class-major queue; a split queue: the kept paths
    for (uint32_t k = 0; k < ic.n_shade; ++k) b.shade_range[k] = ic.shade[k].range ? ic.shade[k].range : split ? 1u : 0u;
    return b;
}

}  // namespace pbrs
