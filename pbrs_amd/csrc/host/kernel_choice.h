// host/kernel_choice.h — which kernels render a scene, as keys: plain C++, no HIP header.
//
// prepare_scene (host/scene_prepare.h) finds out the SceneFacts; choose_kernels turns them, bent by the developer overrides, into a
// KernelChoice of traversal keys and k_shade keys; pbrs_gpu.hip instantiates a kernel per valid key (extend_key_ok, shadow_key_ok,
// PBRS_SHADE_KERNELS) and bind_kernels looks the choice up in those tables.
#pragma once
#include <cstddef>
#include <cstdint>
#include <optional>

#include "../device/scene.h"

namespace pbrs {

// Developer overrides (A/B timing of kernel selection: tools/ab_env.sh): environment variables that builds made with
// -DPBRS_DEV_OVERRIDES read once per context (pbrs_create); every other build leaves the defaults, which bend nothing.  The shipped
// library never reads the environment: a bench line must not depend on the box it ran on.
struct DevOverrides {
    bool overlap_passes = true;   // PBRS_OVERLAP_PASSES=0: every pass on the main stream, as in rounds 1-3
    bool sort_classes = true;     // PBRS_SORT_CLASSES=0: no class sort
    bool split_lambert = true;    // PBRS_SPLIT_LAMBERT=0: one general k_shade launch for all classes
    bool split_fourier = true;    // PBRS_SPLIT_FOURIER=0: one launch of the Fourier variants over every class, as in round 2
    bool split_queue = true;      // PBRS_SPLIT_QUEUE=0: k_extend never splits the path integrator's queue
    bool wide_shadow = true;      // PBRS_WIDE without bit 1: k_shadow keeps the binary walk
    bool lds_scene = true;        // PBRS_LDS_SCENE=0: the traversal kernels never stage the whole scene in LDS
    bool lds_top = true;          // PBRS_LDS_TOP=0: ... nor the TLAS alone
    bool raygen_tiles8 = true;    // PBRS_RAYGEN_TILES8=0: no 8 x 8 pixel tiles in the slot order
    uint32_t shade_spec = ~0u;    // PBRS_SHADE_SPEC: a mask of the path integrator's k_shade specialisation
    uint32_t shade_lds = ~0u;     // PBRS_SHADE_LDS: a mask of what k_shade stages in LDS
    std::optional<bool> long_walks, full_steps;         // PBRS_LONG_WALKS / PBRS_FULL_STEPS
    std::optional<uint32_t> overlap_from, refill_below;  // PBRS_OVERLAP_FROM / PBRS_REFILL_BELOW
    std::optional<uint32_t> raygen_chunk;  // PBRS_RAYGEN_CHUNK: pixels per slot-order chunk (0: the sample index outermost, as in round 1)
    size_t lds_min = 0;           // PBRS_LDS_MIN: dynamic LDS bytes the traversal kernels take at least (lowers their occupancy)
};

// What prepare_scene finds out about a scene that decides which kernels render it (choose_kernels).
struct SceneFacts {
    uint32_t features = 0;      // DevScene::features: PBRS_FEAT_ANALYTIC, _SHADING_CHECK, and _FLAT_TLAS where k_extend scans the TLAS leaves
    bool tlas_scanned = false;  // the TLAS leaf copies exist (DevScene::n_flat): k_shadow scans them
    bool exact_extent = false;  // DevScene::exact_extent: the closest-hit walks follow ray.t_max to the letter (PBRS_FEAT_EXTENT)
    bool long_walks = false;    // a walk of PBRS_LONG_WALK_HEIGHT levels or more: the PBRS_FEAT_LONG_WALKS kernels
    bool full_steps = false;    // ... whose further node steps are full ones (PBRS_FEAT_FULL_STEPS): coordinates outside the guarded range of the division-free box test
    bool entry_nodes = false;   // DevScene::entry_inst names an instance: camera rays may enter its BLAS at per-pixel entry nodes (device/entry_nodes.h)
    bool wide_ok = false;       // k_shadow may walk the four-wide nodes (a scanned TLAS, built wide nodes, a BLAS deep enough)
    size_t stack_bytes = 0;     // a block's stack rows: DevScene::lds_off_words
    size_t wide_stack_bytes = 0;  // ... of the four-wide walk: DevScene::wide_cap rows
    size_t scene_bytes = 0;     // the arrays the walks read, as stage_scene copies them
    size_t top_bytes = 0;       // the TLAS nodes, as stage_top copies them
    uint32_t n_classes = 0;     // DevScene::n_classes
    uint32_t lambert_class = 0; // shading class of the materials that are one untextured Lambertian DiffuseReflect (0: none)
    uint32_t fourier_class = 0; // shading class of the materials that are one Fourier BSDF (0: none)
    bool textured = false;      // some lobe evaluates a non-Solid texture: k_shade<.., true, ..>
    bool fourier = false;       // some lobe is a Fourier BSDF: k_shade<.., PBRS_SHADE_FOURIER>
    bool lambert = false;       // every lobe is an untextured Lambertian DiffuseReflect, at most one per material
    uint32_t light_spec = 0;    // PBRS_SHADE_LIGHT_*: every area light has that shape
    uint32_t shade_lds = 0;     // PBRS_SHADE_LDS_*: what fits k_shade's LDS budget
    size_t shade_rec_bytes = 0, shade_tri_bytes = 0;  // what stage_shade_scene copies for PBRS_SHADE_LDS_RECORDS, and for _TRIS on top
};

// The traversal kernels are instantiated per key (device/scene.h PBRS_FEAT_*): one table entry per valid key, filled at compile
// time (pbrs_gpu.hip); configure_kernels walks the tables and bind_kernels takes its pointers from them alone.  A key is a feature set, plus
// kStatsKey for the instrumented variants, of which there is one per table and scene kind.  k_shadow never evaluates shading frames
// nor follows the extent, so PBRS_FEAT_SHADING_CHECK and _EXTENT do not select it; k_extend walks binary nodes only (PBRS_FEAT_WIDE:
// k_shadow's walk over four-wide nodes, scenes with a scanned TLAS).  `indirect` / `slow_*`: see kernels.h.
constexpr uint32_t kStatsKey = 512u;  // above the PBRS_FEAT_* bits 0 .. 8
constexpr uint32_t kTraversalKeys = 2u * kStatsKey;
// a scene whose closest-hit walks follow the extent: no leaf scan, no staging, one k_extend each way
constexpr uint32_t kExtentFeatures = PBRS_FEAT_ANALYTIC | PBRS_FEAT_SHADING_CHECK | PBRS_FEAT_EXTENT;
constexpr uint32_t kShadowStatsFeatures = PBRS_FEAT_ANALYTIC | PBRS_FEAT_FLAT_TLAS;
constexpr bool extend_key_ok(uint32_t k) {
    const uint32_t f = k & ~kStatsKey;
    if (f & PBRS_FEAT_EXTENT) return f == kExtentFeatures;
    if (k & kStatsKey) return f == PBRS_FEAT_ALL;  // the instrumented kernel carries every feature
    if (f & PBRS_FEAT_WIDE) return false;
    if ((f & PBRS_FEAT_FULL_STEPS) && !(f & PBRS_FEAT_LONG_WALKS)) return false;  // further node steps exist in the long-walk kernels only
    if ((f & PBRS_FEAT_LDS_SCENE) && (f & PBRS_FEAT_FULL_STEPS)) return false;  // a scene of a few KB
    if ((f & PBRS_FEAT_LDS_TOP) && (f & (PBRS_FEAT_LDS_SCENE | PBRS_FEAT_FULL_STEPS | PBRS_FEAT_FLAT_TLAS))) return false;  // a TLAS too large to scan
    return true;
}
// The k_extend instantiations that also exist as the entry variant (k_extend<.., EntryArgs>: bounce 0 enters the table instance's BLAS at the
// pixel's entry nodes, device/entry_nodes.h): those that carry the split-plane cull and walk long — not the instrumented ones (their node
// counts are the oracle's), not the walks that follow the extent, not the kernels that stage the scene or the TLAS in LDS, and not the
// kernels with full further node steps (PBRS_FEAT_FULL_STEPS: a scene outside the guarded range, which gets no table).  The entry
// variants follow the plain ones in what extend_fns() returns: entry_key(k).
// A variant must keep the waves per SIMD of its plain kernel (a wave is worth 8 % of k_extend on C4): kEntryKeysLosingAWave
// lists the keys whose variant does not — their scenes walk every bounce from the root — and `tools/isa_stats.py --check-entry-waves`
// fails when a variant that IS instantiated has fewer waves than its plain kernel.
//    9 (analytic shapes, TLAS walked as a tree):  70 -> 75 VGPRs, 7 -> 6 waves
//   14 (shading check, scanned TLAS):             79 -> 85 VGPRs, 6 -> 5 waves
constexpr uint32_t kEntryKeysLosingAWave[] = {PBRS_FEAT_LONG_WALKS | PBRS_FEAT_ANALYTIC, PBRS_FEAT_LONG_WALKS | PBRS_FEAT_SHADING_CHECK | PBRS_FEAT_FLAT_TLAS};
constexpr bool extend_entry_ok(uint32_t k) {
    for (uint32_t lost : kEntryKeysLosingAWave)
        if (k == lost) return false;
    return k < kTraversalKeys && extend_key_ok(k) &&
           !(k & (kStatsKey | PBRS_FEAT_EXTENT | PBRS_FEAT_LDS_TOP | PBRS_FEAT_LDS_SCENE | PBRS_FEAT_FULL_STEPS)) && (k & PBRS_FEAT_LONG_WALKS);
}
static_assert(extend_entry_ok(13u) && !extend_entry_ok(9u) && !extend_entry_ok(14u) && !extend_entry_ok(45u), "the entry variants' keys");
constexpr uint32_t kExtendKeys = 2u * kTraversalKeys;
constexpr uint32_t entry_key(uint32_t k) { return kTraversalKeys + k; }
constexpr bool shadow_key_ok(uint32_t k) {
    const uint32_t f = k & ~kStatsKey;
    if (k & kStatsKey) return f == kShadowStatsFeatures;
    if (f & (PBRS_FEAT_SHADING_CHECK | PBRS_FEAT_EXTENT)) return false;
    if ((f & PBRS_FEAT_FULL_STEPS) && !(f & PBRS_FEAT_LONG_WALKS)) return false;
    if ((f & PBRS_FEAT_LDS_SCENE) && (f & (PBRS_FEAT_WIDE | PBRS_FEAT_FULL_STEPS))) return false;
    if ((f & PBRS_FEAT_LDS_TOP) && (f & (PBRS_FEAT_LDS_SCENE | PBRS_FEAT_WIDE | PBRS_FEAT_FULL_STEPS | PBRS_FEAT_FLAT_TLAS))) return false;
    if ((f & PBRS_FEAT_WIDE) && !(f & PBRS_FEAT_FLAT_TLAS)) return false;
    return true;
}

// The k_shade instantiations (kernels.h: INTEG, TEX, SPEC) the choices name: X(integrator, textured, spec).
#define PBRS_SHADE_LDS_ALL (PBRS_SHADE_LDS_RECORDS | PBRS_SHADE_LDS_TRIS)
#define PBRS_SHADE_FOURIER_ALONE (PBRS_SHADE_FOURIER | PBRS_SHADE_FOURIER_ONLY)
#define PBRS_SHADE_KERNELS(X)                                                                                                            \
    /* the path integrator's untextured variants, specialised on Lambert-only scenes and their light shape, with the shading records  \
       (and the triangle records) staged in LDS */                                                                                     \
    X(PBRS_INTEGRATOR_PATH, false, 0u)                                                                                                   \
    X(PBRS_INTEGRATOR_PATH, false, PBRS_SHADE_LAMBERT)                                                                                   \
    X(PBRS_INTEGRATOR_PATH, false, PBRS_SHADE_LAMBERT | PBRS_SHADE_LIGHT_SPHERE)                                                         \
    X(PBRS_INTEGRATOR_PATH, false, PBRS_SHADE_LAMBERT | PBRS_SHADE_LIGHT_TRIANGLE)                                                       \
    X(PBRS_INTEGRATOR_PATH, false, PBRS_SHADE_LDS_RECORDS)                                                                               \
    X(PBRS_INTEGRATOR_PATH, false, PBRS_SHADE_LDS_RECORDS | PBRS_SHADE_LAMBERT)                                                          \
    X(PBRS_INTEGRATOR_PATH, false, PBRS_SHADE_LDS_RECORDS | PBRS_SHADE_LAMBERT | PBRS_SHADE_LIGHT_SPHERE)                                \
    X(PBRS_INTEGRATOR_PATH, false, PBRS_SHADE_LDS_RECORDS | PBRS_SHADE_LAMBERT | PBRS_SHADE_LIGHT_TRIANGLE)                              \
    X(PBRS_INTEGRATOR_PATH, false, PBRS_SHADE_LDS_ALL)                                                                                   \
    X(PBRS_INTEGRATOR_PATH, false, PBRS_SHADE_LDS_ALL | PBRS_SHADE_LAMBERT)                                                              \
    X(PBRS_INTEGRATOR_PATH, false, PBRS_SHADE_LDS_ALL | PBRS_SHADE_LAMBERT | PBRS_SHADE_LIGHT_SPHERE)                                    \
    X(PBRS_INTEGRATOR_PATH, false, PBRS_SHADE_LDS_ALL | PBRS_SHADE_LAMBERT | PBRS_SHADE_LIGHT_TRIANGLE)                                  \
    /* textures, the Fourier lobe, the Fourier materials' class alone */                                                                \
    X(PBRS_INTEGRATOR_PATH, true, 0u)                                                                                                    \
    X(PBRS_INTEGRATOR_PATH, true, PBRS_SHADE_FOURIER)                                                                                    \
    X(PBRS_INTEGRATOR_PATH, false, PBRS_SHADE_FOURIER_ALONE)                                                                             \
    X(PBRS_INTEGRATOR_DIRECT, false, 0u)                                                                                                 \
    X(PBRS_INTEGRATOR_DIRECT, true, 0u)                                                                                                  \
    X(PBRS_INTEGRATOR_DIRECT, true, PBRS_SHADE_FOURIER)                                                                                  \
    X(PBRS_INTEGRATOR_DIRECT, false, PBRS_SHADE_FOURIER_ALONE)                                                                           \
    /* the visualisers */                                                                                                               \
    X(PBRS_INTEGRATOR_MATERIALS, false, 0u)                                                                                              \
    X(PBRS_INTEGRATOR_NORMALS, false, 0u)

// A traversal kernel by key, with the dynamic LDS it is launched with: the lanes' stack rows and what the kernel stages.
struct TraversalKey {
    uint32_t key = 0;
    size_t lds = 0;
};
struct ShadeKey {
    uint32_t integ = 0;
    bool tex = false;
    uint32_t spec = 0;
    size_t lds = 0;
    uint32_t range = 0;  // the st.class_range entry the launch covers (PBRS_MAX_CLASSES: the classes before the last one), 0: the queue
};
struct IntegratorChoice {
    enum Order { NO_ORDER, CLASS_SORT, CLASS_MAJOR } order = NO_ORDER;  // how the queue is ordered before k_shade
    uint32_t last_class = 0;  // CLASS_MAJOR: the class that goes last, over PBRS_MAX_CLASSES classes
    uint32_t n_shade = 0;     // one or two k_shade launches
    ShadeKey shade[2];
};
struct KernelChoice {
    TraversalKey extend[2];  // [instrumented]
    TraversalKey shadow[2];
    bool wide_shadow = false;     // the timed k_shadow walks four-wide nodes ...
    TraversalKey shadow_slow;     // ... and this binary-walk kernel works off the rays it refused
    bool entry_extend = false;    // bounce 0 launches the entry variant of extend[0] (extend_entry_ok; pbrse_set_entry_nodes may still turn it off)
    bool split_queue = false;     // k_extend may split the path integrator's queue (one shading class; run_pass decides)
    uint32_t lds_staging = 0;     // PBRS_FEAT_LDS_SCENE, PBRS_FEAT_LDS_TOP or 0: what the traversal kernels stage in LDS
    IntegratorChoice integ[PBRS_INTEGRATOR_NORMALS + 1];
};

// The kernels that render a scene, from what prepare_scene found out about it, bent by the developer overrides.
KernelChoice choose_kernels(const SceneFacts& f, const DevOverrides& dev);

}  // namespace pbrs
