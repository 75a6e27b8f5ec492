// pbrs_gpu.hip — implementation of include/pbrs_gpu.h for gfx950 (MI355X).
//
// Host-side driver of the wavefront pipeline (device/kernels.h names the stages; k_extend, k_shadow and k_shade through kernel_tables.h): owns the HBM copies of the
// flattened scene, the SoA path state, the slot queues and the per-tile accumulator, and issues
//     raygen -> [extend -> shade -> shadow] x max_depth -> accumulate
// per pass of `samples_per_pass` sample indices, all on one HIP stream with no host round trip
// inside a tile: queue lengths stay on the device (kernels read them; empty blocks exit).
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see include/pbrs_numeric.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

#include "../../include/pbrs_gpu.h"
#include "device/raygen.h"
#include "device/class_sort.h"
#include "device/accumulate.h"
#include "device/dev_kernels.h"
#include "kernel_tables.h"
#include "host/scene_prepare.h"
#include "host/arg_checks.h"
#include "host/pass_plan.h"
#include "device/aov.h"
#include "device/film.h"
#include "device/denoise.h"
#include "device/moments.h"
#include "device/matte.h"
#include "device/passes.h"
#include "device/temporal.h"
#include "device/spatial_variance.h"
#include "device/display.h"
#include "device/upsample.h"
#include "device/compare.h"
#include "device/despeckle.h"
#include "device/bloom.h"
#include "device/dof.h"
#include "device/motion_blur.h"

// the host-only upload steps (host/scene_prepare.h, host/kernel_choice.h), argument checks (host/arg_checks.h) and pass driver's decisions (host/pass_plan.h)
using namespace pbrs;

namespace {

#ifndef PBRS_SPLIT_KEEP_PERCENT
#define PBRS_SPLIT_KEEP_PERCENT 85u  // k_extend's queue split stays on where it keeps at most this share of a pass's rays for k_shade
#endif

struct StageEvent {
    int stage;  // 0 raygen, 1 extend, 2 shade, 3 shadow, 4 accumulate
    hipEvent_t a, b;
};

// The developer overrides (host/kernel_choice.h, DevOverrides) of builds made with -DPBRS_DEV_OVERRIDES: read once per context (pbrs_create).
#ifdef PBRS_DEV_OVERRIDES
const char* dev_env(const char* name) { return std::getenv(name); }

DevOverrides read_dev_overrides() {
    DevOverrides o;
    auto flag = [](const char* name, bool& v) {
        if (const char* e = dev_env(name)) v = std::atoi(e) != 0;
    };
    flag("PBRS_OVERLAP_PASSES", o.overlap_passes);
    flag("PBRS_SORT_CLASSES", o.sort_classes);
    flag("PBRS_SPLIT_LAMBERT", o.split_lambert);
    flag("PBRS_SPLIT_FOURIER", o.split_fourier);
    flag("PBRS_SPLIT_QUEUE", o.split_queue);
    flag("PBRS_LDS_SCENE", o.lds_scene);
    flag("PBRS_LDS_TOP", o.lds_top);
    flag("PBRS_RAYGEN_TILES8", o.raygen_tiles8);
    if (const char* e = dev_env("PBRS_WIDE")) o.wide_shadow = (std::atoi(e) & 2) != 0;
    if (const char* e = dev_env("PBRS_SHADE_SPEC")) o.shade_spec = (uint32_t)std::atoi(e);
    if (const char* e = dev_env("PBRS_SHADE_LDS")) o.shade_lds = (uint32_t)std::atoi(e);
    if (const char* e = dev_env("PBRS_LONG_WALKS")) o.long_walks = std::atoi(e) != 0;
    if (const char* e = dev_env("PBRS_FULL_STEPS")) o.full_steps = std::atoi(e) != 0;
    if (const char* e = dev_env("PBRS_OVERLAP_FROM")) o.overlap_from = (uint32_t)std::atoi(e);
    if (const char* e = dev_env("PBRS_REFILL_BELOW")) o.refill_below = (uint32_t)std::atoi(e);
    if (const char* e = dev_env("PBRS_RAYGEN_CHUNK")) {
        const long v = std::atol(e);
        o.raygen_chunk = v > 0 ? (uint32_t)v : 0xffffffffu;
    }
    if (const char* e = dev_env("PBRS_LDS_MIN")) o.lds_min = (size_t)std::atol(e);
    return o;
}
#endif

// The kernels that render the uploaded scene, bound once per upload (bind_kernels): what choose_kernels names (host/kernel_choice.h: the
// keys, the dynamic LDS and the class range of every launch), and the instantiations the keys name.
struct IntegratorPlan {
    IntegratorChoice choice;
    shade_fn_t shade[2] = {};  // [launch], choice.n_shade of them
};
struct KernelPlan {
    KernelChoice choice;  // (its integ[] are the IntegratorPlans' choices)
    extend_fn_t extend[2] = {};  // [instrumented]
    extend_entry_fn_t extend_entry = nullptr;  // where choice.entry_extend: bounce 0's k_extend<.., EntryArgs> (device/entry_nodes.h)
    shadow_fn_t shadow[2] = {};
    shadow_fn_t shadow_slow = nullptr;  // where choice.wide_shadow
    IntegratorPlan integ[PBRS_INTEGRATOR_NORMALS + 1];
};
// A traversal kernel's PBRS_FEAT_* as pbrs_stats::kernel_features_* reports them (0x80000000: instrumented).
uint32_t reported_features(const TraversalKey& k) { return (k.key & ~kStatsKey) | ((k.key & kStatsKey) ? 0x80000000u : 0u); }

// A device buffer of a feature that allocates on first use.  `grow` makes it hold at least `bytes`, grown (not copied): a failure leaves
// the context without it (cap_bytes = 0), usable for every other call.
struct DeviceBuffer {
    void* p = nullptr;
    size_t cap_bytes = 0;
    int grow(pbrs_ctx* c, size_t bytes, const char* what);
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};
// Every first-use buffer of a context (pbrs_ctx::buf).  pbrs_destroy frees the whole array: a new buffer is a new name here and nothing else.
enum BufferId {
    // first-hit AOVs (pbrs_render_tile_aovs*, device/aov.h): the per-pixel running state k_aov folds every pass into (PBRS_AOV_STATE_WORDS per
    // pixel, planar), and the host variant's staging for the finished buffers (the seven of pbrs_aov_buffers, one after the other)
    BUF_AOV_STATE, BUF_AOV_OUT,
    // entry nodes of the camera rays (device/entry_nodes.h): a pbrs_entry_record per pixel of the traced region, then k_entry_nodes' four counts
    BUF_ENTRY_TABLE,
    // filtered film (pbrs_render_tile_filtered*, device/film.h): S.rgb and W of every tile pixel, planar
    BUF_FILTER_SUM,
    // denoisers (pbrs_denoise*, pbrs_denoise_var*, device/denoise.h): two ping-pong colour planes, the guide plane and the instance ids (16 +
    // 16 + 16 + 4 B per pixel, one allocation), and the host variant's staging (denoise_staged).  Each denoiser keeps scratch and staging
    // of its own: + 0 the plain filter's, + 1 the variance-guided one's
    BUF_DENOISE, BUF_DENOISE_VAR, BUF_DENOISE_STAGE, BUF_DENOISE_VAR_STAGE,
    // variance AOV (pbrs_render_tile_aovs_var*, device/moments.h): the per-pixel moments k_moments folds every pass into
    // (PBRS_MOMENT_STATE_WORDS per pixel, planar), and the host variant's staging for the finished buffer
    BUF_MOMENT_STATE, BUF_VARIANCE_OUT,
    // id mattes (pbrs_render_tile_matte*, pbrs_matte_mask*, device/matte.h): the per-pixel tables k_matte folds every pass into
    // (PBRS_MATTE_STATE_WORDS(slots) per pixel, planar), the host variants' staging (ids, coverage, then residual or the mask) and the
    // selection of pbrs_matte_mask* (PBRS_MATTE_MAX_SELECT ids)
    BUF_MATTE_STATE, BUF_MATTE_OUT, BUF_MATTE_SELECT,
    // light passes (pbrs_render_tile_passes*, pbrs_combine_passes, device/passes.h): the per-pixel running state k_pass_fold folds every pass
    // into (PBRS_PASS_STATE_WORDS per pixel, planar), the host variants' staging (the four of pbrs_pass_buffers, one after the other) and the
    // D column of each pass set (PassSet::direct: one float4 per path beside its PathState), held only by a context that has rendered passes
    BUF_PASS_STATE, BUF_PASS_OUT, BUF_PASS_DIRECT, BUF_PASS_DIRECT_SET1,
    // temporal accumulation (pbrs_temporal_accumulate, device/temporal.h): the host variant's staging (the frame, the previous guides,
    // the history in and out, the variance out, one after the other); the device variant needs nothing
    BUF_TEMPORAL_STAGE,
    // moving instances (pbrs_temporal_accumulate_motion*, pbrs_motion_vectors*): the context's copy of the caller's motion table, and
    // the staging of pbrs_motion_vectors' host variant (depth, instance, the vectors, the previous depth, one after the other)
    BUF_MOTION_TABLE, BUF_MOTION_STAGE,
    // spatial variance estimate (pbrs_spatial_variance, device/spatial_variance.h): the host variant's staging (moments, length, the three
    // guides, the variance, which is estimated in place, one after the other); the device variant needs nothing
    BUF_SPATIAL_STAGE,
    // display transform (pbrs_display, device/display.h): the 512-word histogram, the scale word and the host variant's two exposure
    // words (kDisplayScratchWords), and the host variant's staging (the image, the 8-bit result)
    BUF_DISPLAY, BUF_DISPLAY_STAGE,
    // guided upsampling (pbrs_upsample, device/upsample.h): the host variant's staging (the low image and its four guides at the low
    // size, the four full-size guides, the result and its weights, one after the other); the device variant needs nothing
    BUF_UPSAMPLE_STAGE,
    // image comparison (pbrsx_compare, device/compare.h): the per-tile partial sums and the room k_compare_finish quarters them into (64 +
    // 16 B per tile), and the host variant's staging (the two images, the two maps, the 64-byte record, one after the other)
    BUF_COMPARE, BUF_COMPARE_STAGE,
    // despeckle (pbrsi_despeckle, device/despeckle.h): the host variant's staging (the image, the variance, which is treated in place,
    // the result, the mask, the removed energy and the 16-byte record, one after the other); the device variant needs nothing
    BUF_DESPECKLE_STAGE,
    // ... and the per-block counts k_despeckle_finish sums (8 B for each of kDespeckleMaxBlocks blocks), held only by a context that has
    // asked a despeckle call for its record
    BUF_DESPECKLE,
    // bloom (pbrsb_bloom, device/bloom.h): the pyramid, one chain of levels of a float4 per level pixel, held only by a context that has
    // called it with a strength above 0; and the host variant's staging (the image, which the result replaces)
    BUF_BLOOM, BUF_BLOOM_STAGE,
    // depth of field (pbrsf_dof, device/dof.h): the host variant's staging (rgb, depth, the output and the circles); the device call holds nothing
    BUF_DOF_STAGE,
    // motion blur (pbrsm_motion_blur, device/motion_blur.h): the host variant's staging (rgb, depth, motion, the output and the velocities); the device call holds nothing
    BUF_MOTION_BLUR_STAGE,
    N_BUFFERS
};

}  // namespace

struct pbrs_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string error;

    // scene
    bool has_scene = false;
    std::vector<void*> scene_allocs;
    DevScene S{};
    uint32_t stack_depth = 0;

    // Two sets of per-pass working memory (path state, queues, counters) and two streams.  Consecutive passes of a render alternate
    // between the sets; a pass runs its bounces below overlap_from on the main stream and the rest — near-empty launches that end with
    // the latency of their longest walks — on a second, high-priority stream, beside the full kernels of the next pass's first bounces
    // (render_common, run_pass).  cur_set names the set in use (cur(c)); pass set 0 is the one in use between calls.
    struct PassSet {
        void* state_mem = nullptr;    // every per-path array of PathState, carved out of one allocation
        size_t cap_slots = 0;
        PathState st{};
        uint32_t* neeq = nullptr;     // cap_slots: slots of the paths whose estimate waits for two shadow rays
        uint32_t* rng_hi0 = nullptr;  // cap_slots: the RNG's high word of every camera sample, from k_raygen to bounce 0's k_shade (kernels.h, PathState)
        uint32_t* slow = nullptr;     // 2 * cap_slots: queue positions the wide-walk k_shadow handed to the binary-walk kernel
        uint32_t* counters = nullptr; // kCounters.words: the regions of CounterLayout (host/pass_plan.h)
        float4* direct = nullptr;     // light passes: the D column, [slot] = L[slot] as bounce 0 left it (device/passes.h); null unless the render asks for passes
        hipEvent_t accumulated = nullptr;  // the set's last k_accumulate has run (late stream): the set's memory is free for its next pass
        hipEvent_t late = nullptr;         // the set's pass has run its bounces below pbrs_ctx::overlap_from (main stream): the late stream takes over
        bool in_flight = false;            // `accumulated` has been recorded at least once
    } pass_set[2];
    int cur_set = 0;
    hipStream_t main_stream = nullptr;  // the stream of set 0: the context's own, or the caller's (pbrs_set_stream)
    hipStream_t second_stream = nullptr;  // the late stream: the context's own, high priority, ordered against the main one by events
    // Entry nodes of the camera rays (device/entry_nodes.h): pbrse_set_entry_nodes; of the uploaded scene's table instance, the levels of
    // its BLAS and the stack rows a lane has left there (PreparedScene); the table of the render being queued (null: none) and whether the
    // last render had one (pbrse_last_entry_info reads the counts behind the table)
    bool entry_nodes = true;
    uint32_t entry_height = 0, entry_rows = 0;
    const uint4* entry_table = nullptr;
    bool last_entry = false;
    uint32_t last_entry_pixels = 0;
    bool overlap_passes = true;  // pbrs_set_pass_overlap (DevOverrides::overlap_passes): every pass on the main stream, as in rounds 1-3
    // The bounce from which a pass moves to the late stream (and the next pass starts behind it on the main one).  Same-box A/B lines in
    // profiles/r04m_ab_pass_overlap.log: scenes that live in every XCD's L2 gain most from bounce 2 on (C2 +1.9 %, C3 +1.5 %, C5 +3.3 %
    // against one stream; from 1: +1.3 / +1.2 / +2.7, from 3: 0 / +1.4 / +2.3), a scene that lives in the Infinity Cache from bounce 4 on
    // (C4 +1.0 %; from 3: +0.8, from 2 or 5: +0.2) — two passes' full kernels side by side cost it its cache residency (streams by pass,
    // every bounce overlapped: -2.6 %, profiles/r04l_ab_pass_overlap_streams_by_pass.log).
    uint32_t overlap_from = 2;
    // working set
    size_t cap_pixels = 0;
    float* sum = nullptr;         // 3 * cap_pixels, planar
    float* rgb_dev = nullptr;     // 3 * cap_pixels, row-major (for the host-output variant)
    GlobalCounters* gcnt = nullptr;  // [0] extend, [1] shadow
    unsigned long long* nonfinite = nullptr;  // samples of the current render whose radiance is not finite
    unsigned long long* bounce_acc = nullptr; // 2 x PBRS_STATS_MAX_BOUNCES: queue sizes per bounce of the current instrumented render

    // timing
    std::vector<StageEvent> events;
    size_t events_used = 0;
    std::vector<hipEvent_t> total_ev;  // 2
    pbrs_stats pending{};
    bool pending_counters = false, pending_times = false;
    DevOverrides dev;  // read in pbrs_create (-DPBRS_DEV_OVERRIDES builds)
    KernelPlan plan;   // the kernels that render the uploaded scene (bind_kernels)
    // k_extend splits the path integrator's queue of one-class scenes (shaded / terminal / dropped: KernelChoice::split_queue), which
    // pays where many paths are dropped (an open scene: C4 shades in 84 instead of 117 ms per frame) and costs where none are (a
    // closed box: the gathered records cost C2 4 %).  Decided once per uploaded scene, from the counts of the first pass rendered
    // with the path integrator: 0 = not yet, 1 = split, 2 = do not.  The image does not depend on it.
    int split_decision = 0;
    // The counts travel to the host through a pinned buffer behind an event that later passes poll (hipEventQuery): no call of the
    // render path waits for them, so pbrs_render_tile_device stays asynchronous (also on a caller's stream, pbrs_set_stream).
    unsigned long long* split_host = nullptr;  // pinned: (paths kept, paths in all) of the probed pass
    hipEvent_t split_ev = nullptr;
    bool split_probe_in_flight = false;
    bool has_vis_records = false;  // every material names its pbrs_material::vis_bxdf record (normal_visualizer)
    // pbrs_bsdf_eval: what prepare_scene found out about the scene's lobes (SceneFacts::lambert, ::fourier), and each material's flags
    bool lambert_scene = false, fourier_scene = false;
    std::vector<uint32_t> material_flags;
    uint64_t pending_closest = 0;
    pbrs_intersect_info last_intersect{};  // which walks the last pbrs_intersect_rays went through
    DeviceBuffer buf[N_BUFFERS];  // the features' first-use buffers (BufferId)
};

namespace {

#define HIPCHK(ctx, expr)                                                                             \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            (ctx)->error = std::string(#expr) + ": " + hipGetErrorString(e_);                         \
            (void)hipGetLastError(); /* reported: must not resurface in a later call's hipGetLastError() */ \
            return PBRS_E_DEVICE;                                                                     \
        }                                                                                             \
    } while (0)

// The device memory an entry point allocates for one call (the developer entry points: memory held between calls would change the
// free memory that pass_size reads): freed when the call returns, whichever way it does.
struct CallAllocs {
    std::vector<void*> held;
    CallAllocs() = default;
    CallAllocs(const CallAllocs&) = delete;
    CallAllocs& operator=(const CallAllocs&) = delete;
    ~CallAllocs() {
        for (void* p : held) (void)hipFree(p);
    }
    template <class T>
    hipError_t alloc(T** p, size_t bytes) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes);
        if (e == hipSuccess) held.push_back(q);
        *p = static_cast<T*>(q);
        return e;
    }
};

int fail(pbrs_ctx* c, int code, const char* msg) {
    c->error = msg;
    return code;
}
// The verdict of a check of host/arg_checks.h as an entry point returns it.
int fail(pbrs_ctx* c, const Refusal& r) { return r.code ? fail(c, r.code, r.message) : PBRS_OK; }

// How every image operation begins: no context, the refusal of its check (which has touched neither context nor device), and only
// then the context's device.
int enter(pbrs_ctx* c, const Refusal& r) {
    if (!c) return PBRS_E_INVALID;
    if (r.code) return fail(c, r);
    HIPCHK(c, hipSetDevice(c->device));
    return PBRS_OK;
}

template <class T>
int upload(pbrs_ctx* c, const T* src, size_t n, const T** dst) {
    *dst = nullptr;
    size_t bytes = (n ? n : 1) * sizeof(T);
    void* p = nullptr;
    HIPCHK(c, hipMalloc(&p, bytes));
    c->scene_allocs.push_back(p);
    if (n) HIPCHK(c, hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    *dst = static_cast<const T*>(p);
    return PBRS_OK;
}

// The wide nodes and, right behind them in one allocation, the tri_leaf table (DevScene::n_wnodes)
int upload_wide(pbrs_ctx* c, const PreparedScene& P, const pbrs_wnode** dst) {
    *dst = nullptr;
    const size_t wide_bytes = P.wide.size() * sizeof(pbrs_wnode), table_bytes = P.tri_leaf.size() * sizeof(uint32_t);
    void* p = nullptr;
    HIPCHK(c, hipMalloc(&p, wide_bytes + table_bytes));
    c->scene_allocs.push_back(p);
    HIPCHK(c, hipMemcpy(p, P.wide.data(), wide_bytes, hipMemcpyHostToDevice));
    if (table_bytes) HIPCHK(c, hipMemcpy(static_cast<char*>(p) + wide_bytes, P.tri_leaf.data(), table_bytes, hipMemcpyHostToDevice));
    *dst = static_cast<const pbrs_wnode*>(p);
    return PBRS_OK;
}

void free_scene(pbrs_ctx* c) {
    for (void* p : c->scene_allocs) (void)hipFree(p);
    c->scene_allocs.clear();
    c->has_scene = false;
}

// The per-pass working memory in use (pbrs_ctx::pass_set).
pbrs_ctx::PassSet& cur(pbrs_ctx* c) { return c->pass_set[c->cur_set]; }

// Set k becomes the one in use; its stream, the main one, becomes the context's.
void use_pass_set(pbrs_ctx* c, int k) {
    c->cur_set = k;
    c->stream = c->main_stream;
}

void free_paths(pbrs_ctx::PassSet& set) {
    // capacities first: whatever happens below, no later call may take the old pointers for valid
    set.cap_slots = 0;
    set.st = PathState{};
    set.neeq = nullptr;
    set.rng_hi0 = nullptr;
    set.slow = nullptr;
    if (set.state_mem) (void)hipFree(set.state_mem);
    set.state_mem = nullptr;
}

void free_work(pbrs_ctx* c) {
    for (pbrs_ctx::PassSet& set : c->pass_set) free_paths(set);
    c->cap_pixels = 0;
    if (c->sum) (void)hipFree(c->sum);
    if (c->rgb_dev) (void)hipFree(c->rgb_dev);
    c->sum = nullptr;
    c->rgb_dev = nullptr;
}

// Column `col` of a layout (host/pass_plan.h) in the allocation `mem`.
template <class T>
T* column(void* mem, const PathLayout& lay, uint32_t col) {
    return reinterpret_cast<T*>(static_cast<char*>(mem) + lay.offset[col]);
}
// The types ensure_work reads the columns as have the element sizes the table states: a kernel that indexes a column stays in its region.
constexpr bool columns_hold(uint32_t first, uint32_t n, size_t elem) {
    for (uint32_t i = first; i < first + n; ++i)
        if (kPathColumns[i].elem != elem) return false;
    return true;
}
static_assert(columns_hold(COL_Q, 14, sizeof(float4)) && columns_hold(COL_OCC, 1, sizeof(uint8_t)) && columns_hold(COL_NEEQ, 2, sizeof(uint32_t)) &&
                  columns_hold(COL_CLS, 1, sizeof(uint8_t)) && columns_hold(COL_SLOW, 2, sizeof(uint32_t)) && columns_hold(COL_CLASS_RANGE, 1, sizeof(uint2)) &&
                  columns_hold(COL_RNG_HI0, 1, sizeof(uint32_t)),
              "kPathColumns and PathState disagree about a column's element");

// The path state of `set` for n_slots paths, and the context's per-pixel sums for n_pixels.
// The per-path arrays of PathState lie in one allocation, where path_layout (host/pass_plan.h) puts them.  The new
// capacities are published only after every allocation has succeeded: a failure leaves the context without a working
// set (cap_* = 0, PathState cleared), never with pointers into freed memory.
int ensure_work(pbrs_ctx* c, pbrs_ctx::PassSet& set, size_t n_slots, size_t n_pixels) {
    if (n_slots > set.cap_slots) {
        free_paths(set);
        const PathLayout lay = path_layout(n_slots);
        void* mem = nullptr;
        hipError_t e = hipMalloc(&mem, lay.total);
        if (e != hipSuccess) {
            c->error = std::string("hipMalloc of the path state (") + std::to_string(lay.total >> 20) + " MiB): " + hipGetErrorString(e);
            (void)hipGetLastError();  // reported: must not resurface in a later call's hipGetLastError()
            return PBRS_E_DEVICE;
        }
        set.state_mem = mem;
        PathState s{};
        for (uint32_t half = 0; half < 2; ++half)
            for (uint32_t k = 0; k < 3; ++k) s.q[half][k] = column<float4>(mem, lay, COL_Q + 3 * half + k);
        s.hit = column<float4>(mem, lay, COL_HIT);
        s.L = column<float4>(mem, lay, COL_L);
        for (uint32_t k = 0; k < 3; ++k) s.nee[k] = column<float4>(mem, lay, COL_NEE + k);
        for (uint32_t k = 0; k < 3; ++k) s.sr[k] = column<float4>(mem, lay, COL_SR + k);
        s.occ[0] = column<uint8_t>(mem, lay, COL_OCC);
        s.occ[1] = s.occ[0] + n_slots;
        set.neeq = column<uint32_t>(mem, lay, COL_NEEQ);
        s.perm = column<uint32_t>(mem, lay, COL_PERM);
        s.cls = column<uint8_t>(mem, lay, COL_CLS);
        set.slow = column<uint32_t>(mem, lay, COL_SLOW);
        s.tile_hist = column<uint32_t>(mem, lay, COL_TILE_HIST);
        s.class_range = column<uint2>(mem, lay, COL_CLASS_RANGE);
        set.rng_hi0 = column<uint32_t>(mem, lay, COL_RNG_HI0);
        set.st = s;
        set.cap_slots = n_slots;
    }
    if (n_pixels > c->cap_pixels) {
        c->cap_pixels = 0;
        if (c->sum) (void)hipFree(c->sum);
        if (c->rgb_dev) (void)hipFree(c->rgb_dev);
        c->sum = nullptr;
        c->rgb_dev = nullptr;
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->sum), 3 * n_pixels * sizeof(float)));
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->rgb_dev), 3 * n_pixels * sizeof(float)));
        c->cap_pixels = n_pixels;
    }
    return PBRS_OK;
}

int DeviceBuffer::grow(pbrs_ctx* c, size_t bytes, const char* what) {
    if (bytes <= cap_bytes) return PBRS_OK;
    cap_bytes = 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        p = nullptr;
        c->error = std::string("hipMalloc of ") + what + " (" + std::to_string(bytes >> 20) + " MiB): " + hipGetErrorString(e);
        (void)hipGetLastError();  // reported: must not resurface in a later call's hipGetLastError()
        return PBRS_E_DEVICE;
    }
    cap_bytes = bytes;
    return PBRS_OK;
}

// The D column of pass set k (PassSet::direct) for n_slots paths, or none: a render without light passes leaves the column null and
// allocates nothing.
int ensure_direct(pbrs_ctx* c, int k, size_t n_slots, bool wanted) {
    c->pass_set[k].direct = nullptr;
    if (!wanted) return PBRS_OK;
    DeviceBuffer& b = c->buf[BUF_PASS_DIRECT + k];
    const int rc = b.grow(c, n_slots * sizeof(float4), "the light passes' path column");
    if (rc) return rc;
    c->pass_set[k].direct = b.as<float4>();
    return PBRS_OK;
}

// One plane of a host variant's device staging: the host memory copied up into it before the launches (`up`; null: not given), its
// words per pixel, the host memory it is copied back to after them (`down`; null: not wanted), and where `stage` put it on the device
// (null where neither is given).  A result that lands in an input's place is one row with both.  A row of another size than the
// call's P pixels says so in `pixels` (pbrs_upsample's low-resolution planes); 0 is P.
struct Staged {
    const void* up;
    size_t words;
    void* down = nullptr;
    void* dev = nullptr;
    size_t pixels = 0;
    size_t count(size_t P) const { return words * (pixels ? pixels : P); }
    template <class T>
    T* as() const { return static_cast<T*>(dev); }
};

// Lays the planes of `s` out in `buf`, one after the other in the order of `s`, for P pixels.  `buf` is grown to hold all of them, given
// or not: neither its size nor where a plane sits depends on which ones a call asks for.  The allocation, the device pointers and
// (copy_staged) the copies all follow from the words per pixel in `s`.
template <size_t N>
int stage(pbrs_ctx* c, BufferId id, const char* what, Staged (&s)[N], size_t P) {
    size_t words = 0;
    for (const Staged& r : s) words += r.count(P);
    DeviceBuffer& buf = c->buf[id];
    int rc = buf.grow(c, words * sizeof(uint32_t), what);
    if (rc) return rc;
    uint32_t* at = buf.as<uint32_t>();
    for (Staged& r : s) {
        r.dev = (r.up || r.down) ? at : nullptr;
        at += r.count(P);
    }
    return PBRS_OK;
}

// The planes of `s` that have an `up` to the device (hipMemcpyHostToDevice), or those that have a `down` back to the host, in the order of
// `s` on the context's stream.
template <size_t N>
int copy_staged(pbrs_ctx* c, const Staged (&s)[N], size_t P, hipMemcpyKind kind) {
    for (const Staged& r : s) {
        const bool up = kind == hipMemcpyHostToDevice;
        if (!(up ? r.up != nullptr : r.down != nullptr)) continue;
        HIPCHK(c, hipMemcpyAsync(up ? r.dev : r.down, up ? r.up : r.dev, r.count(P) * sizeof(uint32_t), kind, c->stream));
    }
    return PBRS_OK;
}

// A host variant of an image operation, whole: lay `s` out in the operation's staging buffer, copy the given inputs up, queue the
// operation's launches on the staged planes (`launch`, which reads the device pointers from `s`), copy the wanted outputs back, and wait.
template <size_t N, class Launch>
int run_staged(pbrs_ctx* c, BufferId id, const char* what, Staged (&s)[N], size_t P, Launch launch) {
    int rc = stage(c, id, what, s, P);
    if (!rc) rc = copy_staged(c, s, P, hipMemcpyHostToDevice);
    if (!rc) rc = launch();
    if (!rc) rc = copy_staged(c, s, P, hipMemcpyDeviceToHost);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PBRS_OK;
}

constexpr size_t kDenoiseBytesPerPixel = 3 * sizeof(float4) + sizeof(uint32_t);

// What a render produces beside its statistics, as render_common and run_pass see it: device pointers.  Each feature's state lives in
// the context (pbrs_ctx::buf), allocated by `render` before the pass size is computed.
struct RenderTargets {
    float* rgb = nullptr;      // the image: w x h of the params; a filtered render: the tile's filt->w x filt->h pixels
    pbrs_aov_buffers aovs{};   // the first-hit AOVs wanted (all null: none), from the state in BUF_AOV_STATE
    float* variance = nullptr; // the variance AOV (null: none), from the moments in BUF_MOMENT_STATE
    // the id matte (want_matte; arguments checked by check_targets), from the tables in BUF_MATTE_STATE
    bool want_matte = false;
    const pbrs_matte_params* matte = nullptr;
    pbrs_matte_buffers matte_out{};
    pbrs_pass_buffers passes{};  // the light passes wanted (all null: none), from the state in BUF_PASS_STATE
    // a filtered render: the params are then its traced region (filter_setup) and the pass is folded into BUF_FILTER_SUM
    const FilterConst* filt = nullptr;

    bool want_aovs() const {
        const pbrs_aov_buffers& a = aovs;
        return a.albedo || a.normal || a.coverage || a.depth || a.instance || a.material || a.prim;
    }
    bool want_passes() const { return passes.direct || passes.indirect || passes.direct_variance || passes.indirect_variance; }
    // as check_targets reads them (host/arg_checks.h)
    WantedOutputs wanted() const { return {want_aovs(), variance != nullptr, want_passes(), want_matte, matte, matte_out.ids && matte_out.coverage}; }
};

// What check_params (host/arg_checks.h) needs to know of the context.
SceneState scene_state(const pbrs_ctx* c) { return {c->has_scene, c->has_vis_records}; }

// The samples per pass of a render of `p` (checked by check_params), from the memory that is free on the current device NOW: whatever the
// call allocates beside the path state comes first.  `with_direct`: every path carries a record of the D column as well (light passes).
int pass_size(pbrs_ctx* c, const pbrs_render_params* p, uint32_t& K, bool with_direct = false) {
    std::optional<uint64_t> free_bytes;  // (a requested size asks nothing)
    size_t free_b = 0, total_b = 0;
    if (p->samples_per_pass == 0 && hipMemGetInfo(&free_b, &total_b) == hipSuccess) free_bytes = free_b;
    K = samples_per_pass((uint64_t)p->w * p->h, (uint64_t)p->strata_x * p->strata_y, p->samples_per_pass, with_direct,
                         (uint64_t)c->pass_set[0].cap_slots + c->pass_set[1].cap_slots,
                         (uint64_t)c->buf[BUF_PASS_DIRECT].cap_bytes + c->buf[BUF_PASS_DIRECT_SET1].cap_bytes, free_bytes);
    // records keep two flag bits next to the slot index, and 16-byte records are addressed with 32-bit element indices
    if ((uint64_t)p->w * p->h * K >= (1ull << 28)) return fail(c, PBRS_E_LIMIT, "tile x samples_per_pass above 2^28 paths");
    return PBRS_OK;
}

struct Timer {
    pbrs_ctx* c;
    bool on;
    int begin(int stage) {
        if (!on) return 0;
        if (c->events_used == c->events.size()) {
            StageEvent e{};
            if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return -1;
            c->events.push_back(e);
        }
        StageEvent& e = c->events[c->events_used];
        e.stage = stage;
        return hipEventRecord(e.a, c->stream) == hipSuccess ? 0 : -1;
    }
    int end() {
        if (!on) return 0;
        StageEvent& e = c->events[c->events_used++];
        return hipEventRecord(e.b, c->stream) == hipSuccess ? 0 : -1;
    }
};

RenderConst make_const(const pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p) {
    RenderConst rc{};
    rc.cam = *cam;
    rc.x0 = p->x0; rc.y0 = p->y0; rc.w = p->w; rc.h = p->h;
    rc.strata_x = p->strata_x; rc.strata_y = p->strata_y;
    rc.max_depth = p->max_depth;
    rc.n_pixels = p->w * p->h;
    rc.band_rows = p->band_rows; rc.band_count = p->band_count; rc.band_index = p->band_index;
    rc.seed = p->seed;
    rc.integrator = p->integrator;
    // slot order of a pass (kernels.h, sample_of_slot): chunks of 4 K pixels, a multiple of the block and of the wave (C4:
    // 1156 Msamples/s with the sample index outermost, 1208-1211 with chunks of 256 ... 16 K pixels, 1202 with 64 K)
    rc.chunk_pixels = c->dev.raygen_chunk.value_or(4096u);
    if (rc.chunk_pixels > rc.n_pixels) rc.chunk_pixels = rc.n_pixels;  // one chunk: slot = k * P + pixel
    rc.tiles8_per_row = (c->dev.raygen_tiles8 && p->w % 8u == 0u && p->h % 8u == 0u) ? p->w / 8u : 0u;
    return rc;
}

// The kernels a choice names (choose_kernels), from their owners' tables (kernel_tables.h).  False where a table lacks one.
bool bind_kernels(const KernelChoice& ch, KernelPlan& p) {
    p = KernelPlan{};
    p.choice = ch;
    for (int s = 0; s < 2; ++s) {
        p.extend[s] = extend_fns()[ch.extend[s].key];
        p.shadow[s] = shadow_fns()[ch.shadow[s].key];
    }
    if (ch.wide_shadow) p.shadow_slow = shadow_fns()[ch.shadow_slow.key];
    if (ch.entry_extend) p.extend_entry = reinterpret_cast<extend_entry_fn_t>(extend_fns()[entry_key(ch.extend[0].key)]);
    bool ok = p.extend[0] && p.extend[1] && p.shadow[0] && p.shadow[1] && (!ch.wide_shadow || p.shadow_slow) && (!ch.entry_extend || p.extend_entry);
    for (uint32_t i = 0; i <= PBRS_INTEGRATOR_NORMALS; ++i) {
        IntegratorPlan& ip = p.integ[i];
        ip.choice = ch.integ[i];
        for (uint32_t k = 0; k < ip.choice.n_shade; ++k) {
            ip.shade[k] = shade_fn(ip.choice.shade[k]);
            ok = ok && ip.shade[k];
        }
    }
    return ok;
}

// The split probe of an earlier pass (run_pass), if its counts have arrived: keep the queue split where it keeps at most
// PBRS_SPLIT_KEEP_PERCENT of a pass's rays for k_shade.  Never waits.
void poll_split_probe(pbrs_ctx* c) {
    if (!c->split_probe_in_flight || hipEventQuery(c->split_ev) != hipSuccess) {
        (void)hipGetLastError();  // hipErrorNotReady is not an error of this call
        return;
    }
    c->split_probe_in_flight = false;
    c->split_decision = (c->split_host[0] * 100ull <= c->split_host[1] * PBRS_SPLIT_KEEP_PERCENT) ? 1 : 2;
}

// The matte kernels by `slots` (device/matte.h): the table is a register array, so its size is a template argument.
struct MatteKernels {
    void (*fold)(const pbrs_instance*, PathState, uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t);
    void (*finalize)(const uint32_t*, uint32_t, uint32_t, uint32_t, float, uint32_t*, float*, float*);
};
#define PBRS_MATTE_KERNELS(N) {k_matte<N>, k_matte_finalize<N>}
constexpr MatteKernels kMatte[PBRS_MATTE_MAX_SLOTS] = {PBRS_MATTE_KERNELS(1), PBRS_MATTE_KERNELS(2), PBRS_MATTE_KERNELS(3), PBRS_MATTE_KERNELS(4),
                                                       PBRS_MATTE_KERNELS(5), PBRS_MATTE_KERNELS(6), PBRS_MATTE_KERNELS(7), PBRS_MATTE_KERNELS(8)};
#undef PBRS_MATTE_KERNELS

// One pass: kc sample indices starting at `first` for every pixel of the tile.
// `handoff`: the pass moves to the late stream at bounce pbrs_ctx::overlap_from (at the latest for its k_accumulate: the late stream runs
// the passes' accumulations in pass order, src/main.rs:205) and leaves the main stream to the next pass, which works in the other pass set.
// `t`: what the render produces.  The pass folds its first hits into the AOV state (k_aov) and the matte tables (k_matte), its
// radiances into the moments of the variance AOV (k_moments) and, split at the first path vertex (k_pass_direct), into the state of the
// light passes (k_pass_fold), each where asked for; a filtered render (rc is its traced region) folds
// the pass into the filter sums (k_filter_accumulate) instead of k_accumulate.
// Every launch, memset, event and stream call of a pass is here, in order; what they are given beside pointers — the grids, the counter
// regions, and per bounce the split flags, the queue order and the class ranges — is decided in host/pass_plan.h.
int run_pass(pbrs_ctx* c, RenderConst rc, uint32_t first, uint32_t kc, bool stats, Timer& tm, bool handoff, const RenderTargets& t) {
    pbrs_ctx::PassSet& set = cur(c);
    // the set's memory is free once the pass that used it last has accumulated (two passes back, on the late stream)
    if (handoff && set.in_flight) HIPCHK(c, hipStreamWaitEvent(c->stream, set.accumulated, 0));
    auto to_late_stream = [&]() -> hipError_t {
        hipError_t e = hipEventRecord(set.late, c->stream);
        c->stream = c->second_stream;
        return e != hipSuccess ? e : hipStreamWaitEvent(c->stream, set.late, 0);
    };
    const uint32_t P = rc.n_pixels;
    const PassShape shape = pass_shape(P, kc);
    const uint32_t N = shape.n_slots, grid = shape.grid, pgrid = shape.pgrid, n_tiles = shape.n_tiles;
    rc.pass_first_sample = first;
    rc.n_slots = N;
    // the regions of the set's counter block (host/pass_plan.h, CounterLayout)
    uint32_t* act = set.counters + kCounters.act;
    unsigned long long* ns = reinterpret_cast<unsigned long long*>(set.counters + kCounters.ns);
    uint32_t* slows = set.counters + kCounters.slows;
    uint32_t* xhead = set.counters + kCounters.xhead;
    uint32_t* shead = set.counters + kCounters.shead;
    uint32_t* shead2 = set.counters + kCounters.shead2;
    uint32_t* neeq = set.neeq;
    const KernelPlan& plan = c->plan;
    const KernelChoice& choice = plan.choice;
    const IntegratorPlan& ip = plan.integ[rc.integrator];
    const TraversalKey &xk = choice.extend[stats], &sk = choice.shadow[stats];
    // k_extend scans the TLAS leaves only up to PBRS_FLAT_TLAS_MAX instances (S.features); the leaf copies may exist for k_shadow
    // alone, and the instrumented variant, which carries every feature, must then walk the tree like the timed one
    DevScene xS = c->S;
    if (!(xS.features & PBRS_FEAT_FLAT_TLAS)) xS.n_flat = 0u;
    HIPCHK(c, hipMemsetAsync(set.counters, 0, kCounters.words * sizeof(uint32_t), c->stream));
    if (tm.begin(0)) return fail(c, PBRS_E_DEVICE, "event record failed");
    hipLaunchKernelGGL(k_raygen, dim3(grid), dim3(kBlock), 0, c->stream, set.st, rc, set.rng_hi0);
    tm.end();
    poll_split_probe(c);
    const uint32_t n_bounces = bounce_count(rc.integrator, rc.max_depth);
    // L is first written by bounce 0 (k_shade, and k_class_scatter for what a split queue drops): a pass without a bounce is all zeros
    if (n_bounces == 0) HIPCHK(c, hipMemsetAsync(set.st.L, 0, (size_t)N * sizeof(float4), c->stream));
    // this pass counts what k_extend's queue split keeps (the first path-integrator pass of an uploaded one-class scene)
    const bool probe_split = c->split_decision == 0 && !c->split_probe_in_flight && rc.integrator == PBRS_INTEGRATOR_PATH && choice.split_queue && n_bounces > 0;
    for (uint32_t b = 0; b < n_bounces; ++b) {
        if (handoff && b == c->overlap_from) HIPCHK(c, to_late_stream());
        // bounce b reads the path records of set b & 1 (k_raygen wrote set 0) and k_shade writes set (b + 1) & 1; the
        // queue length of bounce 0 is the pass size, later ones are counted on the device
        const uint32_t* cnt_in = b == 0 ? nullptr : act + b;
        const BouncePlan bp = bounce_plan(rc.integrator, choice.split_queue, ip.choice, c->split_decision, b);
        const uint32_t qsplit = bp.split;
        if (tm.begin(1)) return fail(c, PBRS_E_DEVICE, "event record failed");
        // bounce 0 of a render with an entry table (render_common): camera rays enter the table instance's BLAS at their pixel's entry nodes
        if (b == 0 && c->entry_table && !stats)
            hipLaunchKernelGGL(plan.extend_entry, dim3(pgrid), dim3(kBlock), xk.lds, c->stream, xS, set.st, b & 1u, cnt_in, N, xhead + b * kHeadWords, c->gcnt, nullptr,
                               nullptr, nullptr, qsplit, EntryArgs{c->entry_table, P, kc, rc.chunk_pixels});
        else
            hipLaunchKernelGGL(plan.extend[stats], dim3(pgrid), dim3(kBlock), xk.lds, c->stream, xS, set.st, b & 1u, cnt_in, N, xhead + b * kHeadWords, c->gcnt, nullptr,
                               nullptr, nullptr, qsplit);
        c->pending.kernel_features_extend = reported_features(xk);
        tm.end();
        // First-hit AOVs: bounce 0's rays (q[0], at their slots) and hit records, before bounce 1 overwrites them (k_shade writes set 0
        // at bounce 1, k_extend the hit records).  Outside the stage brackets: counted in ms_total only.  The state is shared by the
        // passes, so their k_aov launches must run in pass order on one stream: bounce 0 runs on the main stream for every pass unless
        // overlap_from is 0 (a developer override), and then on the late stream for every pass — one stream either way, in pass order
        // (render_common joins the late stream before k_aov_finalize).
        if (b == 0 && t.want_aovs())
            hipLaunchKernelGGL(k_aov, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, c->S, set.st, c->buf[BUF_AOV_STATE].as<float>(), P, kc,
                               rc.chunk_pixels, qsplit);
        // id mattes: the same hit records, the same place and stream for the same reasons
        if (b == 0 && t.want_matte)
            hipLaunchKernelGGL(kMatte[t.matte->slots - 1u].fold, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, c->S.inst, set.st,
                               c->buf[BUF_MATTE_STATE].as<uint32_t>(), P, kc, rc.chunk_pixels, qsplit, t.matte->key);
        if (tm.begin(2)) return fail(c, PBRS_E_DEVICE, "event record failed");
        if (bp.order == IntegratorChoice::CLASS_MAJOR) {
            const bool two = bp.n_classes == 2u;  // the instantiation: a split queue's two classes, or all of them
            if (two) hipLaunchKernelGGL(k_class_count<2u>, dim3(n_tiles), dim3(kBlock), 0, c->stream, set.st, cnt_in, N);
            else hipLaunchKernelGGL(k_class_count<PBRS_MAX_CLASSES>, dim3(n_tiles), dim3(kBlock), 0, c->stream, set.st, cnt_in, N);
            hipLaunchKernelGGL(k_class_scan, dim3(1), dim3(64 * PBRS_MAX_CLASSES), 0, c->stream, set.st, cnt_in, N, bp.last,
                               (qsplit && probe_split) ? c->bounce_acc + 2 * PBRS_STATS_MAX_BOUNCES : nullptr);
            if (two) hipLaunchKernelGGL(k_class_scatter<2u>, dim3(n_tiles), dim3(kBlock), 0, c->stream, set.st, cnt_in, N, bp.zero_dropped);
            else hipLaunchKernelGGL(k_class_scatter<PBRS_MAX_CLASSES>, dim3(n_tiles), dim3(kBlock), 0, c->stream, set.st, cnt_in, N, bp.zero_dropped);
        } else if (bp.order == IntegratorChoice::CLASS_SORT) {
            hipLaunchKernelGGL(k_class_sort, dim3(n_tiles), dim3(kBlock), 0, c->stream, set.st, cnt_in, N);
        }
        for (uint32_t k = 0; k < ip.choice.n_shade; ++k) {
            const uint2* range = bp.shade_range[k] ? set.st.class_range + bp.shade_range[k] : nullptr;
            hipLaunchKernelGGL(ip.shade[k], dim3(grid), dim3(kBlock), ip.choice.shade[k].lds, c->stream, c->S, set.st, rc, b, cnt_in, N, act + b + 1, neeq, ns + b,
                               bp.sorted, range, set.rng_hi0);
        }
        tm.end();
        if (tm.begin(3)) return fail(c, PBRS_E_DEVICE, "event record failed");
        hipLaunchKernelGGL(plan.shadow[stats], dim3(pgrid), dim3(kBlock), sk.lds, c->stream, c->S, set.st, reinterpret_cast<const uint32_t*>(ns + b),
                           shead + b * kHeadWords, c->gcnt + 1, nullptr, set.slow, slows + b);
        c->pending.kernel_features_shadow = reported_features(sk);
        if (choice.wide_shadow && !stats)  // what the wide walks refused (rays outside the guarded range of the division-free box test, overlong stacks)
            hipLaunchKernelGGL(plan.shadow_slow, dim3(shape.slow_grid), dim3(kBlock), choice.shadow_slow.lds, c->stream, c->S, set.st, slows + b, shead2 + b * kHeadWords,
                               c->gcnt + 1, set.slow, nullptr, nullptr);
        hipLaunchKernelGGL(k_nee_resolve, dim3(shape.sgrid), dim3(kBlock), 0, c->stream, set.st, neeq, reinterpret_cast<const uint32_t*>(ns + b));
        tm.end();
        // light passes: L is now the radiance after the first path vertex; kept in the set's D column before bounce 1 adds to L.  On the
        // stream that ran bounce 0; k_pass_fold reads the column behind the pass's last bounce (the hand-over events order the two).
        // Outside the stage brackets: counted in ms_total only.
        if (b == 0 && t.want_passes()) hipLaunchKernelGGL(k_pass_direct, dim3(grid), dim3(kBlock), 0, c->stream, set.st.L, set.direct, N);
    }
    if (probe_split) {
        // the first pass of this scene through the path integrator: how much of its queues did the split keep for k_shade?  The
        // counts are copied out behind an event; a later pass that finds the event complete takes the decision (poll_split_probe).
        // No synchronisation; the image does not depend on the answer.
        unsigned long long* acc = c->bounce_acc + 2 * PBRS_STATS_MAX_BOUNCES;
        HIPCHK(c, hipMemcpyAsync(c->split_host, acc, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipEventRecord(c->split_ev, c->stream));
        HIPCHK(c, hipMemsetAsync(acc, 0, 2 * sizeof(unsigned long long), c->stream));
        c->split_probe_in_flight = true;
    }
    if (stats)  // queue sizes of this pass, bounce by bounce (the counters are cleared at the start of every pass)
        hipLaunchKernelGGL(k_sum_bounce_counts, dim3(1), dim3(64), 0, c->stream, act, ns, N, n_bounces, c->bounce_acc);
    if (handoff && c->stream != c->second_stream) HIPCHK(c, to_late_stream());
    if (tm.begin(4)) return fail(c, PBRS_E_DEVICE, "event record failed");
    if (const FilterConst* filt = t.filt)
        hipLaunchKernelGGL(k_filter_accumulate, dim3((filt->w + PBRS_FILTER_CELL - 1) / PBRS_FILTER_CELL, (filt->h + PBRS_FILTER_CELL - 1) / PBRS_FILTER_CELL),
                           dim3(kBlock), filter_lds_bytes(filt->hx, filt->hy), c->stream, set.st, c->buf[BUF_FILTER_SUM].as<float>(), rc, *filt, kc, c->nonfinite);
    else
        hipLaunchKernelGGL(k_accumulate, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, set.st, c->sum, P, kc, rc.chunk_pixels, rc.w, rc.tiles8_per_row, c->nonfinite);
    // the variance AOV: the same radiances, on the stream that runs the passes' accumulations in pass order
    if (t.variance)
        hipLaunchKernelGGL(k_moments, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, set.st, c->buf[BUF_MOMENT_STATE].as<float>(), P, kc, rc.chunk_pixels);
    // the light passes: L and the D column of the same samples, on the same stream for the same reason
    if (t.want_passes())
        hipLaunchKernelGGL(k_pass_fold, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, set.st.L, set.direct,
                           c->buf[BUF_PASS_STATE].as<float>(), P, kc, rc.chunk_pixels);
    tm.end();
    if (handoff) {
        HIPCHK(c, hipEventRecord(set.accumulated, c->stream));
        set.in_flight = true;
    }
    HIPCHK(c, hipGetLastError());
    return PBRS_OK;
}

// Queues a render of `p` (checked; K its samples per pass, the working set and the targets' state there) into `t` on the context's stream.
int render_common(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, uint32_t K, const RenderTargets& t) {
    const uint32_t P = p->w * p->h;
    const uint32_t spp = p->strata_x * p->strata_y;
    const FilterConst* filt = t.filt;
    float* aov = t.want_aovs() ? c->buf[BUF_AOV_STATE].as<float>() : nullptr;
    float* moments = t.variance ? c->buf[BUF_MOMENT_STATE].as<float>() : nullptr;
    uint32_t* matte = t.want_matte ? c->buf[BUF_MATTE_STATE].as<uint32_t>() : nullptr;
    float* pass_state = t.want_passes() ? c->buf[BUF_PASS_STATE].as<float>() : nullptr;
    float* filter_sum = c->buf[BUF_FILTER_SUM].as<float>();
    RenderConst rc = make_const(c, cam, p);
    const bool stats = p->collect_counters != 0;
    Timer tm{c, p->time_stages != 0};
    c->events_used = 0;
    c->pending = pbrs_stats{};
    c->pending_counters = stats;
    c->pending_times = p->time_stages != 0;
    c->pending.samples = (uint64_t)P * spp;
    if (stats) HIPCHK(c, hipMemsetAsync(c->gcnt, 0, 2 * sizeof(GlobalCounters), c->stream));
    if (stats) HIPCHK(c, hipMemsetAsync(c->bounce_acc, 0, 2 * PBRS_STATS_MAX_BOUNCES * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(c->nonfinite, 0, sizeof(unsigned long long), c->stream));
    if (c->pending_times) HIPCHK(c, hipEventRecord(c->total_ev[0], c->stream));
    if (filt) HIPCHK(c, hipMemsetAsync(filter_sum, 0, 4 * (size_t)filt->w * filt->h * sizeof(float), c->stream));
    else HIPCHK(c, hipMemsetAsync(c->sum, 0, 3 * (size_t)P * sizeof(float), c->stream));
    if (aov) HIPCHK(c, hipMemsetAsync(aov, 0, PBRS_AOV_STATE_WORDS * (size_t)P * sizeof(float), c->stream));
    if (moments) HIPCHK(c, hipMemsetAsync(moments, 0, PBRS_MOMENT_STATE_WORDS * (size_t)P * sizeof(float), c->stream));
    if (matte) HIPCHK(c, hipMemsetAsync(matte, 0, PBRS_MATTE_STATE_WORDS(t.matte->slots) * (size_t)P * sizeof(uint32_t), c->stream));
    if (pass_state) HIPCHK(c, hipMemsetAsync(pass_state, 0, PBRS_PASS_STATE_WORDS * (size_t)P * sizeof(float), c->stream));
    // Entry nodes of the camera rays (device/entry_nodes.h): one record per pixel of the traced region, written once, read by every
    // pass's bounce 0.  The instrumented render walks from the root (its node counts are the oracle's).  Without memory for the table the
    // render goes on without it.
    c->entry_table = nullptr;
    c->last_entry = false;
    if (c->entry_nodes && c->plan.extend_entry && !stats && bounce_count(rc.integrator, rc.max_depth) > 0) {
        DeviceBuffer& eb = c->buf[BUF_ENTRY_TABLE];
        const size_t table_bytes = (size_t)P * sizeof(pbrs_entry_record);
        if (eb.grow(c, table_bytes + 4 * sizeof(uint32_t), "the entry-node table") == PBRS_OK) {
            uint32_t* info = reinterpret_cast<uint32_t*>(static_cast<char*>(eb.p) + table_bytes);
            HIPCHK(c, hipMemsetAsync(info, 0, 4 * sizeof(uint32_t), c->stream));
            hipLaunchKernelGGL(k_entry_nodes, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, c->S, rc, c->entry_height, c->entry_rows, eb.as<uint4>(), info);
            c->entry_table = eb.as<uint4>();
            c->last_entry = true;
            c->last_entry_pixels = P;
        } else {
            c->error.clear();
        }
    }
    uint32_t passes = 0;
    // Where the render has more than one pass, passes alternate between the two pass sets and hand their late bounces to the second
    // stream: those are near-empty launches that end with the latency of their longest walks (C4: 47 ms per frame in kernels that leave
    // most of the chip idle, profiles/r04k_trace_gaps_c4.log) — the next pass's first bounces, queued behind the hand-over on the main
    // stream, fill it.  The instrumented render keeps one stream (its counters are per pass).
    bool two = c->overlap_passes && !stats && spp > K;
    if (two && (ensure_work(c, c->pass_set[1], (size_t)P * K, P) || ensure_direct(c, 1, (size_t)P * K, pass_state != nullptr))) {
        two = false;  // no memory for the second set (a device shared with other processes): every pass on the main stream, as before
        c->error.clear();
    }
    for (uint32_t first = 0; first < spp; first += K) {
        uint32_t kc = spp - first < K ? spp - first : K;
        if (two) use_pass_set(c, (int)(passes & 1u));  // (also: back to the main stream)
        const int rcode = run_pass(c, rc, first, kc, stats, tm, two, t);
        if (rcode) {
            use_pass_set(c, 0);
            c->entry_table = nullptr;
            return rcode;
        }
        ++passes;
    }
    c->entry_table = nullptr;  // the table is this render's: a pass queued by anything else (pbrs_render_sample_radiance) walks from the root
    if (two) {
        const hipEvent_t last = cur(c).accumulated;
        use_pass_set(c, 0);
        HIPCHK(c, hipStreamWaitEvent(c->main_stream, last, 0));  // the late stream has run every pass's accumulation, in order
    }
    if (filt) {
        const uint32_t PT = filt->w * filt->h;
        hipLaunchKernelGGL(k_filter_finalize, dim3((PT + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, filter_sum, t.rgb, PT);
    } else {
        hipLaunchKernelGGL(k_finalize, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, c->sum, t.rgb, P, 1.0f / (float)spp);
    }
    if (aov)
        hipLaunchKernelGGL(k_aov_finalize, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, aov, c->S.inst, P, rc.w, rc.tiles8_per_row,
                           1.0f / (float)spp, t.aovs);
    if (moments)
        hipLaunchKernelGGL(k_moments_finalize, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, moments, P, rc.w, rc.tiles8_per_row, t.variance);
    if (matte)
        hipLaunchKernelGGL(kMatte[t.matte->slots - 1u].finalize, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, matte, P, rc.w,
                           rc.tiles8_per_row, 1.0f / (float)spp, t.matte_out.ids, t.matte_out.coverage, t.matte_out.residual);
    if (pass_state)
        hipLaunchKernelGGL(k_pass_finalize, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, pass_state, P, rc.w, rc.tiles8_per_row,
                           1.0f / (float)spp, t.passes);
    if (c->pending_times) HIPCHK(c, hipEventRecord(c->total_ev[1], c->stream));
    HIPCHK(c, hipGetLastError());
    c->pending.passes = passes;
    c->pending.launches_extend = c->pending.launches_shade = c->pending.launches_shadow = passes * bounce_count(rc.integrator, rc.max_depth);
    return PBRS_OK;
}

int collect(pbrs_ctx* c, pbrs_stats* out) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    pbrs_stats s = c->pending;
    {
        unsigned long long bad = 0;
        HIPCHK(c, hipMemcpy(&bad, c->nonfinite, sizeof bad, hipMemcpyDeviceToHost));
        s.invalid_samples = bad;
    }
    if (c->pending_counters) {
        GlobalCounters g[2];
        HIPCHK(c, hipMemcpy(g, c->gcnt, sizeof g, hipMemcpyDeviceToHost));
        s.closest_rays = g[0].rays;
        s.shade_events = g[0].hits;
        s.tlas_nodes = g[0].tlas_nodes; s.blas_nodes = g[0].blas_nodes; s.instances = g[0].instances;
        s.instance_hits = g[0].instance_hits; s.triangles = g[0].triangles; s.tri_shading = g[0].tri_shading;
        s.spheres = g[0].spheres; s.quads = g[0].quads; s.cuboids = g[0].cuboids; s.disks = g[0].disks;
        s.shadow_rays = g[1].rays;
        s.shadow_tlas_nodes = g[1].tlas_nodes; s.shadow_blas_nodes = g[1].blas_nodes; s.shadow_instances = g[1].instances;
        s.shadow_triangles = g[1].triangles;
        s.shadow_prims = g[1].spheres + g[1].quads + g[1].cuboids + g[1].disks;
        unsigned long long per_bounce[2 * PBRS_STATS_MAX_BOUNCES];
        HIPCHK(c, hipMemcpy(per_bounce, c->bounce_acc, sizeof per_bounce, hipMemcpyDeviceToHost));
        for (uint32_t b = 0; b < PBRS_STATS_MAX_BOUNCES; ++b) {
            s.paths_at_bounce[b] = per_bounce[b];
            s.shadow_rays_at_bounce[b] = per_bounce[PBRS_STATS_MAX_BOUNCES + b];
        }
    }
    if (c->pending_times) {
        float* acc[5] = {&s.ms_raygen, &s.ms_extend, &s.ms_shade, &s.ms_shadow, &s.ms_accumulate};
        for (size_t i = 0; i < c->events_used; ++i) {
            float ms = 0.0f;
            HIPCHK(c, hipEventElapsedTime(&ms, c->events[i].a, c->events[i].b));
            *acc[c->events[i].stage] += ms;
        }
        HIPCHK(c, hipEventElapsedTime(&s.ms_total, c->total_ev[0], c->total_ev[1]));
    }
    if (out) *out = s;
    return PBRS_OK;
}

// The traversal kernels take their per-lane stacks from dynamic LDS.  The limit a kernel may ask for is per-function state
// of the PROCESS (hipFuncSetAttribute), not of a context: it is raised once per device, to the most any scene may need
// (check_scene refuses stacks above kLdsBytesPerCU / 2), so that contexts holding scenes with different stack depths
// can render side by side — rewriting it per upload let the last upload decide for every context of the process.  Every traversal
// kernel a plan can name sits in the tables (bind_kernels).
std::mutex g_kernel_cfg_mutex;
bool g_kernel_cfg_done[64] = {};
int configure_kernels(pbrs_ctx* c) {
    std::lock_guard<std::mutex> lock(g_kernel_cfg_mutex);
    if (c->device < 64 && g_kernel_cfg_done[c->device]) return PBRS_OK;
    const int cap = (int)(kLdsBytesPerCU / 2);
    std::vector<const void*> traversal_kernels = {reinterpret_cast<const void*>(intersect_fn(false)), reinterpret_cast<const void*>(intersect_fn(true))};
    for (uint32_t k = 0; k < kExtendKeys; ++k)
        if (extend_fns()[k]) traversal_kernels.push_back(reinterpret_cast<const void*>(extend_fns()[k]));
    for (uint32_t k = 0; k < kTraversalKeys; ++k) {
        if (shadow_fns()[k]) traversal_kernels.push_back(reinterpret_cast<const void*>(shadow_fns()[k]));
    }
    for (const void* k : traversal_kernels) HIPCHK(c, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, cap));
    if (c->device < 64) g_kernel_cfg_done[c->device] = true;
    return PBRS_OK;
}

// A filtered render beyond check_params: check_filter's refusals (host/arg_checks.h), then the kernel's constants and `region`, the tile
// plus its halo clipped to the film: the params the render traces (the pass size and ensure_work see the region), checked in their turn.
int filter_setup(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, const pbrs_pixel_filter* f, FilterConst& fc, pbrs_render_params& region) {
    const int rc = fail(c, check_filter(p, f));
    if (rc) return rc;
    fc = FilterConst{};
    fc.kind = f->kind;
    fc.rx = f->radius[0], fc.ry = f->radius[1], fc.a = f->a, fc.b = f->b;
    fc.hx = pf_halo(fc.rx), fc.hy = pf_halo(fc.ry);
    fc.x0 = p->x0, fc.y0 = p->y0, fc.w = p->w, fc.h = p->h;
    region = *p;
    region.x0 = p->x0 > fc.hx ? p->x0 - fc.hx : 0u;
    region.y0 = p->y0 > fc.hy ? p->y0 - fc.hy : 0u;
    region.w = std::min(p->x0 + p->w + fc.hx, cam->width) - region.x0;
    region.h = std::min(p->y0 + p->h + fc.hy, cam->height) - region.y0;
    return fail(c, check_params(scene_state(c), cam, &region));
}

// Every render entry point, after its own argument checks.  `filter`: null, or a filtered render of the tile `p`.  `t`: what the caller
// wants, in device memory, or with `host` in host memory: the render then goes through the context's staging, is copied back and waited
// for.  A device render is only queued; it waits (collect) where the caller asks for the statistics.
int render(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, const pbrs_pixel_filter* filter, RenderTargets t, bool host, pbrs_stats* stats_out) {
    HIPCHK(c, hipSetDevice(c->device));  // first: the buffers below and the pass size, which reads the free memory, are THIS device's
    FilterConst fc;
    pbrs_render_params region;
    int rc = fail(c, check_params(scene_state(c), cam, p));
    if (rc) return rc;
    const size_t PT = (size_t)p->w * p->h;  // the tile's pixels
    if (filter) {
        if ((rc = filter_setup(c, cam, p, filter, fc, region))) return rc;
        t.filt = &fc;
        p = &region;
    }
    if ((rc = fail(c, check_targets(p, t.wanted())))) return rc;
    const size_t P = (size_t)p->w * p->h;  // the pixels traced: a filtered render's region, else the tile
    // Each feature's state and, for a host render, the staging of what it writes: before the pass size reads the free memory.  The staging
    // layouts are these tables: one buffer after the other, in the order of pbrs_aov_buffers, pbrs_matte_buffers and pbrs_pass_buffers;
    // nothing goes up, every buffer given comes back.
    const pbrs_aov_buffers& a = t.aovs;
    Staged aovs[] = {{nullptr, 3, a.albedo}, {nullptr, 3, a.normal}, {nullptr, 1, a.coverage}, {nullptr, 1, a.depth}, {nullptr, 1, a.instance},
                     {nullptr, 1, a.material}, {nullptr, 1, a.prim}};
    Staged variance[] = {{nullptr, 1, t.variance}};
    const size_t slots = t.want_matte ? t.matte->slots : 0;
    Staged matte[] = {{nullptr, slots, t.matte_out.ids}, {nullptr, slots, t.matte_out.coverage}, {nullptr, 1, t.matte_out.residual}};
    Staged passes[] = {{nullptr, 3, t.passes.direct}, {nullptr, 3, t.passes.indirect}, {nullptr, 1, t.passes.direct_variance},
                       {nullptr, 1, t.passes.indirect_variance}};
    float* const rgb_host = t.rgb;
    if (t.filt) rc = c->buf[BUF_FILTER_SUM].grow(c, 4 * PT * sizeof(float), "the filter sums");
    if (t.want_aovs()) {
        if (!rc) rc = c->buf[BUF_AOV_STATE].grow(c, PBRS_AOV_STATE_WORDS * P * sizeof(float), "the AOV state");
        if (!rc && host) rc = stage(c, BUF_AOV_OUT, "the AOV buffers", aovs, P);
    }
    if (t.variance) {
        if (!rc) rc = c->buf[BUF_MOMENT_STATE].grow(c, PBRS_MOMENT_STATE_WORDS * P * sizeof(float), "the variance AOV's moments");
        if (!rc && host) rc = stage(c, BUF_VARIANCE_OUT, "the variance buffer", variance, P);
    }
    if (t.want_matte) {
        if (!rc) rc = c->buf[BUF_MATTE_STATE].grow(c, PBRS_MATTE_STATE_WORDS(slots) * P * sizeof(uint32_t), "the matte state");
        if (!rc && host) rc = stage(c, BUF_MATTE_OUT, "the matte buffers", matte, P);
    }
    if (t.want_passes()) {
        if (!rc) rc = c->buf[BUF_PASS_STATE].grow(c, PBRS_PASS_STATE_WORDS * P * sizeof(float), "the light passes' state");
        if (!rc && host) rc = stage(c, BUF_PASS_OUT, "the light pass buffers", passes, P);
    }
    uint32_t K = 0;
    if (!rc) rc = pass_size(c, p, K, t.want_passes());
    if (!rc) rc = ensure_work(c, cur(c), P * K, P);
    if (!rc) rc = ensure_direct(c, c->cur_set, P * K, t.want_passes());
    if (rc) return rc;
    if (host) {
        t.rgb = c->rgb_dev;  // P pixels: a filtered render's tile fits
        t.aovs = {aovs[0].as<float>(), aovs[1].as<float>(), aovs[2].as<float>(), aovs[3].as<float>(), aovs[4].as<uint32_t>(), aovs[5].as<uint32_t>(), aovs[6].as<uint32_t>()};
        t.variance = variance[0].as<float>();
        t.matte_out = {matte[0].as<uint32_t>(), matte[1].as<float>(), matte[2].as<float>()};
        t.passes = {passes[0].as<float>(), passes[1].as<float>(), passes[2].as<float>(), passes[3].as<float>()};
    }
    rc = render_common(c, cam, p, K, t);
    if (rc) return rc;
    if (!host) return stats_out ? collect(c, stats_out) : PBRS_OK;
    HIPCHK(c, hipMemcpyAsync(rgb_host, t.rgb, 3 * PT * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if ((rc = copy_staged(c, variance, P, hipMemcpyDeviceToHost))) return rc;
    if ((rc = copy_staged(c, aovs, P, hipMemcpyDeviceToHost))) return rc;
    if ((rc = copy_staged(c, matte, P, hipMemcpyDeviceToHost))) return rc;
    if ((rc = copy_staged(c, passes, P, hipMemcpyDeviceToHost))) return rc;
    return collect(c, stats_out);
}

// The targets of the AOV, matte and light pass entry points: the buffers given (null: none).  A matte is wanted where its buffers are given.
RenderTargets make_targets(float* rgb, const pbrs_aov_buffers* aovs, float* variance, const pbrs_matte_params* params, const pbrs_matte_buffers* matte,
                           const pbrs_pass_buffers* passes) {
    RenderTargets t;
    t.rgb = rgb;
    if (aovs) t.aovs = *aovs;
    t.variance = variance;
    t.want_matte = matte != nullptr;
    t.matte = params;
    if (matte) t.matte_out = *matte;
    if (passes) t.passes = *passes;
    return t;
}

}  // namespace

extern "C" {

int pbrs_create(int device_ordinal, pbrs_ctx** out) {
    if (!out) return PBRS_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_ordinal < 0 || device_ordinal >= n) return PBRS_E_DEVICE;
    pbrs_ctx* c = new pbrs_ctx();
    c->device = device_ordinal;
    // every failure below leaves through pbrs_destroy, which releases whatever had been created by then
    // a non-blocking stream: work another library queues on the legacy default stream (torch's copies in bench.py) neither
    // waits for the frames queued here nor holds them up
    bool ok = hipSetDevice(device_ordinal) == hipSuccess && hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) == hipSuccess;
    c->stream = c->main_stream = c->own_stream;
    {
        int least = 0, greatest = 0;  // (numerically lower = higher priority)
        ok = ok && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess &&
             hipStreamCreateWithPriority(&c->second_stream, hipStreamNonBlocking, greatest) == hipSuccess;
    }
    ok = ok && hipEventCreateWithFlags(&c->pass_set[0].accumulated, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&c->pass_set[1].accumulated, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&c->pass_set[0].late, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&c->pass_set[1].late, hipEventDisableTiming) == hipSuccess;
#ifdef PBRS_DEV_OVERRIDES
    c->dev = read_dev_overrides();
#endif
    c->overlap_passes = c->dev.overlap_passes;
    for (int k = 0; ok && k < 2; ++k) {
        hipEvent_t ev = nullptr;
        ok = hipEventCreate(&ev) == hipSuccess;
        if (ok) c->total_ev.push_back(ev);
    }
    for (pbrs_ctx::PassSet& set : c->pass_set) ok = ok && hipMalloc(reinterpret_cast<void**>(&set.counters), kCounters.words * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipMalloc(reinterpret_cast<void**>(&c->gcnt), 2 * sizeof(GlobalCounters)) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&c->nonfinite), sizeof(unsigned long long)) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&c->bounce_acc), (2 * PBRS_STATS_MAX_BOUNCES + 2) * sizeof(unsigned long long)) == hipSuccess &&
         hipMemset(c->bounce_acc, 0, (2 * PBRS_STATS_MAX_BOUNCES + 2) * sizeof(unsigned long long)) == hipSuccess &&
         hipMemset(c->nonfinite, 0, sizeof(unsigned long long)) == hipSuccess &&
         hipHostMalloc(reinterpret_cast<void**>(&c->split_host), 2 * sizeof(unsigned long long), hipHostMallocDefault) == hipSuccess &&
         hipEventCreateWithFlags(&c->split_ev, hipEventDisableTiming) == hipSuccess;
    ok = ok && configure_kernels(c) == PBRS_OK;
    if (!ok) {
        pbrs_destroy(c);
        return PBRS_E_DEVICE;
    }
    *out = c;
    return PBRS_OK;
}

void pbrs_destroy(pbrs_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->second_stream) (void)hipStreamSynchronize(c->second_stream);
    free_scene(c);
    free_work(c);
    for (DeviceBuffer& b : c->buf)
        if (b.p) (void)hipFree(b.p);
    for (pbrs_ctx::PassSet& set : c->pass_set)
        if (set.counters) (void)hipFree(set.counters);
    for (int k = 0; k < 2; ++k)
        if (c->pass_set[k].accumulated) (void)hipEventDestroy(c->pass_set[k].accumulated);
    for (int k = 0; k < 2; ++k)
        if (c->pass_set[k].late) (void)hipEventDestroy(c->pass_set[k].late);
    if (c->second_stream) (void)hipStreamDestroy(c->second_stream);
    if (c->gcnt) (void)hipFree(c->gcnt);
    if (c->nonfinite) (void)hipFree(c->nonfinite);
    if (c->bounce_acc) (void)hipFree(c->bounce_acc);
    if (c->split_host) (void)hipHostFree(c->split_host);
    if (c->split_ev) (void)hipEventDestroy(c->split_ev);
    for (auto& e : c->events) {
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    for (auto& e : c->total_ev) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

const char* pbrs_last_error(const pbrs_ctx* c) { return c ? c->error.c_str() : "null context"; }

int pbrs_set_stream(pbrs_ctx* c, void* hip_stream) {
    if (!c) return PBRS_E_INVALID;
    c->main_stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->own_stream;
    c->stream = c->main_stream;  // (pass set 0 is the one in use between calls)
    return PBRS_OK;
}

int pbrs_set_pass_overlap(pbrs_ctx* c, int enabled) {
    if (!c) return PBRS_E_INVALID;
    c->overlap_passes = enabled != 0;
    return PBRS_OK;
}

int pbrse_set_entry_nodes(pbrs_ctx* c, int enabled) {
    if (!c) return PBRS_E_INVALID;
    c->entry_nodes = enabled != 0;
    return PBRS_OK;
}

int pbrse_last_entry_info(pbrs_ctx* c, pbrs_entry_info* out) {
    if (!c || !out) return PBRS_E_INVALID;
    *out = pbrs_entry_info{};
    if (!c->last_entry) return PBRS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->main_stream));
    uint32_t v[4];
    HIPCHK(c, hipMemcpy(v, static_cast<const char*>(c->buf[BUF_ENTRY_TABLE].p) + (size_t)c->last_entry_pixels * sizeof(pbrs_entry_record), sizeof v, hipMemcpyDeviceToHost));
    *out = pbrs_entry_info{v[0], v[1], v[2], v[3]};
    return PBRS_OK;
}

// Check, prepare and choose on the host (host/scene_prepare.h, host/kernel_choice.h), then bind, and only then touch the device: a
// refusal leaves the context's previous scene in place.  A failing hipMalloc or copy leaves the context without a scene.
int pbrs_upload_scene(pbrs_ctx* c, const pbrs_scene_desc* d) {
    if (!c || !d) return PBRS_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const SceneCheck chk = check_scene(*d);
    if (chk.code != PBRS_OK) return fail(c, chk.code, chk.message);
    PreparedScene P = prepare_scene(*d, chk.levels, c->dev);
    const KernelChoice choice = choose_kernels(P.facts, c->dev);
    KernelPlan plan;
    if (!bind_kernels(choice, plan)) return fail(c, PBRS_E_DEVICE, "no kernel instantiation for this scene's feature set");
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->second_stream);
    free_scene(c);
    c->plan = plan;
    DevScene S = P.S;
    int rc;
    // the split planes ride in the spare bits of the inner BLAS nodes' b words (device/split_planes.h), on the uploaded copy only
    for (size_t i = 0; i < P.nodes.size(); ++i) P.nodes[i].b |= P.node_planes[i];
    if ((rc = upload(c, P.nodes.data(), P.nodes.size(), &S.nodes))) return rc;
    // ... and the leaves' triangles in the wide nodes' references to them (device/scene.h, PBRS_WREF_PACKED), with the table that leads back to the leaf
    pack_wide_leaves(P);
    if (!P.wide.empty() && (rc = upload_wide(c, P, &S.wnodes))) return rc;
    if ((rc = upload(c, P.inst.data(), P.inst.size(), &S.inst))) return rc;
    if ((rc = upload(c, d->shapes, d->n_shapes, &S.shapes))) return rc;
    if ((rc = upload(c, d->meshes, d->n_meshes, &S.meshes))) return rc;
    if ((rc = upload(c, d->tri_verts, d->n_triangles, &S.tv))) return rc;
    if ((rc = upload(c, d->tri_shade, d->n_triangles, &S.ts))) return rc;
    if ((rc = upload(c, d->materials, d->n_materials, &S.mats))) return rc;
    if ((rc = upload(c, d->bxdfs, d->n_bxdfs, &S.bxdfs))) return rc;
    {  // the lights' links to the instances that are the lights ride in the padding of the uploaded copy (host/scene_prepare.h)
        std::vector<pbrs_area_light> lights(d->area_lights, d->area_lights + d->n_area_lights);
        write_light_links(P, lights);
        if ((rc = upload(c, lights.data(), lights.size(), &S.alights))) return rc;
    }
    if ((rc = upload(c, d->delta_lights, d->n_delta_lights, &S.dlights))) return rc;
    if ((rc = upload(c, d->textures, d->n_textures, &S.textures))) return rc;
    if ((rc = upload(c, d->tex_floats, d->n_tex_floats, &S.tex_floats))) return rc;
    if ((rc = upload(c, d->tex_words, d->n_tex_words, &S.tex_words))) return rc;
    if ((rc = upload(c, d->fourier_tables, d->n_fourier_tables, &S.fourier))) return rc;
    // what the plan's traversal kernels stage (kernels.h, stage_scene / stage_top)
    const bool lds_scene = choice.lds_staging == PBRS_FEAT_LDS_SCENE;
    S.lds_off_words = P.stack_depth * kBlock;
    S.lds_nodes = lds_scene ? (uint32_t)P.nodes.size() : choice.lds_staging == PBRS_FEAT_LDS_TOP ? d->n_tlas_nodes : 0u;
    S.lds_tris = lds_scene ? d->n_triangles : 0u;
    S.lds_inst = lds_scene ? d->n_instances : 0u;
    S.lds_shapes = lds_scene ? d->n_shapes : 0u;
    c->S = S;
    c->overlap_from = c->dev.overlap_from.value_or(P.walk_bytes <= (4ull << 20) ? 2u : 4u);  // one XCD's L2 holds the arrays the walks read, or not (pbrs_ctx::overlap_from)
    c->has_vis_records = P.has_vis_records;
    c->lambert_scene = P.facts.lambert;
    c->fourier_scene = P.facts.fourier;
    c->material_flags.resize(d->n_materials);
    for (uint32_t i = 0; i < d->n_materials; ++i) c->material_flags[i] = d->materials[i].flags;
    c->stack_depth = P.stack_depth;
    c->entry_height = P.entry_height;
    c->entry_rows = P.entry_rows;
    c->entry_table = nullptr;
    c->last_entry = false;
    c->has_scene = true;
    c->split_decision = 0;  // (the streams were synchronised above: no probe of the previous scene is in flight)
    c->split_probe_in_flight = false;
    return PBRS_OK;
}

int pbrs_render_tile_passes_device(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, float* rgb_out_device,
                                   const pbrs_aov_buffers* aovs_device, float* variance_device, const pbrs_matte_params* params,
                                   const pbrs_matte_buffers* matte_device, const pbrs_pass_buffers* passes_device, pbrs_stats* stats_out) {
    if (!c) return PBRS_E_INVALID;
    if (!rgb_out_device) return fail(c, PBRS_E_INVALID, "null output");
    return render(c, cam, p, nullptr, make_targets(rgb_out_device, aovs_device, variance_device, params, matte_device, passes_device), false, stats_out);
}

int pbrs_render_tile_matte_device(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, float* rgb_out_device,
                                  const pbrs_aov_buffers* aovs_device, float* variance_device, const pbrs_matte_params* params,
                                  const pbrs_matte_buffers* matte_device, pbrs_stats* stats_out) {
    return pbrs_render_tile_passes_device(c, cam, p, rgb_out_device, aovs_device, variance_device, params, matte_device, nullptr, stats_out);
}

int pbrs_render_tile_aovs_var_device(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, float* rgb_out_device,
                                     const pbrs_aov_buffers* aovs_device, float* variance_device, pbrs_stats* stats_out) {
    return pbrs_render_tile_matte_device(c, cam, p, rgb_out_device, aovs_device, variance_device, nullptr, nullptr, stats_out);
}

int pbrs_render_tile_aovs_device(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, float* rgb_out_device, const pbrs_aov_buffers* aovs_device,
                                 pbrs_stats* stats_out) {
    return pbrs_render_tile_matte_device(c, cam, p, rgb_out_device, aovs_device, nullptr, nullptr, nullptr, stats_out);
}

int pbrs_render_tile_device(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, float* rgb_out_device, pbrs_stats* stats_out) {
    return pbrs_render_tile_matte_device(c, cam, p, rgb_out_device, nullptr, nullptr, nullptr, nullptr, stats_out);
}

int pbrs_render_tile_passes(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, float* rgb_out_host, const pbrs_aov_buffers* aovs_host,
                            float* variance_host, const pbrs_matte_params* params, const pbrs_matte_buffers* matte_host, const pbrs_pass_buffers* passes_host,
                            pbrs_stats* stats_out) {
    if (!c) return PBRS_E_INVALID;
    if (!rgb_out_host) return fail(c, PBRS_E_INVALID, "null output");
    return render(c, cam, p, nullptr, make_targets(rgb_out_host, aovs_host, variance_host, params, matte_host, passes_host), true, stats_out);
}

int pbrs_render_tile_matte(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, float* rgb_out_host, const pbrs_aov_buffers* aovs_host,
                           float* variance_host, const pbrs_matte_params* params, const pbrs_matte_buffers* matte_host, pbrs_stats* stats_out) {
    return pbrs_render_tile_passes(c, cam, p, rgb_out_host, aovs_host, variance_host, params, matte_host, nullptr, stats_out);
}

int pbrs_render_tile_aovs_var(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, float* rgb_out_host, const pbrs_aov_buffers* aovs_host,
                              float* variance_host, pbrs_stats* stats_out) {
    return pbrs_render_tile_matte(c, cam, p, rgb_out_host, aovs_host, variance_host, nullptr, nullptr, stats_out);
}

int pbrs_render_tile_aovs(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, float* rgb_out_host, const pbrs_aov_buffers* aovs_host,
                          pbrs_stats* stats_out) {
    return pbrs_render_tile_matte(c, cam, p, rgb_out_host, aovs_host, nullptr, nullptr, nullptr, stats_out);
}

int pbrs_render_tile(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, float* rgb_out_host, pbrs_stats* stats_out) {
    return pbrs_render_tile_matte(c, cam, p, rgb_out_host, nullptr, nullptr, nullptr, nullptr, stats_out);
}

int pbrs_render_tile_filtered_device(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, const pbrs_pixel_filter* f,
                                     float* rgb_out_device, pbrs_stats* stats_out) {
    if (!c) return PBRS_E_INVALID;
    if (!rgb_out_device) return fail(c, PBRS_E_INVALID, "null output");
    if (!f) return fail(c, PBRS_E_INVALID, "null pixel filter");
    return render(c, cam, p, f, make_targets(rgb_out_device, nullptr, nullptr, nullptr, nullptr, nullptr), false, stats_out);
}

int pbrs_render_tile_filtered(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, const pbrs_pixel_filter* f, float* rgb_out_host,
                              pbrs_stats* stats_out) {
    if (!c) return PBRS_E_INVALID;
    if (!rgb_out_host) return fail(c, PBRS_E_INVALID, "null output");
    if (!f) return fail(c, PBRS_E_INVALID, "null pixel filter");
    return render(c, cam, p, f, make_targets(rgb_out_host, nullptr, nullptr, nullptr, nullptr, nullptr), true, stats_out);
}

// ---- denoisers (include/pbrs_gpu.h, device/denoise.h) ----
static_assert(sizeof(pbrs_denoise_params) == 32, "pbrs_denoise_params is 32 B");
static_assert(sizeof(pbrs_denoise_var_params) == 32, "pbrs_denoise_var_params is 32 B");

namespace {

using DenoiseKernel = void (*)(const float4*, const float4*, const uint32_t*, float4*, DenoiseConst);
#define PBRS_DENOISE_ROW(IDS, VAR)                                                                                             \
    {k_denoise_atrous<0, IDS, VAR>, k_denoise_atrous<1, IDS, VAR>, k_denoise_atrous<2, IDS, VAR>, k_denoise_atrous<3, IDS, VAR>, \
     k_denoise_atrous<4, IDS, VAR>, k_denoise_atrous<5, IDS, VAR>}
// [variance-guided][id stop][iteration]
constexpr DenoiseKernel kDenoiseAtrous[2][2][PBRS_DENOISE_MAX_ITERATIONS] = {{PBRS_DENOISE_ROW(false, false), PBRS_DENOISE_ROW(true, false)},
                                                                             {PBRS_DENOISE_ROW(false, true), PBRS_DENOISE_ROW(true, true)}};
#undef PBRS_DENOISE_ROW

// The launches of one denoise on the context's stream (arguments checked, scratch there): pack, the iterations ping-pong, unpack.
// g.variance chooses the filter: given, the variance-guided one, whose first sigma is sigma_luminance.
int denoise_launch(pbrs_ctx* c, const pbrs_denoise_params& p, const float* rgb_in, const DenoiseGuides& g, float* rgb_out, float* variance_out) {
    const bool var = g.variance != nullptr;
    const uint32_t P = p.w * p.h;
    const DeviceBuffer& scratch = c->buf[BUF_DENOISE + var];
    const size_t cap = scratch.cap_bytes / kDenoiseBytesPerPixel;
    float4* plane[2] = {scratch.as<float4>(), scratch.as<float4>() + cap};
    float4* guide = plane[1] + cap;
    uint32_t* ids = reinterpret_cast<uint32_t*>(guide + cap);
    const uint32_t demod = p.flags & PBRS_DENOISE_DEMODULATE;
    const bool id_stop = (p.flags & PBRS_DENOISE_ID_STOP) != 0;
    DenoiseGuides packed = g;
    if (!id_stop) packed.instance = nullptr;
    const dim3 lin((P + kBlock - 1) / kBlock), cells((p.w + PBRS_DENOISE_CELL - 1) / PBRS_DENOISE_CELL, (p.h + PBRS_DENOISE_CELL - 1) / PBRS_DENOISE_CELL);
    hipLaunchKernelGGL(k_denoise_pack, lin, dim3(kBlock), 0, c->stream, rgb_in, packed, P, demod, p.albedo_floor, plane[0], guide, ids);
    DenoiseConst k{};
    k.w = p.w, k.h = p.h;
    k.c1 = p.sigma_color;  // variance-guided: sigma_luminance, the same at every iteration
    k.in = 1.0f / (p.sigma_normal * p.sigma_normal);
    k.id = 1.0f / (p.sigma_depth * p.sigma_depth);
    for (uint32_t it = 0; it < p.iterations; ++it) {
        if (!var) {
            const float sc = p.sigma_color * pn_exp2i(-(int)it);
            k.c1 = 1.0f / (sc * sc);
        }
        hipLaunchKernelGGL(kDenoiseAtrous[var][id_stop][it], cells, dim3(kBlock), 0, c->stream, plane[it & 1u], guide, ids, plane[(it + 1u) & 1u], k);
    }
    hipLaunchKernelGGL(k_denoise_unpack, lin, dim3(kBlock), 0, c->stream, plane[p.iterations & 1u], g.albedo, P, demod, p.albedo_floor, rgb_out,
                       variance_out);
    HIPCHK(c, hipGetLastError());
    return PBRS_OK;
}

// A denoiser's scratch for P pixels.  The variance-guided denoiser keeps scratch of its own (the planes have the plain one's size).
int grow_denoise(pbrs_ctx* c, bool var, size_t P) {
    return c->buf[BUF_DENOISE + var].grow(c, P * kDenoiseBytesPerPixel, var ? "the variance-guided denoiser's scratch" : "the denoiser's scratch");
}

// The host variants: the image and the given guides go through the denoiser's device staging (the image, filtered in place; the guides;
// variance-guided: the variance in and out — the plain denoiser's staging ends with the instance ids), and the call waits for the result.
int denoise_staged(pbrs_ctx* c, const pbrs_denoise_params& p, const float* rgb_in_host, const DenoiseGuides& host, float* rgb_out_host,
                   float* variance_out_host) {
    const bool var = host.variance != nullptr;
    const size_t P = (size_t)p.w * p.h;
    const int rc = grow_denoise(c, var, P);
    if (rc) return rc;
    const size_t v = var ? 1 : 0;
    Staged s[] = {{rgb_in_host, 3, rgb_out_host}, {host.albedo, 3}, {host.normal, 3}, {host.depth, 1}, {host.instance, 1}, {host.variance, v},
                  {nullptr, v, variance_out_host}};
    return run_staged(c, BufferId(BUF_DENOISE_STAGE + var), var ? "the variance-guided denoiser's staging" : "the denoiser's staging", s, P, [&] {
        float* rgb = s[0].as<float>();
        return denoise_launch(c, p, rgb, {s[1].as<float>(), s[2].as<float>(), s[3].as<float>(), s[4].as<uint32_t>(), s[5].as<float>()}, rgb, s[6].as<float>());
    });
}

}  // namespace

int pbrs_denoise_device(pbrs_ctx* c, const pbrs_denoise_params* p, const float* rgb_in_device, const pbrs_denoise_guides* guides_device,
                        float* rgb_out_device) {
    int rc = enter(c, check_denoise(p, rgb_in_device, guides_device, rgb_out_device));
    if (!rc) rc = grow_denoise(c, false, (size_t)p->w * p->h);
    if (rc) return rc;
    const pbrs_denoise_guides& g = *guides_device;
    return denoise_launch(c, *p, rgb_in_device, {g.albedo, g.normal, g.depth, g.instance, nullptr}, rgb_out_device, nullptr);
}

int pbrs_denoise(pbrs_ctx* c, const pbrs_denoise_params* p, const float* rgb_in_host, const pbrs_denoise_guides* guides_host, float* rgb_out_host) {
    const int rc = enter(c, check_denoise(p, rgb_in_host, guides_host, rgb_out_host));
    if (rc) return rc;
    const pbrs_denoise_guides& g = *guides_host;
    return denoise_staged(c, *p, rgb_in_host, {g.albedo, g.normal, g.depth, g.instance, nullptr}, rgb_out_host, nullptr);
}

int pbrs_denoise_var_device(pbrs_ctx* c, const pbrs_denoise_var_params* p, const float* rgb_in_device, const pbrs_denoise_var_guides* guides_device,
                            float* rgb_out_device, float* variance_out_device) {
    int rc = enter(c, check_denoise_var(p, rgb_in_device, guides_device, rgb_out_device));
    if (!rc) rc = grow_denoise(c, true, (size_t)p->w * p->h);
    if (rc) return rc;
    return denoise_launch(c, plain_params(*p), rgb_in_device, *guides_device, rgb_out_device, variance_out_device);
}

int pbrs_denoise_var(pbrs_ctx* c, const pbrs_denoise_var_params* p, const float* rgb_in_host, const pbrs_denoise_var_guides* guides_host,
                     float* rgb_out_host, float* variance_out_host) {
    const int rc = enter(c, check_denoise_var(p, rgb_in_host, guides_host, rgb_out_host));
    if (rc) return rc;
    return denoise_staged(c, plain_params(*p), rgb_in_host, *guides_host, rgb_out_host, variance_out_host);
}

// ---- id mattes: the mask of a selection (include/pbrs_gpu.h, device/matte.h) ----
static_assert(sizeof(pbrs_matte_params) == 8, "pbrs_matte_params is 8 B");

namespace {

// The selection to the device and the kernel, on the context's stream (arguments checked).
int matte_mask_launch(pbrs_ctx* c, uint32_t P, uint32_t slots, const uint32_t* ids, const float* coverage, const uint32_t* select, uint32_t n_select, float* mask) {
    DeviceBuffer& sel = c->buf[BUF_MATTE_SELECT];
    int rc = sel.grow(c, PBRS_MATTE_MAX_SELECT * sizeof(uint32_t), "the matte selection");
    if (rc) return rc;
    // from the caller's memory: the runtime has taken the bytes when the call returns, and the copy runs in the stream's order
    if (n_select) HIPCHK(c, hipMemcpyAsync(sel.p, select, n_select * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_matte_mask, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), n_select * sizeof(uint32_t), c->stream, ids, coverage, sel.as<uint32_t>(), n_select,
                       P, slots, mask);
    HIPCHK(c, hipGetLastError());
    return PBRS_OK;
}

}  // namespace

int pbrs_matte_mask_device(pbrs_ctx* c, uint32_t w, uint32_t h, uint32_t slots, const uint32_t* ids_device, const float* coverage_device,
                           const uint32_t* select, uint32_t n_select, float* mask_out_device) {
    const int rc = enter(c, check_matte_mask(w, h, slots, ids_device, coverage_device, select, n_select, mask_out_device));
    if (rc) return rc;
    return matte_mask_launch(c, w * h, slots, ids_device, coverage_device, select, n_select, mask_out_device);
}

int pbrs_matte_mask(pbrs_ctx* c, uint32_t w, uint32_t h, uint32_t slots, const uint32_t* ids_host, const float* coverage_host,
                    const uint32_t* select, uint32_t n_select, float* mask_out_host) {
    const int rc = enter(c, check_matte_mask(w, h, slots, ids_host, coverage_host, select, n_select, mask_out_host));
    if (rc) return rc;
    const size_t P = (size_t)w * h;
    Staged s[] = {{ids_host, slots}, {coverage_host, slots}, {nullptr, 1, mask_out_host}};  // the staging of a matte render, the mask in the residual's place
    return run_staged(c, BUF_MATTE_OUT, "the matte buffers", s, P,
                      [&] { return matte_mask_launch(c, (uint32_t)P, slots, s[0].as<uint32_t>(), s[1].as<float>(), select, n_select, s[2].as<float>()); });
}

namespace {

// The add over the 3 * P words of an image, on the context's stream (arguments checked).
int combine_launch(pbrs_ctx* c, size_t P, const float* direct, const float* indirect, float* rgb_out) {
    const uint32_t n = (uint32_t)(3 * P);
    const uint32_t grid = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_combine_passes, dim3(grid < kStreamGridCap ? grid : kStreamGridCap), dim3(kBlock), 0, c->stream, direct, indirect, rgb_out, n);
    HIPCHK(c, hipGetLastError());
    return PBRS_OK;
}

}  // namespace

int pbrs_combine_passes_device(pbrs_ctx* c, uint32_t w, uint32_t h, const float* direct_device, const float* indirect_device, float* rgb_out_device) {
    const int rc = enter(c, check_combine(w, h, direct_device, indirect_device, rgb_out_device));
    if (rc) return rc;
    return combine_launch(c, (size_t)w * h, direct_device, indirect_device, rgb_out_device);
}

int pbrs_combine_passes(pbrs_ctx* c, uint32_t w, uint32_t h, const float* direct_host, const float* indirect_host, float* rgb_out_host) {
    const int rc = enter(c, check_combine(w, h, direct_host, indirect_host, rgb_out_host));
    if (rc) return rc;
    const size_t P = (size_t)w * h;
    // the staging of a render with passes; the sum lands in the direct layer's place
    Staged s[] = {{direct_host, 3, rgb_out_host}, {indirect_host, 3}, {nullptr, 1}, {nullptr, 1}};
    return run_staged(c, BUF_PASS_OUT, "the light pass buffers", s, P, [&] { return combine_launch(c, P, s[0].as<float>(), s[1].as<float>(), s[0].as<float>()); });
}

// ---- temporal accumulation (include/pbrs_gpu.h, device/temporal.h) ----
static_assert(sizeof(pbrs_temporal_params) == 32, "pbrs_temporal_params is 32 B");
static_assert(sizeof(pbrs_instance_motion) == 96 && offsetof(pbrs_instance_motion, n) == 48 && offsetof(pbrs_instance_motion, flags) == 84,
              "pbrs_instance_motion is 96 B: temporal_reproject reads it as six float4");

namespace {

using TemporalKernel = void (*)(TemporalIn, TemporalOut, TemporalConst);
// [normal test][id test], with a history; without one no tap is read
constexpr TemporalKernel kTemporal[2][2] = {{k_temporal<true, false, false>, k_temporal<true, false, true>},
                                            {k_temporal<true, true, false>, k_temporal<true, true, true>}};
// the same with a motion table
constexpr TemporalKernel kTemporalMotion[2][2] = {{k_temporal<true, false, false, true>, k_temporal<true, false, true, true>},
                                                  {k_temporal<true, true, false, true>, k_temporal<true, true, true, true>}};

// with a clip (always with a history): [motion table][normal test][id test]
using TemporalClipKernel = void (*)(TemporalIn, TemporalOut, TemporalConst, TemporalClipConst);
constexpr TemporalClipKernel kTemporalClip[2][2][2] = {
    {{k_temporal_clip<false, false, false>, k_temporal_clip<false, true, false>}, {k_temporal_clip<true, false, false>, k_temporal_clip<true, true, false>}},
    {{k_temporal_clip<false, false, true>, k_temporal_clip<false, true, true>}, {k_temporal_clip<true, false, true>, k_temporal_clip<true, true, true>}}};

// The caller's table (host memory) into the context's copy, on the context's stream: ordered behind the kernels of earlier calls that read
// the copy, and the runtime has taken the bytes when the call returns.  -> the device table in *dev (null without a table).
int upload_motion_table(pbrs_ctx* c, const pbrs_instance_motion* motion, uint32_t n_motion, const pbrs_instance_motion** dev) {
    *dev = nullptr;
    if (!motion) return PBRS_OK;
    DeviceBuffer& b = c->buf[BUF_MOTION_TABLE];
    const int rc = b.grow(c, (size_t)n_motion * sizeof(pbrs_instance_motion), "the instance motion table");
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(b.p, motion, (size_t)n_motion * sizeof(pbrs_instance_motion), hipMemcpyHostToDevice, c->stream));
    *dev = b.as<pbrs_instance_motion>();
    return PBRS_OK;
}

// What depends on the cameras alone, in the header's order (this file is compiled without contraction, host side included).
void temporal_cameras(TemporalConst& k, const pbrs_camera& cam, const pbrs_camera* cam_prev) {
    for (int i = 0; i < 3; ++i) k.center[i] = cam.center[i], k.c[i] = cam.c[i], k.a[i] = cam.a[i], k.b[i] = cam.b[i];
    if (!cam_prev) return;
    for (int i = 0; i < 3; ++i) k.center_prev[i] = cam_prev->center[i];
    temporal_cross(cam_prev->b, cam_prev->c, k.nu);
    temporal_cross(cam_prev->c, cam_prev->a, k.nv);
    temporal_cross(cam_prev->a, cam_prev->b, k.nw);
    k.D = temporal_dot(cam_prev->a, k.nu);
}

// The one launch on the context's stream (arguments checked; device pointers, the motion table the caller's host memory).  Without a
// history no tap is read and the table is not needed, and there is nothing to clip.  With a history and a clip: k_temporal_clip, one
// 16 x 16 block per cell of the image.
int temporal_launch(pbrs_ctx* c, const pbrs_temporal_params& p, const pbrs_camera& cam, const pbrs_camera* cam_prev, const pbrs_temporal_frame& f,
                    const pbrs_temporal_guides* prev, const pbrs_temporal_history* hin, const pbrs_temporal_history& hout, float* variance_out,
                    const pbrs_instance_motion* motion, uint32_t n_motion, const pbrs_history_clip_params* clip = nullptr) {
    TemporalConst k{};
    k.w = p.w, k.h = p.h;
    k.max_history = p.max_history, k.depth_tolerance = p.depth_tolerance, k.min_temporal = p.min_temporal;
    k.normal_tolerance2 = p.normal_tolerance * p.normal_tolerance;
    temporal_cameras(k, cam, hin ? cam_prev : nullptr);
    TemporalIn in{f.rgb, f.variance, f.depth, f.normal, f.instance, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0u};
    TemporalKernel fn = k_temporal<false, false, false>;
    if (hin) {
        in.depth_prev = prev->depth, in.normal_prev = prev->normal, in.instance_prev = prev->instance;
        in.rgb_hist = hin->rgb, in.moments_hist = hin->moments, in.length_hist = hin->length;
        const int rc = upload_motion_table(c, motion, n_motion, &in.motion);
        if (rc) return rc;
        in.n_motion = in.motion ? n_motion : 0u;
        fn = (in.motion ? kTemporalMotion : kTemporal)[f.normal != nullptr][(p.flags & PBRS_TEMPORAL_ID_TEST) != 0];
        if (clip) {
            const dim3 grid((p.w + PBRS_DENOISE_CELL - 1) / PBRS_DENOISE_CELL, (p.h + PBRS_DENOISE_CELL - 1) / PBRS_DENOISE_CELL);
            hipLaunchKernelGGL(kTemporalClip[in.motion != nullptr][f.normal != nullptr][(p.flags & PBRS_TEMPORAL_ID_TEST) != 0], grid, dim3(kBlock), 0,
                               c->stream, in, TemporalOut{hout.rgb, hout.moments, hout.length, variance_out}, k,
                               TemporalClipConst{clip->radius, clip->gamma, clip->clip_history});
            HIPCHK(c, hipGetLastError());
            return PBRS_OK;
        }
    }
    const uint32_t P = p.w * p.h;
    hipLaunchKernelGGL(fn, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, in, TemporalOut{hout.rgb, hout.moments, hout.length, variance_out}, k);
    HIPCHK(c, hipGetLastError());
    return PBRS_OK;
}

// The host variants' call (arguments checked): the frame, the previous guides and the history staged, the launch, the new history and
// the variance copied back, one wait.
int temporal_staged(pbrs_ctx* c, const pbrs_temporal_params* p, const pbrs_camera* cam, const pbrs_camera* cam_prev, const pbrs_temporal_frame& f,
                    const pbrs_temporal_guides* prev_host, const pbrs_temporal_history* history_in_host, const pbrs_temporal_history& ho,
                    float* variance_out_host, const pbrs_instance_motion* motion, uint32_t n_motion, const pbrs_history_clip_params* clip) {
    const size_t P = (size_t)p->w * p->h;
    const pbrs_temporal_guides g = history_in_host ? *prev_host : pbrs_temporal_guides{};  // without a history the previous frame is not read
    const pbrs_temporal_history hi = history_in_host ? *history_in_host : pbrs_temporal_history{};
    Staged s[] = {{f.rgb, 3}, {f.variance, 1}, {f.depth, 1}, {f.normal, 3}, {f.instance, 1}, {g.depth, 1}, {g.normal, 3}, {g.instance, 1},
                  {hi.rgb, 3}, {hi.moments, 2}, {hi.length, 1},
                  {nullptr, 3, ho.rgb}, {nullptr, 2, ho.moments}, {nullptr, 1, ho.length}, {nullptr, 1, variance_out_host}};
    return run_staged(c, BUF_TEMPORAL_STAGE, "the temporal accumulation's staging", s, P, [&] {
        const pbrs_temporal_frame fd{s[0].as<float>(), s[1].as<float>(), s[2].as<float>(), s[3].as<float>(), s[4].as<uint32_t>()};
        const pbrs_temporal_guides gd{s[5].as<float>(), s[6].as<float>(), s[7].as<uint32_t>()};
        const pbrs_temporal_history hid{s[8].as<float>(), s[9].as<float>(), s[10].as<float>()}, hod{s[11].as<float>(), s[12].as<float>(), s[13].as<float>()};
        return temporal_launch(c, *p, *cam, cam_prev, fd, &gd, history_in_host ? &hid : nullptr, hod, s[14].as<float>(), motion, n_motion, clip);
    });
}

}  // namespace

int pbrs_temporal_accumulate_motion_device(pbrs_ctx* c, const pbrs_temporal_params* p, const pbrs_camera* cam, const pbrs_camera* cam_prev,
                                           const pbrs_temporal_frame* frame_device, const pbrs_temporal_guides* prev_device,
                                           const pbrs_temporal_history* history_in_device, const pbrs_temporal_history* history_out_device,
                                           float* variance_out_device, const pbrs_instance_motion* motion, uint32_t n_motion) {
    const int rc = enter(c, check_temporal_motion(p, cam, cam_prev, frame_device, prev_device, history_in_device, history_out_device, motion, n_motion));
    if (rc) return rc;
    return temporal_launch(c, *p, *cam, cam_prev, *frame_device, prev_device, history_in_device, *history_out_device, variance_out_device, motion,
                           n_motion);
}

int pbrs_temporal_accumulate_device(pbrs_ctx* c, const pbrs_temporal_params* p, const pbrs_camera* cam, const pbrs_camera* cam_prev,
                                    const pbrs_temporal_frame* frame_device, const pbrs_temporal_guides* prev_device,
                                    const pbrs_temporal_history* history_in_device, const pbrs_temporal_history* history_out_device,
                                    float* variance_out_device) {
    return pbrs_temporal_accumulate_motion_device(c, p, cam, cam_prev, frame_device, prev_device, history_in_device, history_out_device,
                                                  variance_out_device, nullptr, 0);
}

int pbrs_temporal_accumulate(pbrs_ctx* c, const pbrs_temporal_params* p, const pbrs_camera* cam, const pbrs_camera* cam_prev,
                             const pbrs_temporal_frame* frame_host, const pbrs_temporal_guides* prev_host,
                             const pbrs_temporal_history* history_in_host, const pbrs_temporal_history* history_out_host, float* variance_out_host) {
    return pbrs_temporal_accumulate_motion(c, p, cam, cam_prev, frame_host, prev_host, history_in_host, history_out_host, variance_out_host, nullptr, 0);
}

int pbrs_temporal_accumulate_motion(pbrs_ctx* c, const pbrs_temporal_params* p, const pbrs_camera* cam, const pbrs_camera* cam_prev,
                                    const pbrs_temporal_frame* frame_host, const pbrs_temporal_guides* prev_host,
                                    const pbrs_temporal_history* history_in_host, const pbrs_temporal_history* history_out_host,
                                    float* variance_out_host, const pbrs_instance_motion* motion, uint32_t n_motion) {
    const int rc = enter(c, check_temporal_motion(p, cam, cam_prev, frame_host, prev_host, history_in_host, history_out_host, motion, n_motion));
    if (rc) return rc;
    return temporal_staged(c, p, cam, cam_prev, *frame_host, prev_host, history_in_host, *history_out_host, variance_out_host, motion, n_motion, nullptr);
}

// ---- history clipping (include/pbrs_gpu.h, device/temporal.h) ----
static_assert(sizeof(pbrs_history_clip_params) == 16, "pbrs_history_clip_params is 16 B");
static_assert(PBRS_CLIP_MAX_TILE <= PBRS_CLIP_PITCH && PBRS_CLIP_PITCH % 16u == 0, "k_temporal_clip's LDS rows hold the largest halo at a conflict-free pitch");

int pbrs_temporal_accumulate_clip_device(pbrs_ctx* c, const pbrs_temporal_params* p, const pbrs_camera* cam, const pbrs_camera* cam_prev,
                                         const pbrs_temporal_frame* frame_device, const pbrs_temporal_guides* prev_device,
                                         const pbrs_temporal_history* history_in_device, const pbrs_temporal_history* history_out_device,
                                         float* variance_out_device, const pbrs_instance_motion* motion, uint32_t n_motion,
                                         const pbrs_history_clip_params* clip) {
    if (!clip)
        return pbrs_temporal_accumulate_motion_device(c, p, cam, cam_prev, frame_device, prev_device, history_in_device, history_out_device,
                                                      variance_out_device, motion, n_motion);
    const int rc = enter(c, check_temporal_clip(p, cam, cam_prev, frame_device, prev_device, history_in_device, history_out_device, motion, n_motion, clip));
    if (rc) return rc;
    return temporal_launch(c, *p, *cam, cam_prev, *frame_device, prev_device, history_in_device, *history_out_device, variance_out_device, motion,
                           n_motion, clip);
}

int pbrs_temporal_accumulate_clip(pbrs_ctx* c, const pbrs_temporal_params* p, const pbrs_camera* cam, const pbrs_camera* cam_prev,
                                  const pbrs_temporal_frame* frame_host, const pbrs_temporal_guides* prev_host,
                                  const pbrs_temporal_history* history_in_host, const pbrs_temporal_history* history_out_host,
                                  float* variance_out_host, const pbrs_instance_motion* motion, uint32_t n_motion,
                                  const pbrs_history_clip_params* clip) {
    if (!clip)
        return pbrs_temporal_accumulate_motion(c, p, cam, cam_prev, frame_host, prev_host, history_in_host, history_out_host, variance_out_host, motion,
                                               n_motion);
    const int rc = enter(c, check_temporal_clip(p, cam, cam_prev, frame_host, prev_host, history_in_host, history_out_host, motion, n_motion, clip));
    if (rc) return rc;
    return temporal_staged(c, p, cam, cam_prev, *frame_host, prev_host, history_in_host, *history_out_host, variance_out_host, motion, n_motion, clip);
}

// ---- motion vectors (include/pbrs_gpu.h, device/temporal.h) ----
namespace {

// The table's copy and the one launch on the context's stream (arguments checked; device pointers, the table host memory).
int motion_vectors_launch(pbrs_ctx* c, uint32_t w, uint32_t h, const pbrs_camera& cam, const pbrs_camera& cam_prev, const float* depth,
                          const uint32_t* instance, const pbrs_instance_motion* motion, uint32_t n_motion, float* motion_out, float* prev_depth_out) {
    TemporalConst k{};
    k.w = w, k.h = h;
    temporal_cameras(k, cam, &cam_prev);
    const pbrs_instance_motion* table = nullptr;
    const int rc = upload_motion_table(c, motion, n_motion, &table);
    if (rc) return rc;
    const uint32_t P = w * h;
    hipLaunchKernelGGL(table ? k_motion_vectors<true> : k_motion_vectors<false>, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, depth,
                       instance, table, table ? n_motion : 0u, motion_out, prev_depth_out, k);
    HIPCHK(c, hipGetLastError());
    return PBRS_OK;
}

}  // namespace

int pbrs_motion_vectors_device(pbrs_ctx* c, uint32_t w, uint32_t h, const pbrs_camera* cam, const pbrs_camera* cam_prev, const float* depth_device,
                               const uint32_t* instance_device, const pbrs_instance_motion* motion, uint32_t n_motion, float* motion_out_device,
                               float* prev_depth_out_device) {
    const int rc = enter(c, check_motion_vectors(w, h, cam, cam_prev, depth_device, instance_device, motion, n_motion, motion_out_device));
    if (rc) return rc;
    return motion_vectors_launch(c, w, h, *cam, *cam_prev, depth_device, instance_device, motion, n_motion, motion_out_device, prev_depth_out_device);
}

int pbrs_motion_vectors(pbrs_ctx* c, uint32_t w, uint32_t h, const pbrs_camera* cam, const pbrs_camera* cam_prev, const float* depth_host,
                        const uint32_t* instance_host, const pbrs_instance_motion* motion, uint32_t n_motion, float* motion_out_host,
                        float* prev_depth_out_host) {
    const int rc = enter(c, check_motion_vectors(w, h, cam, cam_prev, depth_host, instance_host, motion, n_motion, motion_out_host));
    if (rc) return rc;
    const size_t P = (size_t)w * h;
    Staged s[] = {{depth_host, 1}, {instance_host, 1}, {nullptr, 2, motion_out_host}, {nullptr, 1, prev_depth_out_host}};
    return run_staged(c, BUF_MOTION_STAGE, "the motion vectors' staging", s, P, [&] {
        return motion_vectors_launch(c, w, h, *cam, *cam_prev, s[0].as<float>(), s[1].as<uint32_t>(), motion, n_motion, s[2].as<float>(), s[3].as<float>());
    });
}

// ---- spatial variance estimate (include/pbrs_gpu.h, device/spatial_variance.h) ----
static_assert(sizeof(pbrs_spatial_variance_params) == 32, "pbrs_spatial_variance_params is 32 B");
static_assert(PBRS_SPATIAL_MAX_TILE == PBRS_DENOISE_CELL + 2u * PBRS_SPATIAL_MAX_RADIUS, "k_spatial_variance's LDS tile holds the largest halo");

namespace {

using SpatialVarKernel = void (*)(SpatialVarIn, float*, SpatialVarConst);
// [normal stop][id stop]
constexpr SpatialVarKernel kSpatialVar[2][2] = {{k_spatial_variance<false, false>, k_spatial_variance<false, true>},
                                                {k_spatial_variance<true, false>, k_spatial_variance<true, true>}};

// The one launch on the context's stream (arguments checked; device pointers).
int spatial_variance_launch(pbrs_ctx* c, const pbrs_spatial_variance_params& p, const float* moments, const float* length,
                            const pbrs_spatial_variance_guides& g, const float* variance_in, float* variance_out) {
    SpatialVarConst k{};
    k.w = p.w, k.h = p.h, k.radius = p.radius;
    k.only_unknown = (p.flags & PBRS_SPATIAL_ONLY_UNKNOWN) ? 1u : 0u;
    k.in = 1.0f / (p.sigma_normal * p.sigma_normal);
    k.id = 1.0f / (p.sigma_depth * p.sigma_depth);
    k.min_temporal = p.min_temporal;
    const bool ids = (p.flags & PBRS_SPATIAL_ID_STOP) != 0;
    const SpatialVarIn in{moments, length, g.depth, g.normal, ids ? g.instance : nullptr, variance_in};
    const dim3 grid((p.w + PBRS_DENOISE_CELL - 1) / PBRS_DENOISE_CELL, (p.h + PBRS_DENOISE_CELL - 1) / PBRS_DENOISE_CELL);
    hipLaunchKernelGGL(kSpatialVar[g.normal != nullptr][ids], grid, dim3(kBlock), 0, c->stream, in, variance_out, k);
    HIPCHK(c, hipGetLastError());
    return PBRS_OK;
}

}  // namespace

int pbrs_spatial_variance_device(pbrs_ctx* c, const pbrs_spatial_variance_params* p, const float* moments_device, const float* length_device,
                                 const pbrs_spatial_variance_guides* guides_device, const float* variance_in_device, float* variance_out_device) {
    const int rc = enter(c, check_spatial_variance(p, moments_device, length_device, guides_device, variance_in_device, variance_out_device));
    if (rc) return rc;
    return spatial_variance_launch(c, *p, moments_device, length_device, guides_device ? *guides_device : pbrs_spatial_variance_guides{},
                                   variance_in_device, variance_out_device);
}

int pbrs_spatial_variance(pbrs_ctx* c, const pbrs_spatial_variance_params* p, const float* moments_host, const float* length_host,
                          const pbrs_spatial_variance_guides* guides_host, const float* variance_in_host, float* variance_out_host) {
    const int rc = enter(c, check_spatial_variance(p, moments_host, length_host, guides_host, variance_in_host, variance_out_host));
    if (rc) return rc;
    const size_t P = (size_t)p->w * p->h;
    const pbrs_spatial_variance_guides g = guides_host ? *guides_host : pbrs_spatial_variance_guides{};
    // the variance is estimated in place in its staging plane
    Staged s[] = {{moments_host, 2}, {length_host, 1}, {g.depth, 1}, {g.normal, 3}, {g.instance, 1}, {variance_in_host, 1, variance_out_host}};
    return run_staged(c, BUF_SPATIAL_STAGE, "the spatial variance estimate's staging", s, P, [&] {
        const pbrs_spatial_variance_guides gd{s[2].as<float>(), s[3].as<float>(), s[4].as<uint32_t>()};
        return spatial_variance_launch(c, *p, s[0].as<float>(), s[1].as<float>(), gd, s[5].as<float>(), s[5].as<float>());
    });
}

// ---- display transform (include/pbrs_gpu.h, device/display.h) ----
static_assert(sizeof(pbrs_display_params) == 64, "pbrs_display_params is 64 B");
static_assert(PBRS_DISPLAY_BINS == 512u && PBRS_DISPLAY_BINS % 64u == 0, "k_display_resolve holds the bins in one wave, eight per lane");

namespace {

using DisplayApplyKernel = void (*)(const float*, uint32_t*, DisplayApply);
// [curve][encode][both planes 16-byte aligned]
#define PBRS_DISPLAY_ROW(C) {{k_display_apply<C, PBRS_ENCODE_SQRT, false>, k_display_apply<C, PBRS_ENCODE_SQRT, true>}, \
                             {k_display_apply<C, PBRS_ENCODE_SRGB, false>, k_display_apply<C, PBRS_ENCODE_SRGB, true>}}
constexpr DisplayApplyKernel kDisplayApply[3][2][2] = {PBRS_DISPLAY_ROW(PBRS_CURVE_NONE), PBRS_DISPLAY_ROW(PBRS_CURVE_REINHARD), PBRS_DISPLAY_ROW(PBRS_CURVE_ACES)};
#undef PBRS_DISPLAY_ROW

uint32_t display_grid(uint32_t work, uint32_t cap = kDisplayMaxBlocks) { return std::min((work + kDisplayBlock - 1) / kDisplayBlock, cap); }

// The launches on the context's stream (arguments checked; device pointers, `io` by value with NULL for what is not given).  Without the
// auto exposure and without `histogram` (the caller wants the counts) only k_display_apply runs and the scratch is not touched.
int display_launch(pbrs_ctx* c, const pbrs_display_params& p, const float* rgb, const pbrs_display_io& io, uint32_t* out, bool histogram) {
    const uint32_t P = p.w * p.h;
    const bool auto_exposure = (p.flags & PBRS_DISPLAY_AUTO_EXPOSURE) != 0;
    DisplayApply a{};
    a.w = p.w, a.P = P;
    a.scale = p.exposure;  // e = 1
    a.iw2 = 1.0f / (p.white * p.white);
    a.d = p.quantize == PBRS_QUANT_ROUND ? 0.5f : 0.0f;
    a.dither = p.quantize == PBRS_QUANT_DITHER;
    a.exposure_out = io.exposure_out;
    if (auto_exposure || histogram) {
        uint32_t* scratch = c->buf[BUF_DISPLAY].as<uint32_t>();
        HIPCHK(c, hipMemsetAsync(scratch, 0, PBRS_DISPLAY_BINS * sizeof(uint32_t), c->stream));
        const bool rgb_aligned = (reinterpret_cast<uintptr_t>(rgb) & 15u) == 0;
        hipLaunchKernelGGL(rgb_aligned ? k_display_hist<true> : k_display_hist<false>, dim3(display_grid((P + 3u) / 4u, kDisplayHistMaxBlocks)),
                           dim3(kDisplayBlock), 0, c->stream, rgb, P, scratch);
        HIPCHK(c, hipGetLastError());
        float* scale_word = reinterpret_cast<float*>(scratch + kDisplayScaleWord);
        const DisplayResolve r{auto_exposure ? 1u : 0u, p.exposure, p.key, p.min_exposure, p.max_exposure, p.adapt, p.low_q16, p.high_q16,
                               auto_exposure ? io.exposure_in : nullptr, io.exposure_out, io.histogram_out};
        hipLaunchKernelGGL(k_display_resolve, dim3(1), dim3(64), 0, c->stream, scratch, scale_word, r);
        HIPCHK(c, hipGetLastError());
        a.scale_word = scale_word;
        a.exposure_out = nullptr;  // the resolve has written it
    }
    const bool aligned = ((reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
    hipLaunchKernelGGL(kDisplayApply[p.curve][p.encode][aligned], dim3(display_grid((P + 3u) / 4u)), dim3(kDisplayBlock), 0, c->stream, rgb, out, a);
    HIPCHK(c, hipGetLastError());
    return PBRS_OK;
}

// The scratch, for the calls that fill it.
int display_scratch(pbrs_ctx* c, bool needed) {
    return needed ? c->buf[BUF_DISPLAY].grow(c, kDisplayScratchWords * sizeof(uint32_t), "the display transform's histogram") : PBRS_OK;
}

}  // namespace

int pbrs_display_device(pbrs_ctx* c, const pbrs_display_params* p, const float* rgb_device, const pbrs_display_io* io_device, uint32_t* rgba8_out_device) {
    int rc = enter(c, check_display(p, rgb_device, io_device, rgba8_out_device));
    if (rc) return rc;
    const pbrs_display_io io = io_device ? *io_device : pbrs_display_io{};
    if ((rc = display_scratch(c, (p->flags & PBRS_DISPLAY_AUTO_EXPOSURE) || io.histogram_out))) return rc;
    return display_launch(c, *p, rgb_device, io, rgba8_out_device, io.histogram_out != nullptr);
}

int pbrs_display(pbrs_ctx* c, const pbrs_display_params* p, const float* rgb_host, const pbrs_display_io* io_host, uint32_t* rgba8_out_host) {
    int rc = enter(c, check_display(p, rgb_host, io_host, rgba8_out_host));
    if (rc) return rc;
    const pbrs_display_io io = io_host ? *io_host : pbrs_display_io{};
    const bool auto_exposure = (p->flags & PBRS_DISPLAY_AUTO_EXPOSURE) != 0;
    // the io words pass through the scratch: the histogram is copied back from where it was counted
    if ((rc = display_scratch(c, auto_exposure || io.histogram_out || io.exposure_out))) return rc;
    const size_t P = (size_t)p->w * p->h;
    Staged s[] = {{rgb_host, 3}, {nullptr, 1, rgba8_out_host}};
    return run_staged(c, BUF_DISPLAY_STAGE, "the display transform's staging", s, P, [&] {
        uint32_t* scratch = c->buf[BUF_DISPLAY].as<uint32_t>();
        pbrs_display_io iod{};
        if (auto_exposure && io.exposure_in) {
            iod.exposure_in = reinterpret_cast<const float*>(scratch + kDisplayPrevWord);
            HIPCHK(c, hipMemcpyAsync(scratch + kDisplayPrevWord, io.exposure_in, sizeof(float), hipMemcpyHostToDevice, c->stream));
        }
        if (io.exposure_out) iod.exposure_out = reinterpret_cast<float*>(scratch + kDisplayExposureWord);
        const int lrc = display_launch(c, *p, s[0].as<float>(), iod, s[1].as<uint32_t>(), io.histogram_out != nullptr);
        if (lrc) return lrc;
        if (io.exposure_out) HIPCHK(c, hipMemcpyAsync(io.exposure_out, scratch + kDisplayExposureWord, sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (io.histogram_out) HIPCHK(c, hipMemcpyAsync(io.histogram_out, scratch, PBRS_DISPLAY_BINS * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        return (int)PBRS_OK;
    });
}

// ---- guided upsampling (include/pbrs_gpu.h, device/upsample.h) ----
static_assert(sizeof(pbrs_upsample_params) == 48, "pbrs_upsample_params is 48 B");
static_assert(PBRS_UPSAMPLE_MIN_FACTOR == 2u && PBRS_UPSAMPLE_MAX_FACTOR == 4u && PBRS_UPSAMPLE_MAX_RADIUS == 2u, "kUpsample holds every factor and radius");

namespace {

using UpsampleKernel = void (*)(UpsampleIn, float*, float*, UpsampleConst);
// [factor - 2][radius - 1][id stop]
#define PBRS_UPSAMPLE_ROW(F) {{k_upsample<F, 1u, false>, k_upsample<F, 1u, true>}, {k_upsample<F, 2u, false>, k_upsample<F, 2u, true>}}
constexpr UpsampleKernel kUpsample[3][2][2] = {PBRS_UPSAMPLE_ROW(2u), PBRS_UPSAMPLE_ROW(3u), PBRS_UPSAMPLE_ROW(4u)};
#undef PBRS_UPSAMPLE_ROW

// The one launch on the context's stream (arguments checked; device pointers).  A plane the call's flags and pairs leave unread goes to
// the kernel as null.
int upsample_launch(pbrs_ctx* c, const pbrs_upsample_params& p, const float* rgb_lo, const pbrs_denoise_guides& lo, const pbrs_denoise_guides& hi,
                    float* out, float* weight_out) {
    UpsampleConst k{};
    k.w = p.w, k.h = p.h;
    k.wl = (p.w + p.factor - 1) / p.factor, k.hl = (p.h + p.factor - 1) / p.factor;
    k.in = 1.0f / (p.sigma_normal * p.sigma_normal);
    k.id = 1.0f / (p.sigma_depth * p.sigma_depth);
    k.albedo_floor = p.albedo_floor, k.min_weight = p.min_weight;
    const bool demodulate = (p.flags & PBRS_UPSAMPLE_DEMODULATE) != 0, ids = (p.flags & PBRS_UPSAMPLE_ID_STOP) != 0;
    const UpsampleIn in{rgb_lo, demodulate ? lo.albedo : nullptr, lo.normal, lo.depth, ids ? lo.instance : nullptr,
                        demodulate ? hi.albedo : nullptr, hi.normal, hi.depth, ids ? hi.instance : nullptr};
    const dim3 grid((p.w + PBRS_DENOISE_CELL - 1) / PBRS_DENOISE_CELL, (p.h + PBRS_DENOISE_CELL - 1) / PBRS_DENOISE_CELL);
    hipLaunchKernelGGL(kUpsample[p.factor - 2u][p.radius - 1u][ids], grid, dim3(kBlock), 0, c->stream, in, out, weight_out, k);
    HIPCHK(c, hipGetLastError());
    return PBRS_OK;
}

}  // namespace

int pbrs_upsample_device(pbrs_ctx* c, const pbrs_upsample_params* p, const float* rgb_lo_device, const pbrs_denoise_guides* guides_lo_device,
                         const pbrs_denoise_guides* guides_hi_device, float* out_device, float* weight_out_device) {
    const int rc = enter(c, check_upsample(p, rgb_lo_device, guides_lo_device, guides_hi_device, out_device, weight_out_device));
    if (rc) return rc;
    return upsample_launch(c, *p, rgb_lo_device, *guides_lo_device, *guides_hi_device, out_device, weight_out_device);
}

int pbrs_upsample(pbrs_ctx* c, const pbrs_upsample_params* p, const float* rgb_lo_host, const pbrs_denoise_guides* guides_lo_host,
                  const pbrs_denoise_guides* guides_hi_host, float* out_host, float* weight_out_host) {
    const int rc = enter(c, check_upsample(p, rgb_lo_host, guides_lo_host, guides_hi_host, out_host, weight_out_host));
    if (rc) return rc;
    const size_t P = (size_t)p->w * p->h;
    const size_t Pl = (size_t)((p->w + p->factor - 1) / p->factor) * ((p->h + p->factor - 1) / p->factor);
    const pbrs_denoise_guides &lo = *guides_lo_host, &hi = *guides_hi_host;
    Staged s[] = {{rgb_lo_host, 3, nullptr, nullptr, Pl}, {lo.albedo, 3, nullptr, nullptr, Pl}, {lo.normal, 3, nullptr, nullptr, Pl},
                  {lo.depth, 1, nullptr, nullptr, Pl},    {lo.instance, 1, nullptr, nullptr, Pl},
                  {hi.albedo, 3}, {hi.normal, 3}, {hi.depth, 1}, {hi.instance, 1}, {nullptr, 3, out_host}, {nullptr, 1, weight_out_host}};
    return run_staged(c, BUF_UPSAMPLE_STAGE, "the guided upsampling's staging", s, P, [&] {
        const pbrs_denoise_guides lod{s[1].as<float>(), s[2].as<float>(), s[3].as<float>(), s[4].as<uint32_t>()};
        const pbrs_denoise_guides hid{s[5].as<float>(), s[6].as<float>(), s[7].as<float>(), s[8].as<uint32_t>()};
        return upsample_launch(c, *p, s[0].as<float>(), lod, hid, s[9].as<float>(), s[10].as<float>());
    });
}

// ---- image comparison (include/pbrs_gpu.h, device/compare.h) ----
static_assert(sizeof(pbrs_compare_params) == 32, "pbrs_compare_params is 32 B");
static_assert(sizeof(pbrs_compare_result) == 64 && offsetof(pbrs_compare_result, n_valid) == 40, "pbrs_compare_result is 64 B");

namespace {

using CompareKernel = void (*)(const float*, const float*, CompareRecords, CompareConst);
// [transform][ssim]
constexpr CompareKernel kCompare[2][2] = {{k_compare_tile<PBRS_COMPARE_LINEAR, false>, k_compare_tile<PBRS_COMPARE_LINEAR, true>},
                                          {k_compare_tile<PBRS_COMPARE_REINHARD, false>, k_compare_tile<PBRS_COMPARE_REINHARD, true>}};

uint32_t compare_tiles(uint32_t extent) { return (extent + PBRS_COMPARE_TILE - 1u) / PBRS_COMPARE_TILE; }

// The scratch of a call with n tiles: n records, then the (n + 3) / 4 of k_compare_finish's second buffer.  A planar record is 52 B (five
// f64 sums, three u32 counts); each buffer gets 64 B per record, which keeps the second one's f64 planes aligned.
constexpr size_t kCompareRecordBytes = 64;
uint32_t compare_quarter(uint32_t n) { return (n + 3u) / 4u; }
size_t compare_scratch_bytes(uint32_t n) { return kCompareRecordBytes * ((size_t)n + compare_quarter(n)); }

int compare_scratch(pbrs_ctx* c, const pbrs_compare_params& p) {
    return c->buf[BUF_COMPARE].grow(c, compare_scratch_bytes(compare_tiles(p.w) * compare_tiles(p.h)), "the comparison's tile sums");
}

// The two launches on the context's stream (arguments checked, the scratch grown; device pointers, `maps` by value with NULL for what is
// not wanted).
int compare_launch(pbrs_ctx* c, const pbrs_compare_params& p, const float* a, const float* b, const pbrs_compare_maps& maps, pbrs_compare_result* result) {
    const bool ssim = (p.flags & PBRS_COMPARE_SSIM) != 0;
    const uint32_t tiles_x = compare_tiles(p.w), n = tiles_x * compare_tiles(p.h);  // at most 2^28 pixels: at most 2^28 tiles
    // the layout compare_scratch_bytes sizes: in each buffer the five f64 planes, then the three u32 planes
    char* base = c->buf[BUF_COMPARE].as<char>();
    const uint32_t n2 = compare_quarter(n);
    const CompareRecords tiles{reinterpret_cast<double*>(base), reinterpret_cast<uint32_t*>(base + 40 * (size_t)n), n};
    char* base2 = base + kCompareRecordBytes * (size_t)n;
    const CompareRecords halved{reinterpret_cast<double*>(base2), reinterpret_cast<uint32_t*>(base2 + 40 * (size_t)n2), n2};
    const CompareConst k{p.w, p.h, tiles_x, p.peak, (double)p.rel_epsilon, maps.error_out, ssim ? maps.ssim_out : nullptr};
    hipLaunchKernelGGL(kCompare[p.transform][ssim], dim3(n), dim3(kCompareBlock), 0, c->stream, a, b, tiles, k);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_compare_finish, dim3(1), dim3(kCompareFinishBlock), 0, c->stream, tiles, halved, n, ssim ? 1u : 0u, result);
    HIPCHK(c, hipGetLastError());
    return PBRS_OK;
}

}  // namespace

int pbrsx_compare_device(pbrs_ctx* c, const pbrs_compare_params* p, const float* a_device, const float* b_device, const pbrs_compare_maps* maps_device,
                        pbrs_compare_result* result_device) {
    int rc = enter(c, check_compare(p, a_device, b_device, maps_device, result_device));
    if (rc) return rc;
    if ((rc = compare_scratch(c, *p))) return rc;
    return compare_launch(c, *p, a_device, b_device, maps_device ? *maps_device : pbrs_compare_maps{}, result_device);
}

int pbrsx_compare(pbrs_ctx* c, const pbrs_compare_params* p, const float* a_host, const float* b_host, const pbrs_compare_maps* maps_host,
                 pbrs_compare_result* result_host) {
    int rc = enter(c, check_compare(p, a_host, b_host, maps_host, result_host));
    if (rc) return rc;
    if ((rc = compare_scratch(c, *p))) return rc;
    const pbrs_compare_maps maps = maps_host ? *maps_host : pbrs_compare_maps{};
    const size_t P = (size_t)p->w * p->h;
    Staged s[] = {{a_host, 3}, {b_host, 3}, {nullptr, 1, maps.error_out}, {nullptr, 1, maps.ssim_out},
                  {nullptr, sizeof(pbrs_compare_result) / sizeof(uint32_t), result_host, nullptr, 1}};
    return run_staged(c, BUF_COMPARE_STAGE, "the comparison's staging", s, P, [&] {
        return compare_launch(c, *p, s[0].as<float>(), s[1].as<float>(), pbrs_compare_maps{s[2].as<float>(), s[3].as<float>()}, s[4].as<pbrs_compare_result>());
    });
}

// ---- despeckle (include/pbrs_gpu.h, device/despeckle.h) ----
static_assert(sizeof(pbrs_despeckle_params) == 32, "pbrs_despeckle_params is 32 B");
static_assert(sizeof(pbrs_despeckle_result) == 16 && offsetof(pbrs_despeckle_result, n_repaired) == 4, "pbrs_despeckle_result is 16 B");
static_assert(PBRS_DESPECKLE_MAX_RADIUS == 2u && PBRS_DESPECKLE_MAX_RANK == 4u, "kDespeckle holds every radius; k_despeckle keeps four taps");

namespace {

using DespeckleKernel = void (*)(DespeckleConst);
// [radius - 1]
constexpr DespeckleKernel kDespeckle[2] = {k_despeckle<1u>, k_despeckle<2u>};

uint32_t despeckle_tiles(uint32_t extent) { return (extent + PBRS_DESPECKLE_TILE - 1u) / PBRS_DESPECKLE_TILE; }

// The launches on the context's stream (arguments checked; device pointers, NULL for what is not wanted): the image kernel and, where
// the record is wanted, the finish over the blocks' counts, whose scratch the first such call allocates.
int despeckle_launch(pbrs_ctx* c, const pbrs_despeckle_params& p, const pbrs_despeckle_io& io, pbrs_despeckle_result* result) {
    const uint32_t tiles_x = despeckle_tiles(p.w), n = tiles_x * despeckle_tiles(p.h);  // at most 2^28 pixels: at most 2^28 tiles
    const uint32_t blocks = std::min(n, kDespeckleMaxBlocks);
    uint32_t* block_counts = nullptr;
    if (result) {
        const int rc = c->buf[BUF_DESPECKLE].grow(c, 2 * sizeof(uint32_t) * kDespeckleMaxBlocks, "the despeckle blocks' counts");
        if (rc) return rc;
        block_counts = c->buf[BUF_DESPECKLE].as<uint32_t>();
    }
    const DespeckleConst k{p.w, p.h, tiles_x, n, p.rank, p.gain, p.floor, io.rgb_in, io.rgb_out, reinterpret_cast<const uint32_t*>(io.variance_in),
                           reinterpret_cast<uint32_t*>(io.variance_out), io.mask_out, io.removed_out, block_counts};
    hipLaunchKernelGGL(kDespeckle[p.radius - 1u], dim3(blocks), dim3(kDespeckleBlock), 0, c->stream, k);
    HIPCHK(c, hipGetLastError());
    if (result) {
        hipLaunchKernelGGL(k_despeckle_finish, dim3(1), dim3(256), 0, c->stream, block_counts, blocks, result);
        HIPCHK(c, hipGetLastError());
    }
    return PBRS_OK;
}

}  // namespace

int pbrsi_despeckle_device(pbrs_ctx* c, const pbrs_despeckle_params* p, const pbrs_despeckle_io* io_device, pbrs_despeckle_result* result_device) {
    const int rc = enter(c, check_despeckle(p, io_device));
    if (rc) return rc;
    return despeckle_launch(c, *p, *io_device, result_device);
}

int pbrsi_despeckle(pbrs_ctx* c, const pbrs_despeckle_params* p, const pbrs_despeckle_io* io_host, pbrs_despeckle_result* result_host) {
    const int rc = enter(c, check_despeckle(p, io_host));
    if (rc) return rc;
    const pbrs_despeckle_io& io = *io_host;
    const size_t P = (size_t)p->w * p->h;
    Staged s[] = {{io.rgb_in, 3}, {io.variance_in, 1, io.variance_out}, {nullptr, 3, io.rgb_out}, {nullptr, 1, io.mask_out}, {nullptr, 3, io.removed_out},
                  {nullptr, sizeof(pbrs_despeckle_result) / sizeof(uint32_t), result_host, nullptr, 1}};
    return run_staged(c, BUF_DESPECKLE_STAGE, "the despeckle staging", s, P, [&] {
        return despeckle_launch(c, *p, pbrs_despeckle_io{s[0].as<float>(), s[2].as<float>(), s[1].as<float>(), s[1].as<float>(), s[3].as<uint32_t>(), s[4].as<float>()},
                                s[5].as<pbrs_despeckle_result>());
    });
}

// ---- bloom (include/pbrs_gpu.h, device/bloom.h) ----
static_assert(sizeof(pbrs_bloom_params) == 32 && offsetof(pbrs_bloom_params, threshold) == 16, "pbrs_bloom_params is 32 B");

namespace {

using BloomDownKernel = void (*)(BloomDown);
using BloomCompositeKernel = void (*)(BloomComposite);
// a level's source; the image through a scalar path; the image through 16-byte loads
constexpr BloomDownKernel kBloomDown[3] = {k_bloom_down<false, false>, k_bloom_down<true, false>, k_bloom_down<true, true>};
// [PBRS_BLOOM_MIX][both planes 16-byte aligned]
constexpr BloomCompositeKernel kBloomComposite[2][2] = {{k_bloom_composite<false, false>, k_bloom_composite<false, true>},
                                                        {k_bloom_composite<true, false>, k_bloom_composite<true, true>}};

// The launches on the context's stream (arguments checked; device pointers).  PBRS_BLOOM_NO_TAIL (a developer build's define, for
// tools/bloom_cost.py) takes every level through k_bloom_down and k_bloom_up; the bits are the same.
int bloom_launch(pbrs_ctx* c, const pbrs_bloom_params& p, const float* rgb, float* out) {
    const size_t P = (size_t)p.w * p.h;
    if (p.strength == 0.0f) {  // the input's bits
        if (out != rgb) HIPCHK(c, hipMemcpyAsync(out, rgb, 3 * P * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        return PBRS_OK;
    }
    uint32_t lw[PBRS_BLOOM_MAX_LEVELS], lh[PBRS_BLOOM_MAX_LEVELS];
    size_t first[PBRS_BLOOM_MAX_LEVELS + 1];  // a level's first pixel in the chain; [N]: the chain's pixels
    uint32_t N = 0;
    first[0] = 0;
    for (uint32_t w = p.w, h = p.h; N < p.levels;) {
        w = (w + 1u) / 2u, h = (h + 1u) / 2u;
        lw[N] = w, lh[N] = h;
        first[N + 1] = first[N] + (size_t)w * h;
        ++N;
        if (w == 1u && h == 1u) break;
    }
    const int rc = c->buf[BUF_BLOOM].grow(c, first[N] * sizeof(float4), "the bloom pyramid");
    if (rc) return rc;
    float4* const chain = c->buf[BUF_BLOOM].as<float4>();
    // the level at which k_bloom_tail takes over: the first one that fits its LDS with every level below it; N - 1 where it would have
    // nothing to do (the last level is its own u)
    uint32_t T = 0;
#ifdef PBRS_BLOOM_NO_TAIL
    T = N - 1u;
#else
    while (T < N - 1u && first[N] - first[T] > kBloomTailPixels) ++T;
#endif
    const float k = p.threshold * p.knee;
    BloomDown d{};
    d.bright = BloomBright{p.threshold, k, p.threshold - k, p.threshold + k, 1.0f / (4.0f * k)};
    for (uint32_t l = 0; l <= T; ++l) {
        d.rgb = l ? nullptr : rgb, d.src = l ? chain + first[l - 1] : nullptr, d.dst = chain + first[l];
        d.sw = l ? lw[l - 1] : p.w, d.sh = l ? lh[l - 1] : p.h, d.dw = lw[l], d.dh = lh[l];
        d.tiles_x = (d.dw + kBloomTile - 1u) / kBloomTile;
        const uint32_t tiles = d.tiles_x * ((d.dh + kBloomTile - 1u) / kBloomTile);  // at most 2^26 pixels: at most 2^26 tiles
        const bool aligned = (reinterpret_cast<uintptr_t>(rgb) & 15u) == 0;
        hipLaunchKernelGGL(kBloomDown[l ? 0 : (aligned ? 2 : 1)], dim3(tiles), dim3(kBloomBlock), 0, c->stream, d);
        HIPCHK(c, hipGetLastError());
    }
    if (T < N - 1u) {
        hipLaunchKernelGGL(k_bloom_tail, dim3(1), dim3(kBloomTailBlock), 0, c->stream, BloomTail{chain + first[T], lw[T], lh[T], N - T, p.spread});
        HIPCHK(c, hipGetLastError());
    }
    for (uint32_t l = T; l-- > 0;) {
        const uint32_t n = lw[l] * lh[l];
        hipLaunchKernelGGL(k_bloom_up, dim3((n + kBloomBlock - 1u) / kBloomBlock), dim3(kBloomBlock), 0, c->stream,
                           BloomUp{chain + first[l + 1], chain + first[l], lw[l + 1], lh[l + 1], lw[l], lh[l], p.spread});
        HIPCHK(c, hipGetLastError());
    }
    const BloomComposite b{rgb, out, chain, p.w, (uint32_t)P, lw[0], lh[0], p.strength};
    const bool aligned = ((reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
    const bool mix = (p.flags & PBRS_BLOOM_MIX) != 0;
    const uint32_t groups = (uint32_t)((P + 3u) / 4u);
    hipLaunchKernelGGL(kBloomComposite[mix][aligned], dim3((groups + kBloomBlock - 1u) / kBloomBlock), dim3(kBloomBlock), 0, c->stream, b);
    HIPCHK(c, hipGetLastError());
    return PBRS_OK;
}

}  // namespace

int pbrsb_bloom_device(pbrs_ctx* c, const pbrs_bloom_params* p, const float* rgb_device, float* rgb_out_device) {
    const int rc = enter(c, check_bloom(p, rgb_device, rgb_out_device));
    if (rc) return rc;
    return bloom_launch(c, *p, rgb_device, rgb_out_device);
}

int pbrsb_bloom(pbrs_ctx* c, const pbrs_bloom_params* p, const float* rgb_host, float* rgb_out_host) {
    const int rc = enter(c, check_bloom(p, rgb_host, rgb_out_host));
    if (rc) return rc;
    Staged s[] = {{rgb_host, 3, rgb_out_host}};  // in place on the staged image
    return run_staged(c, BUF_BLOOM_STAGE, "the bloom staging", s, (size_t)p->w * p->h, [&] { return bloom_launch(c, *p, s[0].as<float>(), s[0].as<float>()); });
}

// ---- depth of field (include/pbrs_gpu.h, device/dof.h) ----
static_assert(sizeof(pbrs_dof_params) == 32 && offsetof(pbrs_dof_params, focus) == 16 && offsetof(pbrs_dof_params, reserved) == 24, "pbrs_dof_params is 32 B");

namespace {

using DofKernel = void (*)(Dof);
// [halo class: 4, 8, 16][both planes 16-byte aligned]
constexpr DofKernel kDof[3][2] = {{k_dof<4u, false>, k_dof<4u, true>}, {k_dof<8u, false>, k_dof<8u, true>}, {k_dof<16u, false>, k_dof<16u, true>}};
static_assert(PBRS_DOF_MAX_RADIUS == 16u, "the halo classes end at the largest radius");

// The one launch on the context's stream (arguments checked; device pointers).  scale 0 is the header's step 0: a copy.
int dof_launch(pbrs_ctx* c, const pbrs_dof_params& p, const float* rgb, const float* depth, float* out, float* coc) {
    const size_t P = (size_t)p.w * p.h;
    if (p.scale == 0.0f) {
        HIPCHK(c, hipMemcpyAsync(out, rgb, 3 * P * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        if (coc) HIPCHK(c, hipMemsetAsync(coc, 0, P * sizeof(float), c->stream));
        return PBRS_OK;
    }
    const uint32_t tiles_x = (p.w + kDofTile - 1u) / kDofTile;
    const uint32_t tiles = tiles_x * ((p.h + kDofTile - 1u) / kDofTile);  // at most 2^28 pixels: at most 2^28 tiles
    const uint32_t halo = p.max_radius <= 4u ? 0u : (p.max_radius <= 8u ? 1u : 2u);  // the smallest class that holds max_radius
    const bool aligned = ((reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(depth)) & 15u) == 0;
    hipLaunchKernelGGL(kDof[halo][aligned], dim3(tiles), dim3(kDofBlock), 0, c->stream, Dof{rgb, depth, out, coc, p.w, p.h, tiles_x, p.max_radius, p.focus, p.scale});
    HIPCHK(c, hipGetLastError());
    return PBRS_OK;
}

}  // namespace

int pbrsf_dof_device(pbrs_ctx* c, const pbrs_dof_params* p, const float* rgb_device, const float* depth_device, float* rgb_out_device, float* coc_out_device) {
    const int rc = enter(c, check_dof(p, rgb_device, depth_device, rgb_out_device));
    if (rc) return rc;
    return dof_launch(c, *p, rgb_device, depth_device, rgb_out_device, coc_out_device);
}

int pbrsf_dof(pbrs_ctx* c, const pbrs_dof_params* p, const float* rgb_host, const float* depth_host, float* rgb_out_host, float* coc_out_host) {
    const int rc = enter(c, check_dof(p, rgb_host, depth_host, rgb_out_host));
    if (rc) return rc;
    Staged s[] = {{rgb_host, 3}, {depth_host, 1}, {nullptr, 3, rgb_out_host}, {nullptr, 1, coc_out_host}};
    return run_staged(c, BUF_DOF_STAGE, "the depth of field staging", s, (size_t)p->w * p->h,
                      [&] { return dof_launch(c, *p, s[0].as<float>(), s[1].as<float>(), s[2].as<float>(), s[3].as<float>()); });
}

// ---- motion blur (include/pbrs_gpu.h, device/motion_blur.h) ----
static_assert(sizeof(pbrs_motion_blur_params) == 32 && offsetof(pbrs_motion_blur_params, shutter) == 20 && offsetof(pbrs_motion_blur_params, reserved) == 28,
              "pbrs_motion_blur_params is 32 B");

namespace {

using MotionBlurKernel = void (*)(MotionBlur);
// [halo class: 4, 8, 16][rgb and depth 16-byte aligned][PBRS_MOTION_BLUR_JITTER]
constexpr MotionBlurKernel kMotionBlur[3][2][2] = {
    {{k_motion_blur<4u, false, false>, k_motion_blur<4u, false, true>}, {k_motion_blur<4u, true, false>, k_motion_blur<4u, true, true>}},
    {{k_motion_blur<8u, false, false>, k_motion_blur<8u, false, true>}, {k_motion_blur<8u, true, false>, k_motion_blur<8u, true, true>}},
    {{k_motion_blur<16u, false, false>, k_motion_blur<16u, false, true>}, {k_motion_blur<16u, true, false>, k_motion_blur<16u, true, true>}}};
static_assert(PBRS_MOTION_BLUR_MAX_RADIUS == 16u, "the halo classes end at the largest radius");

// The one launch on the context's stream (arguments checked; device pointers).  shutter 0 is the header's step 0: a copy.
int motion_blur_launch(pbrs_ctx* c, const pbrs_motion_blur_params& p, const float* rgb, const float* depth, const float* motion, float* out, float* velocity) {
    const size_t P = (size_t)p.w * p.h;
    if (p.shutter == 0.0f) {
        HIPCHK(c, hipMemcpyAsync(out, rgb, 3 * P * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        if (velocity) HIPCHK(c, hipMemsetAsync(velocity, 0, 2 * P * sizeof(float), c->stream));
        return PBRS_OK;
    }
    const uint32_t tiles_x = (p.w + kMotionBlurTile - 1u) / kMotionBlurTile;
    const uint32_t tiles = tiles_x * ((p.h + kMotionBlurTile - 1u) / kMotionBlurTile);  // at most 2^28 pixels: at most 2^28 tiles
    const uint32_t halo = p.max_radius <= 4u ? 0u : (p.max_radius <= 8u ? 1u : 2u);    // the smallest class that holds max_radius
    const bool aligned = ((reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(depth)) & 15u) == 0;
    const bool jitter = (p.flags & PBRS_MOTION_BLUR_JITTER) != 0u;
    hipLaunchKernelGGL(kMotionBlur[halo][aligned][jitter], dim3(tiles), dim3(kMotionBlurBlock), 0, c->stream,
                       MotionBlur{rgb, depth, motion, out, velocity, p.w, p.h, tiles_x, p.max_radius, p.taps, p.shutter * 0.5f, p.z_rel});
    HIPCHK(c, hipGetLastError());
    return PBRS_OK;
}

}  // namespace

int pbrsm_motion_blur_device(pbrs_ctx* c, const pbrs_motion_blur_params* p, const float* rgb_device, const float* depth_device, const float* motion_device,
                             float* rgb_out_device, float* velocity_out_device) {
    const int rc = enter(c, check_motion_blur(p, rgb_device, depth_device, motion_device, rgb_out_device));
    if (rc) return rc;
    return motion_blur_launch(c, *p, rgb_device, depth_device, motion_device, rgb_out_device, velocity_out_device);
}

int pbrsm_motion_blur(pbrs_ctx* c, const pbrs_motion_blur_params* p, const float* rgb_host, const float* depth_host, const float* motion_host, float* rgb_out_host,
                      float* velocity_out_host) {
    const int rc = enter(c, check_motion_blur(p, rgb_host, depth_host, motion_host, rgb_out_host));
    if (rc) return rc;
    Staged s[] = {{rgb_host, 3}, {depth_host, 1}, {motion_host, 2}, {nullptr, 3, rgb_out_host}, {nullptr, 2, velocity_out_host}};
    return run_staged(c, BUF_MOTION_BLUR_STAGE, "the motion blur staging", s, (size_t)p->w * p->h,
                      [&] { return motion_blur_launch(c, *p, s[0].as<float>(), s[1].as<float>(), s[2].as<float>(), s[3].as<float>(), s[4].as<float>()); });
}

int pbrs_collect_stats(pbrs_ctx* c, pbrs_stats* stats_out) {
    if (!c) return PBRS_E_INVALID;
    return collect(c, stats_out);
}

int pbrs_intersect_rays(pbrs_ctx* c, uint32_t n, const float* origins, const float* dirs, const float* tmax, pbrs_hit_record* hits_out,
                        uint8_t* occluded_out) {
    if (!c) return PBRS_E_INVALID;
    if (!c->has_scene) return fail(c, PBRS_E_NO_SCENE, "no scene uploaded");
    if (n == 0) return PBRS_OK;
    if (!origins || !dirs || !tmax) return fail(c, PBRS_E_INVALID, "null ray arrays");
    HIPCHK(c, hipSetDevice(c->device));
    float4 *d_o = nullptr, *d_d = nullptr;
    float* d_t = nullptr;
    pbrs_hit_record* d_h = nullptr;
    uint8_t* d_occ = nullptr;
    uint32_t* d_info = nullptr;
    CallAllocs mem;
    // rays travel as 16-byte records, the form the walks re-read their ray in (traverse.h, reload_world)
    std::vector<float4> h_o(n), h_d(n);
    for (uint32_t i = 0; i < n; ++i) {
        h_o[i] = make_float4(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2], 0.0f);
        h_d[i] = make_float4(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], 0.0f);
    }
    HIPCHK(c, mem.alloc(&d_o, (size_t)n * 16));
    HIPCHK(c, mem.alloc(&d_d, (size_t)n * 16));
    HIPCHK(c, mem.alloc(&d_t, (size_t)n * 4));
    if (hits_out) HIPCHK(c, mem.alloc(&d_h, (size_t)n * sizeof(pbrs_hit_record)));
    if (occluded_out) HIPCHK(c, mem.alloc(&d_occ, (size_t)n));
    HIPCHK(c, mem.alloc(&d_info, 2 * sizeof(uint32_t)));
    HIPCHK(c, hipMemsetAsync(d_info, 0, 2 * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemcpyAsync(d_o, h_o.data(), (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_d, h_d.data(), (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_t, tmax, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    {
        // the walks the pipeline runs for this scene: any-hit over four-wide nodes where k_shadow walks them (the binary walk takes
        // what that one refuses, as in the pipeline), else the binary walks
        const uint32_t rows = std::max(c->stack_depth, c->S.wide_cap);
        const size_t lds = (size_t)(rows + c->S.n_flat) * kBlock * sizeof(uint32_t);
        const dim3 grid(std::min<uint32_t>((n + kBlock - 1) / kBlock, kPersistentBlocks));
        // each query through the walk its stage runs in the pipeline (KernelPlan): occlusion through the four-wide any-hit walk whenever
        // k_shadow takes it, closest hits through the binary walk
        const bool wide = c->plan.choice.wide_shadow;
        c->last_intersect = pbrs_intersect_info{wide ? 1u : 0u, 0u, 0u, 0u};
        hipLaunchKernelGGL(intersect_fn(wide), grid, dim3(kBlock), lds, c->stream, c->S, n, d_o, d_d, d_t, d_h, d_occ, d_info);
    }
    HIPCHK(c, hipGetLastError());
    if (hits_out) HIPCHK(c, hipMemcpyAsync(hits_out, d_h, (size_t)n * sizeof(pbrs_hit_record), hipMemcpyDeviceToHost, c->stream));
    if (occluded_out) HIPCHK(c, hipMemcpyAsync(occluded_out, d_occ, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    uint32_t slow[2] = {0u, 0u};
    HIPCHK(c, hipMemcpyAsync(slow, d_info, sizeof slow, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->last_intersect.slow_any = slow[0];
    c->last_intersect.slow_closest = slow[1];
    return PBRS_OK;
}

int pbrs_last_intersect_info(const pbrs_ctx* c, pbrs_intersect_info* out) {
    if (!c || !out) return PBRS_E_INVALID;
    *out = c->last_intersect;
    return PBRS_OK;
}

int pbrs_camera_rays(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, uint32_t sample_index, float* origins_out, float* dirs_out) {
    if (!c) return PBRS_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = fail(c, check_params(scene_state(c), cam, p));
    if (rc) return rc;
    if (!origins_out || !dirs_out) return fail(c, PBRS_E_INVALID, "null output");
    const uint32_t P = p->w * p->h;
    uint32_t K;
    if ((rc = pass_size(c, p, K))) return rc;  // (the render's limit; one sample index here)
    rc = ensure_work(c, cur(c), P, P);
    if (rc) return rc;
    RenderConst k = make_const(c, cam, p);
    k.tiles8_per_row = 0u;  // one sample index, exported by pixel: slot = pixel
    k.pass_first_sample = sample_index;
    k.n_slots = P;
    hipLaunchKernelGGL(k_raygen, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, cur(c).st, k, cur(c).rng_hi0);  // (the rays are read back, nothing else)
    float *d_o = nullptr, *d_d = nullptr;
    CallAllocs mem;
    HIPCHK(c, mem.alloc(&d_o, (size_t)P * 12));
    HIPCHK(c, mem.alloc(&d_d, (size_t)P * 12));
    hipLaunchKernelGGL(k_export_rays, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, cur(c).st, P, d_o, d_d);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(origins_out, d_o, (size_t)P * 12, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dirs_out, d_d, (size_t)P * 12, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PBRS_OK;
}

int pbrs_numeric_eval(pbrs_ctx* c, uint32_t fn, uint32_t n, const float* x, const float* y, float* out) {
    if (!c) return PBRS_E_INVALID;
    if (n == 0) return PBRS_OK;
    if (!x || !out || fn > PN_PROBE_LAST) return fail(c, PBRS_E_INVALID, "bad numeric_eval arguments");
    HIPCHK(c, hipSetDevice(c->device));
    float *d_x = nullptr, *d_y = nullptr, *d_r = nullptr;
    CallAllocs mem;
    HIPCHK(c, mem.alloc(&d_x, (size_t)n * 4));
    HIPCHK(c, mem.alloc(&d_r, (size_t)n * 4));
    HIPCHK(c, hipMemcpyAsync(d_x, x, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (y) {
        HIPCHK(c, mem.alloc(&d_y, (size_t)n * 4));
        HIPCHK(c, hipMemcpyAsync(d_y, y, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    }
    hipLaunchKernelGGL(k_numeric_eval, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, fn, n, d_x, d_y, d_r);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, d_r, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PBRS_OK;
}

int pbrs_numeric_eval_k(pbrs_ctx* c, uint32_t fn, uint32_t n, uint32_t k, const uint32_t* ops, uint32_t* out) {
    if (!c) return PBRS_E_INVALID;
    if (n == 0) return PBRS_OK;
    if (!ops || !out || fn > PN_PROBE_K_LAST || k > PN_PROBE_MAX_K || k < pn_probe_k_operands(fn))
        return fail(c, PBRS_E_INVALID, "bad numeric_eval_k arguments");
    HIPCHK(c, hipSetDevice(c->device));
    uint32_t *d_ops = nullptr, *d_r = nullptr;
    CallAllocs mem;
    HIPCHK(c, mem.alloc(&d_ops, (size_t)n * k * 4));
    HIPCHK(c, mem.alloc(&d_r, (size_t)n * 4));
    HIPCHK(c, hipMemcpyAsync(d_ops, ops, (size_t)n * k * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_numeric_eval_k, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, fn, n, k, d_ops, d_r);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, d_r, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PBRS_OK;
}

int pbrs_bsdf_eval(pbrs_ctx* c, uint32_t op, uint32_t lambert, uint32_t n, const uint32_t* queries, uint32_t* results) {
    if (!c) return PBRS_E_INVALID;
    if (n == 0) return PBRS_OK;
    if (!c->has_scene) return fail(c, PBRS_E_INVALID, "bsdf_eval: no scene uploaded");
    if (!queries || !results) return fail(c, PBRS_E_INVALID, "bsdf_eval: null queries or results");
    if (op > PBRS_BSDF_SAMPLE_SPECULAR) return fail(c, PBRS_E_INVALID, "bsdf_eval: unknown op");
    if (lambert && !c->lambert_scene) return fail(c, PBRS_E_INVALID, "bsdf_eval: the Lambert variant needs a scene whose every lobe is an untextured Lambertian");
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t m = queries[(size_t)i * PBRS_BSDF_QUERY_WORDS];
        if (m >= c->material_flags.size()) return fail(c, PBRS_E_INVALID, "bsdf_eval: material index out of range");
        if (c->material_flags[m] & PBRS_MATERIAL_TEXTURED)
            return fail(c, PBRS_E_INVALID, "bsdf_eval: textured materials are out of scope (a query carries no uv or position)");
        if (op == PBRS_BSDF_SAMPLE) {  // bsdf_sample_l picks lobe (uint32_t)(u * n): k_shade's u comes from the RNG, below 1; this one from the caller
            float u;
            std::memcpy(&u, queries + (size_t)i * PBRS_BSDF_QUERY_WORDS + 13, sizeof u);
            if (!(u >= 0.0f && u < 1.0f)) return fail(c, PBRS_E_INVALID, "bsdf_eval: u outside [0, 1) would pick a lobe the material does not have");
        }
    }
    const bsdf_eval_fn_t fn = bsdf_eval_fn(lambert != 0, c->fourier_scene);
    if (!fn) return fail(c, PBRS_E_DEVICE, "bsdf_eval: no kernel instantiation for this scene");
    HIPCHK(c, hipSetDevice(c->device));
    uint32_t *d_q = nullptr, *d_r = nullptr;
    CallAllocs mem;
    const size_t q_bytes = (size_t)n * PBRS_BSDF_QUERY_WORDS * 4, r_bytes = (size_t)n * PBRS_BSDF_RESULT_WORDS * 4;
    HIPCHK(c, mem.alloc(&d_q, q_bytes));
    HIPCHK(c, mem.alloc(&d_r, r_bytes));
    HIPCHK(c, hipMemcpyAsync(d_q, queries, q_bytes, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(fn, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, c->S, op, n, d_q, d_r);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(results, d_r, r_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PBRS_OK;
}

int pbrs_render_sample_radiance(pbrs_ctx* c, const pbrs_camera* cam, const pbrs_render_params* p, uint32_t sample_index, float* rgb_out_host) {
    if (!c) return PBRS_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = fail(c, check_params(scene_state(c), cam, p));
    if (rc) return rc;
    if (!rgb_out_host) return fail(c, PBRS_E_INVALID, "null output");
    const uint32_t P = p->w * p->h;
    uint32_t K;
    if ((rc = pass_size(c, p, K))) return rc;  // (the render's limit; one sample index here)
    rc = ensure_work(c, cur(c), P, P);
    if (rc) return rc;
    RenderConst k = make_const(c, cam, p);
    k.tiles8_per_row = 0u;  // one sample index, exported by pixel: slot = pixel
    Timer tm{c, false};
    HIPCHK(c, hipMemsetAsync(c->sum, 0, 3 * (size_t)P * sizeof(float), c->stream));
    c->entry_table = nullptr;  // (no pre-pass here: every ray walks from the root)
    rc = run_pass(c, k, sample_index, 1, false, tm, false, RenderTargets{});
    if (rc) return rc;
    hipLaunchKernelGGL(k_export_radiance, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, cur(c).st, P, c->rgb_dev);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(rgb_out_host, c->rgb_dev, 3 * (size_t)P * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PBRS_OK;
}

}  // extern "C"
