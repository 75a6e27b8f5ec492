// device/extend.h — the extend stage (device/kernels.h): k_extend, and what the traversal kernels share (k_shadow: device/shadow.h):
// the round of the traversal loop, the waves' work fetch, the slow list and the scene staging in LDS.
#pragma once
#include "path_state.h"
#include "traverse.h"

template <bool STATS>
PD void flush_counters(const Cnt<STATS>& cnt, GlobalCounters* g, bool valid, uint32_t rays, uint32_t hits) {
    if (!STATS) return;
    const WorkCounters& c = cnt.c;
    uint32_t v[12] = {c.tlas_nodes, c.blas_nodes, c.instances, c.instance_hits, c.triangles, c.tri_shading,
                      c.spheres,    c.quads,      c.cuboids,   c.disks,         rays,        hits};
    unsigned long long* out = reinterpret_cast<unsigned long long*>(g);
    for (int k = 0; k < 12; ++k) {
        uint32_t x = valid ? v[k] : 0u;
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if ((threadIdx.x & 63u) == 0 && x) atomicAdd(out + k, (unsigned long long)x);
    }
}

// ---- extend ----------------------------------------------------------------------------------------------------
// PBRS_REFILL_BELOW_* (when a wave takes new rays) and PBRS_LONG_WALK_HEIGHT: device/scene.h
#ifndef PBRS_NODE_STEPS_LONG
#define PBRS_NODE_STEPS_LONG 3u
#endif
#ifndef PBRS_CHUNK_MAX
#define PBRS_CHUNK_MAX 512u
#endif
#ifndef PBRS_TRAV_WAVES  // min waves per SIMD asked of the register allocator for k_extend / k_shadow
#define PBRS_TRAV_WAVES 5
#endif
#ifndef PBRS_LEAN_EXTEND_WAVES  // ... and for the k_extend variants without the per-candidate shading check: 80 VGPRs, two
#define PBRS_LEAN_EXTEND_WAVES 6  // dwords of the shared leaf step spilled — C2 extend 13.6 -> 12.8 ms per 16 spp over 5 waves
#endif
#ifndef PBRS_SHADOW_WAVES  // ... and for k_shadow: 76-80 VGPRs without a spill (C4 shadow 347 -> 317 ms, C3 198 -> 180 ms over 5 waves)
#define PBRS_SHADOW_WAVES 6
#endif

// One round of the traversal loop ("if-if"): lanes in the node state take a node step, then the wave tests the primitives
// of its held leaves (leaf_wave: triangle tests shared out over all 64 lanes), so lanes in different phases of their walks
// share the instruction stream.  Lanes waiting at an instance boundary cross it together once PBRS_XFER_MIN of them wait,
// leaves are tested once PBRS_LEAF_MIN lanes hold one — or when no lane of the wave can do anything else.
// The thresholds differ per kernel (measured, C2 / C4): closest-hit walks gain from batching both (a triangle test with
// its four divisions is the longest step); any-hit walks end at the first hit, where waiting at a boundary costs more
// than it saves.
#ifndef PBRS_EXT_XFER_MIN
#define PBRS_EXT_XFER_MIN 8
#endif
#ifndef PBRS_EXT_LEAF_MIN
#define PBRS_EXT_LEAF_MIN 10
#endif
#ifndef PBRS_SHD_XFER_MIN
#define PBRS_SHD_XFER_MIN 2
#endif
#ifndef PBRS_SHD_LEAF_MIN
#define PBRS_SHD_LEAF_MIN 8
#endif
// Scenes with long walks (a BLAS of PBRS_LONG_WALK_HEIGHT levels or more: PBRS_FEAT_LONG_WALKS) take PBRS_NODE_STEPS_LONG
// node steps per loop round: most rounds of a deep walk are node steps, and the checks around them (who waits at a
// boundary, who holds a leaf, who is done) then run a third as often.  C4 (23 levels), ms per frame extend / shadow at
// 1 / 2 / 3 / 4 / 6 steps: 562 / 530 / 523 / 523 / 537 and 321 / 301 / 295 / 295 / 301; short walks lose (two steps: C2 -2 %,
// C3 -1 %: the later steps run at few lanes) and keep one.
// A round's further node steps are LEAN ones (traverse.h, node_step_fast: pop, test, push; a lane at the floor of its tree, or on the
// literal divisions, waits for the round's first step): C4 +2 %, c4xl +2.6 % (profiles/r04p_ab_c4xl_fast_box_test_lean_vs_full.log).  A scene
// whose node coordinates leave the guarded range of the division-free box test walks EVERY ray on the literal divisions, which the
// lean steps do not carry — they would all sit idle: such a scene gets FULL further steps (PBRS_FEAT_FULL_STEPS, pbrs_upload_scene).
// (Round 3 measured "lean steps cost the out-of-cache scene 11 %" on c4xl: that scene had lost the division-free test over three
// vertex heights below 2^-20 — a bound since lowered to 2^-60, host/scene_prepare.cpp — and with it everything built on it.)
#define PBRS_MORE_NODE_STEPS(walk, S, stk, cnt, NSTEPS, FULL)                      \
    do {                                                                           \
        _Pragma("unroll") for (uint32_t k_ = 1; k_ < (NSTEPS); ++k_) {             \
            PBRS_KP_LANE(5 + (k_ < 2u ? k_ : 2u), walk.mode == PBRS_WALK_NODE);    \
            if (walk.mode == PBRS_WALK_NODE) {                                     \
                if constexpr (FULL) walk.node_step(S, stk, cnt);                   \
                else walk.node_step_fast(S, stk, cnt);                             \
            }                                                                      \
        }                                                                          \
    } while (0)
#define PBRS_STEP_WALK(walk, S, stk, cnt, XFER_MIN, LEAF_MIN, NSTEPS, FULL)                                                \
    do {                                                                                                       \
        PBRS_KP_WAVE(0);                                                                                       \
        PBRS_KP_LANE(10, walk.mode == PBRS_WALK_NODE || walk.mode == PBRS_WALK_LEAF || walk.mode == PBRS_WALK_XFER); \
        const uint32_t nx = (uint32_t)__popcll(__ballot(walk.mode == PBRS_WALK_XFER));                         \
        if (nx) {                                                                                              \
            if (nx >= XFER_MIN || __ballot(walk.mode == PBRS_WALK_NODE || walk.mode == PBRS_WALK_LEAF) == 0) { \
                PBRS_PROBE_XFER_COUNT(cnt);                                                                    \
                PBRS_KP_WAVE(3);                                                                               \
                PBRS_KP_LANE(4, walk.mode == PBRS_WALK_XFER);                                                  \
                if (walk.mode == PBRS_WALK_XFER) walk.xfer_step(S, stk, cnt);                                   \
            }                                                                                                  \
        }                                                                                                      \
        PBRS_TT(1);                                                                                            \
        PBRS_PROBE_UTIL_COUNT(walk, cnt);                                                                      \
        PBRS_KP_LANE(5, walk.mode == PBRS_WALK_NODE);                                                          \
        if (__ballot(walk.mode == PBRS_WALK_NODE)) PBRS_KP_WAVE(11);                                           \
        if (walk.mode == PBRS_WALK_NODE) walk.node_step(S, stk, cnt);                                          \
        PBRS_MORE_NODE_STEPS(walk, S, stk, cnt, NSTEPS, FULL);                                                            \
        PBRS_TT(2);                                                                                            \
        const uint32_t nl = (uint32_t)__popcll(__ballot(walk.mode == PBRS_WALK_LEAF));                         \
        if (nl && (nl >= LEAF_MIN || __ballot(walk.mode == PBRS_WALK_NODE) == 0)) {                            \
            PBRS_PROBE_LEAF_COUNT(cnt);                                                                        \
            PBRS_KP_WAVE(8);                                                                                   \
            PBRS_KP_LANE(9, walk.mode == PBRS_WALK_LEAF);                                                      \
            walk.leaf_wave(S, cnt);                                                                            \
        }                                                                                                      \
        PBRS_TT(3);                                                                                            \
    } while (0)
// Work fetch of the persistent traversal kernels.  A wave owns a private range [cur, end) of queue items and hands
// them to its idle lanes without touching memory; only when the range is empty does its first idle lane take a new
// chunk with one atomicAdd.  A single device-wide head word serialises at ~10 ns per atomic, which capped the kernels
// at chunk / 10 ns items per second, so the queue is cut into PBRS_WORK_HEADS contiguous segments, each with its own
// head word on its own 128-byte line.  A block starts on segment blockIdx.x % 8 — blocks are dealt round-robin to
// the 8 XCDs, so neighbouring rays stay within one XCD's L2 — and moves on to the next segment when its own is empty.
// All values are wave-uniform.  (PBRS_WORK_HEADS, PBRS_WORK_HEAD_STRIDE: device/scene.h)
struct WaveWork {
    uint32_t cur, end, chunk;
    uint32_t head, tried;  // segment in use; segments found empty so far
    PD bool left() const { return tried < PBRS_WORK_HEADS || cur < end; }
};
PD WaveWork wave_work_init(uint32_t n) {
    // small queues (late bounces) get small chunks so that every wave still finds work
    uint32_t waves = gridDim.x * (blockDim.x >> 6);
    uint32_t chunk = n / (waves * 4u);
    chunk = chunk < 64u ? 64u : (chunk > PBRS_CHUNK_MAX ? PBRS_CHUNK_MAX : (chunk & ~63u));
    return WaveWork{0u, 0u, chunk, blockIdx.x % PBRS_WORK_HEADS, 0u};
}
PD uint32_t work_segment(uint32_t n, uint32_t h) {
    return h >= PBRS_WORK_HEADS ? n : (uint32_t)(((unsigned long long)n * h / PBRS_WORK_HEADS) & ~63ull);
}
// Lanes with `need` get an item index < n (returned; 0xffffffff = none).  Items left in the wave's range are handed
// out first; if they do not cover every idle lane a new chunk is taken in the same call, so a refill never leaves
// lanes idle while the queue still holds work.
PD uint32_t wave_fetch(WaveWork& w, bool need, uint32_t* heads, uint32_t n) {
    const uint64_t mask = __ballot(need);
    const uint32_t want = (uint32_t)__popcll(mask), rank = lane_prefix(mask);
    const uint32_t avail = w.end - w.cur;
    uint32_t idx = (need && rank < avail) ? w.cur + rank : 0xffffffffu;
    if (want <= avail) {
        w.cur += want;
        return idx;
    }
    w.cur = w.end;
    const int leader = __ffsll((unsigned long long)mask) - 1;
    while (w.tried < PBRS_WORK_HEADS) {  // ends: every pass either returns or retires one segment
        const uint32_t seg_lo = work_segment(n, w.head), seg_hi = work_segment(n, w.head + 1);
        uint32_t base = 0;
        if ((int)(threadIdx.x & 63u) == leader) base = atomicAdd(heads + w.head * PBRS_WORK_HEAD_STRIDE, w.chunk);
        base = __shfl(base, leader, 64);
        const uint32_t len = seg_hi - seg_lo;
        const uint32_t lo = seg_lo + (base < len ? base : len), hi = seg_lo + (base + w.chunk < len ? base + w.chunk : len);
        if (base + w.chunk >= len) {  // nothing beyond this chunk in the segment
            w.head = (w.head + 1u) % PBRS_WORK_HEADS;
            w.tried++;
        }
        if (lo == hi) continue;
        const uint32_t rest = want - avail, got = hi - lo;
        if (need && rank >= avail && rank - avail < got) idx = lo + (rank - avail);
        w.cur = lo + (rest < got ? rest : got);
        w.end = hi;
        break;
    }
    return idx;
}
// Rays a wide-walk kernel cannot take (traverse.h, PBRS_WALK_SLOW) go, whole, into a list that the binary-walk kernel of the
// same stage works off right after it: one atomic per wave and batch.
PD void wave_append_slow(bool slow, uint32_t item, uint32_t* list, uint32_t* count) {
    const uint64_t m = __ballot(slow);
    if (m == 0) return;
    const int leader = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0;
    if ((int)(threadIdx.x & 63u) == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = __shfl(base, leader, 64);
    if (slow) list[base + lane_prefix(m)] = item;
}
#ifndef PBRS_WIDE_SHADOW_WAVES  // min waves per SIMD asked of the register allocator for the wide-walk kernels
#define PBRS_WIDE_SHADOW_WAVES 5
#endif
#ifndef PBRS_WIDE_NODE_STEPS  // node steps per loop round of the wide walks in scenes with long walks
#define PBRS_WIDE_NODE_STEPS 2u
#endif
template <uint32_t ARITY, bool STATS, uint32_t FEAT>  // ARITY 0: the binary walk; 4: the walk over four-wide nodes (device/wide.h)
struct AnySel {
    typedef AnyWalkW<FEAT> type;
};
template <bool STATS, uint32_t FEAT>
struct AnySel<0u, STATS, FEAT> {
    // (k_shadow's: where the TLAS is not scanned, the tree walk passes over the light a ray was aimed at, AnyWalk::skip)
    typedef AnyWalk<STATS, (FEAT & (PBRS_FEAT_ALL | PBRS_FEAT_LDS_TOP)), !STATS && !(FEAT & PBRS_FEAT_FLAT_TLAS)> type;
};
#define PBRS_WALK_ARITY(STATS, FEAT) ((STATS) ? 0u : ((FEAT) & PBRS_FEAT_WIDE) ? 4u : 0u)
#ifndef PBRS_NODE_STEPS_SHORT  // node steps per round in scenes with short walks: one (two, the second a lean one: C2 -2.3 %, C3 -3.2 %)
#define PBRS_NODE_STEPS_SHORT 1u
#endif
#define PBRS_WALK_NSTEPS(FEAT, ARITY) \
    (!((FEAT) & PBRS_FEAT_LONG_WALKS) ? ((ARITY) == 0u ? PBRS_NODE_STEPS_SHORT : 1u) : (ARITY) == 4u ? PBRS_WIDE_NODE_STEPS : PBRS_NODE_STEPS_LONG)
// PBRS_FEAT_LDS_SCENE: a random 16-byte read costs the CU's texture path 2 cycles per lane (a 32-byte node 129 cycles per wave, a
// 48-byte triangle ~190) and the LDS 0.37 (a node 46-58, a triangle 36-50: tools/microbench/gather_lds_coop.hip,
// profiles/r04_microbench_gather_lds_coop.log), at a third of the latency.  Where the arrays a walk reads fit next to the block's stack
// rows (pbrs_upload_scene: C2 / C3, 8 KB) every block copies them in once and the walk's scene view points into the copy: node,
// triangle, instance and shape fetches become ds_read_b128; what stays on the texture path is a ray's own record (fetched at its
// start, read again when it leaves an instance) and its result.
PD DevScene stage_scene(const DevScene& G, uint32_t* lds_base) {
    DevScene S = G;
    uint4* dst = reinterpret_cast<uint4*>(__builtin_assume_aligned(lds_base + G.lds_off_words, 16));
    S.nodes = reinterpret_cast<const pbrs_node*>(dst);
    dst = stage_array(dst, G.nodes, G.lds_nodes * (uint32_t)(sizeof(pbrs_node) / 16));
    S.tv = reinterpret_cast<const pbrs_tri_verts*>(dst);
    dst = stage_array(dst, G.tv, G.lds_tris * (uint32_t)(sizeof(pbrs_tri_verts) / 16));
    S.inst = reinterpret_cast<const pbrs_instance*>(dst);
    dst = stage_array(dst, G.inst, G.lds_inst * (uint32_t)(sizeof(pbrs_instance) / 16));
    S.shapes = reinterpret_cast<const pbrs_shape*>(dst);
    stage_array(dst, G.shapes, G.lds_shapes * (uint32_t)(sizeof(pbrs_shape) / 16));
    __syncthreads();
    return S;
}
static_assert(sizeof(pbrs_node) % 16 == 0 && sizeof(pbrs_tri_verts) % 16 == 0 && sizeof(pbrs_instance) % 16 == 0 && sizeof(pbrs_shape) % 16 == 0, "stage_scene copies 16-byte pieces");

// PBRS_FEAT_LDS_TOP: scenes whose arrays do not fit as a whole but whose TLAS does (C5: 130 instances, 259 nodes, 8 KB) get the head of the
// node array staged — a ray of such a scene tests some thirty TLAS boxes, five of a BLAS.
PD DevScene stage_top(const DevScene& G, uint32_t* lds_base) {
    DevScene S = G;
    uint4* dst = reinterpret_cast<uint4*>(__builtin_assume_aligned(lds_base + G.lds_off_words, 16));
    S.nodes_top = reinterpret_cast<const pbrs_node*>(dst);
    stage_array(dst, G.nodes, G.lds_nodes * (uint32_t)(sizeof(pbrs_node) / 16));
    __syncthreads();
    return S;
}

// Persistent: every wave keeps pulling rays from the queue until it is empty; a lane whose walk ends is
// handed a new ray at the next refill, the walks of the other lanes continue where they were.
// `indirect` (binary-walk kernels working off a slow list): the queue positions to trace, `count` of them.  (k_extend walks binary
// only: the host passes null for `indirect` and the slow list.)
// ENTRY: nothing, or — bounce 0 of a render with an entry table (device/entry_nodes.h; kernel_tables.h, extend_entry_fn_t) — one EntryArgs:
// camera rays then enter the table instance's BLAS at their pixel's entry nodes.  (A pack, so that every other k_extend keeps its arguments,
// and with them its instructions.)
template <bool STATS, uint32_t FEAT, class... ENTRY>
__global__ void __launch_bounds__(256, STATS ? 3 : (FEAT & PBRS_FEAT_SHADING_CHECK) ? PBRS_TRAV_WAVES : PBRS_LEAN_EXTEND_WAVES)
    k_extend(DevScene G, PathState st, uint32_t set, const uint32_t* count, uint32_t n_direct, uint32_t* next, GlobalCounters* gc, const uint32_t* indirect,
             uint32_t* slow_list, uint32_t* slow_count, uint32_t split, ENTRY... entry) {
    static_assert(sizeof...(ENTRY) <= 1, "at most the entry table's arguments");
    constexpr bool HAS_ENTRY = sizeof...(ENTRY) != 0;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const DevScene S = (!STATS && (FEAT & PBRS_FEAT_LDS_SCENE)) ? stage_scene(G, lds_stack) : (!STATS && (FEAT & PBRS_FEAT_LDS_TOP)) ? stage_top(G, lds_stack) : G;
    const uint32_t n = count ? *count : n_direct;
    const float4* q0 = st.q[set][0];
    const float4* q1 = st.q[set][1];
    LaneStack stk{lds_stack + threadIdx.x, q0, q1, 0u};
    Cnt<STATS> cnt;
    cnt.init();
    uint32_t nrays = 0, nhit = 0;
    ClosestWalk<STATS, (FEAT & (PBRS_FEAT_ALL | PBRS_FEAT_LDS_TOP | PBRS_FEAT_EXTENT)), HAS_ENTRY> walk;
    if constexpr (HAS_ENTRY) walk.a = (entry, ...);
    walk.mode = PBRS_WALK_IDLE;
    PBRS_KP_DECL(walk);
    PBRS_TT_DECL;
    uint32_t item = 0;  // queue position of the lane's ray; bit 31: the path record's "after a specular bounce" flag (queues stay below 2^28)
    WaveWork work = wave_work_init(n);
    for (;;) {
        uint64_t live = __ballot(walk.mode == PBRS_WALK_NODE || walk.mode == PBRS_WALK_LEAF || walk.mode == PBRS_WALK_XFER);
        if ((uint32_t)__popcll(live) < S.refill_below) {
            PBRS_KP_WAVE(1);
            if (walk.mode == PBRS_WALK_DONE) {  // finished walks are retired in batches, at refill time
                walk.finish(cnt);  // a walk that ended inside an instance: its candidate meets the best hit here
                const Hit& h = walk.best;
                nhit += h.inst != 0xffffffffu ? 1u : 0u;
                // k_shade rebuilds the Interaction from (t, inst, prim): the barycentrics are recomputed there, as the
                // reference's intersect does for the winning primitive
                // the 4th word names the hit's shading class (pbrs_upload_scene: DevScene::inst_class), 0 for a miss
                uint32_t cls = (S.n_classes > 1u && h.inst != 0xffffffffu) ? S.inst[h.inst].pad[0] : 0u;
                if (split) {
                    // The path integrator's queue of a scene with one shading class, split by what src/pathintegrator.rs does with
                    // the result (class 1 = kept for k_shade, 0 = dropped; k_class_count / _scan / _scatter then list the kept
                    // positions, in queue order).  A hit is kept: a surface with lobes is shaded (:31-71), an emitter adds its
                    // emission and the empty light estimate and ends.  A miss that sees the environment (the first bounce or after a
                    // specular one, :19-22) is kept: it adds the environment and ends.  Any other miss adds nothing (`break` at
                    // :25-27 with nothing before it) and is dropped — in an open scene most of a bounce's queue; so is a miss of the
                    // first bounce under a black environment: L = 0 + 1 * 0 there, which k_class_scatter stores for it.  (After a
                    // specular bounce under a black environment beta may be infinite: beta * 0 is kept for k_shade to add.)
                    cls = 1u;
                    if (h.inst == 0xffffffffu) {
                        // (the path record's flag rides in `item` since the ray was fetched: reading the record again here put a
                        // memory round trip into every refill of an open scene)
                        const bool specular = (item >> 31) != 0u;
                        cls = (specular || ((split & PBRS_QSPLIT_ENV) && S.has_env != 0u)) ? 1u : 0u;
                    }
                }
                const uint32_t pos = item & 0x7fffffffu;
                if (!split || cls) st_stream(&st.hit[pos], make_float4(h.t, __uint_as_float(h.inst), __uint_as_float(h.prim), __uint_as_float(split ? 0u : cls)));
                if (S.n_classes > 1u || split) st.cls[pos] = (uint8_t)cls;  // what the class sort reads: 1 byte per path instead of a 16-byte record
                walk.mode = PBRS_WALK_IDLE;
            }
            if (work.left()) {
                uint32_t idx = wave_fetch(work, walk.mode == PBRS_WALK_IDLE, next, n);
                if (idx != 0xffffffffu) {
                    if (indirect) idx = indirect[idx];
                    stk.item = idx;
                    const float4 a = q0[idx], b = q1[idx];
                    item = idx | (__float_as_uint(a.w) & 0x80000000u);
                    walk.start(S, xyz(a), xyz(b), pn_inf(), stk);
                    nrays++;
                    PBRS_KP_LANE(2, true);
                }
                walk.scan_wave(S, cnt);
                live = __ballot(walk.mode == PBRS_WALK_NODE || walk.mode == PBRS_WALK_LEAF || walk.mode == PBRS_WALK_XFER);
            }
            if (live == 0) break;
        }
        PBRS_TT(0);
        PBRS_STEP_WALK(walk, S, stk, cnt, PBRS_EXT_XFER_MIN, PBRS_EXT_LEAF_MIN, PBRS_WALK_NSTEPS(FEAT, 0u), ((FEAT & PBRS_FEAT_FULL_STEPS) != 0u));
    }
    flush_counters<STATS>(cnt, gc, true, nrays, nhit);
    if (!STATS) PBRS_KP_FLUSH(0, walk);
    if (!STATS) PBRS_TT_FLUSH(0);
}
