// device/shadow.h — the shadow stage (device/kernels.h): k_shadow, on the traversal loop of device/extend.h.
#pragma once
#include "extend.h"

// ---- shadow ----------------------------------------------------------------------------------------------------
// One work item per shadow ray (persistent, same refill scheme as k_extend); writes one occlusion byte.
template <bool STATS, uint32_t FEAT>
__global__ void __launch_bounds__(256, STATS ? 3 : (FEAT & PBRS_FEAT_WIDE) ? PBRS_WIDE_SHADOW_WAVES : PBRS_SHADOW_WAVES)
    k_shadow(DevScene G, PathState st, const uint32_t* count, uint32_t* next, GlobalCounters* gc, const uint32_t* indirect, uint32_t* slow_list,
             uint32_t* slow_count) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const DevScene S = (!STATS && (FEAT & PBRS_FEAT_LDS_SCENE)) ? stage_scene(G, lds_stack) : (!STATS && (FEAT & PBRS_FEAT_LDS_TOP)) ? stage_top(G, lds_stack) : G;
    constexpr uint32_t ARITY = PBRS_WALK_ARITY(STATS, FEAT);
    constexpr bool WIDE = ARITY != 0u;
    const uint32_t n = indirect ? count[0] : count[1];  // a slow list's length, or the high half of the packed (nee paths, shadow rays) counter
    LaneStack stk{lds_stack + threadIdx.x, st.sr[0], st.sr[1], 0u};
    Cnt<STATS> cnt;
    cnt.init();
    uint32_t nrays = 0;
    typename AnySel<ARITY, STATS, (FEAT & (PBRS_FEAT_ALL | PBRS_FEAT_LDS_TOP))>::type walk;
    walk.mode = PBRS_WALK_IDLE;
    PBRS_KP_DECL(walk);
    PBRS_TT_DECL;
    uint32_t item = 0, rec = 0;
    f3 l_vis = gray(0.0f);  // a lone ray's "unoccluded" outcome, fetched with the ray: read at retire time it put a memory round trip into every refill
    WaveWork work = wave_work_init(n);
    for (;;) {
        uint64_t live = __ballot(walk.mode == PBRS_WALK_NODE || walk.mode == PBRS_WALK_LEAF || walk.mode == PBRS_WALK_XFER);
        if ((uint32_t)__popcll(live) < S.refill_below_shadow) {
            PBRS_KP_WAVE(1);
            if constexpr (WIDE) {
                wave_append_slow(walk.mode == PBRS_WALK_SLOW, rec, slow_list, slow_count);
                if (walk.mode == PBRS_WALK_SLOW) walk.mode = PBRS_WALK_IDLE;
                walk.settle(S);  // the leaf boxes the finished walks still owe; a lane whose box fails walks on
                live = __ballot(walk.mode == PBRS_WALK_NODE || walk.mode == PBRS_WALK_LEAF || walk.mode == PBRS_WALK_XFER);
            }
            if (walk.mode == PBRS_WALK_DONE) {
                const bool occluded = walk.occluded;
                const uint32_t slot = item & PBRS_SLOT_MASK, r = item >> 31;
                if (item & 0x40000000u) {
                    // the path's only shadow ray: k_shade stored the occluded outcome in L and sent the other one along
                    if (!occluded) {
                        float* l = reinterpret_cast<float*>(st.L + slot);  // .w (the direct integrator's 1 / mass) stays
                        l[0] = l_vis.x;
                        l[1] = l_vis.y;
                        l[2] = l_vis.z;
                    }
                } else {
                    at(st.occ[r], slot) = occluded ? 1 : 0;
                }
                walk.mode = PBRS_WALK_IDLE;
            }
            if (work.left()) {
                uint32_t idx = wave_fetch(work, walk.mode == PBRS_WALK_IDLE, next, n);
                if (idx != 0xffffffffu) {
                    if (indirect) idx = indirect[idx];
                    rec = idx;
                    stk.item = idx;
                    const float4 q0 = st.sr[0][idx], q1 = st.sr[1][idx];
                    item = __float_as_uint(q1.w);
                    uint32_t tag = 0u;
                    if (item & 0x40000000u) {
                        const float4 q2 = st.sr[2][idx];
                        l_vis = xyz(q2);
                        tag = __float_as_uint(q2.w);  // the light the ray was aimed at, where its own test is known to be false (AnyWalk::skip)
                    }
                    walk.start(S, mk3(q0.x, q0.y, q0.z), mk3(q1.x, q1.y, q1.z), q0.w, stk);
                    if constexpr (!STATS) {
                        walk.skip = tag & PBRS_SKIP_INST_MASK;  // read by the walks of a TLAS that is not scanned
                        walk.skip_scanned(tag);                 // ... and where it is: out of the mask the scan is about to hand the lane
                    }
                    nrays++;
                    PBRS_KP_LANE(2, true);
                }
                if constexpr (WIDE) walk.scan_wave(S, stk);
                else walk.scan_wave(S, cnt);
                live = __ballot(walk.mode == PBRS_WALK_NODE || walk.mode == PBRS_WALK_LEAF || walk.mode == PBRS_WALK_XFER);
            }
            if (live == 0) {
                if constexpr (WIDE) {
                    walk.forget_reciprocals();
                    if (__ballot(walk.mode == PBRS_WALK_SLOW || walk.mode == PBRS_WALK_DONE)) continue;
                }
                break;
            }
        }
        PBRS_TT(0);
        PBRS_STEP_WALK(walk, S, stk, cnt, PBRS_SHD_XFER_MIN, PBRS_SHD_LEAF_MIN, PBRS_WALK_NSTEPS(FEAT, ARITY), ((FEAT & PBRS_FEAT_FULL_STEPS) != 0u));
        if constexpr (WIDE) walk.forget_reciprocals();
    }
    flush_counters<STATS>(cnt, gc, true, nrays, 0u);
    if (!STATS) PBRS_KP_FLUSH(1, walk);
    if (!STATS) PBRS_TT_FLUSH(1);
}
