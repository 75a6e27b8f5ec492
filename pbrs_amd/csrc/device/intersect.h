// device/intersect.h — the parity harness's ray queries (pbrs_intersect_rays) through the walks of the traversal kernels.
#pragma once
#include "extend.h"

// ---- parity-harness kernels --------------------------------------------------------------------------------------------
// The walks the pipeline runs for the scene (pbrs_gpu.hip, KernelPlan): closest hits through k_extend's binary walk; WIDE_ANY =
// occlusion queries go through the four-wide any-hit walk of k_shadow (AnyWalkW, with its hand-off of refused rays to the binary
// walk).  info[0]: rays the wide any-hit walk refused (info[1], the closest-hit walk's, stays 0).
template <bool WIDE_ANY>
__global__ void __launch_bounds__(256) k_intersect_rays(DevScene S, uint32_t n, const float4* origins, const float4* dirs, const float* tmax,
                                                       pbrs_hit_record* hits, uint8_t* occluded, uint32_t* info) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    LaneStack stk{lds_stack + threadIdx.x, origins, dirs, 0u};
    Cnt<false> cnt;
    // grid <= PBRS_PERSISTENT_BLOCKS; whole blocks stay in the loop together (the walks share work across a wave)
    for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
        const uint32_t i = base + threadIdx.x;
        const bool active = i < n;
        f3 o = gray(0.0f), d = gray(1.0f);
        float t_max = 0.0f;
        if (active) {
            o = xyz(origins[i]);
            d = xyz(dirs[i]);
            t_max = tmax[i];
            stk.item = i;
        }
        if (hits) {
            Hit h;
            if (S.exact_extent) tlas_closest<false, PBRS_FEAT_EXTENT>(S, active, o, d, t_max, stk, h, cnt);  // as the scene's k_extend
            else tlas_closest<false>(S, active, o, d, t_max, stk, h, cnt);
            if (active) {
                pbrs_hit_record r;
                r.t = h.t;
                r.inst = h.inst;
                r.prim = 0;
                if (h.inst != 0xffffffffu && S.inst[h.inst].shape_kind == PBRS_SHAPE_MESH) r.prim = S.ts[h.prim].orig;
                r.b1 = h.b1;
                r.b2 = h.b2;
                hits[i] = r;
            }
        }
        if (occluded) {
            bool slow = false;
            const bool occ = WIDE_ANY ? tlas_any_wide(S, active, o, d, t_max, stk, slow) : tlas_any<false>(S, active, o, d, t_max, stk, cnt);
            if (active) {
                occluded[i] = occ ? 1 : 0;
                if (slow) atomicAdd(info, 1u);
            }
        }
    }
}
