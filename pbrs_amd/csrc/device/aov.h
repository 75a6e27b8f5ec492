// device/aov.h — first-hit AOVs (include/pbrs_gpu.h, pbrs_aov_buffers): albedo, normal, coverage, depth, instance, material, prim.
//
// The camera samples of the render itself: right after bounce 0's k_extend a pass holds every sample's ray (q[0][0..1], at the
// sample's slot: bounce 0's queue position is its slot, k_raygen) and its hit record (hit[slot]).  k_aov folds them into a per-pixel
// running state in sample-index order, pass after pass; k_aov_finalize scales the sums once the last pass has run.
//
// State: planar words by pixel ORDER (order_of_pixel), 10 per pixel — albedo sum xyz, normal sum xyz, n_hit, best t, inst, prim.  It
// starts as zeros (pbrs_gpu.hip, render_common): n_hit == 0 means "no hit yet", so best t / inst / prim need no other initial value.
#pragma once
#include "lights.h"
#include "path_state.h"
#include "textures.h"

#define PBRS_AOV_STATE_WORDS 10u

// The colour k_shade's per-hit lobe list gives every lobe the material pushes at this hit (kernels.h, k_shade, TEX), summed in lobe
// order from +0: a textured lobe takes tex_value at the hit, an Uber lobe whose texture is black there is not pushed, a Fourier lobe
// counts as white.  Restated rather than shared, so that k_shade compiles to the instructions it had.
PD f3 aov_lobe_albedo(const DevScene& S, const pbrs_material& mat, const Isect& is) {
    f3 a = gray(0.0f);
    for (uint32_t k = 0; k < mat.n_bxdfs; ++k) {
        const pbrs_bxdf& lb = S.bxdfs[mat.first_bxdf + k];
        f3 colour = ld3(lb.albedo);
        if (lb.tex) {
            colour = tex_value(S, (lb.tex & ~PBRS_BXDF_TEX_DROP_IF_BLACK) - 1u, is.u, is.v, is.pos);
            if ((lb.tex & PBRS_BXDF_TEX_DROP_IF_BLACK) && is_black(colour)) continue;
        }
        if (lb.kind == PBRS_BXDF_FOURIER) colour = gray(1.0f);
        a = a + colour;
    }
    return mk3(fminf(fmaxf(a.x, 0.0f), 1.0f), fminf(fmaxf(a.y, 0.0f), 1.0f), fminf(fmaxf(a.z, 0.0f), 1.0f));
}

// One thread per pixel, by pixel order q: a sample index's loads are contiguous per wave (slot_of_sample).  The pass's kc sample
// indices in order.  `qsplit`: k_extend's split flags (PBRS_QSPLIT_*, device/scene.h; not 0: PBRS_QSPLIT_ON): it split the queue and wrote no hit record for the paths it dropped —
// misses under a black environment, cls[slot] == 0.  S is the global scene: this kernel stages nothing in LDS.
__global__ void __launch_bounds__(256) k_aov(DevScene S, PathState st, float* aov, uint32_t n_pixels, uint32_t k_count, uint32_t chunk, uint32_t qsplit) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pixels) return;
    f3 a = mk3(aov[q], aov[n_pixels + q], aov[2 * n_pixels + q]);
    f3 nsum = mk3(aov[3 * n_pixels + q], aov[4 * n_pixels + q], aov[5 * n_pixels + q]);
    uint32_t n_hit = __float_as_uint(aov[6 * n_pixels + q]);
    float best_t = aov[7 * n_pixels + q];
    uint32_t best_inst = __float_as_uint(aov[8 * n_pixels + q]);
    uint32_t best_prim = __float_as_uint(aov[9 * n_pixels + q]);
    for (uint32_t k = 0; k < k_count; ++k) {
        const uint32_t slot = slot_of_sample(k, q, n_pixels, k_count, chunk);
        if (qsplit && st.cls[slot] == 0) continue;  // dropped by the split: a miss
        const float4 rh = st.hit[slot];
        Hit h;
        h.t = rh.x;
        h.inst = __float_as_uint(rh.y);
        h.prim = __float_as_uint(rh.z);
        h.b1 = h.b2 = 0.0f;
        if (h.inst == 0xffffffffu) continue;
        const f3 o = xyz(st.q[0][0][slot]), d = xyz(st.q[0][1][slot]);
        const Isect is = reconstruct_isect(S, h, o, d);
        const pbrs_instance& in = S.inst[h.inst];
        a = a + aov_lobe_albedo(S, S.mats[in.material], is);
        nsum = nsum + is.normal;
        // nearest hit; a tie keeps the lower sample index (the earlier one: passes run in sample order)
        if (n_hit == 0u || h.t < best_t) {
            best_t = h.t;
            best_inst = h.inst;
            best_prim = in.shape_kind == PBRS_SHAPE_MESH ? S.ts[h.prim].orig : 0u;  // pbrs_hit_record::prim (k_intersect_rays)
        }
        ++n_hit;
    }
    aov[q] = a.x;
    aov[n_pixels + q] = a.y;
    aov[2 * n_pixels + q] = a.z;
    aov[3 * n_pixels + q] = nsum.x;
    aov[4 * n_pixels + q] = nsum.y;
    aov[5 * n_pixels + q] = nsum.z;
    aov[6 * n_pixels + q] = __uint_as_float(n_hit);
    aov[7 * n_pixels + q] = best_t;
    aov[8 * n_pixels + q] = __uint_as_float(best_inst);
    aov[9 * n_pixels + q] = __uint_as_float(best_prim);
}

// The sums scaled as k_finalize scales the radiance (* (1 / spp)), into the requested buffers (device pointers, row-major; null = not
// wanted); one thread per row-major pixel p.
__global__ void __launch_bounds__(256) k_aov_finalize(const float* aov, const pbrs_instance* inst, uint32_t n_pixels, uint32_t w, uint32_t tiles8_per_row,
                                                      float inv_spp, pbrs_aov_buffers out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    const uint32_t q = order_of_pixel(p, w, tiles8_per_row);
    const uint32_t n_hit = __float_as_uint(aov[6 * n_pixels + q]);
    const bool hit = n_hit != 0u;
    if (out.albedo)
        for (uint32_t c = 0; c < 3u; ++c) out.albedo[3 * p + c] = aov[c * n_pixels + q] * inv_spp;
    if (out.normal)
        for (uint32_t c = 0; c < 3u; ++c) out.normal[3 * p + c] = aov[(3 + c) * n_pixels + q] * inv_spp;
    if (out.coverage) out.coverage[p] = (float)n_hit * inv_spp;
    if (out.depth) out.depth[p] = hit ? aov[7 * n_pixels + q] : pn_inf();
    const uint32_t i = __float_as_uint(aov[8 * n_pixels + q]);
    if (out.instance) out.instance[p] = hit ? i : 0xffffffffu;
    if (out.material) out.material[p] = hit ? inst[i].material : 0xffffffffu;
    if (out.prim) out.prim[p] = hit ? __float_as_uint(aov[9 * n_pixels + q]) : 0xffffffffu;
}
