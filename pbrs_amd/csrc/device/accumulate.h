// device/accumulate.h — the end of a bounce and of a pass (device/kernels.h): the estimates that waited for two shadow rays
// (k_nee_resolve), the per-pixel sums (k_accumulate, k_finalize) and the instrumented renders' queue sizes.
#pragma once
#include "path_state.h"

// The radiance add of uniform_sample_one_light / path_integrator for paths whose estimate had to wait for
// visibility: Ld terms in the reference's order (directlighting.rs:193, :219), * n_lights (:98), * beta
// (pathintegrator.rs:35).
__global__ void __launch_bounds__(256) k_nee_resolve(PathState st, const uint32_t* queue, const uint32_t* count) {
  const uint32_t n = count[0];  // low half of the packed (nee paths, shadow rays) counter
  // A capped grid in strides (host/pass_plan.h, kStreamGridCap): the number of two-ray estimates is only known on the device — a
  // few % of a bounce's vertices — and a grid sized for the whole pass costs 0.17 ms per launch in blocks that find nothing
  // to do (an empty block is dispatched in ≈0.2 ns): 7 ms per frame of C4.
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    uint32_t slot = queue[i];
    // only area-light estimates cast two rays: Ld = term 1 (light sample, :193) + term 2 (BSDF sample, :219)
    bool occ0 = at(st.occ[0], slot) != 0, occ1 = at(st.occ[1], slot) != 0;
    const float4 n0 = st.nee[0][slot], n1 = st.nee[1][slot], n2 = st.nee[2][slot];
    f3 c1 = xyz(n0), c2 = xyz(n1);
    f3 one = gray(0.0f);
    if (!occ0) one = one + c1;
    if (!occ1) one = one + c2;
    f3 nb = xyz(n2);
    const float4 rl = st.L[slot];
    f3 L = xyz(rl);
    L = L + cmul(nb, one * n0.w) * n1.w;  // the post factor is 1 for the path integrator: x * 1 == x bit for bit
    st.L[slot] = pack4(L, rl.w);
  }
}

// ---- accumulate / finalize -----------------------------------------------------------------------------------------
// color_sum = color_sum + integrator(...) for strictly increasing sample index (src/main.rs:205)
// Also counts the samples whose radiance is not finite (pbrs_stats.invalid_samples): one atomic per wave that saw any.
__global__ void __launch_bounds__(256) k_accumulate(PathState st, float* sum, uint32_t n_pixels, uint32_t k_count, uint32_t chunk, uint32_t w,
                                                     uint32_t tiles8_per_row, unsigned long long* nonfinite) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    f3 s = mk3(sum[p], sum[n_pixels + p], sum[2 * n_pixels + p]);
    uint32_t bad = 0;
    for (uint32_t k = 0; k < k_count; ++k) {
        const uint32_t slot = slot_of_sample(k, order_of_pixel(p, w, tiles8_per_row), n_pixels, k_count, chunk);
        const f3 l = xyz(st.L[slot]);
        bad += (pn_isfinite(l.x) && pn_isfinite(l.y) && pn_isfinite(l.z)) ? 0u : 1u;
        s = s + l;
    }
    if (__ballot(bad != 0u)) {
        for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
        if ((threadIdx.x & 63u) == 0) atomicAdd(nonfinite, (unsigned long long)bad);
    }
    sum[p] = s.x;
    sum[n_pixels + p] = s.y;
    sum[2 * n_pixels + p] = s.z;
}
// color_sum.scale_down_by(msaa*msaa) (src/main.rs:208, color.rs:90-95): * (1.0 / n as f32); planar -> row-major RGB
__global__ void __launch_bounds__(256) k_finalize(const float* sum, float* rgb, uint32_t n_pixels, float inv_spp) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    rgb[3 * p] = sum[p] * inv_spp;
    rgb[3 * p + 1] = sum[n_pixels + p] * inv_spp;
    rgb[3 * p + 2] = sum[2 * n_pixels + p] * inv_spp;
}

// Instrumented renders only: the queue sizes of one pass, bounce by bounce, added to the render's totals (pbrs_stats).
// act[b] = paths entering bounce b >= 1 (bounce 0: the pass itself), ns[b] = (shadow rays << 32 | two-ray estimates) of bounce b.
__global__ void k_sum_bounce_counts(const uint32_t* act, const unsigned long long* ns, uint32_t n_pass, uint32_t n_bounces, unsigned long long* acc) {
    const uint32_t b = threadIdx.x;
    if (b >= n_bounces) return;
    const uint32_t at = b < PBRS_STATS_MAX_BOUNCES ? b : PBRS_STATS_MAX_BOUNCES - 1u;
    atomicAdd(acc + at, (unsigned long long)(b == 0 ? n_pass : act[b]));
    atomicAdd(acc + PBRS_STATS_MAX_BOUNCES + at, ns[b] >> 32);
}
