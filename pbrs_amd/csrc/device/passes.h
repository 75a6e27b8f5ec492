// device/passes.h — light passes (include/pbrs_gpu.h, pbrs_render_tile_passes*): direct and indirect light of the render's own samples
// beside the image, each with the variance of its pixel mean's luminance, and the sum that puts the two back together.
//
// Once bounce 0's k_shade, k_shadow (with its slow-list launch) and k_nee_resolve have run, st.L[slot] is the reference's `radiance`
// after the first iteration of its loop (src/pathintegrator.rs:14-71): emission or environment, plus the light estimate at the first
// hit — D_i.  k_pass_direct keeps it in D[slot], a column of one float4 per path that a pass set holds beside its PathState (not inside
// it: the struct is an argument of every kernel of the pipeline, and a render without passes runs those unchanged), before bounce 1 adds
// to L.  When the pass is accumulated, L - D is I_i: k_pass_fold, launched right behind k_accumulate / k_moments on the same stream (so the
// pass overlap keeps the passes in order: moments.h), folds both into a per-pixel running state in sample-index order; k_pass_finalize
// writes the wanted buffers once the last pass has run.
//
// State: planar words by pixel ORDER (order_of_pixel), 12 per pixel — sum of D xyz, sum of I xyz, (m1, m2, n) of lum(D), (m1, m2, n) of
// lum(I).  It starts as zeros (pbrs_gpu.hip, render_common).
#pragma once
#include "moments.h"

#define PBRS_PASS_STATE_WORDS 12u

// The variance AOV's recipe (moments.h: k_moments, k_moments_finalize, which stay as they are) for a layer's luminances: one sample into
// a pixel's moments, the non-finite ones skipped ...
PD void moments_fold(float y, float& m1, float& m2, uint32_t& n) {
    if (pn_isfinite(y)) {
        m1 = m1 + y;
        m2 = m2 + y * y;
        ++n;
    }
}
// ... and the variance of the mean from the moments of n finite samples; +inf ("unknown") below two.
PD float moments_variance(float m1, float m2, uint32_t n) {
    if (n < 2u) return pn_inf();
    const float inv_n = 1.0f / (float)n;
    const float mean = m1 * inv_n;
    float v = m2 * inv_n - mean * mean;
    v = v < 0.0f ? 0.0f : v;
    return v * (1.0f / (float)(n - 1u));
}

// L -> D for the pass's n slots.  Both are stream records (kernels.h): read once here, written once, read once by k_pass_fold.
__global__ void __launch_bounds__(256) k_pass_direct(const float4* L, float4* D, uint32_t n_slots) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_slots) return;
    st_stream(&D[slot], ld_stream(&L[slot]));
}

// One thread per pixel, by pixel order q: a sample index's loads are contiguous per wave (slot_of_sample), as in k_moments.
__global__ void __launch_bounds__(256) k_pass_fold(const float4* L, const float4* D, float* state, uint32_t n_pixels, uint32_t k_count, uint32_t chunk) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pixels) return;
    float w[PBRS_PASS_STATE_WORDS];
    for (uint32_t j = 0; j < PBRS_PASS_STATE_WORDS; ++j) w[j] = state[j * n_pixels + q];
    f3 sd = mk3(w[0], w[1], w[2]), si = mk3(w[3], w[4], w[5]);
    uint32_t nd = __float_as_uint(w[8]), ni = __float_as_uint(w[11]);
    for (uint32_t k = 0; k < k_count; ++k) {
        const uint32_t slot = slot_of_sample(k, q, n_pixels, k_count, chunk);
        const f3 d = xyz(ld_stream(&D[slot]));
        const f3 i = xyz(L[slot]) - d;
        sd = sd + d;
        si = si + i;
        moments_fold(luminance(d), w[6], w[7], nd);
        moments_fold(luminance(i), w[9], w[10], ni);
    }
    w[0] = sd.x, w[1] = sd.y, w[2] = sd.z;
    w[3] = si.x, w[4] = si.y, w[5] = si.z;
    w[8] = __uint_as_float(nd), w[11] = __uint_as_float(ni);
    for (uint32_t j = 0; j < PBRS_PASS_STATE_WORDS; ++j) state[j * n_pixels + q] = w[j];
}

// The sums scaled as k_finalize scales the radiance, the moments through the variance AOV's recipe, into the wanted buffers (device
// pointers, row-major; null = not wanted); one thread per row-major pixel p.
__global__ void __launch_bounds__(256) k_pass_finalize(const float* state, uint32_t n_pixels, uint32_t w, uint32_t tiles8_per_row, float inv_spp,
                                                       pbrs_pass_buffers out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    const uint32_t q = order_of_pixel(p, w, tiles8_per_row);
    if (out.direct)
        for (uint32_t c = 0; c < 3u; ++c) out.direct[3 * p + c] = state[c * n_pixels + q] * inv_spp;
    if (out.indirect)
        for (uint32_t c = 0; c < 3u; ++c) out.indirect[3 * p + c] = state[(3 + c) * n_pixels + q] * inv_spp;
    if (out.direct_variance)
        out.direct_variance[p] = moments_variance(state[6 * n_pixels + q], state[7 * n_pixels + q], __float_as_uint(state[8 * n_pixels + q]));
    if (out.indirect_variance)
        out.indirect_variance[p] = moments_variance(state[9 * n_pixels + q], state[10 * n_pixels + q], __float_as_uint(state[11 * n_pixels + q]));
}

// out = a + b over n words, in strides; out may be a or b (every word is read before it is written, by the thread that writes it).
__global__ void __launch_bounds__(256) k_combine_passes(const float* a, const float* b, float* out, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = a[i] + b[i];
}
