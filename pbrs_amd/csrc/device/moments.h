// device/moments.h — the variance AOV (include/pbrs_gpu.h, pbrs_render_tile_aovs_var*): the variance of a pixel's mean luminance from
// the radiances of its own samples.
//
// A pass holds every sample's radiance in st.L[slot] when k_accumulate folds it; k_moments, launched right behind k_accumulate on the
// same stream (so the pass overlap keeps the passes in order), folds the same samples into a per-pixel running state in sample-index
// order; k_moments_finalize writes the buffer once the last pass has run.  k_accumulate itself is not touched.
//
// State: planar words by pixel ORDER (order_of_pixel), 3 per pixel — m1, m2, n.  It starts as zeros (pbrs_gpu.hip, render_common).
#pragma once
#include "path_state.h"

#define PBRS_MOMENT_STATE_WORDS 3u

// One thread per pixel, by pixel order q: a sample index's loads are contiguous per wave (slot_of_sample), as in k_aov.
__global__ void __launch_bounds__(256) k_moments(PathState st, float* mom, uint32_t n_pixels, uint32_t k_count, uint32_t chunk) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pixels) return;
    float m1 = mom[q], m2 = mom[n_pixels + q];
    uint32_t n = __float_as_uint(mom[2 * n_pixels + q]);
    for (uint32_t k = 0; k < k_count; ++k) {
        const float y = luminance(xyz(st.L[slot_of_sample(k, q, n_pixels, k_count, chunk)]));
        if (pn_isfinite(y)) {
            m1 = m1 + y;
            m2 = m2 + y * y;
            ++n;
        }
    }
    mom[q] = m1;
    mom[n_pixels + q] = m2;
    mom[2 * n_pixels + q] = __uint_as_float(n);
}

// variance of the mean, row-major; one thread per row-major pixel p.
__global__ void __launch_bounds__(256) k_moments_finalize(const float* mom, uint32_t n_pixels, uint32_t w, uint32_t tiles8_per_row, float* variance) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    const uint32_t q = order_of_pixel(p, w, tiles8_per_row);
    const uint32_t n = __float_as_uint(mom[2 * n_pixels + q]);
    float out = pn_inf();
    if (n >= 2u) {
        const float inv_n = 1.0f / (float)n;
        const float mean = mom[q] * inv_n;
        float v = mom[n_pixels + q] * inv_n - mean * mean;
        v = v < 0.0f ? 0.0f : v;
        out = v * (1.0f / (float)(n - 1u));
    }
    variance[p] = out;
}
