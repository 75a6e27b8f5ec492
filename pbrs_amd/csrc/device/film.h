// device/film.h — the filtered film (include/pbrs_gpu.h, pbrs_render_tile_filtered*): the pass's samples reconstructed with a
// pixel filter instead of k_accumulate's plain per-pixel sum.
//
// A gather, not a scatter: every output pixel folds the samples of its (2hx+1) x (2hy+1) neighbourhood itself, in the
// order the header prescribes (sample index, then dy, then dx), so no atomics and the same bits whatever the launch shape.
// The pass traces the tile plus its halo (the "region", clipped to the film); its radiance sits in st.L by the region's
// slot order.  State: planar f32 by row-major TILE pixel, 4 planes: S.rgb, W (zeroed by render_common).
#pragma once
#include "path_state.h"
#include "../../../include/pbrs_filter.h"

#define PBRS_FILTER_CELL 16u  // a block owns a 16 x 16 cell of tile pixels, one thread each

struct FilterConst {
    uint32_t kind;
    float rx, ry, a, b;
    uint32_t hx, hy;          // halo per axis, pf_halo(r) <= 4
    uint32_t x0, y0, w, h;    // the tile, in film pixels (the region is RenderConst's x0, y0, w, h)
};

// LDS per block: per staged sample of the (16 + 2hx) x (16 + 2hy) neighbourhood a float4 {L.rgb, support mask} and its 1-D
// factors, plane by offset: fx[j][s] for output pixel col - (j - hx), fy[j][s] for row - (j - hy).  Planes keep the gather's
// reads contiguous across a row of lanes (LDS banks).  At h = 4: 576 x (16 + 72) B = 50.7 KB, three blocks per CU.
inline size_t filter_lds_bytes(uint32_t hx, uint32_t hy) {
    const size_t ns = (size_t)(PBRS_FILTER_CELL + 2 * hx) * (PBRS_FILTER_CELL + 2 * hy);
    return ns * (sizeof(float4) + sizeof(float) * (2 * hx + 1 + 2 * hy + 1));
}

// One block per 16 x 16 cell of the tile.  For each of the pass's kc sample indices: stage the neighbourhood's samples
// (radiance from st.L through the region's slot order, jitter recomputed as k_raygen draws it, the factors of every offset
// and the support mask), then each thread folds its (2hx+1)(2hy+1) terms.  Non-finite samples of the cell's own pixels are
// counted while staging (pbrs_stats.invalid_samples: the tile's pixels only, as the plain render counts them).
__global__ void __launch_bounds__(256) k_filter_accumulate(PathState st, float* fsum, RenderConst rc, FilterConst f, uint32_t kc,
                                                           unsigned long long* nonfinite) {
    extern __shared__ float4 filter_lds[];
    const uint32_t sw = PBRS_FILTER_CELL + 2 * f.hx, sh = PBRS_FILTER_CELL + 2 * f.hy, ns = sw * sh;
    const uint32_t nx = 2 * f.hx + 1, ny = 2 * f.hy + 1;
    float4* rec = filter_lds;
    float* fx = reinterpret_cast<float*>(rec + ns);
    float* fy = fx + nx * ns;
    const uint32_t lx = threadIdx.x % PBRS_FILTER_CELL, ly = threadIdx.x / PBRS_FILTER_CELL;
    const uint32_t cx = blockIdx.x * PBRS_FILTER_CELL, cy = blockIdx.y * PBRS_FILTER_CELL;  // the cell, in tile pixels
    const bool own = cx + lx < f.w && cy + ly < f.h;
    const uint32_t P = f.w * f.h, p = (cy + ly) * f.w + cx + lx;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, wsum = 0.0f;
    if (own) s0 = fsum[p], s1 = fsum[P + p], s2 = fsum[2 * P + p], wsum = fsum[3 * P + p];
    // film column / row of staged sample (0, 0); may be negative (outside the film: nothing staged there)
    const int col0 = (int)(f.x0 + cx) - (int)f.hx, row0 = (int)(f.y0 + cy) - (int)f.hy;
    uint32_t bad = 0;
    for (uint32_t k = 0; k < kc; ++k) {
        const uint32_t i = rc.pass_first_sample + k;
        for (uint32_t s = threadIdx.x; s < ns; s += blockDim.x) {
            const uint32_t sy = s / sw, sx = s - sy * sw;
            const int col = col0 + (int)sx, row = row0 + (int)sy;
            uint32_t mask = 0;
            f3 L = gray(0.0f);
            if (col >= (int)rc.x0 && col < (int)(rc.x0 + rc.w) && row >= (int)rc.y0 && row < (int)(rc.y0 + rc.h)) {
                const uint32_t pix = ((uint32_t)row - rc.y0) * rc.w + ((uint32_t)col - rc.x0);
                L = xyz(st.L[slot_of_sample(k, order_of_pixel(pix, rc.w, rc.tiles8_per_row), rc.n_pixels, kc, rc.chunk_pixels)]);
                // the cell's own pixels (inside the tile): what the plain render would count
                if (sx - f.hx < PBRS_FILTER_CELL && sy - f.hy < PBRS_FILTER_CELL && (uint32_t)col < f.x0 + f.w && (uint32_t)row < f.y0 + f.h)
                    bad += (pn_isfinite(L.x) && pn_isfinite(L.y) && pn_isfinite(L.z)) ? 0u : 1u;
                // k_raygen's jitter (kernels.h)
                uint64_t rng = pn_rng_init(rc.seed, (uint32_t)row * rc.cam.width + (uint32_t)col, i);
                const float r0 = pn_rng_f32(&rng), r1 = pn_rng_f32(&rng);
                const float jx = ((float)(i / rc.strata_y) + r0) / (float)rc.strata_x;
                const float jy = ((float)(i % rc.strata_y) + r1) / (float)rc.strata_y;
                const float xs = (float)col + pn_fract(jx);
                const float ys = (float)row + pn_fract(jy);
                // offset j: the output pixel j - h to the left of / above this sample's pixel
                for (uint32_t j = 0; j < nx; ++j) {
                    const float o = xs - ((float)(col - ((int)j - (int)f.hx)) + 0.5f);
                    const bool in = pn_abs(o) <= f.rx;
                    fx[j * ns + s] = in ? pf_factor(f.kind, o, f.rx, f.a, f.b) : 0.0f;
                    mask |= in ? 1u << j : 0u;
                }
                for (uint32_t j = 0; j < ny; ++j) {
                    const float o = ys - ((float)(row - ((int)j - (int)f.hy)) + 0.5f);
                    const bool in = pn_abs(o) <= f.ry;
                    fy[j * ns + s] = in ? pf_factor(f.kind, o, f.ry, f.a, f.b) : 0.0f;
                    mask |= in ? 1u << (16 + j) : 0u;
                }
            }
            rec[s] = pack4(L, mask);
        }
        __syncthreads();
        if (own) {
            for (uint32_t jy = 0; jy < ny; ++jy) {      // dy = jy - hy
                for (uint32_t jx = 0; jx < nx; ++jx) {  // dx = jx - hx
                    const uint32_t s = (ly + jy) * sw + lx + jx;
                    const float4 r = rec[s];
                    const uint32_t m = __float_as_uint(r.w);
                    if ((m >> jx) & (m >> (16 + jy)) & 1u) {
                        const float w = fx[jx * ns + s] * fy[jy * ns + s];
                        s0 = s0 + w * r.x;
                        s1 = s1 + w * r.y;
                        s2 = s2 + w * r.z;
                        wsum = wsum + w;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (own) fsum[p] = s0, fsum[P + p] = s1, fsum[2 * P + p] = s2, fsum[3 * P + p] = wsum;
    if (__ballot(bad != 0u)) {
        for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
        if ((threadIdx.x & 63u) == 0) atomicAdd(nonfinite, (unsigned long long)bad);
    }
}

// W == 0: 0; else S * (1 / W), negative lobes clamped to +0 (a NaN stays a NaN).  Row-major RGB of the tile's pixels.
__global__ void __launch_bounds__(256) k_filter_finalize(const float* fsum, float* rgb, uint32_t n_pixels) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    const float w = fsum[3 * n_pixels + p];
    for (uint32_t c = 0; c < 3u; ++c) {
        float v = 0.0f;
        if (w != 0.0f) {
            v = fsum[c * n_pixels + p] * (1.0f / w);
            v = v < 0.0f ? 0.0f : v;
        }
        rgb[3 * p + c] = v;
    }
}
