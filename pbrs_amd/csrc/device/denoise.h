// device/denoise.h — the two edge-avoiding a-trous denoisers (include/pbrs_gpu.h): the plain one (pbrs_denoise*) and the
// variance-guided one (pbrs_denoise_var*), which is the plain one with the colour stop replaced by SVGF's luminance stop and the variance
// filtered along with the colour.  Both are a post-process over a finished image and its first-hit AOVs; no kernel of the render path is
// involved.  The kernels are written once; what the variance-guided filter does differently stands behind `if constexpr (VAR)`.
//
// k_denoise_pack demodulates and packs the caller's buffers into 16-byte records, so that a tap is two 16-byte loads (a lane's load
// costs the L1 the same at 4 B and at 16 B): colour {c.rgb, 4th word} and guides {normal.xyz, depth}; the instance
// ids sit beside them as one word, read only with PBRS_DENOISE_ID_STOP.  A guide the caller did not give is packed as the value that
// makes its stop 1.0f by the header's own formulas (normal 0: pn_exp(-0) = 1; depth +inf: "both infinite"), so the kernels need no
// variants per guide and give the bits of the stop being off.  k_denoise_atrous<S_LOG2> is one iteration, a gather in the header's
// order (dy outer, dx inner) with no atomics; k_denoise_unpack remodulates.
//
// The colour record's 4th word says whether the pixel counts (it does not outside the image or with a non-finite colour) and is
//   plain:  the finite flag, 1.0f or 0.0f = "does not count";
//   VAR:    the variance v, NaN = "does not count" (the header defines a non-finite colour's variance as +inf, so nothing is lost); a
//           record that counts holds v in [+0, +inf].  A tap stays two 16-byte reads and one compare.
// VAR's 3 x 3 prefilter of the variance reads the ring at distance 1: nine ds_read_b32 of the staged plane (the halo is 2s >= 2), nine
// 4-byte loads in the global variants.  The luminance of c_k(q) is recomputed per tap (three products, two sums: what the plain
// filter's three differences and d2 cost) and not kept in LDS: a fifth word per record would break the 16-byte read, and a separate
// plane adds 4 KB to the 36 KB of s = 4 (the fourth block per CU would no longer fit beside it) and a third ds_read per tap.
#pragma once
#include "path_state.h"

#define PBRS_DENOISE_CELL 16u  // a block owns a 16 x 16 cell of pixels, one thread each

struct DenoiseConst {
    uint32_t w, h;
    float c1;  // the first stop's parameter.  plain: 1.0f / (sc_k * sc_k) of this iteration; VAR: sigma_luminance
    float in;  // 1.0f / (sigma_normal * sigma_normal)
    float id;  // 1.0f / (sigma_depth * sigma_depth)
};

// The caller's guides as the kernels take them: pbrs_denoise_var_guides, the variance NULL for the plain filter.
using DenoiseGuides = pbrs_denoise_var_guides;

__device__ __forceinline__ float denoise_finite_flag(float x, float y, float z) {
    return (pn_isfinite(x) && pn_isfinite(y) && pn_isfinite(z)) ? 1.0f : 0.0f;
}

// d of the header's demodulation for one channel.
__device__ __forceinline__ float denoise_divisor(float a, float albedo_floor) { return a > albedo_floor ? a : 1.0f; }

// The 4th word of a pixel that does not count, and its test.
template <bool VAR>
__device__ __forceinline__ float denoise_skip() {
    return VAR ? pn_nan() : 0.0f;
}
template <bool VAR>
__device__ __forceinline__ bool denoise_skipped(float w4) {
    return VAR ? w4 != w4 : w4 == 0.0f;
}

// g.variance chooses the record: given, {c.rgb, v}; NULL, {c.rgb, finite flag}.
__global__ void __launch_bounds__(256) k_denoise_pack(const float* __restrict__ rgb, DenoiseGuides g, uint32_t n_pixels, uint32_t demodulate,
                                                      float albedo_floor, float4* __restrict__ colour, float4* __restrict__ guide,
                                                      uint32_t* __restrict__ ids) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    float c[3], d[3] = {1.0f, 1.0f, 1.0f};
    for (uint32_t k = 0; k < 3u; ++k) {
        c[k] = rgb[3 * p + k];
        if (demodulate) {
            d[k] = denoise_divisor(g.albedo[3 * p + k], albedo_floor);
            c[k] = c[k] / d[k];
        }
    }
    float w4 = denoise_finite_flag(c[0], c[1], c[2]);
    if (g.variance) {
        float v = g.variance[p];
        if (v != v || v < 0.0f) v = pn_inf();
        if (demodulate) {
            const float ld = luminance(mk3(d[0], d[1], d[2]));
            v = v / (ld * ld);
            if (v != v) v = pn_inf();
        }
        w4 = w4 == 0.0f ? pn_nan() : v;  // does not count
    }
    colour[p] = make_float4(c[0], c[1], c[2], w4);
    float4 gd = make_float4(0.0f, 0.0f, 0.0f, pn_inf());
    if (g.normal) gd.x = g.normal[3 * p], gd.y = g.normal[3 * p + 1], gd.z = g.normal[3 * p + 2];
    if (g.depth) gd.w = g.depth[p];
    guide[p] = gd;
    if (g.instance) ids[p] = g.instance[p];
}

// One tap q of pixel p: the stops of the header, folded into S and W (VAR: and V).  `cq.w` is the staged 4th word.  VAR: lp =
// lum(c_k(p)), sd the header's; plain: neither is read.  inv_s = 1 / (float)s, a power of two: the product is the quotient the header
// writes.
// `vsum` is null without VAR and the skip test is written as "skipped": a fifth sum taken by reference, even an unused one, or the
// opposite branch polarity reorders the accumulators' registers, and the kernels would no longer be the measured ones instruction for
// instruction ("One filter, written once").
template <bool VAR>
__device__ __forceinline__ void denoise_tap(const float4 cq, const float4 gq, const bool same_id, const float4 cp, const float4 gp, const float lp,
                                            const float sd, const float hw, const float inv_s, const DenoiseConst& k, float& s0, float& s1,
                                            float& s2, float& wsum, float* vsum) {
    if (denoise_skipped<VAR>(cq.w)) return;
    float w1;
    if constexpr (VAR) {
        const float dl = pn_abs(luminance(mk3(cq.x, cq.y, cq.z)) - lp);
        if (pn_isinf(sd)) w1 = 1.0f;
        else if (sd == 0.0f) w1 = dl == 0.0f ? 1.0f : 0.0f;
        else w1 = pn_exp(-(dl / sd));
    } else {
        const float er = cq.x - cp.x, eg = cq.y - cp.y, eb = cq.z - cp.z;
        w1 = pn_exp(-((er * er + eg * eg) + eb * eb) * k.c1);
    }
    const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
    const float wn = pn_exp(-((nx * nx + ny * ny) + nz * nz) * k.in);
    const bool pinf = pn_isinf(gp.w), qinf = pn_isinf(gq.w);
    float wd;
    if (pinf || qinf) {
        wd = (pinf && qinf) ? 1.0f : 0.0f;
    } else {
        const float r = ((gq.w - gp.w) / gp.w) * inv_s;
        wd = pn_exp(-(r * r) * k.id);
    }
    float wgt = ((hw * w1) * wn) * wd;
    if (!same_id) wgt = 0.0f;
    if (wgt != wgt) return;
    s0 = s0 + wgt * cq.x;
    s1 = s1 + wgt * cq.y;
    s2 = s2 + wgt * cq.z;
    wsum = wsum + wgt;
    if constexpr (VAR) {
        const float ww = wgt * wgt;
        if (ww != 0.0f) *vsum = *vsum + ww * cq.w;
    }
}

// The B3 spline's product for a tap offset (exact in f32).
__device__ __forceinline__ float denoise_spline(int dx, int dy) {
    const float kx = dx == 0 ? 0.375f : (dx == 1 || dx == -1) ? 0.25f : 0.0625f;
    const float ky = dy == 0 ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f;
    return kx * ky;
}

// One iteration at tap spacing s = 1 << S_LOG2.  At s = 1, 2, 4 the block's (16 + 4s)^2 neighbourhood is reused 16x, 11x and 6x, and
// fits LDS as two float4 planes (12.8, 18 and 32 KB; with the ids 14.4, 20.3 and 36 KB): it is staged there and every tap is two
// ds_read_b128 from static __shared__ arrays (address_space(3), never a flat pointer).  At s >= 8 the reuse inside a block is under
// 3x and 48^2 x 32 B would leave one or two blocks per CU: the taps are read from global memory (the planes live in the L2 /
// Infinity Cache: 2 M pixels x 32 B = 66 MB).
template <uint32_t S_LOG2, bool IDS, bool VAR>
__global__ void __launch_bounds__(256) k_denoise_atrous(const float4* __restrict__ cin, const float4* __restrict__ guide, const uint32_t* __restrict__ ids,
                                                        float4* __restrict__ cout, DenoiseConst k) {
    constexpr int s = 1 << S_LOG2;
    constexpr bool STAGED = S_LOG2 <= 2u;
    constexpr uint32_t T = PBRS_DENOISE_CELL + 4u * (uint32_t)s;  // staged neighbourhood, per axis
    constexpr uint32_t NS = STAGED ? T * T : 1u;
    constexpr float inv_s = 1.0f / (float)s;
    __shared__ float4 lds_c[NS];
    __shared__ float4 lds_g[NS];
    __shared__ uint32_t lds_i[IDS ? NS : 1u];
    const uint32_t lx = threadIdx.x % PBRS_DENOISE_CELL, ly = threadIdx.x / PBRS_DENOISE_CELL;
    const uint32_t cx = blockIdx.x * PBRS_DENOISE_CELL, cy = blockIdx.y * PBRS_DENOISE_CELL;
    const uint32_t x = cx + lx, y = cy + ly;
    const bool own = x < k.w && y < k.h;
    const uint32_t p = y * k.w + x;
    if constexpr (STAGED) {
        for (uint32_t i = threadIdx.x; i < NS; i += 256u) {
            const uint32_t sy = i / T, sx = i - sy * T;
            const int qx = (int)(cx + sx) - 2 * s, qy = (int)(cy + sy) - 2 * s;
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g = c;
            c.w = denoise_skip<VAR>();
            uint32_t id = 0u;
            if (qx >= 0 && qx < (int)k.w && qy >= 0 && qy < (int)k.h) {
                const uint32_t q = (uint32_t)qy * k.w + (uint32_t)qx;
                c = cin[q];
                g = guide[q];
                if (IDS) id = ids[q];
            }
            lds_c[i] = c;
            lds_g[i] = g;
            if (IDS) lds_i[i] = id;
        }
        __syncthreads();
    }
    if (!own) return;
    float4 cp, gp;
    uint32_t idp = 0u;
    if constexpr (STAGED) {
        const uint32_t i = (ly + 2u * s) * T + lx + 2u * s;
        cp = lds_c[i];
        gp = lds_g[i];
        if (IDS) idp = lds_i[i];
    } else {
        cp = cin[p];
        gp = guide[p];
        if (IDS) idp = ids[p];
    }
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, wsum = 0.0f, vsum = 0.0f;
    if (!denoise_skipped<VAR>(cp.w)) {
        float lp = 0.0f, sd = 0.0f;
        if constexpr (VAR) {
            // the prefiltered variance: 3 x 3 at spacing 1 whatever s is, fetched together like a row of taps
            float vn[9];
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int j = 3 * (dy + 1) + dx + 1;
                    if constexpr (STAGED) {
                        vn[j] = lds_c[(uint32_t)((int)ly + 2 * s + dy) * T + (uint32_t)((int)lx + 2 * s + dx)].w;
                    } else {
                        const int qx = (int)x + dx, qy = (int)y + dy;
                        const bool inside = qx >= 0 && qx < (int)k.w && qy >= 0 && qy < (int)k.h;
                        vn[j] = cin[inside ? (uint32_t)qy * k.w + (uint32_t)qx : p].w;
                        if (!inside) vn[j] = pn_nan();
                    }
                }
            }
            float A = 0.0f, B = 0.0f;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const float G = j == 4 ? 0.25f : (j & 1) ? 0.125f : 0.0625f;
                if (pn_isfinite(vn[j])) {
                    A = A + G * vn[j];
                    B = B + G;
                }
            }
            const float vbar = B == 0.0f ? pn_inf() : A * (1.0f / B);
            sd = k.c1 * pn_sqrt(vbar);
            lp = luminance(mk3(cp.x, cp.y, cp.z));
        }
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
            // a row's five taps are fetched together (pinned: left alone the compiler sinks each load behind the previous tap's
            // branches and a row costs five round trips instead of one), then folded in order
            float4 cq[5], gq[5];
            uint32_t idq[5] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int j = dx + 2;
                if constexpr (STAGED) {
                    const uint32_t i = (uint32_t)((int)ly + 2 * s + s * dy) * T + (uint32_t)((int)lx + 2 * s + s * dx);
                    cq[j] = lds_c[i];
                    gq[j] = lds_g[i];
                    if (IDS) idq[j] = lds_i[i];
                } else {
                    const int qx = (int)x + s * dx, qy = (int)y + s * dy;
                    const bool inside = qx >= 0 && qx < (int)k.w && qy >= 0 && qy < (int)k.h;
                    const uint32_t q = inside ? (uint32_t)qy * k.w + (uint32_t)qx : p;
                    cq[j] = cin[q];
                    gq[j] = guide[q];
                    if (IDS) idq[j] = ids[q];
                    if (!inside) cq[j].w = denoise_skip<VAR>();
                }
            }
#pragma unroll
            for (int j = 0; j < 5; ++j) asm volatile("" : "+v"(cq[j].x), "+v"(cq[j].y), "+v"(cq[j].z), "+v"(cq[j].w), "+v"(gq[j].x), "+v"(gq[j].y), "+v"(gq[j].z), "+v"(gq[j].w));
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx)
                denoise_tap<VAR>(cq[dx + 2], gq[dx + 2], idq[dx + 2] == idp, cp, gp, lp, sd, denoise_spline(dx, dy), inv_s, k, s0, s1, s2, wsum,
                                 VAR ? &vsum : nullptr);
        }
    }
    float4 out = cp;
    if (wsum != 0.0f) {
        const float iw = 1.0f / wsum;
        out.x = s0 * iw;
        out.y = s1 * iw;
        out.z = s2 * iw;
        if constexpr (VAR) {
            float v = vsum * (iw * iw);
            if (v != v) v = pn_inf();
            out.w = denoise_finite_flag(out.x, out.y, out.z) != 0.0f ? v : pn_nan();
        } else {
            out.w = denoise_finite_flag(out.x, out.y, out.z);
        }
    }
    cout[p] = out;
}

// out = c_N * d, row-major RGB, and the filtered variance where it is wanted (the variance-guided filter only); d as k_denoise_pack
// takes it.
__global__ void __launch_bounds__(256) k_denoise_unpack(const float4* __restrict__ colour, const float* __restrict__ albedo, uint32_t n_pixels,
                                                        uint32_t demodulate, float albedo_floor, float* __restrict__ rgb,
                                                        float* __restrict__ variance_out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    const float4 c4 = colour[p];
    const float c[3] = {c4.x, c4.y, c4.z};
    float d[3] = {1.0f, 1.0f, 1.0f};
    for (uint32_t k = 0; k < 3u; ++k) {
        float v = c[k];
        if (demodulate) {
            d[k] = denoise_divisor(albedo[3 * p + k], albedo_floor);
            v = v * d[k];
        }
        rgb[3 * p + k] = v;
    }
    if (variance_out) {
        float v = c4.w != c4.w ? pn_inf() : c4.w;
        if (demodulate) {
            const float ld = luminance(mk3(d[0], d[1], d[2]));
            v = v * (ld * ld);
        }
        variance_out[p] = v;
    }
}
