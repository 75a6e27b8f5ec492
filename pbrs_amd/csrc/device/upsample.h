// device/upsample.h — guided upsampling (include/pbrs_gpu.h, pbrs_upsample*): a low-resolution image rebuilt at full size by joint
// bilateral upsampling, the weights taken between the low-resolution guides and the full-resolution ones.  A post-process like the
// denoisers: no kernel of the render path is involved.
//
// k_upsample<F, R, IDS> in the mould of k_denoise_atrous: one thread per full pixel, a 256-thread block per 16 x 16 full-resolution cell,
// one launch, no atomics and no scratch.  The cell's pixels reach ceil(15 / F) + 2R low pixels per axis (12 at F = 2, R = 2): the block
// stages them in LDS once as 16-byte records, colour {c.rgb, counts (1.0f / 0.0f)}, demodulated as it is staged, and guides {normal.xyz,
// depth}, with IDS a word of ids beside them: at most 144 records of 36 B, 5.2 KB.  A low pixel outside the image is staged as "does not
// count" and no index outside a plane is ever formed.  A guide pair the call does not have is staged (and loaded for p) as the value
// that makes its stop 1.0f by the header's own formulas (normal 0: pn_exp(-0) = 1; depth +inf: "both infinite"), as k_denoise_pack does
// it, so only the id stop, the factor and the radius are template parameters: 12 kernels, each with its taps fully unrolled.  A tap is
// two ds_read_b128; a thread loads its own full-resolution guides straight from memory.
//
// The tent.  With x = F * k + m the integer nx of the header for the j-th tap of a row, X = X0 - R + 1 + j, is
// |2F * (floor_div(2m + 1 - F, 2F) - R + 1 + j) + F - 2m - 1|: it depends on m = x mod F and on j alone, and the same holds for y.  The
// block's first F * 2R threads write (float)(D - n) / (float)D, or -1.0f for "n >= D: skipped", into a table in LDS; a thread reads its
// 2R factors per axis from it and a tap's hw is one product.  A cell starts at a multiple of 16, so m is x mod F whatever F is.
#pragma once
#include "denoise.h"  // PBRS_DENOISE_CELL, denoise_divisor, denoise_finite_flag

struct UpsampleConst {
    uint32_t w, h;    // the full size
    uint32_t wl, hl;  // the low size
    float in;         // 1.0f / (sigma_normal * sigma_normal)
    float id;         // 1.0f / (sigma_depth * sigma_depth)
    float albedo_floor;
    float min_weight;
};

// The caller's planes as the kernel takes them (pointers at the caller's layouts), low then full.  The albedos are null without
// PBRS_UPSAMPLE_DEMODULATE, a normal or depth pair is null when the stop is off, the ids are read with IDS only.
struct UpsampleIn {
    const float* rgb_lo;
    const float* albedo_lo;
    const float* normal_lo;
    const float* depth_lo;
    const uint32_t* id_lo;
    const float* albedo_hi;
    const float* normal_hi;
    const float* depth_hi;
    const uint32_t* id_hi;
};

__device__ __forceinline__ int upsample_floor_div(int a, int b) {  // b > 0
    const int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

template <uint32_t F, uint32_t R, bool IDS>
__global__ void __launch_bounds__(256) k_upsample(UpsampleIn in, float* __restrict__ out, float* __restrict__ weight_out, UpsampleConst k) {
    constexpr uint32_t NT = 2u * R;                                     // taps per axis
    constexpr uint32_t T = (PBRS_DENOISE_CELL - 1u + F - 1u) / F + NT;  // staged low pixels per axis
    constexpr uint32_t NS = T * T;
    constexpr int D = (int)(2u * F * R);
    static_assert(NS <= 256u, "one staging pass");
    __shared__ float4 lds_c[NS];  // {c.rgb, 1.0f / 0.0f = "does not count"}
    __shared__ float4 lds_g[NS];  // {normal.xyz, depth}
    __shared__ uint32_t lds_i[IDS ? NS : 1u];
    __shared__ float lds_tent[F * NT];
    const uint32_t lx = threadIdx.x % PBRS_DENOISE_CELL, ly = threadIdx.x / PBRS_DENOISE_CELL;
    const uint32_t cx = blockIdx.x * PBRS_DENOISE_CELL, cy = blockIdx.y * PBRS_DENOISE_CELL;
    // the first low pixel the cell reaches, per axis (may be negative)
    const int bx = upsample_floor_div(2 * (int)cx + 1 - (int)F, 2 * (int)F) - (int)R + 1;
    const int by = upsample_floor_div(2 * (int)cy + 1 - (int)F, 2 * (int)F) - (int)R + 1;
    if (threadIdx.x < F * NT) {
        const int m = (int)(threadIdx.x / NT), j = (int)(threadIdx.x % NT);
        int n = 2 * (int)F * (upsample_floor_div(2 * m + 1 - (int)F, 2 * (int)F) - (int)R + 1 + j) + (int)F - 2 * m - 1;
        n = n < 0 ? -n : n;
        lds_tent[threadIdx.x] = n < D ? (float)(D - n) / (float)D : -1.0f;
    }
    if (threadIdx.x < NS) {
        const uint32_t i = threadIdx.x, sy = i / T, sx = i - sy * T;
        const int qx = bx + (int)sx, qy = by + (int)sy;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g = c;
        uint32_t id = 0u;
        if (qx >= 0 && qx < (int)k.wl && qy >= 0 && qy < (int)k.hl) {
            const uint32_t q = (uint32_t)qy * k.wl + (uint32_t)qx;
            c.x = in.rgb_lo[3 * q], c.y = in.rgb_lo[3 * q + 1], c.z = in.rgb_lo[3 * q + 2];
            if (in.albedo_lo) {
                c.x = c.x / denoise_divisor(in.albedo_lo[3 * q], k.albedo_floor);
                c.y = c.y / denoise_divisor(in.albedo_lo[3 * q + 1], k.albedo_floor);
                c.z = c.z / denoise_divisor(in.albedo_lo[3 * q + 2], k.albedo_floor);
            }
            c.w = denoise_finite_flag(c.x, c.y, c.z);
            if (in.normal_lo) g.x = in.normal_lo[3 * q], g.y = in.normal_lo[3 * q + 1], g.z = in.normal_lo[3 * q + 2];
            g.w = in.depth_lo ? in.depth_lo[q] : pn_inf();
            if (IDS) id = in.id_lo[q];
        }
        lds_c[i] = c;
        lds_g[i] = g;
        if (IDS) lds_i[i] = id;
    }
    __syncthreads();
    const uint32_t x = cx + lx, y = cy + ly;
    if (x >= k.w || y >= k.h) return;
    const uint32_t p = y * k.w + x;
    // p's own guides
    float4 gp = make_float4(0.0f, 0.0f, 0.0f, pn_inf());
    if (in.normal_hi) gp.x = in.normal_hi[3 * p], gp.y = in.normal_hi[3 * p + 1], gp.z = in.normal_hi[3 * p + 2];
    if (in.depth_hi) gp.w = in.depth_hi[p];
    uint32_t idp = 0u;
    if (IDS) idp = in.id_hi[p];
    float d0 = 1.0f, d1 = 1.0f, d2 = 1.0f;
    if (in.albedo_hi) {
        d0 = denoise_divisor(in.albedo_hi[3 * p], k.albedo_floor);
        d1 = denoise_divisor(in.albedo_hi[3 * p + 1], k.albedo_floor);
        d2 = denoise_divisor(in.albedo_hi[3 * p + 2], k.albedo_floor);
    }
    const bool pinf = pn_isinf(gp.w);
    // the footprint: its first tap in the tile and the 2R tent factors per axis
    const uint32_t mx = x % F, my = y % F;
    const uint32_t tx = (uint32_t)(upsample_floor_div(2 * (int)x + 1 - (int)F, 2 * (int)F) - (int)R + 1 - bx);
    const uint32_t ty = (uint32_t)(upsample_floor_div(2 * (int)y + 1 - (int)F, 2 * (int)F) - (int)R + 1 - by);
    float hx[NT], hy[NT];
#pragma unroll
    for (uint32_t j = 0; j < NT; ++j) hx[j] = lds_tent[mx * NT + j], hy[j] = lds_tent[my * NT + j];
    float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, V = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, W = 0.0f;
#pragma unroll
    for (uint32_t iy = 0; iy < NT; ++iy) {
        // a row's taps are fetched together, then folded in order (k_denoise_atrous)
        float4 cq[NT], gq[NT];
        uint32_t idq[NT];
#pragma unroll
        for (uint32_t j = 0; j < NT; ++j) {
            const uint32_t i = (ty + iy) * T + tx + j;
            cq[j] = lds_c[i];
            gq[j] = lds_g[i];
            idq[j] = IDS ? lds_i[i] : 0u;
        }
#pragma unroll
        for (uint32_t j = 0; j < NT; ++j) asm volatile("" : "+v"(cq[j].x), "+v"(cq[j].y), "+v"(cq[j].z), "+v"(cq[j].w), "+v"(gq[j].x), "+v"(gq[j].y), "+v"(gq[j].z), "+v"(gq[j].w));
#pragma unroll
        for (uint32_t j = 0; j < NT; ++j) {
            if (hx[j] < 0.0f || hy[iy] < 0.0f || cq[j].w == 0.0f) continue;
            const float hw = hx[j] * hy[iy];
            t0 = t0 + hw * cq[j].x;
            t1 = t1 + hw * cq[j].y;
            t2 = t2 + hw * cq[j].z;
            V = V + hw;
            const float nx = gq[j].x - gp.x, ny = gq[j].y - gp.y, nz = gq[j].z - gp.z;
            const float wn = pn_exp(-((nx * nx + ny * ny) + nz * nz) * k.in);
            const bool qinf = pn_isinf(gq[j].w);
            float wd;
            if (pinf || qinf) {
                wd = (pinf && qinf) ? 1.0f : 0.0f;
            } else {
                const float r = ((gq[j].w - gp.w) / gp.w) / (float)F;
                wd = pn_exp(-(r * r) * k.id);
            }
            float g = (hw * wn) * wd;
            if (IDS && idq[j] != idp) g = 0.0f;
            if (g != g) continue;
            s0 = s0 + g * cq[j].x;
            s1 = s1 + g * cq[j].y;
            s2 = s2 + g * cq[j].z;
            W = W + g;
        }
    }
    float r0, r1, r2;
    if (W > k.min_weight) {
        const float iw = 1.0f / W;
        r0 = s0 * iw, r1 = s1 * iw, r2 = s2 * iw;
    } else if (V > 0.0f) {
        const float iv = 1.0f / V;
        r0 = t0 * iv, r1 = t1 * iv, r2 = t2 * iv;
    } else {
        const float4 cn = lds_c[(uint32_t)((int)(y / F) - by) * T + (uint32_t)((int)(x / F) - bx)];
        r0 = cn.x, r1 = cn.y, r2 = cn.z;
    }
    out[3 * p] = r0 * d0;
    out[3 * p + 1] = r1 * d1;
    out[3 * p + 2] = r2 * d2;
    if (weight_out) weight_out[p] = W;
}
