// device/spatial_variance.h — the spatial variance estimate for pixels with a short temporal history (include/pbrs_gpu.h,
// pbrs_spatial_variance*): SVGF's guide-weighted estimate of the luminance moments over the (2 * radius + 1)^2 neighbourhood, for the
// pixels whose history is shorter than min_temporal and whose variance rule D of the temporal accumulation therefore could not take
// from the moments.  A post-process like the denoisers: no kernel of the render path is involved.
//
// One thread per pixel in 16 x 16 blocks, one launch.  A block first reads its own pixels' length and variance_in and votes on "any
// short pixel here": in a converged sequence almost every block has none, writes variance_in through and returns before any halo
// load, so a long-history frame costs about the copy of one plane (8 B read, 4 B written per pixel).  A block with a short pixel stages
// its tile plus a halo of `radius` (at most 22 x 22 pixels) in LDS once, as 16-byte records: {m1, m2, valid, depth}, valid folding
// length > 0 and the two finiteness tests of the tap rule, and with a normal or an id stop a second record {normal.xyz, id}.  That is
// 16 or 32 B per staged pixel, at most 15.5 KB per block, against up to 49 gathers of 4 to 9 words each per pixel; a halo pixel outside
// the image is staged as invalid and no index outside a plane is ever formed.  A depth guide the call does not have is staged as +inf,
// which makes the depth stop 1.0f by the header's own "both infinite" case (as k_denoise_pack does); a missing normal or id guide is a
// template parameter, as in k_temporal.  The taps keep the header's order (dy outer, dx inner) with sequential f32 sums; the radius is
// a runtime loop bound.  No atomics.
//
// LDS banks.  A tap is one or two ds_read_b128 from rows of T = 16 + 2 * radius records.  The hardware serves a ds_read_b128 in four
// groups of 16 lanes, each made of lanes of two neighbouring pixel rows ("Spatial variance estimate"), which
// is conflict-free only when the row pitch is a multiple of 16 records: at T = 18, 20, 22 two lanes of a group share a 16-byte slot of
// the 256-byte bank row and a read costs 8 LDS cycles instead of 4.  A pitch of 32 records would remove that at 22.5 KB per block; it
// is not taken: a tap's arithmetic (two pn_exp) is an order of magnitude above its LDS cycles either way.
#pragma once
#include "denoise.h"  // PBRS_DENOISE_CELL

#define PBRS_SPATIAL_MAX_TILE (PBRS_DENOISE_CELL + 2u * PBRS_SPATIAL_MAX_RADIUS)  // 22

struct SpatialVarConst {
    uint32_t w, h;
    uint32_t radius;        // 1 .. PBRS_SPATIAL_MAX_RADIUS
    uint32_t only_unknown;  // PBRS_SPATIAL_ONLY_UNKNOWN
    float in;               // 1.0f / (sigma_normal * sigma_normal)
    float id;               // 1.0f / (sigma_depth * sigma_depth)
    float min_temporal;
};

// The caller's planes as the kernel takes them (pointers at the caller's layouts).  variance_out may be variance_in: a pixel reads only
// its own variance_in, before the block's vote, and is the only one that writes it.
struct SpatialVarIn {
    const float* moments;
    const float* length;
    const float* depth;        // null: the stop is off
    const float* normal;       // read with NORMAL
    const uint32_t* instance;  // read with IDS
    const float* variance;
};

template <bool NORMAL, bool IDS>
__global__ void __launch_bounds__(256) k_spatial_variance(SpatialVarIn in, float* variance_out, SpatialVarConst k) {
    constexpr bool SECOND = NORMAL || IDS;
    constexpr uint32_t NS = PBRS_SPATIAL_MAX_TILE * PBRS_SPATIAL_MAX_TILE;
    __shared__ float4 lds_a[NS];               // {m1, m2, valid (1.0f / 0.0f), depth}
    __shared__ float4 lds_b[SECOND ? NS : 1u]; // {normal.xyz, id}
    const uint32_t lx = threadIdx.x % PBRS_DENOISE_CELL, ly = threadIdx.x / PBRS_DENOISE_CELL;
    const uint32_t cx = blockIdx.x * PBRS_DENOISE_CELL, cy = blockIdx.y * PBRS_DENOISE_CELL;
    const uint32_t x = cx + lx, y = cy + ly;
    const bool own = x < k.w && y < k.h;
    const uint32_t p = own ? y * k.w + x : 0u;
    float n = 0.0f, vin = 0.0f;
    bool is_short = false;
    if (own) {
        n = in.length[p];
        vin = in.variance[p];
        is_short = n > 0.0f && n < k.min_temporal;  // a NaN length is not short
        if (k.only_unknown && !(vin != vin || vin < 0.0f || vin == pn_inf())) is_short = false;
    }
    // the steady state: no short pixel in this block
    if (!__syncthreads_or(is_short ? 1 : 0)) {
        if (own) variance_out[p] = vin;
        return;
    }
    const uint32_t r = k.radius, T = PBRS_DENOISE_CELL + 2u * r;
    for (uint32_t i = threadIdx.x; i < T * T; i += 256u) {
        const uint32_t sy = i / T, sx = i - sy * T;
        const int qx = (int)(cx + sx) - (int)r, qy = (int)(cy + sy) - (int)r;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
        if (qx >= 0 && qx < (int)k.w && qy >= 0 && qy < (int)k.h) {
            const uint32_t q = (uint32_t)qy * k.w + (uint32_t)qx;
            const float lq = in.length[q];
            a.x = in.moments[2 * q], a.y = in.moments[2 * q + 1];
            a.z = (lq > 0.0f && pn_isfinite(a.x) && pn_isfinite(a.y)) ? 1.0f : 0.0f;
            a.w = in.depth ? in.depth[q] : pn_inf();
            if (NORMAL) b.x = in.normal[3 * q], b.y = in.normal[3 * q + 1], b.z = in.normal[3 * q + 2];
            if (IDS) b.w = __uint_as_float(in.instance[q]);
        }
        lds_a[i] = a;
        if (SECOND) lds_b[i] = b;
    }
    __syncthreads();
    if (!own) return;
    float out = vin;
    if (is_short) {
        const uint32_t ci = (ly + r) * T + lx + r;
        const float4 ap = lds_a[ci];
        float4 bp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (SECOND) bp = lds_b[ci];
        const bool pinf = pn_isinf(ap.w);
        float M1 = 0.0f, M2 = 0.0f, W = 0.0f;
        const int ri = (int)r;
        for (int dy = -ri; dy <= ri; ++dy) {
            const uint32_t row = (uint32_t)((int)(ly + r) + dy) * T + lx + r;
            for (int dx = -ri; dx <= ri; ++dx) {
                const uint32_t i = (uint32_t)((int)row + dx);
                const float4 aq = lds_a[i];
                if (aq.z == 0.0f) continue;
                float4 bq = bp;
                if (SECOND) bq = lds_b[i];
                float wn = 1.0f;
                if (NORMAL) {
                    const float nx = bq.x - bp.x, ny = bq.y - bp.y, nz = bq.z - bp.z;
                    wn = pn_exp(-((nx * nx + ny * ny) + nz * nz) * k.in);
                }
                const bool qinf = pn_isinf(aq.w);
                float wd;
                if (pinf || qinf) {
                    wd = (pinf && qinf) ? 1.0f : 0.0f;
                } else {
                    const float rr = (aq.w - ap.w) / ap.w;  // s = 1
                    wd = pn_exp(-(rr * rr) * k.id);
                }
                float wgt = wn * wd;  // (1.0f * wn) * wd
                if (IDS && __float_as_uint(bq.w) != __float_as_uint(bp.w)) wgt = 0.0f;
                if (wgt != wgt) continue;
                M1 = M1 + wgt * aq.x;
                M2 = M2 + wgt * aq.y;
                W = W + wgt;
            }
        }
        if (W != 0.0f) {
            const float iw = 1.0f / W;
            const float a = M1 * iw, b = M2 * iw;
            float v = b - a * a;
            v = v < 0.0f ? 0.0f : v;
            if (v != v) v = pn_inf();
            out = v * (1.0f / n);
        }
    }
    variance_out[p] = out;
}
