// device/compare.h — image comparison (include/pbrs_gpu.h, pbrsx_compare*): MSE, relative MSE, MAE, the largest difference and SSIM of an
// image against a reference, with per-pixel maps.  A post-process like the denoisers: no kernel of the render path is involved.  Two
// kernels, wave64:
//
//   k_compare_tile<TRANSFORM, SSIM>  one 256-thread block per PBRS_COMPARE_TILE x PBRS_COMPARE_TILE tile, one pixel per thread, thread
//                      16 * ty + tx at (tx, ty): a wave holds four rows, so lane order is the tile's row-major order.  With SSIM the block
//                      stages x, y and m of the 26 x 26 tile plus halo in LDS (+0 outside the image and at invalid pixels: adding
//                      g * +0 to a sum that starts at +0 is the skipped tap, bit for bit), runs the row pass into LDS (26 rows x 16
//                      columns x 6 fields) and takes the column pass from there.  Without SSIM none of that exists: no halo, no LDS
//                      tile, no second pass.  Every thread forms its f64 terms; the block reduces them in the contract's order: inside
//                      a wave lane i adds lane i ^ 1, then i ^ 2, ... i ^ 32, which is the adjacent-pair tree (both lanes of a pair
//                      form the same sum: addition commutes), across the four waves (w0 + w1) + (w2 + w3) through LDS.  One record
//                      of partials per tile: pbrs_compare_result's fields with sums in the place of means, planar (CompareRecords).
//   k_compare_finish   one 1024-thread block: the tile records, row-major, reduced by the same tree level by level, a level's odd last
//                      record joined with +0.0.  While more than 512 records are left a thread joins four into one, two levels of the
//                      tree, from one buffer into the other and back (no trip reads what it writes); the last 512 go through LDS, a
//                      level per trip.  Then the divisions, and the 64-byte result.  (One level per trip through memory took 13 trips
//                      for a 1920 x 1080 image and more time than k_compare_tile: DESIGN.md section 4, "Image comparison".)
//
// No atomics, no float value that depends on which block finishes first; every value is written with an ordinary vector-memory store.
//
// LDS banking (ds_read_b32: bank = dword % 32 per 32-lane half).  Column pass: a half reads two 16-float rows that follow each other,
// 32 consecutive dwords, no conflict.  Row pass: a half reads 16 + 16 consecutive dwords of two tile rows 26 apart, which overlap in ten
// banks: two-way on those lanes.  A pitch of 48 would free them at 7 KiB more LDS per block; the row pass is some 54 of a thread's 120
// LDS reads, and only ten lanes of a half pay.  k_compare_finish's LDS levels read every second f64 of a plane (ds_read_b64, 64 banks:
// lanes l and l + 16 of a half share banks, two-way) and write consecutive ones.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/pbrs_gpu.h"
#include "../../../include/pbrs_numeric.h"

constexpr uint32_t kCompareBlock = PBRS_COMPARE_TILE * PBRS_COMPARE_TILE;
constexpr uint32_t kCompareHalo = 5;                                       // the 11-tap window's reach
constexpr uint32_t kCompareSpan = PBRS_COMPARE_TILE + 2u * kCompareHalo;   // 26
constexpr uint32_t kCompareFinishBlock = 1024;
constexpr uint32_t kCompareFinishLds = 512;  // records k_compare_finish reduces in LDS (26 KiB, planar)
static_assert(kCompareBlock == 256 && PBRS_COMPARE_TILE == 16u, "k_compare_tile: four waves of four 16-pixel rows");

struct CompareConst {
    uint32_t w, h, tiles_x;
    float peak;
    double eps;
    float* error_out;  // null: not wanted
    float* ssim_out;   // null: not wanted
};

// Records of partials in memory, planar: field f of record i at sums[f * stride + i] (T(se), T(re), T(ae), T(ssim), the largest
// difference: pbrs_compare_result's order) and counts[f * stride + i] (n_valid, n_invalid, n_ssim), so that the lanes of a wave read
// neighbouring words; k_compare_finish's LDS copy has the same layout.  In registers a record is a pbrs_compare_result with sums in the
// place of means.
struct CompareRecords {
    double* sums;
    uint32_t* counts;
    uint32_t stride;
};
__device__ __forceinline__ pbrs_compare_result compare_get(const CompareRecords& s, uint32_t i) {
    pbrs_compare_result r{};
    r.mse = s.sums[i], r.rel_mse = s.sums[s.stride + i], r.mae = s.sums[2u * s.stride + i], r.ssim = s.sums[3u * s.stride + i];
    r.max_abs = s.sums[4u * s.stride + i];
    r.n_valid = s.counts[i], r.n_invalid = s.counts[s.stride + i], r.n_ssim = s.counts[2u * s.stride + i];
    return r;
}
__device__ __forceinline__ void compare_put(const CompareRecords& s, uint32_t i, const pbrs_compare_result& r) {
    s.sums[i] = r.mse, s.sums[s.stride + i] = r.rel_mse, s.sums[2u * s.stride + i] = r.mae, s.sums[3u * s.stride + i] = r.ssim;
    s.sums[4u * s.stride + i] = r.max_abs;
    s.counts[i] = r.n_valid, s.counts[s.stride + i] = r.n_invalid, s.counts[2u * s.stride + i] = r.n_ssim;
}

template <uint32_t TRANSFORM>
__device__ __forceinline__ float compare_transform(float x) {
    if (TRANSFORM == PBRS_COMPARE_LINEAR) return x;
    const float xp = x < 0.0f ? 0.0f : x;
    return xp / (1.0f + xp);
}

__device__ __forceinline__ float compare_luminance(const float (&c)[3]) { return (0.21267127f * c[0] + 0.71515972f * c[1]) + 0.07216883f * c[2]; }

// Pixel p of both images, transformed -> whether it is valid (ta and tb mean nothing where it is not).
template <uint32_t TRANSFORM>
__device__ __forceinline__ bool compare_load(const float* a, const float* b, size_t p, float (&ta)[3], float (&tb)[3]) {
    bool valid = true;
    for (uint32_t i = 0; i < 3; ++i) {
        const float va = a[3 * p + i], vb = b[3 * p + i];
        valid = valid && pn_isfinite(va) && pn_isfinite(vb);
        ta[i] = compare_transform<TRANSFORM>(va), tb[i] = compare_transform<TRANSFORM>(vb);
    }
    return valid;
}

// The sum of `v` over the wave in the adjacent-pair order, in every lane.
__device__ __forceinline__ double compare_wave_sum(double v) {
    for (uint32_t d = 1; d < 64u; d <<= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ double compare_wave_max(double v) {
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const double o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

template <uint32_t TRANSFORM, bool SSIM>
__global__ void __launch_bounds__(256) k_compare_tile(const float* a, const float* b, CompareRecords tiles, CompareConst k) {
    const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
    const uint32_t tile_y = blockIdx.x / k.tiles_x, tile_x = blockIdx.x - tile_y * k.tiles_x;
    const uint32_t x0 = tile_x * PBRS_COMPARE_TILE, y0 = tile_y * PBRS_COMPARE_TILE, x = x0 + tx, y = y0 + ty;
    const bool inside = x < k.w && y < k.h;
    const size_t p = (size_t)y * k.w + x;
    float ta[3], tb[3];
    const bool valid = inside && compare_load<TRANSFORM>(a, b, p, ta, tb);

    double se = 0.0, ae = 0.0, re = 0.0, mx = 0.0;
    if (valid) {
        double D[3], R[3];
        for (uint32_t i = 0; i < 3; ++i) {
            const double B = (double)tb[i];
            D[i] = (double)ta[i] - B;
            R[i] = D[i] * D[i] / (B * B + k.eps);
        }
        se = (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2];
        ae = (fabs(D[0]) + fabs(D[1])) + fabs(D[2]);
        re = (R[0] + R[1]) + R[2];
        mx = fabs(D[0]) > fabs(D[1]) ? fabs(D[0]) : fabs(D[1]);
        mx = fabs(D[2]) > mx ? fabs(D[2]) : mx;
    }

    float s = 0.0f;
    bool kept = false;
    if constexpr (SSIM) {
        __shared__ float fx[kCompareSpan * kCompareSpan], fy[kCompareSpan * kCompareSpan], fm[kCompareSpan * kCompareSpan];
        __shared__ float rows[6][kCompareSpan * PBRS_COMPARE_TILE];
        const float g[11] = {PBRS_COMPARE_G5, PBRS_COMPARE_G4, PBRS_COMPARE_G3, PBRS_COMPARE_G2, PBRS_COMPARE_G1, PBRS_COMPARE_G0,
                             PBRS_COMPARE_G1, PBRS_COMPARE_G2, PBRS_COMPARE_G3, PBRS_COMPARE_G4, PBRS_COMPARE_G5};
        for (uint32_t i = tid; i < kCompareSpan * kCompareSpan; i += kCompareBlock) {
            const uint32_t r = i / kCompareSpan, c = i - r * kCompareSpan;
            const int64_t qx = (int64_t)x0 + c - kCompareHalo, qy = (int64_t)y0 + r - kCompareHalo;
            float vx = 0.0f, vy = 0.0f, vm = 0.0f;
            if (qx >= 0 && qx < (int64_t)k.w && qy >= 0 && qy < (int64_t)k.h) {
                float qa[3], qb[3];
                if (compare_load<TRANSFORM>(a, b, (size_t)qy * k.w + (size_t)qx, qa, qb)) vx = compare_luminance(qa), vy = compare_luminance(qb), vm = 1.0f;
            }
            fx[i] = vx, fy[i] = vy, fm[i] = vm;
        }
        __syncthreads();
        for (uint32_t o = tid; o < kCompareSpan * PBRS_COMPARE_TILE; o += kCompareBlock) {
            const uint32_t at = (o >> 4) * kCompareSpan + (o & 15u);
            float A[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (uint32_t j = 0; j < 11; ++j) {
                const float vx = fx[at + j], vy = fy[at + j], vm = fm[at + j];
                A[0] = A[0] + g[j] * vm;
                A[1] = A[1] + g[j] * vx;
                A[2] = A[2] + g[j] * vy;
                A[3] = A[3] + g[j] * (vx * vx);
                A[4] = A[4] + g[j] * (vy * vy);
                A[5] = A[5] + g[j] * (vx * vy);
            }
#pragma unroll
            for (uint32_t f = 0; f < 6; ++f) rows[f][o] = A[f];
        }
        __syncthreads();
        if (valid) {
            float S[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (uint32_t j = 0; j < 11; ++j) {
#pragma unroll
                for (uint32_t f = 0; f < 6; ++f) S[f] = S[f] + g[j] * rows[f][(ty + j) * PBRS_COMPARE_TILE + tx];
            }
            const float iw = 1.0f / S[0], ux = S[1] * iw, uy = S[2] * iw;
            const float sxx = S[3] * iw - ux * ux, syy = S[4] * iw - uy * uy, sxy = S[5] * iw - ux * uy;
            const float C1 = (0.01f * k.peak) * (0.01f * k.peak), C2 = (0.03f * k.peak) * (0.03f * k.peak);
            s = ((2.0f * (ux * uy) + C1) * (2.0f * sxy + C2)) / (((ux * ux + uy * uy) + C1) * ((sxx + syy) + C2));
            kept = pn_isfinite(s);
        }
    }

    if (inside) {
        if (k.error_out) k.error_out[p] = valid ? (float)se : pn_nan();
        if (SSIM && k.ssim_out) k.ssim_out[p] = valid ? s : pn_nan();
    }

    __shared__ double part[4][5];
    __shared__ uint32_t count[4][3];
    const double w_se = compare_wave_sum(se), w_ae = compare_wave_sum(ae), w_re = compare_wave_sum(re);
    const double w_ss = SSIM ? compare_wave_sum(kept ? (double)s : 0.0) : 0.0, w_mx = compare_wave_max(mx);
    const uint32_t n_valid = (uint32_t)__popcll(__ballot(valid)), n_invalid = (uint32_t)__popcll(__ballot(inside && !valid));
    const uint32_t n_ssim = (uint32_t)__popcll(__ballot(kept));
    const uint32_t wave = tid >> 6;
    if ((tid & 63u) == 0) {
        part[wave][0] = w_se, part[wave][1] = w_ae, part[wave][2] = w_re, part[wave][3] = w_ss, part[wave][4] = w_mx;
        count[wave][0] = n_valid, count[wave][1] = n_invalid, count[wave][2] = n_ssim;
    }
    __syncthreads();
    if (tid == 0) {
        double t[5];
        for (uint32_t f = 0; f < 4; ++f) t[f] = (part[0][f] + part[1][f]) + (part[2][f] + part[3][f]);
        const double m01 = part[0][4] > part[1][4] ? part[0][4] : part[1][4], m23 = part[2][4] > part[3][4] ? part[2][4] : part[3][4];
        t[4] = m01 > m23 ? m01 : m23;
        pbrs_compare_result r{};
        r.mse = t[0], r.mae = t[1], r.rel_mse = t[2], r.ssim = t[3], r.max_abs = t[4];
        r.n_valid = (count[0][0] + count[1][0]) + (count[2][0] + count[3][0]);
        r.n_invalid = (count[0][1] + count[1][1]) + (count[2][1] + count[3][1]);
        r.n_ssim = (count[0][2] + count[1][2]) + (count[2][2] + count[3][2]);
        compare_put(tiles, blockIdx.x, r);
    }
}

// Two records of partials as one: the sums in the tree's order (l before r), the largest difference, the counts.
__device__ __forceinline__ pbrs_compare_result compare_join(const pbrs_compare_result& l, const pbrs_compare_result& r) {
    pbrs_compare_result o{};
    o.mse = l.mse + r.mse, o.rel_mse = l.rel_mse + r.rel_mse, o.mae = l.mae + r.mae, o.ssim = l.ssim + r.ssim;
    o.max_abs = r.max_abs > l.max_abs ? r.max_abs : l.max_abs;
    o.n_valid = l.n_valid + r.n_valid, o.n_invalid = l.n_invalid + r.n_invalid, o.n_ssim = l.n_ssim + r.n_ssim;
    return o;
}

// The records [4 g, 4 g + 4) of the m at `src` as two levels of the tree join them: the element 2 g of the level between is l, the
// element 2 g + 1 is r where it exists, and a level's odd last record is joined with +0.0.
__device__ __forceinline__ pbrs_compare_result compare_join4(const CompareRecords& src, uint32_t g, uint32_t m) {
    const uint32_t i = 4u * g;
    const pbrs_compare_result zero{};
    const pbrs_compare_result l = compare_join(compare_get(src, i), i + 1u < m ? compare_get(src, i + 1u) : zero);
    if (i + 2u >= m) return compare_join(l, zero);
    return compare_join(l, compare_join(compare_get(src, i + 2u), i + 3u < m ? compare_get(src, i + 3u) : zero));
}

// One block.  `x` holds the n tile records, `y` room for (n + 3) / 4; both are overwritten.  Two levels per trip through memory while
// more than kCompareFinishLds records are left, then one level per trip through LDS (read, barrier, write, barrier).
__global__ void __launch_bounds__(kCompareFinishBlock) k_compare_finish(CompareRecords x, CompareRecords y, uint32_t n, uint32_t ssim,
                                                                        pbrs_compare_result* out) {
    __shared__ double lds_sums[5u * kCompareFinishLds];
    __shared__ uint32_t lds_counts[3u * kCompareFinishLds];
    const CompareRecords lds{lds_sums, lds_counts, kCompareFinishLds};  // planar like the records in memory: a level reads every second word
    CompareRecords src = x, dst = y;
    uint32_t m = n;
    while (m > kCompareFinishLds) {
        const uint32_t quarter = (m + 3u) / 4u;
        for (uint32_t j = threadIdx.x; j < quarter; j += kCompareFinishBlock) compare_put(dst, j, compare_join4(src, j, m));
        __syncthreads();  // the two levels are written (and visible to the block) before the next trip reads them
        const CompareRecords t = src;
        src = dst, dst = t;
        m = quarter;
    }
    if (threadIdx.x < m) compare_put(lds, threadIdx.x, compare_get(src, threadIdx.x));
    __syncthreads();
    for (; m > 1; m = (m + 1u) / 2u) {
        const uint32_t j = threadIdx.x, half = (m + 1u) / 2u;
        pbrs_compare_result v{};
        if (j < half) v = compare_join(compare_get(lds, 2u * j), 2u * j + 1u < m ? compare_get(lds, 2u * j + 1u) : pbrs_compare_result{});  // +0.0: the tree's padding
        __syncthreads();
        if (j < half) compare_put(lds, j, v);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const pbrs_compare_result t = compare_get(lds, 0);
    pbrs_compare_result r{};
    const double n3 = (double)(3u * t.n_valid);
    r.mse = t.mse / n3, r.rel_mse = t.rel_mse / n3, r.mae = t.mae / n3;
    r.ssim = ssim ? t.ssim / (double)t.n_ssim : 0.0;
    r.max_abs = t.max_abs;
    r.n_valid = t.n_valid, r.n_invalid = t.n_invalid, r.n_ssim = ssim ? t.n_ssim : 0u;
    *out = r;
}
