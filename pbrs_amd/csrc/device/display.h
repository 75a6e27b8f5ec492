// device/display.h — the display transform (include/pbrs_gpu.h, pbrs_display*): exposure, tone curve, transfer function and quantiser
// from an f32 radiance plane to 8-bit RGBA, with an exposure that can follow the image.  A post-process like the denoisers: no kernel of
// the render path is involved.  Three kernels, wave64, 256-thread blocks:
//
//   k_display_hist     the 512-bin luminance histogram.  Four consecutive pixels per thread and trip of a grid-stride loop (the grid is
//                      capped at kDisplayMaxBlocks), read like k_display_apply's; a block counts into an LDS histogram with LDS integer
//                      adds and then adds each non-zero bin to the global one with one integer atomicAdd.  Integer adds commute: the
//                      counts do not depend on arrival order.
//   k_display_resolve  one wave, eight bins per lane: a wave prefix sum of the counts, the trimmed mean bin in integers, and the few f32
//                      operations from there to the exposure.  Writes the scale word k_display_apply reads, exposure_out and
//                      histogram_out.
//   k_display_apply    the per-pixel part, templated on curve and encode; the quantiser's offset is a runtime value.  A thread takes
//                      four consecutive pixels of the flat plane per trip: three 16-byte loads and one 16-byte store where the planes
//                      are 16-byte aligned (VEC; the histogram asks that of the image only), twelve 4-byte loads and four 4-byte
//                      stores otherwise, and always for the last w * h % 4 pixels.  Grid-stride under the same cap.
//
// No float atomics; every value is written with an ordinary vector-memory store.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/pbrs_gpu.h"
#include "../../../include/pbrs_numeric.h"

constexpr uint32_t kDisplayBlock = 256;
constexpr uint32_t kDisplayMaxBlocks = 2048;  // 256 CUs x 8 blocks: the rest of a larger image is reached by the grid-stride loops
// k_display_hist's own cap, one block per CU: every block ends in one atomicAdd per bin it has filled, and those on one word queue up
// behind each other.  Histogram, memset and resolve of a 1920 x 1080 noise image beside the apply kernel, by cap: 2048 blocks 43 us,
// 1024 25 us, 512 15 us, 256 12 us, 128 12 us (and 20 us on a constant image); DESIGN.md section 4, "Display transform".
constexpr uint32_t kDisplayHistMaxBlocks = 256;
constexpr uint32_t kDisplayFirstBits = 0x2F800000u;  // 2^-32: the first bin's lower edge
constexpr uint32_t kDisplayInfBits = 0x7F800000u;

// The scratch of a context that has called pbrs_display* (BUF_DISPLAY), in words.
constexpr uint32_t kDisplayScaleWord = PBRS_DISPLAY_BINS;        // scale = e * exposure, written by k_display_resolve
constexpr uint32_t kDisplayExposureWord = PBRS_DISPLAY_BINS + 1; // the host variant's exposure_out
constexpr uint32_t kDisplayPrevWord = PBRS_DISPLAY_BINS + 2;     // the host variant's exposure_in
constexpr uint32_t kDisplayScratchWords = PBRS_DISPLAY_BINS + 4;

__device__ __forceinline__ float display_luminance(float r, float g, float b) { return (0.21267127f * r + 0.71515972f * g) + 0.07216883f * b; }

// One pixel into the block's histogram.
__device__ __forceinline__ void display_count(uint32_t* bins, float r, float g, float b) {
    const uint32_t u = pn_bits(display_luminance(r, g, b));
    if (u >= kDisplayFirstBits && u < kDisplayInfBits) {
        const uint32_t bin = (u - kDisplayFirstBits) >> 20;
        atomicAdd(&bins[bin < PBRS_DISPLAY_BINS - 1u ? bin : PBRS_DISPLAY_BINS - 1u], 1u);
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_display_hist(const float* __restrict__ rgb, uint32_t P, uint32_t* __restrict__ hist) {
    __shared__ uint32_t bins[PBRS_DISPLAY_BINS];
    for (uint32_t b = threadIdx.x; b < PBRS_DISPLAY_BINS; b += kDisplayBlock) bins[b] = 0u;
    __syncthreads();
    const uint32_t groups = (P + 3u) / 4u, stride = gridDim.x * kDisplayBlock;
    for (uint32_t grp = blockIdx.x * kDisplayBlock + threadIdx.x; grp < groups; grp += stride) {
        const uint32_t p0 = 4u * grp;
        if (VEC && p0 + 4u <= P) {
            const float4* src = reinterpret_cast<const float4*>(rgb + 3 * (size_t)p0);
            const float4 a = src[0], b = src[1], c = src[2];
            display_count(bins, a.x, a.y, a.z);
            display_count(bins, a.w, b.x, b.y);
            display_count(bins, b.z, b.w, c.x);
            display_count(bins, c.y, c.z, c.w);
        } else {
            const uint32_t end = p0 + 4u < P ? p0 + 4u : P;
            for (uint32_t p = p0; p < end; ++p) {
                const size_t at = 3 * (size_t)p;
                display_count(bins, rgb[at], rgb[at + 1], rgb[at + 2]);
            }
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < PBRS_DISPLAY_BINS; b += kDisplayBlock) {
        const uint32_t n = bins[b];
        if (n) atomicAdd(&hist[b], n);
    }
}

struct DisplayResolve {
    uint32_t auto_exposure;
    float exposure, key, min_exposure, max_exposure, adapt;
    uint32_t low_q16, high_q16;
    const float* exposure_in;  // null: none
    float* exposure_out;       // null: not wanted
    uint32_t* histogram_out;   // null: not wanted
};

// One wave.  Lane l holds bins 8 l .. 8 l + 7.
__global__ void __launch_bounds__(64) k_display_resolve(const uint32_t* __restrict__ hist, float* __restrict__ scale_out, DisplayResolve k) {
    constexpr uint32_t PER_LANE = PBRS_DISPLAY_BINS / 64u;
    const uint32_t lane = threadIdx.x;
    uint32_t n[PER_LANE];
    uint32_t mine = 0;
    for (uint32_t i = 0; i < PER_LANE; ++i) {
        n[i] = hist[lane * PER_LANE + i];
        mine += n[i];
        if (k.histogram_out) k.histogram_out[lane * PER_LANE + i] = n[i];
    }
    uint32_t incl = mine;  // the inclusive prefix sum over the lanes (at most 2^28 pixels: no overflow)
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    const uint32_t N = __shfl(incl, 63, 64);
    uint64_t lo = ((uint64_t)N * k.low_q16) >> 16, hi = ((uint64_t)N * k.high_q16) >> 16;
    if (hi == lo) lo = 0, hi = N;
    uint64_t c = incl - mine, S = 0;
    for (uint32_t i = 0; i < PER_LANE; ++i) {
        const uint64_t first = c > lo ? c : lo, last = c + n[i] < hi ? c + n[i] : hi;
        if (last > first) S += (last - first) * (2u * (lane * PER_LANE + i) + 1u);
        c += n[i];
    }
    uint32_t s_lo = (uint32_t)S, s_hi = (uint32_t)(S >> 32);
    for (uint32_t d = 32; d > 0; d >>= 1) {  // integer sums: the order does not matter
        const uint64_t other = ((uint64_t)__shfl_xor(s_hi, d, 64) << 32) | __shfl_xor(s_lo, d, 64);
        S += other;
        s_lo = (uint32_t)S, s_hi = (uint32_t)(S >> 32);
    }
    if (lane != 0) return;
    float e = 1.0f;
    if (k.auto_exposure) {
        const float prev = k.exposure_in ? *k.exposure_in : 0.0f;
        const bool has_prev = k.exposure_in && pn_isfinite(prev) && prev > 0.0f;
        if (N == 0) {
            e = has_prev ? prev : 1.0f;
        } else {
            const uint64_t Q = (S << 8) / (hi - lo);
            const float lavg = pn_ldexp(pn_exp((float)(uint32_t)(Q & 4095u) * (0.6931472f * 0.000244140625f)), (int)(Q >> 12) - 32);
            const float a = pn_clamp(k.key / lavg, k.min_exposure, k.max_exposure);
            e = has_prev ? prev + (a - prev) * k.adapt : a;
        }
    }
    if (k.exposure_out) *k.exposure_out = e;
    *scale_out = e * k.exposure;
}

struct DisplayApply {
    uint32_t w, P;
    const float* scale_word;  // the word k_display_resolve wrote; null: `scale` (no resolve ran: e = 1)
    float scale;
    float iw2;                // REINHARD: 1.0f / (white * white)
    float d;                  // the quantiser's offset without a dither
    uint32_t dither;
    float* exposure_out;      // without a resolve: receives e = 1.0f (null: not wanted)
};

template <uint32_t CURVE, uint32_t ENCODE>
__device__ __forceinline__ uint32_t display_channel(float c, float scale, float iw2, float d) {
    float v = c * scale;
    v = v > 0.0f ? v : 0.0f;
    v = pn_min(v, 65504.0f);
    float t = v;
    if (CURVE == PBRS_CURVE_REINHARD) t = (v * (1.0f + v * iw2)) / (1.0f + v);
    if (CURVE == PBRS_CURVE_ACES) t = (v * (2.51f * v + 0.03f)) / (v * (2.43f * v + 0.59f) + 0.14f);
    t = t < 1.0f ? t : 1.0f;
    float g;
    if (ENCODE == PBRS_ENCODE_SQRT) {
        g = pn_sqrt(t);
    } else {
        if (t <= 0.0031308f) g = 12.92f * t;
        else if (t >= 1.0f) g = 1.0f;
        else g = 1.055f * pn_exp(pn_ln(t) * (1.0f / 2.4f)) - 0.055f;
    }
    const float q = g * 255.0f + d;
    return q >= 255.0f ? 255u : (uint32_t)q;
}

// The 4 x 4 Bayer matrix {{0, 8, 2, 10}, {12, 4, 14, 6}, {3, 11, 1, 9}, {15, 7, 13, 5}}, four bits per entry, entry [y][x] at 4 * (4 y + x).
constexpr uint64_t kDisplayBayer = 0x5D7F91B36E4CA280ull;

template <uint32_t CURVE, uint32_t ENCODE>
__device__ __forceinline__ uint32_t display_pixel(float r, float g, float b, uint32_t x, uint32_t y, float scale, const DisplayApply& k) {
    float d = k.d;
    if (k.dither) d = ((float)(uint32_t)((kDisplayBayer >> (4u * (4u * (y & 3u) + (x & 3u)))) & 15u) + 0.5f) * 0.0625f;
    return display_channel<CURVE, ENCODE>(r, scale, k.iw2, d) | display_channel<CURVE, ENCODE>(g, scale, k.iw2, d) << 8 |
           display_channel<CURVE, ENCODE>(b, scale, k.iw2, d) << 16 | 255u << 24;
}

template <uint32_t CURVE, uint32_t ENCODE, bool VEC>
__global__ void __launch_bounds__(256) k_display_apply(const float* rgb, uint32_t* out, DisplayApply k) {
    const float scale = k.scale_word ? *k.scale_word : k.scale;
    const uint32_t first = blockIdx.x * kDisplayBlock + threadIdx.x;
    if (k.exposure_out && first == 0) *k.exposure_out = 1.0f;
    const uint32_t groups = (k.P + 3u) / 4u, stride = gridDim.x * kDisplayBlock;
    for (uint32_t grp = first; grp < groups; grp += stride) {
        const uint32_t p0 = 4u * grp;
        uint32_t y = p0 / k.w, x = p0 - y * k.w;
        if (VEC && p0 + 4u <= k.P) {
            const float4* src = reinterpret_cast<const float4*>(rgb + 3 * (size_t)p0);
            const float4 a = src[0], b = src[1], c = src[2];
            const float ch[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
            uint32_t word[4];
            for (uint32_t i = 0; i < 4; ++i) {
                word[i] = display_pixel<CURVE, ENCODE>(ch[3 * i], ch[3 * i + 1], ch[3 * i + 2], x, y, scale, k);
                if (++x == k.w) x = 0, ++y;
            }
            *reinterpret_cast<uint4*>(out + p0) = make_uint4(word[0], word[1], word[2], word[3]);
        } else {
            const uint32_t end = p0 + 4u < k.P ? p0 + 4u : k.P;
            for (uint32_t p = p0; p < end; ++p) {
                const size_t at = 3 * (size_t)p;
                out[p] = display_pixel<CURVE, ENCODE>(rgb[at], rgb[at + 1], rgb[at + 2], x, y, scale, k);
                if (++x == k.w) x = 0, ++y;
            }
        }
    }
}
