// device/despeckle.h — despeckle (include/pbrs_gpu.h, pbrsi_despeckle*): fireflies scaled down to gain times the rank-th brightest
// neighbour, non-finite pixels rebuilt from their neighbours.  A post-process like the denoisers: no kernel of the render path is
// involved.  Two kernels, wave64:
//
//   k_despeckle<RADIUS>  a 256-thread block per PBRS_DESPECKLE_TILE x PBRS_DESPECKLE_TILE tile, one pixel per thread, thread
//                        16 * ly + lx at (lx, ly); at most kDespeckleMaxBlocks blocks, a block taking every gridDim.x-th tile (see
//                        "Counts").  The block stages a tile plus a halo of RADIUS (18 x 18 or 20 x 20 pixels) in LDS
//                        once, as four f32 planes: r, g, b and the luminance.  The luminance slot of a pixel that is not good, or that
//                        lies outside the image, holds a NaN and its colour slots +0, so "good" is one compare per tap and no index
//                        outside a plane is ever formed.  A good pixel's own colour comes back from its slots with its bits.
//   k_despeckle_finish   one 256-thread block, only where the call wants the record: the blocks' counts summed, the 16-byte record
//                        written, pads included.
//
// Selection.  The window's 8 or 24 luminances go through a fixed insertion chain into four registers that hold the four largest in
// order (a tap that is not good enters as -inf, which no good pixel's finite luminance equals): max/min pairs, no indexed local array
// and therefore no scratch.  The k-th is picked by selects on k = min(rank, n).
//
// Repair.  Rare and divergent: a pixel that is not good sums the window's colour slots in row-major order.  Slots that are not good hold
// +0, and adding +0 to a sum that started at +0 leaves its bits (such a sum is never -0), which is the header's "over G(p)": the loop
// needs no test per tap and may include the centre.
//
// Counts.  Integers: a ballot and a popcount per wave and tile, kept in a register over the block's tiles, the four waves' counts through
// LDS at the end, and one plain store of the block's two counts into its own slot of a scratch of kDespeckleMaxBlocks slots;
// k_despeckle_finish sums the slots.  No atomics of any kind.  The earlier versions added each block's counts to the record with
// integer atomics, and adds to one address cost 11 to 12 ns each, one after the other, whichever block they come from: 97.9 us for the
// kernel with a block per tile (8160 adds at 1920 x 1080), 36.5 us with the grid capped at 2048 blocks, 13.9 us for the same kernel when
// no record is asked for ("Despeckle").  The cap stays (eight blocks for each of 256 CUs, a block walks its tiles):
// it bounds the scratch and the finish.
//
// LDS banking (ds_read_b32: bank = dword % 32 per 32-lane half).  A half reads one tap of two tile rows, 16 + 16 consecutive dwords a
// row pitch apart: at the pitch of 48 dwords (kDespecklePitch, a multiple of 32 plus 16) the second row starts 16 banks after the first
// and the half covers all 32 banks once.  At the natural pitches of 18 and 20 the two rows would share 14 and 12 banks, two-way on most
// lanes of every tap.  4 planes x 20 rows x 48 dwords = 15 KiB per block at radius 2, 13.5 KiB at radius 1.  The staging stores meet at
// most two-way where a halo row wraps, which a ds_write_b32 does not pay for.  None of this is a measured cycle count;
// tools/despeckle_cost.py times the kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/pbrs_gpu.h"
#include "../../../include/pbrs_numeric.h"

constexpr uint32_t kDespeckleBlock = PBRS_DESPECKLE_TILE * PBRS_DESPECKLE_TILE;
constexpr uint32_t kDespecklePitch = 48;
constexpr uint32_t kDespeckleMaxBlocks = 2048;
static_assert(kDespeckleBlock == 256 && PBRS_DESPECKLE_TILE == 16u, "k_despeckle: four waves of four 16-pixel rows");
static_assert(kDespecklePitch >= PBRS_DESPECKLE_TILE + 2u * PBRS_DESPECKLE_MAX_RADIUS && kDespecklePitch % 32u == 16u, "see \"LDS banking\"");

struct DespeckleConst {
    uint32_t w, h, tiles_x, n_tiles, rank;
    float gain, floor;
    const float* rgb_in;
    float* rgb_out;
    const uint32_t* variance_in;  // null with variance_out: not given; words, so that a NaN keeps its payload
    uint32_t* variance_out;
    uint32_t* mask_out;     // null: not wanted
    float* removed_out;     // null: not wanted
    uint32_t* block_counts; // n_clamped, n_repaired of block b at [2 b], [2 b + 1]: gridDim.x slots; null: not wanted
};

__device__ __forceinline__ float despeckle_luminance(float r, float g, float b) { return (0.21267127f * r + 0.71515972f * g) + 0.07216883f * b; }

// One tap into the four largest so far, m0 >= m1 >= m2 >= m3 (no NaN on either side: the caller has replaced them).
__device__ __forceinline__ void despeckle_insert(float x, float& m0, float& m1, float& m2, float& m3) {
    float t;
    t = fmaxf(m0, x), x = fminf(m0, x), m0 = t;
    t = fmaxf(m1, x), x = fminf(m1, x), m1 = t;
    t = fmaxf(m2, x), x = fminf(m2, x), m2 = t;
    m3 = fmaxf(m3, x);
}

template <uint32_t RADIUS>
__global__ void __launch_bounds__(256) k_despeckle(DespeckleConst k) {
    static_assert(RADIUS >= 1u && RADIUS <= PBRS_DESPECKLE_MAX_RADIUS, "the header's radii");
    constexpr uint32_t T = PBRS_DESPECKLE_TILE + 2u * RADIUS, PLANE = T * kDespecklePitch;
    constexpr int R = (int)RADIUS, PITCH = (int)kDespecklePitch;
    __shared__ float lds[4u * PLANE];  // r, g, b, luminance
    __shared__ uint32_t s_wave[4][2];
    float* const sr = lds;
    float* const sg = lds + PLANE;
    float* const sb = lds + 2u * PLANE;
    float* const sl = lds + 3u * PLANE;
    uint32_t wave_clamped = 0, wave_repaired = 0;  // this wave's counts over the block's tiles: the same in all its lanes
    for (uint32_t tile = blockIdx.x; tile < k.n_tiles; tile += gridDim.x) {  // uniform over the block: every thread reaches the barriers
        const uint32_t tile_y = tile / k.tiles_x, tile_x = tile - tile_y * k.tiles_x;
        const uint32_t cx = tile_x * PBRS_DESPECKLE_TILE, cy = tile_y * PBRS_DESPECKLE_TILE;
        for (uint32_t i = threadIdx.x; i < T * T; i += kDespeckleBlock) {
            const uint32_t sy = i / T, sx = i - sy * T;
            const int qx = (int)(cx + sx) - R, qy = (int)(cy + sy) - R;
            float r = 0.0f, g = 0.0f, b = 0.0f, l = pn_nan();
            if (qx >= 0 && qx < (int)k.w && qy >= 0 && qy < (int)k.h) {
                const float* c = k.rgb_in + 3u * ((uint32_t)qy * k.w + (uint32_t)qx);  // at most 2^28 pixels: 3 p stays below 2^32
                const float cr = c[0], cg = c[1], cb = c[2];
                const float y = despeckle_luminance(cr, cg, cb);
                if (pn_isfinite(cr) && pn_isfinite(cg) && pn_isfinite(cb) && pn_isfinite(y)) r = cr, g = cg, b = cb, l = y;
            }
            const uint32_t at = sy * kDespecklePitch + sx;
            sr[at] = r, sg[at] = g, sb[at] = b, sl[at] = l;
        }
        __syncthreads();
        const uint32_t lx = threadIdx.x % PBRS_DESPECKLE_TILE, ly = threadIdx.x / PBRS_DESPECKLE_TILE;
        const uint32_t px = cx + lx, py = cy + ly;
        const bool inside = px < k.w && py < k.h;
        bool clamped = false, repaired = false;
        if (inside) {
            const int center = (int)((ly + RADIUS) * kDespecklePitch + lx + RADIUS);
            const float ninf = -pn_inf();
            float m0 = ninf, m1 = ninf, m2 = ninf, m3 = ninf;
            uint32_t n = 0;
#pragma unroll
            for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
                for (int dx = -R; dx <= R; ++dx) {
                    if (dx == 0 && dy == 0) continue;
                    const float v = sl[center + dy * PITCH + dx];
                    const bool good = v == v;
                    n += good ? 1u : 0u;
                    despeckle_insert(good ? v : ninf, m0, m1, m2, m3);
                }
            }
            float lp = sl[center];
            float cr = sr[center], cg = sg[center], cb = sb[center];
            repaired = lp != lp;
            if (repaired) {
                lp = 0.0f;  // the slots hold +0: c' with n == 0
                if (n != 0u) {
                    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
                    for (int dy = -R; dy <= R; ++dy) {
                        const int row = center + dy * PITCH;
                        for (int dx = -R; dx <= R; ++dx) ar = ar + sr[row + dx], ag = ag + sg[row + dx], ab = ab + sb[row + dx];
                    }
                    const float fn = (float)n;
                    ar = ar / fn, ag = ag / fn, ab = ab / fn;
                    const float y = despeckle_luminance(ar, ag, ab);
                    if (pn_isfinite(ar) && pn_isfinite(ag) && pn_isfinite(ab) && pn_isfinite(y)) cr = ar, cg = ag, cb = ab, lp = y;
                }
            }
            float outr = cr, outg = cg, outb = cb, s = 1.0f;
            if (n != 0u) {
                const uint32_t kth = k.rank < n ? k.rank : n;
                const float S = kth == 1u ? m0 : (kth == 2u ? m1 : (kth == 3u ? m2 : m3));
                float limit = k.gain * S + k.floor;
                if (!(limit > 0.0f)) limit = 0.0f;
                if (lp > limit) {
                    clamped = true;
                    s = limit / lp;
                    outr = cr * s, outg = cg * s, outb = cb * s;
                }
            }
            const uint32_t p = py * k.w + px;
            k.rgb_out[3u * p] = outr, k.rgb_out[3u * p + 1u] = outg, k.rgb_out[3u * p + 2u] = outb;
            if (k.variance_out) {
                uint32_t word = k.variance_in[p];
                if (repaired) {
                    word = 0x7f800000u;
                } else if (clamped) {
                    const float v = pn_from_bits(word);
                    if (pn_isfinite(v)) word = pn_bits((v * s) * s);
                }
                k.variance_out[p] = word;
            }
            if (k.mask_out) k.mask_out[p] = (clamped ? PBRS_DESPECKLE_CLAMPED : 0u) | (repaired ? PBRS_DESPECKLE_REPAIRED : 0u);
            if (k.removed_out) {
                float* rm = k.removed_out + 3u * p;
                rm[0] = clamped ? cr - outr : 0.0f, rm[1] = clamped ? cg - outg : 0.0f, rm[2] = clamped ? cb - outb : 0.0f;
            }
        }
        wave_clamped += (uint32_t)__popcll(__ballot(clamped)), wave_repaired += (uint32_t)__popcll(__ballot(repaired));
        __syncthreads();  // the next tile's staging overwrites the planes
    }
    if (k.block_counts) {  // uniform over the grid: every thread of the block reaches the barrier
        const uint32_t wave = threadIdx.x / 64u;
        if (threadIdx.x % 64u == 0u) s_wave[wave][0] = wave_clamped, s_wave[wave][1] = wave_repaired;
        __syncthreads();
        if (threadIdx.x < 2u) {
            const uint32_t c = (s_wave[0][threadIdx.x] + s_wave[1][threadIdx.x]) + (s_wave[2][threadIdx.x] + s_wave[3][threadIdx.x]);
            k.block_counts[2u * blockIdx.x + threadIdx.x] = c;
        }
    }
}

// The record from the n_blocks slots k_despeckle has written (n_blocks <= kDespeckleMaxBlocks): one block of 256 threads.
__global__ void __launch_bounds__(256) k_despeckle_finish(const uint32_t* block_counts, uint32_t n_blocks, pbrs_despeckle_result* result) {
    __shared__ uint32_t s_wave[4][2];
    uint32_t c = 0, r = 0;
    for (uint32_t b = threadIdx.x; b < n_blocks; b += 256u) c += block_counts[2u * b], r += block_counts[2u * b + 1u];
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off), r += __shfl_xor(r, off);
    if (threadIdx.x % 64u == 0u) s_wave[threadIdx.x / 64u][0] = c, s_wave[threadIdx.x / 64u][1] = r;
    __syncthreads();
    if (threadIdx.x == 0u) {
        result->n_clamped = (s_wave[0][0] + s_wave[1][0]) + (s_wave[2][0] + s_wave[3][0]);
        result->n_repaired = (s_wave[0][1] + s_wave[1][1]) + (s_wave[2][1] + s_wave[3][1]);
        result->pad[0] = 0u, result->pad[1] = 0u;
    }
}
