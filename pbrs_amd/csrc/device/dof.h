// device/dof.h — depth of field (include/pbrs_gpu.h, pbrsf_dof*): a thin-lens blur of an image from its depth AOV, the circle of
// confusion and the gather in one launch.  A post-process like the denoisers: no kernel of the render path is involved.  One kernel,
// wave64, 256-thread blocks:
//
//   k_dof<HALO, VEC>  a block per 16 x 16 tile of the output, thread 16 * ly + lx at (lx, ly).  The block stages the tile and a halo of
//                     HALO pixels on every side in LDS as five planes (r, g, b, the circle of confusion, the depth), a row every
//                     kDofPitch floats.  A slot's place depends only on its offset from the tile, so the tap loop forms no coordinate
//                     test: the rectangle that is loaded is cut at the image's edge, and every slot outside the image, like every pixel
//                     with a non-finite rgb, gets the circle -1.  With e <= -1 the header's cov is (e - dist) + 0.5 <= -0.5: such a tap
//                     is left out by the arithmetic every tap goes through, without a branch of its own.  HALO is 4, 8 or 16; the host
//                     launches the smallest that holds max_radius, and the loop's bound stays max_radius.  VEC reads rgb and depth as
//                     aligned groups of four floats where both planes are 16-byte aligned (a staged row starts at any float, so a
//                     group's floats outside the row are dropped), float by float otherwise: the same bytes either way.
//
// Step 1 of the header is computed while staging (a second pass over the staged slots, once the loads of a pixel's four floats have
// landed), so there is no intermediate plane.  A pixel's acc, W and n are one thread's, in the header's order: no atomics, no scratch,
// no reduction of a sum across lanes.  The one value the block shares is the largest staged circle, a maximum (exact in any order),
// through one shuffle tree per wave and four LDS words.  It buys the two shortcuts that the header's "left out" rule makes bit-neutral:
//   - a block whose staged circles are all <= 0.5 copies its tile: every tap but the centre has dist >= 1 and cov <= 0;
//   - the loops run to L = min(max_radius, ceil(emax)), and a tap (dx, dy) with (emax - dist) + 0.5f <= 0 is left out by the whole
//     block: e <= emax for every pixel and every tap, rounding is monotone, so cov <= 0 for all of them.  That turns the square of
//     taps into the disk: seventeen threads find, per |dy|, the largest |dx| that passes, and a row's loop runs over that interval.
// dist comes from a table of sqrt((float)(dx * dx + dy * dy)) over |dx|, |dy| <= 16 that the block fills (correctly rounded square
// roots, 289 of them) and reads at one address for all lanes.  A tap's six LDS values (circle, depth, r, g, b, dist) are read one tap
// ahead of their use, rgb whether the tap counts or not: the first version read the distance, then the circle and the depth, then the
// channels, three dependent LDS round trips per tap, and took 2.36 ms for the fully blurred 1080p image at R = 16.
//
// LDS.  Five planes of (16 + 2 HALO) rows of kDofPitch = 48 floats: 22.5, 30 and 45 KiB for HALO 4, 8 and 16, plus 1.2 KiB of table;
// six, five and three blocks fit a CU's 160 KiB.  A tap reads the circle, the depth and the three channels, each a ds_read_b32 at
// (row + ly) * 48 + lx + const dwords.  ds_read_b32 banks are dword mod 32 and its lane groups the two 32-lane halves, a
// half being two tile rows of 16 consecutive dwords each: with 48 = 16 mod 32 the second row's banks are the first's plus 16, so the 32
// lanes cover the 32 banks once and the tap reads are conflict-free for every (dx, dy) (a pitch of 24 or 32, the staged width for HALO 4
// and 8, would give two-way conflicts; the cost is the unused half of a HALO-4 row).  Five reads are 10 LDS cycles per wave and tap; the
// table read is a broadcast.  A counted tap is some 35 vector instructions, twelve of them the correctly rounded division, so the
// loop is bound by vector issue, not by the LDS: four SIMDs take 4 x 10 LDS cycles per 35 x 3 to 4 issue cycles each.  The staging
// stores de-interleave rgb (stride 3 in the source, stride 1 in a plane) and are not conflict-free.  None of this is a measured cycle
// count or counter; tools/dof_cost.py times the call (1.85 ms for the fully blurred 1080p image at R = 16, 861 taps per pixel).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/pbrs_gpu.h"
#include "../../../include/pbrs_numeric.h"

constexpr uint32_t kDofBlock = 256;
constexpr uint32_t kDofTile = 16;
constexpr uint32_t kDofPitch = 48;                             // floats per staged row of a plane
constexpr uint32_t kDofDistSide = PBRS_DOF_MAX_RADIUS + 1u;    // the table of distances: |dx|, |dy| = 0 .. 16
constexpr uint32_t kDofDistEntries = kDofDistSide * kDofDistSide;
static_assert(kDofBlock == kDofTile * kDofTile, "k_dof: a thread per pixel of the tile");
static_assert(kDofTile + 2u * PBRS_DOF_MAX_RADIUS <= kDofPitch && kDofPitch % 32u == 16u, "a staged row fits the pitch, which is 16 mod 32");
static_assert(kDofDistEntries <= 2u * kDofBlock, "the table is filled in two trips");

struct Dof {
    const float* rgb;    // w x h pixels of three floats
    const float* depth;  // w x h
    float* out;          // w x h pixels of three floats; not rgb
    float* coc;          // w x h, or null
    uint32_t w, h, tiles_x;
    uint32_t R;  // max_radius, 1 .. HALO
    float F, K;  // focus, scale (> 0: the host copies where it is 0)
};

// Step 1 of the header.
__device__ __forceinline__ float dof_circle(float z, float F, float K, float Rf) {
    if (!(z > 0.0f)) return 0.0f;
    const float q = pn_isinf(z) ? 1.0f : pn_abs(z - F) / z;
    const float r = K * q;
    return r < Rf ? r : Rf;
}

// A value every lane holds alike, as the scalar it is.
__device__ __forceinline__ float dof_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

template <uint32_t HALO, bool VEC>
__global__ void __launch_bounds__(256) k_dof(Dof k) {
    constexpr uint32_t S = kDofTile + 2u * HALO;  // staged rows and columns
    constexpr uint32_t PLANE = S * kDofPitch;
    constexpr uint32_t GR = (3u * S + 6u) / 4u;  // 3 S floats that start at any float of a group of four span at most this many groups
    constexpr uint32_t GD = (S + 6u) / 4u;
    static_assert(4u * GR >= 3u * S + 3u && 4u * GD >= S + 3u, "the groups that cover a staged row");
    __shared__ float lds[5u * PLANE];
    __shared__ float dist_table[kDofDistEntries];
    __shared__ float wave_max[kDofBlock / 64u];
    __shared__ int reach[kDofDistSide];  // per |dy|: the largest |dx| the block does not leave out, -1 where there is none
    float* const LR = lds;
    float* const LC = lds + 3u * PLANE;  // the circle of confusion, -1 where the slot can never contribute
    float* const LZ = lds + 4u * PLANE;  // the depth
    const uint32_t tile_y = blockIdx.x / k.tiles_x, tile_x = blockIdx.x - tile_y * k.tiles_x;
    const uint32_t X0 = tile_x * kDofTile, Y0 = tile_y * kDofTile;  // X0 < w, Y0 < h
    // the rectangle that is loaded, [gx0, gx1) x [gy0, gy1), and the slot of its first pixel
    const uint32_t gx0 = X0 > HALO ? X0 - HALO : 0u, gy0 = Y0 > HALO ? Y0 - HALO : 0u;
    const uint32_t gx1 = X0 + kDofTile + HALO < k.w ? X0 + kDofTile + HALO : k.w;
    const uint32_t gy1 = Y0 + kDofTile + HALO < k.h ? Y0 + kDofTile + HALO : k.h;
    const uint32_t ox = gx0 + HALO - X0, oy = gy0 + HALO - Y0;  // 0 .. HALO
    const uint32_t cols = gx1 - gx0, rows = gy1 - gy0;          // 1 .. S each, ox + cols <= S, oy + rows <= S
    const size_t pixels = (size_t)k.w * k.h;

    for (uint32_t i = threadIdx.x; i < kDofDistEntries; i += kDofBlock) {
        const uint32_t ay = i / kDofDistSide, ax = i - ay * kDofDistSide;
        dist_table[i] = __builtin_sqrtf((float)(ax * ax + ay * ay));
    }
    if (VEC) {
        const uint32_t nf = 3u * cols;  // floats of a staged rgb row
        for (uint32_t i = threadIdx.x; i < rows * GR; i += kDofBlock) {
            const uint32_t r = i / GR, j = i - r * GR;
            const size_t a = 3u * ((size_t)(gy0 + r) * k.w + gx0);  // the row's first float
            const size_t f0 = 4u * (a / 4u + j);
            if (f0 >= a + nf) continue;
            float v[4];
            if (f0 + 4u <= 3u * pixels) {
                const float4 q = *reinterpret_cast<const float4*>(k.rgb + f0);
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            } else {  // the plane's last, short group
#pragma unroll
                for (uint32_t e = 0; e < 4u; ++e) v[e] = f0 + e < 3u * pixels ? k.rgb[f0 + e] : 0.0f;
            }
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e) {
                const size_t f = f0 + e;
                if (f >= a && f < a + nf) {
                    const uint32_t jj = (uint32_t)(f - a), px = jj / 3u, ch = jj - 3u * px;
                    LR[ch * PLANE + (oy + r) * kDofPitch + ox + px] = v[e];
                }
            }
        }
        for (uint32_t i = threadIdx.x; i < rows * GD; i += kDofBlock) {
            const uint32_t r = i / GD, j = i - r * GD;
            const size_t a = (size_t)(gy0 + r) * k.w + gx0;
            const size_t f0 = 4u * (a / 4u + j);
            if (f0 >= a + cols) continue;
            float v[4];
            if (f0 + 4u <= pixels) {
                const float4 q = *reinterpret_cast<const float4*>(k.depth + f0);
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            } else {
#pragma unroll
                for (uint32_t e = 0; e < 4u; ++e) v[e] = f0 + e < pixels ? k.depth[f0 + e] : 0.0f;
            }
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e) {
                const size_t f = f0 + e;
                if (f >= a && f < a + cols) LZ[(oy + r) * kDofPitch + ox + (uint32_t)(f - a)] = v[e];
            }
        }
    } else {
        for (uint32_t i = threadIdx.x; i < rows * cols; i += kDofBlock) {
            const uint32_t r = i / cols, cx = i - r * cols;
            const size_t p = (size_t)(gy0 + r) * k.w + gx0 + cx;
            const uint32_t slot = (oy + r) * kDofPitch + ox + cx;
            LR[slot] = k.rgb[3u * p], LR[PLANE + slot] = k.rgb[3u * p + 1u], LR[2u * PLANE + slot] = k.rgb[3u * p + 2u];
            LZ[slot] = k.depth[p];
        }
    }
    __syncthreads();
    // the circles: step 1 on what was loaded, -1 on a pixel whose rgb is not finite and on every slot outside the image
    const float Rf = (float)k.R;
    float emax = -1.0f;
    for (uint32_t i = threadIdx.x; i < S * S; i += kDofBlock) {
        const uint32_t sy = i / S, sx = i - sy * S;
        const uint32_t slot = sy * kDofPitch + sx;
        float c = -1.0f;
        if (sx >= ox && sx < ox + cols && sy >= oy && sy < oy + rows) {
            if (pn_isfinite(LR[slot]) && pn_isfinite(LR[PLANE + slot]) && pn_isfinite(LR[2u * PLANE + slot])) c = dof_circle(LZ[slot], k.F, k.K, Rf);
        } else {
            LZ[slot] = 0.0f;
        }
        LC[slot] = c;
        emax = c > emax ? c : emax;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float o = __shfl_xor(emax, m, 64);
        emax = o > emax ? o : emax;
    }
    if ((threadIdx.x & 63u) == 0u) wave_max[threadIdx.x >> 6] = emax;
    __syncthreads();
    emax = wave_max[0];
#pragma unroll
    for (uint32_t i = 1; i < kDofBlock / 64u; ++i) emax = wave_max[i] > emax ? wave_max[i] : emax;
    emax = dof_uniform(emax);
    // the disk: (emax - dist) + 0.5f > 0 falls with |dx|, so each row of taps is one interval
    if (threadIdx.x < kDofDistSide) {
        int far = -1;
        for (uint32_t ax = 0; ax < kDofDistSide; ++ax)
            if ((emax - dist_table[threadIdx.x * kDofDistSide + ax]) + 0.5f > 0.0f) far = (int)ax;
        reach[threadIdx.x] = far;
    }
    __syncthreads();

    const uint32_t lx = threadIdx.x % kDofTile, ly = threadIdx.x / kDofTile;
    const uint32_t X = X0 + lx, Y = Y0 + ly;
    if (X >= k.w || Y >= k.h) return;  // (after the last barrier)
    const uint32_t centre = (ly + HALO) * kDofPitch + lx + HALO;
    const size_t p = (size_t)Y * k.w + X;
    const float pr = LR[centre], pg = LR[PLANE + centre], pb = LR[2u * PLANE + centre], zp = LZ[centre];
    if (k.coc) {
        const float r = dof_circle(zp, k.F, k.K, Rf);  // (the staged circle is -1 where rgb is not finite)
        k.coc[p] = zp < k.F ? pn_from_bits(pn_bits(r) | 0x80000000u) : r;
    }
    float o0 = pr, o1 = pg, o2 = pb;
    const float rp = LC[centre];
    // rp < 0: the pixel's own rgb is not finite, it passes through.  emax <= 0.5: every tap but the centre is left out.
    if (rp >= 0.0f && emax > 0.5f) {
        const float top = __builtin_ceilf(emax);  // 1 .. 16
        const int L = (int)(top < Rf ? top : Rf);
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, W = 0.0f;
        uint32_t n = 0;
        for (int dy = -L; dy <= L; ++dy) {
            const uint32_t ady = (uint32_t)(dy < 0 ? -dy : dy);
            int xl = __builtin_amdgcn_readfirstlane(reach[ady]);
            xl = xl < L ? xl : L;
            if (xl < 0) continue;  // the whole block leaves the row out
            const float* const dist_row = dist_table + ady * kDofDistSide;
            uint32_t slot = (uint32_t)((int)centre + dy * (int)kDofPitch - xl);
            // a tap's six values are read one tap ahead of their use, so that an LDS round trip is not in every tap's way
            float rq = LC[slot], zq = LZ[slot], c0 = LR[slot], c1 = LR[PLANE + slot], c2 = LR[2u * PLANE + slot], dist = dist_row[xl];
            for (int dx = -xl; dx <= xl; ++dx) {
                const float rq_ = rq, zq_ = zq, t0 = c0, t1 = c1, t2 = c2, dist_ = dist;
                if (dx < xl) {
                    ++slot;
                    rq = LC[slot], zq = LZ[slot], c0 = LR[slot], c1 = LR[PLANE + slot], c2 = LR[2u * PLANE + slot];
                    dist = dist_row[dx + 1 < 0 ? -(dx + 1) : dx + 1];
                }
                const float e = zq_ < zp ? rq_ : (rq_ < rp ? rq_ : rp);
                float cov = (e - dist_) + 0.5f;
                if (cov > 0.0f) {
                    cov = cov < 1.0f ? cov : 1.0f;
                    const float rr = e > 0.5f ? e : 0.5f;
                    const float wgt = cov / (rr * rr);
                    a0 = a0 + wgt * t0, a1 = a1 + wgt * t1, a2 = a2 + wgt * t2;
                    W = W + wgt;
                    ++n;
                }
            }
        }
        if (n != 1u) o0 = a0 / W, o1 = a1 / W, o2 = a2 / W;
    }
    k.out[3u * p] = o0, k.out[3u * p + 1u] = o1, k.out[3u * p + 2u] = o2;
}
