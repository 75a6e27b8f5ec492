// device/motion_blur.h — motion blur (include/pbrs_gpu.h, pbrsm_motion_blur*): a shutter as an image operation, the half-exposure
// velocities, each tile's dominant velocity and the gather along it in one launch.  A post-process like device/dof.h, whose mould this
// file follows: no kernel of the render path is involved.  One kernel, wave64, 256-thread blocks:
//
//   k_motion_blur<HALO, VEC, JIT>  a block per 16 x 16 tile of the output (the header's tile), thread 16 * ly + lx at (lx, ly).  The block
//                     stages the tile and a halo of HALO pixels on every side in LDS as five planes (r, g, b, zeff, len), a row every
//                     kMotionBlurPitch floats.  A slot's place depends only on its offset from the tile, so the tap loop forms no
//                     coordinate test: the rectangle that is loaded is cut at the image's edge, and every slot outside the image, like
//                     every pixel with a non-finite rgb, gets zeff = 0 and len = -1.  Every real zeff is > 0, so such a tap has f = 1 and
//                     wgt = 1 * cyl(dist, -1) + 0 * cyl(dist, len(p)) = 0 + 0: it is left out by the arithmetic every tap goes through,
//                     without a branch of its own.  HALO is 4, 8 or 16; the host launches the smallest that holds max_radius.  VEC reads
//                     rgb and depth as aligned groups of four floats where both planes are 16-byte aligned (a staged row starts at any
//                     float, so a group's floats outside the row are dropped), float by float otherwise: the same bytes either way.
//                     The motion vectors are read once per slot, two floats, in the second pass.  JIT is PBRS_MOTION_BLUR_JITTER.
//
// Step 1 of the header is computed while staging (a second pass over the staged slots, once the loads have landed): the slot's
// velocity goes to velocity_out where the slot is a pixel of the tile, its (ll, index) into the thread's running maximum where the slot
// lies within max_radius of the tile, and its len, or the -1, into the plane.  Step 2 is that maximum over the block: the key
// (ll, -index) is a total order, so a shuffle tree per wave and four LDS records across the waves give the header's pixel whatever the
// order; the winner's velocity rides along, and every lane then holds vn as the scalar it is.  A tile with len(vn) <= 0.5 copies.
// A pixel's acc, W and n are one thread's, in the header's order: no atomics, no scratch, no sum across lanes.  All taps lie within
// p +- max_radius (|vn| <= R, |t| < 1; the offsets are clamped to that besides, which changes nothing and keeps a read inside the
// planes whatever the arithmetic does), so the gather never leaves LDS.
//
// Without JIT the offset (dx, dy) of tap i and its dist are the same for the whole tile: S threads compute them once into a table, and
// the loop reads them at one address for all lanes (a broadcast) and skips a centre tap as a block.  With JIT they are a lane's own.
//
// LDS.  Five planes of (16 + 2 HALO) rows of 48 floats: 22.5, 30 and 45 KiB for HALO 4, 8 and 16, plus 0.6 KiB of table and records;
// six, five and three blocks fit a CU's 160 KiB.  A tap reads len, zeff and the three channels, each a ds_read_b32 at
// (row + ly + dy) * 48 + lx + dx dwords.  The lanes of a wave differ only by their own (lx, ly) when (dx, dy) is the tile's, and then
// device/dof.h's argument holds as it stands: ds_read_b32 banks are dword mod 32, its lane groups the two 32-lane halves, a half is two
// tile rows of 16 consecutive dwords, and with 48 = 16 mod 32 the second row's banks are the first's plus 16: conflict-free for every
// (dx, dy).  With JIT two lanes' t differ by up to (15 / 16) * 2 / S, so their offsets differ by up to 1.875 |vn| / S pixels per axis,
// rounded up: one pixel where S >= 2 |vn|, two at the defaults' worst (|vn| = 16, S = 16).  A half holds two tile rows and so eight of
// the sixteen jitter values; the four lanes of one value sit four columns apart in one row and never meet on a bank, and two lanes
// that read the same slot broadcast.  Lanes of different offsets can meet on a bank at different addresses, so a read costs at most
// as many LDS cycles as the half has distinct offsets, eight at the very worst and two or three where the offsets differ by a pixel.
// That is reasoning from the addresses, not a counter.  The loop is short (S taps of some forty vector instructions, a division
// among them only where the tap is behind the pixel); the call is mostly its staging.  tools/motion_blur_cost.py times the call: at
// 1080p and max_radius 16 a field in which nothing moves takes 139 us, one in which every pixel gathers 16 taps 172 us (with JIT 197).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/pbrs_gpu.h"
#include "../../../include/pbrs_numeric.h"

constexpr uint32_t kMotionBlurBlock = 256;
constexpr uint32_t kMotionBlurTile = 16;
constexpr uint32_t kMotionBlurPitch = 48;  // floats per staged row of a plane
static_assert(kMotionBlurBlock == kMotionBlurTile * kMotionBlurTile, "k_motion_blur: a thread per pixel of the tile");
static_assert(kMotionBlurTile + 2u * PBRS_MOTION_BLUR_MAX_RADIUS <= kMotionBlurPitch && kMotionBlurPitch % 32u == 16u,
              "a staged row fits the pitch, which is 16 mod 32");
static_assert(PBRS_MOTION_BLUR_MAX_TAPS <= kMotionBlurBlock, "the table of taps is filled in one trip");

struct MotionBlur {
    const float* rgb;     // w x h pixels of three floats
    const float* depth;   // w x h
    const float* motion;  // w x h pixels of two floats
    float* out;           // w x h pixels of three floats; not rgb
    float* velocity;      // w x h pixels of two floats, or null
    uint32_t w, h, tiles_x;
    uint32_t R;  // max_radius, 1 .. HALO
    uint32_t S;  // taps, 2 .. 64
    float k;     // shutter * 0.5f (> 0: the host copies where shutter is 0)
    float z_rel;
};

// Step 1 of the header: the half-exposure vector of a motion vector, its squared length and its length.
__device__ __forceinline__ void motion_blur_velocity(float mx, float my, float k, float Rf, float& vx, float& vy, float& ll, float& len) {
    vx = 0.0f, vy = 0.0f;
    if (pn_isfinite(mx) && pn_isfinite(my)) vx = mx * k, vy = my * k;
    ll = vx * vx + vy * vy;
    len = __builtin_sqrtf(ll);
    if (len > Rf) {
        const float s = Rf / len;
        vx = vx * s, vy = vy * s;
        ll = vx * vx + vy * vy;
        len = __builtin_sqrtf(ll);
        len = len < Rf ? len : Rf;
    }
}

// Tap i of the line through a pixel whose jitter is j: the offset (dx, dy), each within +-R.
__device__ __forceinline__ void motion_blur_tap(float vnx, float vny, uint32_t i, float j, float Sf, int R, int& dx, int& dy) {
    const float t = (((float)i + 0.5f) + j) / Sf * 2.0f - 1.0f;
    dx = (int)pn_floor(vnx * t + 0.5f), dy = (int)pn_floor(vny * t + 0.5f);
    dx = dx < -R ? -R : (dx > R ? R : dx), dy = dy < -R ? -R : (dy > R ? R : dy);  // (never taken: |vn| <= R and |t| < 1)
}

// cyl of the header.
__device__ __forceinline__ float motion_blur_cyl(float d, float l) {
    float c = (l - d) + 0.5f;
    c = c > 0.0f ? c : 0.0f;
    return c < 1.0f ? c : 1.0f;
}

// A value every lane holds alike, as the scalar it is.
__device__ __forceinline__ float motion_blur_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

template <uint32_t HALO, bool VEC, bool JIT>
__global__ void __launch_bounds__(256) k_motion_blur(MotionBlur k) {
    constexpr uint32_t S = kMotionBlurTile + 2u * HALO;  // staged rows and columns
    constexpr uint32_t PLANE = S * kMotionBlurPitch;
    constexpr uint32_t GR = (3u * S + 6u) / 4u;  // 3 S floats that start at any float of a group of four span at most this many groups
    constexpr uint32_t GD = (S + 6u) / 4u;
    constexpr uint32_t WAVES = kMotionBlurBlock / 64u;
    static_assert(4u * GR >= 3u * S + 3u && 4u * GD >= S + 3u, "the groups that cover a staged row");
    __shared__ float lds[5u * PLANE];
    __shared__ float best_ll[WAVES], best_vx[WAVES], best_vy[WAVES];  // a wave's maximum: the key's ll, the winner's velocity
    __shared__ uint32_t best_index[WAVES];                            // and the key's row-major index
    __shared__ int tap_offset[PBRS_MOTION_BLUR_MAX_TAPS];             // without JIT: dy * pitch + dx of tap i, 0 for a centre tap
    __shared__ float tap_dist[PBRS_MOTION_BLUR_MAX_TAPS];
    float* const LR = lds;
    float* const LZ = lds + 3u * PLANE;  // zeff, 0 where the slot can never contribute
    float* const LL = lds + 4u * PLANE;  // len, -1 where the slot can never contribute
    const uint32_t tile_y = blockIdx.x / k.tiles_x, tile_x = blockIdx.x - tile_y * k.tiles_x;
    const uint32_t X0 = tile_x * kMotionBlurTile, Y0 = tile_y * kMotionBlurTile;  // X0 < w, Y0 < h
    // the rectangle that is loaded, [gx0, gx1) x [gy0, gy1), and the slot of its first pixel
    const uint32_t gx0 = X0 > HALO ? X0 - HALO : 0u, gy0 = Y0 > HALO ? Y0 - HALO : 0u;
    const uint32_t gx1 = X0 + kMotionBlurTile + HALO < k.w ? X0 + kMotionBlurTile + HALO : k.w;
    const uint32_t gy1 = Y0 + kMotionBlurTile + HALO < k.h ? Y0 + kMotionBlurTile + HALO : k.h;
    const uint32_t ox = gx0 + HALO - X0, oy = gy0 + HALO - Y0;  // 0 .. HALO
    const uint32_t cols = gx1 - gx0, rows = gy1 - gy0;          // 1 .. S each, ox + cols <= S, oy + rows <= S
    const size_t pixels = (size_t)k.w * k.h;

    if (VEC) {
        const uint32_t nf = 3u * cols;  // floats of a staged rgb row
        for (uint32_t i = threadIdx.x; i < rows * GR; i += kMotionBlurBlock) {
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
                    LR[ch * PLANE + (oy + r) * kMotionBlurPitch + ox + px] = v[e];
                }
            }
        }
        for (uint32_t i = threadIdx.x; i < rows * GD; i += kMotionBlurBlock) {
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
                if (f >= a && f < a + cols) LZ[(oy + r) * kMotionBlurPitch + ox + (uint32_t)(f - a)] = v[e];
            }
        }
    } else {
        for (uint32_t i = threadIdx.x; i < rows * cols; i += kMotionBlurBlock) {
            const uint32_t r = i / cols, cx = i - r * cols;
            const size_t p = (size_t)(gy0 + r) * k.w + gx0 + cx;
            const uint32_t slot = (oy + r) * kMotionBlurPitch + ox + cx;
            LR[slot] = k.rgb[3u * p], LR[PLANE + slot] = k.rgb[3u * p + 1u], LR[2u * PLANE + slot] = k.rgb[3u * p + 2u];
            LZ[slot] = k.depth[p];
        }
    }
    __syncthreads();
    // Steps 1 and 2 on what was loaded; zeff = 0 and len = -1 on a pixel whose rgb is not finite and on every slot outside the image
    const float Rf = (float)k.R;
    float top_ll = -1.0f, top_vx = 0.0f, top_vy = 0.0f;  // (ll >= 0 and the tile's first pixel is in the window: every block finds a pixel)
    uint32_t top_index = 0xFFFFFFFFu;
    for (uint32_t i = threadIdx.x; i < S * S; i += kMotionBlurBlock) {
        const uint32_t sy = i / S, sx = i - sy * S;
        const uint32_t slot = sy * kMotionBlurPitch + sx;
        float len_slot = -1.0f, zeff = 0.0f;
        if (sx >= ox && sx < ox + cols && sy >= oy && sy < oy + rows) {
            const uint32_t index = (gy0 + (sy - oy)) * k.w + gx0 + (sx - ox);  // < 2^28
            float vx, vy, ll, len;
            motion_blur_velocity(k.motion[2u * (size_t)index], k.motion[2u * (size_t)index + 1u], k.k, Rf, vx, vy, ll, len);
            if (k.velocity && sx >= HALO && sx < HALO + kMotionBlurTile && sy >= HALO && sy < HALO + kMotionBlurTile)
                k.velocity[2u * (size_t)index] = vx, k.velocity[2u * (size_t)index + 1u] = vy;
            if (sx + k.R >= HALO && sx < HALO + kMotionBlurTile + k.R && sy + k.R >= HALO && sy < HALO + kMotionBlurTile + k.R &&
                (ll > top_ll || (ll == top_ll && index < top_index)))
                top_ll = ll, top_index = index, top_vx = vx, top_vy = vy;
            if (pn_isfinite(LR[slot]) && pn_isfinite(LR[PLANE + slot]) && pn_isfinite(LR[2u * PLANE + slot])) {
                const float z = LZ[slot];
                len_slot = len, zeff = z > 0.0f ? z : pn_inf();
            }
        }
        LZ[slot] = zeff, LL[slot] = len_slot;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float o_ll = __shfl_xor(top_ll, m, 64), o_vx = __shfl_xor(top_vx, m, 64), o_vy = __shfl_xor(top_vy, m, 64);
        const uint32_t o_index = (uint32_t)__shfl_xor((int)top_index, m, 64);
        if (o_ll > top_ll || (o_ll == top_ll && o_index < top_index)) top_ll = o_ll, top_index = o_index, top_vx = o_vx, top_vy = o_vy;
    }
    if ((threadIdx.x & 63u) == 0u) {
        const uint32_t wave = threadIdx.x >> 6;
        best_ll[wave] = top_ll, best_index[wave] = top_index, best_vx[wave] = top_vx, best_vy[wave] = top_vy;
    }
    __syncthreads();
    top_ll = best_ll[0], top_index = best_index[0], top_vx = best_vx[0], top_vy = best_vy[0];
#pragma unroll
    for (uint32_t i = 1; i < WAVES; ++i)
        if (best_ll[i] > top_ll || (best_ll[i] == top_ll && best_index[i] < top_index))
            top_ll = best_ll[i], top_index = best_index[i], top_vx = best_vx[i], top_vy = best_vy[i];
    const float vnx = motion_blur_uniform(top_vx), vny = motion_blur_uniform(top_vy);
    float vn_len = __builtin_sqrtf(motion_blur_uniform(top_ll));  // len of step 1 from the ll it left: the square root, then the cap
    vn_len = vn_len < Rf ? vn_len : Rf;
    const bool moving = vn_len > 0.5f;
    const float Sf = (float)k.S;
    if (!JIT) {
        if (moving && threadIdx.x < k.S) {
            int dx, dy;
            motion_blur_tap(vnx, vny, threadIdx.x, 0.0f, Sf, (int)k.R, dx, dy);
            tap_offset[threadIdx.x] = dy * (int)kMotionBlurPitch + dx;  // 0 only for (0, 0): |dx| <= 16 < the pitch
            tap_dist[threadIdx.x] = __builtin_sqrtf((float)(dx * dx + dy * dy));
        }
        __syncthreads();
    }

    const uint32_t lx = threadIdx.x % kMotionBlurTile, ly = threadIdx.x / kMotionBlurTile;
    const uint32_t X = X0 + lx, Y = Y0 + ly;
    if (X >= k.w || Y >= k.h) return;  // (after the last barrier)
    const uint32_t centre = (ly + HALO) * kMotionBlurPitch + lx + HALO;
    const size_t p = (size_t)Y * k.w + X;
    const float pr = LR[centre], pg = LR[PLANE + centre], pb = LR[2u * PLANE + centre];
    float o0 = pr, o1 = pg, o2 = pb;
    const float lp = LL[centre];
    // lp < 0: the pixel's own rgb is not finite, it passes through.  !moving: the tile copies.
    if (moving && lp >= 0.0f) {
        const float zp = LZ[centre], den = k.z_rel * zp;
        float jit = 0.0f;
        if (JIT) jit = ((float)(uint32_t)((0x5D7F91B36E4CA280ull >> (4u * (4u * (Y & 3u) + (X & 3u)))) & 15u) + 0.5f) / 16.0f - 0.5f;  // M[y & 3][x & 3]
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, W = 0.0f;
        uint32_t n = 0;
        for (uint32_t i = 0; i < k.S; ++i) {
            int offset;
            float dist;
            if (JIT) {
                int dx, dy;
                motion_blur_tap(vnx, vny, i, jit, Sf, (int)k.R, dx, dy);
                offset = dy * (int)kMotionBlurPitch + dx;
                dist = __builtin_sqrtf((float)(dx * dx + dy * dy));
            } else {
                offset = __builtin_amdgcn_readfirstlane(tap_offset[i]);
                dist = tap_dist[i];
            }
            if (offset == 0) continue;  // the centre tap is left out
            const uint32_t slot = (uint32_t)((int)centre + offset);
            const float lq = LL[slot], zq = LZ[slot];
            float f = 1.0f;
            if (!(zq <= zp)) {
                const float a = 1.0f - (zq - zp) / den;
                f = a > 0.0f ? a : 0.0f;
            }
            const float wgt = f * motion_blur_cyl(dist, lq) + (1.0f - f) * motion_blur_cyl(dist, lp);
            if (wgt > 0.0f) {
                a0 = a0 + wgt * LR[slot], a1 = a1 + wgt * LR[PLANE + slot], a2 = a2 + wgt * LR[2u * PLANE + slot];
                W = W + wgt;
                ++n;
            }
        }
        if (n != 0u) {
            const float rest = Sf - W;
            o0 = (a0 + rest * pr) / Sf, o1 = (a1 + rest * pg) / Sf, o2 = (a2 + rest * pb) / Sf;
        }
    }
    k.out[3u * p] = o0, k.out[3u * p + 1u] = o1, k.out[3u * p + 2u] = o2;
}
