// device/bloom.h — bloom (include/pbrs_gpu.h, pbrsb_bloom*): the bright part of an image down a pyramid of half-size levels, back up
// with each coarser level mixed into the finer one, and added to the image.  A post-process like the denoisers: no kernel of the
// render path is involved.  The pyramid is one chain of levels in BUF_BLOOM, a float4 (r, g, b, 0) per level pixel, so that every access
// to a level is one aligned 16-byte load or store.  Four kernels, wave64, 256-thread blocks but for the tail's:
//
//   k_bloom_down<FIRST, VEC>  a block per 16 x 16 destination tile, thread 16 * ly + lx at (lx, ly).  The block stages the source
//                             pixels its 16 taps per thread reach (at most 34 x 34: two per destination and a halo of one, cut at the
//                             source's edge) in LDS, r g b interleaved, a row every kBloomPitch floats.  Coordinates are clamped
//                             before the tap is read, so no slot outside the staged rectangle is ever formed.  FIRST reads the
//                             image: rows of packed floats, as aligned groups of four where the plane is 16-byte aligned (VEC; a row
//                             starts at any float, so a group's floats outside the row are dropped), float by float otherwise, the
//                             same bytes either way; then the bright pass in place on the staged pixels.  Otherwise a level's float4.
//   k_bloom_tail              one block of 1024 threads.  Once a level and everything below it hold at most kBloomTailPixels pixels,
//                             the block loads that level into LDS, runs the rest of the way down and all the way back up there, and
//                             stores the merged level over the one it read: one launch in the place of two per level.  The loops
//                             are those of k_bloom_down and k_bloom_up on another address: the bits do not depend on where the tail
//                             begins.
//   k_bloom_up                a thread per pixel of the finer level: four float4 taps of the coarser one, d_l read and u_l written in
//                             place.
//   k_bloom_composite<MIX, VEC>  up(u_0) and the composite.  A thread takes four consecutive pixels of the flat plane: three 16-byte
//                             loads of rgb and three 16-byte stores of out where both planes are 16-byte aligned (VEC), twelve 4-byte
//                             ones otherwise and for the last w * h % 4 pixels; four float4 taps of u_0 per pixel.  rgb is read only at
//                             the thread's own pixels, before they are written: out may be rgb.
//
// No atomics, no reduction across lanes: a pixel's sums are one thread's, in the header's order.
//
// LDS.  k_bloom_down holds 34 rows of kBloomPitch = 104 floats, 13.8 KiB.  A tap is a ds_read_b32 at 6 lx + const dwords: the 16 lanes
// of a tile row cover 16 distinct even banks, and the second row of a 32-lane half lands on the same parity, so most taps are two-way
// conflicts; a stride-two gather has that with any pitch.  k_bloom_tail holds 3 x 5461 floats, 64 KiB less 4 B, one block on its CU.
// None of this is a measured cycle count; tools/bloom_cost.py times the call.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/pbrs_gpu.h"
#include "../../../include/pbrs_numeric.h"

constexpr uint32_t kBloomBlock = 256;
constexpr uint32_t kBloomTile = 16;
constexpr uint32_t kBloomSrc = 2u * kBloomTile + 2u;  // source rows and columns a tile reaches, at most
constexpr uint32_t kBloomPitch = 104;                 // floats per staged row
constexpr uint32_t kBloomRowGroups = 27;              // 102 floats that start at any float of a group of four span at most 27 groups
// The tail takes over at the first level l whose pixels, with those of every level below it, are at most this many: a 64 x 64 level
// with all its successors (4096 + 1024 + ... + 1 = 5461), three floats each, in the 64 KiB a block may declare.
constexpr uint32_t kBloomTailPixels = 5461;
// k_bloom_tail's block: sixteen waves on the one CU it has.  With 256 threads the kernel took 17 us on a 64 x 64 level, most of it the
// latency of sixteen dependent trips through the loop that loads the level, more than the six launches it replaces.
constexpr uint32_t kBloomTailBlock = 1024;
constexpr uint32_t kBloomTailLoads = 6;  // float4 loads a thread has in flight: 6 x 1024 >= kBloomTailPixels, one trip
static_assert(kBloomTailLoads * kBloomTailBlock >= kBloomTailPixels, "k_bloom_tail loads its level in one trip");
static_assert(kBloomBlock == kBloomTile * kBloomTile, "k_bloom_down: a thread per destination pixel of the tile");
static_assert(kBloomPitch >= 3u * kBloomSrc && 4u * kBloomRowGroups >= 3u * kBloomSrc + 3u, "a staged row and the groups that cover it");
static_assert(3u * kBloomTailPixels * sizeof(float) <= 65536u, "k_bloom_tail's levels fit the LDS a block may declare");

// The bright pass's constants, from the host: t, k = t * knee, t - k, t + k, 1.0f / (4.0f * k).
struct BloomBright {
    float t, k, lo, hi, inv4k;
};

__device__ __forceinline__ float bloom_luminance(float r, float g, float b) { return (0.21267127f * r + 0.71515972f * g) + 0.07216883f * b; }

// Step 2 of the header on one pixel, in place.
__device__ __forceinline__ void bloom_bright(const BloomBright& k, float& r, float& g, float& b) {
    if (!(pn_isfinite(r) && pn_isfinite(g) && pn_isfinite(b))) {
        r = 0.0f, g = 0.0f, b = 0.0f;
        return;
    }
    r = r > 0.0f ? r : 0.0f, g = g > 0.0f ? g : 0.0f, b = b > 0.0f ? b : 0.0f;
    const float Y = bloom_luminance(r, g, b);
    float f;
    if (Y <= k.lo) {
        f = 0.0f;
    } else if (Y >= k.hi) {
        f = (Y - k.t) / Y;
    } else {
        const float s = (Y - k.t) + k.k;
        f = ((s * s) * k.inv4k) / Y;
    }
    r = r * f, g = g * f, b = b * f;
}

__device__ __forceinline__ float bloom_down_weight(int i) { return (i == 0 || i == 3) ? 0.125f : 0.375f; }

// Step 3 at destination (X, Y) of a source of sw x sh pixels: `s` holds the source's pixels from (xs, ys) on, three floats each, a row
// every `pitch` floats.  Every clamped coordinate of the taps lies in what `s` holds.
__device__ __forceinline__ void bloom_down_pixel(const float* s, uint32_t pitch, uint32_t xs, uint32_t ys, uint32_t sw, uint32_t sh, uint32_t X, uint32_t Y,
                                                 float& r, float& g, float& b) {
    r = 0.0f, g = 0.0f, b = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 2; ++dy) {
        int sy = (int)(2u * Y) + dy;
        sy = sy < 0 ? 0 : (sy > (int)sh - 1 ? (int)sh - 1 : sy);
        const float* row = s + ((uint32_t)sy - ys) * pitch;
#pragma unroll
        for (int dx = -1; dx <= 2; ++dx) {
            int sx = (int)(2u * X) + dx;
            sx = sx < 0 ? 0 : (sx > (int)sw - 1 ? (int)sw - 1 : sx);
            const float* c = row + 3u * ((uint32_t)sx - xs);
            const float wgt = bloom_down_weight(dx + 1) * bloom_down_weight(dy + 1);
            r = r + wgt * c[0], g = g + wgt * c[1], b = b + wgt * c[2];
        }
    }
}

// The four taps of up() at (x, y) into a level of cw x ch pixels: X0 <= cw - 1 because cw = (fw + 1) / 2 and x < fw.
struct BloomTaps {
    uint32_t x0, x1, y0, y1;
};
__device__ __forceinline__ BloomTaps bloom_up_taps(uint32_t x, uint32_t y, uint32_t cw, uint32_t ch) {
    BloomTaps t;
    t.x0 = x >> 1, t.y0 = y >> 1;
    t.x1 = (x & 1u) ? (t.x0 + 1u < cw ? t.x0 + 1u : cw - 1u) : (t.x0 ? t.x0 - 1u : 0u);
    t.y1 = (y & 1u) ? (t.y0 + 1u < ch ? t.y0 + 1u : ch - 1u) : (t.y0 ? t.y0 - 1u : 0u);
    return t;
}
// One channel of up(): the taps at (X0, Y0), (X1, Y0), (X0, Y1), (X1, Y1).
__device__ __forceinline__ float bloom_up_sum(float a, float b, float c, float d) {
    float acc = 0.0f;
    acc = acc + (0.75f * 0.75f) * a;
    acc = acc + (0.25f * 0.75f) * b;
    acc = acc + (0.75f * 0.25f) * c;
    acc = acc + (0.25f * 0.25f) * d;
    return acc;
}
// up(v)(x, y) of a level in global memory.
__device__ __forceinline__ void bloom_up_global(const float4* v, uint32_t cw, uint32_t ch, uint32_t x, uint32_t y, float& r, float& g, float& b) {
    const BloomTaps t = bloom_up_taps(x, y, cw, ch);
    const float4 a = v[(size_t)t.y0 * cw + t.x0], bb = v[(size_t)t.y0 * cw + t.x1], c = v[(size_t)t.y1 * cw + t.x0], d = v[(size_t)t.y1 * cw + t.x1];
    r = bloom_up_sum(a.x, bb.x, c.x, d.x), g = bloom_up_sum(a.y, bb.y, c.y, d.y), b = bloom_up_sum(a.z, bb.z, c.z, d.z);
}

struct BloomDown {
    const float* rgb;   // FIRST: the image, sw x sh pixels of three floats
    const float4* src;  // otherwise: the level above, sw x sh
    float4* dst;        // dw x dh
    uint32_t sw, sh, dw, dh, tiles_x;
    BloomBright bright;
};

template <bool FIRST, bool VEC>
__global__ void __launch_bounds__(256) k_bloom_down(BloomDown k) {
    __shared__ float lds[kBloomSrc * kBloomPitch];
    const uint32_t tile_y = blockIdx.x / k.tiles_x, tile_x = blockIdx.x - tile_y * k.tiles_x;
    const uint32_t X0 = tile_x * kBloomTile, Y0 = tile_y * kBloomTile;  // X0 < dw, Y0 < dh: 2 X0 <= sw - 1
    const uint32_t xs = X0 ? 2u * X0 - 1u : 0u, ys = Y0 ? 2u * Y0 - 1u : 0u;
    const uint32_t xe = 2u * X0 + kBloomSrc - 1u < k.sw ? 2u * X0 + kBloomSrc - 1u : k.sw;
    const uint32_t ye = 2u * Y0 + kBloomSrc - 1u < k.sh ? 2u * Y0 + kBloomSrc - 1u : k.sh;
    const uint32_t cols = xe - xs, rows = ye - ys;  // 1 .. 34 each
    if (FIRST) {
        const uint32_t nf = 3u * cols;  // floats of a staged row
        const size_t total = 3u * (size_t)k.sw * k.sh;
        if (VEC) {
            for (uint32_t i = threadIdx.x; i < rows * kBloomRowGroups; i += kBloomBlock) {
                const uint32_t r = i / kBloomRowGroups, j = i - r * kBloomRowGroups;
                const size_t a = 3u * ((size_t)(ys + r) * k.sw + xs);  // the row's first float
                const size_t f0 = 4u * (a / 4u + j);
                if (f0 >= a + nf) continue;
                float v[4];
                if (f0 + 4u <= total) {
                    const float4 q = *reinterpret_cast<const float4*>(k.rgb + f0);
                    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                } else {  // the plane's last, short group
#pragma unroll
                    for (uint32_t e = 0; e < 4u; ++e) v[e] = f0 + e < total ? k.rgb[f0 + e] : 0.0f;
                }
#pragma unroll
                for (uint32_t e = 0; e < 4u; ++e) {
                    const size_t f = f0 + e;
                    if (f >= a && f < a + nf) lds[r * kBloomPitch + (uint32_t)(f - a)] = v[e];
                }
            }
        } else {
            for (uint32_t i = threadIdx.x; i < rows * nf; i += kBloomBlock) {
                const uint32_t r = i / nf, j = i - r * nf;
                lds[r * kBloomPitch + j] = k.rgb[3u * ((size_t)(ys + r) * k.sw + xs) + j];
            }
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < rows * cols; i += kBloomBlock) {
            const uint32_t r = i / cols, cx = i - r * cols;
            float* c = lds + r * kBloomPitch + 3u * cx;
            float cr = c[0], cg = c[1], cb = c[2];
            bloom_bright(k.bright, cr, cg, cb);
            c[0] = cr, c[1] = cg, c[2] = cb;
        }
    } else {
        for (uint32_t i = threadIdx.x; i < rows * cols; i += kBloomBlock) {
            const uint32_t r = i / cols, cx = i - r * cols;
            const float4 v = k.src[(size_t)(ys + r) * k.sw + xs + cx];
            float* c = lds + r * kBloomPitch + 3u * cx;
            c[0] = v.x, c[1] = v.y, c[2] = v.z;
        }
    }
    __syncthreads();
    const uint32_t X = X0 + threadIdx.x % kBloomTile, Y = Y0 + threadIdx.x / kBloomTile;
    if (X < k.dw && Y < k.dh) {
        float r, g, b;
        bloom_down_pixel(lds, kBloomPitch, xs, ys, k.sw, k.sh, X, Y, r, g, b);
        k.dst[(size_t)Y * k.dw + X] = make_float4(r, g, b, 0.0f);
    }
}

struct BloomUp {
    const float4* coarse;  // u_{l+1}, cw x ch
    float4* fine;          // d_l in, u_l out, fw x fh
    uint32_t cw, ch, fw, fh;
    float spread;
};

__global__ void __launch_bounds__(256) k_bloom_up(BloomUp k) {
    const uint32_t p = blockIdx.x * kBloomBlock + threadIdx.x;  // a level holds at most 2^26 pixels
    if (p >= k.fw * k.fh) return;
    const uint32_t y = p / k.fw, x = p - y * k.fw;
    float r, g, b;
    bloom_up_global(k.coarse, k.cw, k.ch, x, y, r, g, b);
    const float4 d = k.fine[p];
    k.fine[p] = make_float4(d.x + k.spread * (r - d.x), d.y + k.spread * (g - d.y), d.z + k.spread * (b - d.z), 0.0f);
}

struct BloomTail {
    float4* level;  // the first of the tail's levels: d in, u out, w x h
    uint32_t w, h;
    uint32_t n;     // the tail's levels, >= 2; together at most kBloomTailPixels pixels
    float spread;
};

__global__ void __launch_bounds__(1024) k_bloom_tail(BloomTail k) {
    __shared__ float lds[3u * kBloomTailPixels];  // the levels one after the other, r g b interleaved
    const uint32_t n0 = k.w * k.h;
    {  // every load of the thread is issued before the first is waited for
        float4 v[kBloomTailLoads];
#pragma unroll
        for (uint32_t j = 0; j < kBloomTailLoads; ++j) {
            const uint32_t i = threadIdx.x + j * kBloomTailBlock;
            v[j] = i < n0 ? k.level[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (uint32_t j = 0; j < kBloomTailLoads; ++j) {
            const uint32_t i = threadIdx.x + j * kBloomTailBlock;
            if (i < n0) lds[3u * i] = v[j].x, lds[3u * i + 1u] = v[j].y, lds[3u * i + 2u] = v[j].z;
        }
    }
    __syncthreads();
    {
        uint32_t off = 0, w = k.w, h = k.h;  // the source level: its first pixel and its size
        for (uint32_t j = 1; j < k.n; ++j) {
            const uint32_t dw = (w + 1u) / 2u, dh = (h + 1u) / 2u, doff = off + w * h;
            for (uint32_t i = threadIdx.x; i < dw * dh; i += kBloomTailBlock) {
                const uint32_t Y = i / dw, X = i - Y * dw;
                float r, g, b;
                bloom_down_pixel(lds + 3u * off, 3u * w, 0u, 0u, w, h, X, Y, r, g, b);
                float* c = lds + 3u * (doff + i);
                c[0] = r, c[1] = g, c[2] = b;
            }
            __syncthreads();
            off = doff, w = dw, h = dh;
        }
    }
    for (int j = (int)k.n - 2; j >= 0; --j) {
        uint32_t foff = 0, fw = k.w, fh = k.h;  // level j of the tail, from the first one
        for (int q = 0; q < j; ++q) foff += fw * fh, fw = (fw + 1u) / 2u, fh = (fh + 1u) / 2u;
        const uint32_t coff = foff + fw * fh, cw = (fw + 1u) / 2u, ch = (fh + 1u) / 2u;
        const float* cs = lds + 3u * coff;
        for (uint32_t i = threadIdx.x; i < fw * fh; i += kBloomTailBlock) {
            const uint32_t y = i / fw, x = i - y * fw;
            const BloomTaps t = bloom_up_taps(x, y, cw, ch);
            const float* a = cs + 3u * (t.y0 * cw + t.x0);
            const float* bb = cs + 3u * (t.y0 * cw + t.x1);
            const float* c = cs + 3u * (t.y1 * cw + t.x0);
            const float* d = cs + 3u * (t.y1 * cw + t.x1);
            float* f = lds + 3u * (foff + i);
#pragma unroll
            for (uint32_t e = 0; e < 3u; ++e) {
                const float up = bloom_up_sum(a[e], bb[e], c[e], d[e]);
                f[e] = f[e] + k.spread * (up - f[e]);
            }
        }
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < n0; i += kBloomTailBlock) k.level[i] = make_float4(lds[3u * i], lds[3u * i + 1u], lds[3u * i + 2u], 0.0f);
}

struct BloomComposite {
    const float* rgb;
    float* out;
    const float4* u0;  // cw x ch
    uint32_t w, P, cw, ch;
    float strength;
};

// Step 5 on one pixel, in place.
template <bool MIX>
__device__ __forceinline__ void bloom_composite_pixel(const BloomComposite& k, uint32_t x, uint32_t y, float& r, float& g, float& b) {
    if (!(pn_isfinite(r) && pn_isfinite(g) && pn_isfinite(b))) return;
    float br, bg, bb;
    bloom_up_global(k.u0, k.cw, k.ch, x, y, br, bg, bb);
    if (MIX) {
        r = r + k.strength * (br - r), g = g + k.strength * (bg - g), b = b + k.strength * (bb - b);
    } else {
        r = r + k.strength * br, g = g + k.strength * bg, b = b + k.strength * bb;
    }
}

template <bool MIX, bool VEC>
__global__ void __launch_bounds__(256) k_bloom_composite(BloomComposite k) {
    const uint32_t p0 = 4u * (blockIdx.x * kBloomBlock + threadIdx.x);  // at most 2^28 pixels
    if (p0 >= k.P) return;
    uint32_t y = p0 / k.w, x = p0 - y * k.w;
    if (VEC && p0 + 4u <= k.P) {
        const float4* src = reinterpret_cast<const float4*>(k.rgb + 3 * (size_t)p0);
        const float4 a = src[0], b = src[1], c = src[2];
        float ch[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            bloom_composite_pixel<MIX>(k, x, y, ch[3 * i], ch[3 * i + 1], ch[3 * i + 2]);
            if (++x == k.w) x = 0, ++y;
        }
        float4* dst = reinterpret_cast<float4*>(k.out + 3 * (size_t)p0);
        dst[0] = make_float4(ch[0], ch[1], ch[2], ch[3]), dst[1] = make_float4(ch[4], ch[5], ch[6], ch[7]), dst[2] = make_float4(ch[8], ch[9], ch[10], ch[11]);
    } else {
        const uint32_t end = p0 + 4u < k.P ? p0 + 4u : k.P;
        for (uint32_t p = p0; p < end; ++p) {
            const size_t at = 3 * (size_t)p;
            float r = k.rgb[at], g = k.rgb[at + 1], b = k.rgb[at + 2];
            bloom_composite_pixel<MIX>(k, x, y, r, g, b);
            k.out[at] = r, k.out[at + 1] = g, k.out[at + 2] = b;
            if (++x == k.w) x = 0, ++y;
        }
    }
}
