// device/temporal.h — temporal accumulation (include/pbrs_gpu.h, pbrs_temporal_accumulate*): the previous frame's history (colour,
// luminance moments, length) reprojected through the two cameras and the depth AOV, tested against the previous frame's guides and
// blended with this frame.  A post-process like the denoisers: no kernel of the render path is involved.
//
// One thread per pixel, one launch.  What depends on the cameras alone (the three cross products and D of the header) is computed once
// on the host, in the header's order and under the same no-contraction flags, and travels in TemporalConst.  The four taps are a
// gather from the previous planes at the caller's layouts: 11 words (44 B) per tap, fetched together before the first test so that a
// pixel pays one round trip, not one per test; neighbouring lanes reproject to neighbouring pixels, so the taps of a wave fall into a
// few lines.  A guide the call does not have is a template parameter, not a test per tap; the first frame (no history) is the
// instantiation without any tap.  No atomics, no LDS.
//
// Moving instances (pbrs_temporal_accumulate_motion*, pbrs_motion_vectors*): temporal_reproject is the one place that turns a pixel and
// its depth into (wq, xq, yq), with the instance's motion record applied to the surface point when MOTION is set; k_temporal<.., MOTION>
// and k_motion_vectors both call it, so the AOV and the accumulation cannot disagree.  The record is a 96-byte gather by instance id
// through plain global loads (six 16-byte loads: the table is the context's own allocation, so every record is 16-byte aligned);
// neighbouring lanes mostly share an id, so a wave touches a few lines.  The dependency chain of a MOTION pixel is
// {depth, instance, normal, colour}(p) -> record(instance) -> the four taps: the id travels with the first round trip, the record is a
// second one (the tap addresses depend on it), the taps the third; without MOTION there are two.
#pragma once
#include "denoise.h"  // denoise_finite_flag

struct TemporalConst {
    uint32_t w, h;
    float max_history, depth_tolerance, normal_tolerance2, min_temporal;
    float center[3], c[3], a[3], b[3];      // this frame's camera
    float center_prev[3], nu[3], nv[3], nw[3], D;  // the previous one: nu = cross(b', c'), nv = cross(c', a'), nw = cross(a', b'), D = dot(a', nu)
};

// The header's dot and cross for the host side of the call (dmath.h's are device functions of the same expressions).
inline float temporal_dot(const float* p, const float* q) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }
inline void temporal_cross(const float* p, const float* q, float* out) {
    out[0] = p[1] * q[2] - p[2] * q[1];
    out[1] = p[2] * q[0] - p[0] * q[2];
    out[2] = p[0] * q[1] - p[1] * q[0];
}

// This frame and the previous frame's guides and history as the kernel takes them (pointers at the caller's layouts).
struct TemporalIn {
    const float* rgb;
    const float* variance;  // null: unknown (+inf)
    const float* depth;
    const float* normal;    // read with NORMAL
    const uint32_t* instance;  // read with IDS
    const float* depth_prev;
    const float* normal_prev;
    const uint32_t* instance_prev;
    const float* rgb_hist;
    const float* moments_hist;
    const float* length_hist;
    const pbrs_instance_motion* motion;  // read with MOTION: the context's copy of the caller's table, n_motion records
    uint32_t n_motion;
};
struct TemporalOut {
    float* rgb;
    float* moments;
    float* length;
    float* variance;  // null: not wanted
};

// Rule B from the pixel and its depth (finite and > 0: the caller's test) to (wq, xq, yq), without any rejection: xq and yq mean
// something only where the caller finds wq finite and > 0.  MOTION: the surface point goes through record `id` of the table unless the id
// lies at or above n_motion or the record is flagged PBRS_MOTION_IDENTITY; with NORMAL `nrm` (normal(p) on entry) becomes nm.
template <bool MOTION, bool NORMAL>
__device__ __forceinline__ void temporal_reproject(const TemporalConst& k, uint32_t px, uint32_t py, float z, const pbrs_instance_motion* motion,
                                                   uint32_t n_motion, uint32_t id, f3& nrm, float& wq, float& xq, float& yq) {
    const float x = (float)px + 0.5f, yc = (float)py + 0.5f;
    const f3 dir = ld3(k.c) + ld3(k.a) * x + ld3(k.b) * yc;
    f3 P = ld3(k.center) + dir * z;
    if constexpr (MOTION) {
        if (id < n_motion) {
            const float4* rec = reinterpret_cast<const float4*>(motion + id);
            const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3], r4 = rec[4], r5 = rec[5];
            if (!(__float_as_uint(r5.y) & PBRS_MOTION_IDENTITY)) {
                P = mk3(((r0.x * P.x + r0.y * P.y) + r0.z * P.z) + r0.w, ((r1.x * P.x + r1.y * P.y) + r1.z * P.z) + r1.w,
                        ((r2.x * P.x + r2.y * P.y) + r2.z * P.z) + r2.w);
                if (NORMAL)
                    nrm = mk3((r3.x * nrm.x + r3.y * nrm.y) + r3.z * nrm.z, (r3.w * nrm.x + r4.x * nrm.y) + r4.y * nrm.z,
                              (r4.z * nrm.x + r4.w * nrm.y) + r5.x * nrm.z);
            }
        }
    }
    const f3 e = P - ld3(k.center_prev);
    wq = dot(e, ld3(k.nw)) / k.D;
    xq = (dot(e, ld3(k.nu)) / k.D) / wq;
    yq = (dot(e, ld3(k.nv)) / k.D) / wq;
}

template <bool HISTORY, bool NORMAL, bool IDS, bool MOTION = false>
__global__ void __launch_bounds__(256) k_temporal(TemporalIn in, TemporalOut out, TemporalConst k) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= k.w * k.h) return;
    const f3 cur = ld3(in.rgb + 3 * p);
    // rule A
    if (denoise_finite_flag(cur.x, cur.y, cur.z) == 0.0f) {
        out.rgb[3 * p] = cur.x, out.rgb[3 * p + 1] = cur.y, out.rgb[3 * p + 2] = cur.z;
        out.moments[2 * p] = 0.0f, out.moments[2 * p + 1] = 0.0f;
        out.length[p] = 0.0f;
        if (out.variance) out.variance[p] = pn_inf();
        return;
    }
    const float y = luminance(cur);
    f3 S = mk3(0.0f, 0.0f, 0.0f);
    float A1 = 0.0f, A2 = 0.0f, N = 0.0f, W = 0.0f;
    if constexpr (HISTORY) {
        // rule B
        const uint32_t py = p / k.w, px = p - py * k.w;
        const float z = in.depth[p];
        if (pn_isfinite(z) && z > 0.0f) {
            // this pixel's normal and id travel with its depth: with MOTION the record's address waits for the id
            f3 np = mk3(0.0f, 0.0f, 0.0f);
            uint32_t idp = 0u;
            if (NORMAL) np = ld3(in.normal + 3 * p);
            if (IDS || MOTION) idp = in.instance[p];
            float wq, xq, yq;
            temporal_reproject<MOTION, NORMAL>(k, px, py, z, in.motion, in.n_motion, idp, np, wq, xq, yq);  // np is nm from here on
            if (pn_isfinite(wq) && wq > 0.0f) {
                const float fx = xq - 0.5f, fy = yq - 0.5f;
                if (fx > -1.0f && fx < (float)k.w && fy > -1.0f && fy < (float)k.h) {
                    const float flx = pn_floor(fx), fly = pn_floor(fy);
                    const int ix = pn_f32_to_i32(flx), iy = pn_f32_to_i32(fly);  // -1 .. w-1, -1 .. h-1
                    const float tx = fx - flx, ty = fy - fly;
                    // the four taps' records, fetched together; a tap outside the image reads pixel p's and does not count
                    f3 cq[4], nq[4];
                    float m1q[4], m2q[4], lq[4], zq[4];
                    uint32_t idq[4] = {0u, 0u, 0u, 0u};
                    bool inside[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int qx = ix + (t & 1), qy = iy + (t >> 1);
                        inside[t] = qx >= 0 && qx < (int)k.w && qy >= 0 && qy < (int)k.h;
                        const uint32_t q = inside[t] ? (uint32_t)qy * k.w + (uint32_t)qx : p;
                        lq[t] = in.length_hist[q];
                        cq[t] = ld3(in.rgb_hist + 3 * q);
                        m1q[t] = in.moments_hist[2 * q], m2q[t] = in.moments_hist[2 * q + 1];
                        zq[t] = in.depth_prev[q];
                        nq[t] = mk3(0.0f, 0.0f, 0.0f);
                        if (NORMAL) nq[t] = ld3(in.normal_prev + 3 * q);
                        if (IDS) idq[t] = in.instance_prev[q];
                    }
                    const float dtol = k.depth_tolerance * wq;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {  // j = t >> 1 outer, i = t & 1 inner
                        const float bw = ((t & 1) ? tx : 1.0f - tx) * ((t >> 1) ? ty : 1.0f - ty);
                        bool ok = inside[t] && bw > 0.0f && lq[t] > 0.0f;
                        ok = ok && denoise_finite_flag(cq[t].x, cq[t].y, cq[t].z) != 0.0f && pn_isfinite(m1q[t]) && pn_isfinite(m2q[t]);
                        ok = ok && pn_isfinite(zq[t]) && pn_abs(zq[t] - wq) <= dtol;
                        if (NORMAL) {
                            const f3 d = nq[t] - np;
                            ok = ok && (d.x * d.x + d.y * d.y) + d.z * d.z <= k.normal_tolerance2;
                        }
                        if (IDS) ok = ok && idq[t] == idp;
                        if (ok) {
                            S = S + cq[t] * bw;
                            A1 = A1 + bw * m1q[t];
                            A2 = A2 + bw * m2q[t];
                            N = N + bw * lq[t];
                            W = W + bw;
                        }
                    }
                }
            }
        }
    }
    // rule C
    f3 o = cur;
    float m1 = y, m2 = y * y, len = 1.0f;
    if (HISTORY && W != 0.0f) {
        const float iw = 1.0f / W;
        const f3 H = S * iw;
        const float h1 = A1 * iw, h2 = A2 * iw, n = N * iw;
        len = pn_min(n + 1.0f, k.max_history);
        const float al = 1.0f / len;
        o = H + (cur - H) * al;
        m1 = h1 + al * (y - h1);
        m2 = h2 + al * (y * y - h2);
    }
    out.rgb[3 * p] = o.x, out.rgb[3 * p + 1] = o.y, out.rgb[3 * p + 2] = o.z;
    out.moments[2 * p] = m1, out.moments[2 * p + 1] = m2;
    out.length[p] = len;
    // rule D
    if (out.variance) {
        float v;
        if (len >= k.min_temporal) {
            v = m2 - m1 * m1;
            v = v < 0.0f ? 0.0f : v;
            if (v != v) v = pn_inf();
        } else {
            v = pn_inf();
            if (in.variance) {
                const float vin = in.variance[p];
                if (!(vin != vin || vin < 0.0f)) v = vin;
            }
        }
        out.variance[p] = v * (1.0f / len);
    }
}

// pbrs_motion_vectors*: temporal_reproject written out per pixel.  One thread per pixel; no LDS, no atomics.
template <bool MOTION>
__global__ void __launch_bounds__(256) k_motion_vectors(const float* depth, const uint32_t* instance, const pbrs_instance_motion* motion, uint32_t n_motion,
                                                        float* motion_out, float* prev_depth_out, TemporalConst k) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= k.w * k.h) return;
    const uint32_t py = p / k.w, px = p - py * k.w;
    const float z = depth[p];
    float mx = 0.0f, my = 0.0f, wo = pn_inf();
    if (pn_isfinite(z) && z > 0.0f) {
        uint32_t id = 0u;
        if (MOTION) id = instance[p];
        f3 unused = mk3(0.0f, 0.0f, 0.0f);
        float wq, xq, yq;
        temporal_reproject<MOTION, false>(k, px, py, z, motion, n_motion, id, unused, wq, xq, yq);
        if (pn_isfinite(wq) && wq > 0.0f) {
            mx = xq - ((float)px + 0.5f), my = yq - ((float)py + 0.5f);
            wo = wq;
        }
    }
    motion_out[2 * p] = mx, motion_out[2 * p + 1] = my;
    if (prev_depth_out) prev_depth_out[p] = wo;
}
