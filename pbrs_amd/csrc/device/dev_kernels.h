// device/dev_kernels.h — the developer entry points' kernels: the numeric contract's functions on the device (pbrs_numeric_eval*) and
// the exports of a pass's camera rays and radiances (pbrs_camera_rays, pbrs_render_sample_radiance).
#pragma once
#include "path_state.h"
#include "../../../include/pbrs_numeric_probe.h"

__global__ void __launch_bounds__(256) k_numeric_eval(uint32_t fn, uint32_t n, const float* x, const float* y, float* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a = x[i], b = y ? y[i] : 0.0f, r = 0.0f;
    switch (fn) {
        case 0: r = pn_sin(a); break;
        case 1: r = pn_cos(a); break;
        case 2: r = pn_tan(a); break;
        case 3: r = pn_atan(a); break;
        case 4: r = pn_atan2(a, b); break;
        case 5: r = pn_acos(a); break;
        case 6: r = pn_exp(a); break;
        case 7: r = pn_ln(a); break;
        case 8: r = pn_hypot(a, b); break;
        case 9: r = a / b; break;
        case 10: r = pn_sqrt(a); break;
        case 11: r = pn_asin(a); break;
        case 12: r = pn_powi(a, (int)b); break;
        case 13: r = pn_fract(a); break;
        case 14: r = pn_floor(a); break;
        case 15: r = qdiv(-a, b, -(1.0f / b)); break;  // the box test's quotient (traverse.h): must equal a / b in its guarded range
        default: r = pn_from_bits(pn_probe_eval(fn, a, b)); break;  // ids 16 on: include/pbrs_numeric_probe.h (raw words)
    }
    reinterpret_cast<uint32_t*>(out)[i] = pn_bits(r);
}
// functions of more than two operands: row i of the n x k operand matrix (words) -> one word
__global__ void __launch_bounds__(256) k_numeric_eval_k(uint32_t fn, uint32_t n, uint32_t k, const uint32_t* ops, uint32_t* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t w[PN_PROBE_MAX_K];
    for (uint32_t j = 0; j < PN_PROBE_MAX_K; ++j) w[j] = j < k ? ops[(size_t)i * k + j] : 0u;
    out[i] = pn_probe_eval_k(fn, w);
}

__global__ void __launch_bounds__(256) k_export_rays(PathState st, uint32_t n, float* origins, float* dirs) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 o = st.q[0][0][i], d = st.q[0][1][i];  // as k_raygen leaves them: queue position = slot
    origins[3 * i] = o.x; origins[3 * i + 1] = o.y; origins[3 * i + 2] = o.z;
    dirs[3 * i] = d.x; dirs[3 * i + 1] = d.y; dirs[3 * i + 2] = d.z;
}
__global__ void __launch_bounds__(256) k_export_radiance(PathState st, uint32_t n, float* rgb) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 l = st.L[i];
    rgb[3 * i] = l.x; rgb[3 * i + 1] = l.y; rgb[3 * i + 2] = l.z;
}
