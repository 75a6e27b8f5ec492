// host/arg_checks_motion_blur.cpp — check_motion_blur of arg_checks.h and the filler pbrsm_motion_blur_params_default
// (include/pbrs_gpu.h, "motion blur"), in a file of their own like arg_checks_dof.cpp: tests/motion_blur_check.cpp holds one row against
// every refusal site of this file and pins their number.  Every refusal returns refuse(CODE, "message") on the spot, in the order the
// header states.
#include "arg_checks.h"

#include "../../../include/pbrs_numeric.h"

namespace pbrs {
namespace {

Refusal refuse(int code, const char* message) { return Refusal{code, message}; }
constexpr uint64_t kMaxPixels = 1ull << 28;

}  // namespace

Refusal check_motion_blur(const pbrs_motion_blur_params* p, const float* rgb, const float* depth, const float* motion, const float* rgb_out) {
    if (!p || !rgb || !depth || !motion || !rgb_out) return refuse(PBRS_E_INVALID, "null motion blur params, rgb, depth, motion or rgb_out");
    if (rgb_out == rgb) return refuse(PBRS_E_INVALID, "the motion blur output must not be its input: a gather reads its neighbours");
    if (p->w == 0 || p->h == 0) return refuse(PBRS_E_INVALID, "empty image");
    if (p->max_radius < 1u || p->max_radius > PBRS_MOTION_BLUR_MAX_RADIUS) return refuse(PBRS_E_INVALID, "the motion blur max_radius must be 1 .. 16");
    if (p->taps < 2u || p->taps > PBRS_MOTION_BLUR_MAX_TAPS) return refuse(PBRS_E_INVALID, "the motion blur taps must be 2 .. 64");
    if ((p->flags & ~PBRS_MOTION_BLUR_JITTER) != 0u) return refuse(PBRS_E_INVALID, "unknown motion blur flag bits");
    if (p->reserved != 0u) return refuse(PBRS_E_INVALID, "the motion blur reserved word must be 0");
    if (!pn_isfinite(p->shutter) || !(p->shutter >= 0.0f) || !(p->shutter <= 1.0f)) return refuse(PBRS_E_INVALID, "the motion blur shutter must be finite and 0 .. 1");
    if (!pn_isfinite(p->z_rel) || !(p->z_rel > 0.0f)) return refuse(PBRS_E_INVALID, "the motion blur z_rel must be finite and > 0");
    if ((uint64_t)p->w * p->h > kMaxPixels) return refuse(PBRS_E_LIMIT, "more than 2^28 pixels");
    return Refusal{};
}

}  // namespace pbrs

extern "C" void pbrsm_motion_blur_params_default(uint32_t w, uint32_t h, pbrs_motion_blur_params* out) {
    if (!out) return;
    *out = pbrs_motion_blur_params{};
    out->w = w, out->h = h;
    out->max_radius = 16u, out->taps = 16u;
    out->shutter = 0.5f, out->z_rel = 0.05f;
}
