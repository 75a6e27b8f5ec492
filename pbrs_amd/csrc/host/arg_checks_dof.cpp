// host/arg_checks_dof.cpp — check_dof of arg_checks.h and the filler pbrsf_dof_params_default (include/pbrs_gpu.h, "depth of field"),
// in a file of their own like arg_checks_bloom.cpp: tests/dof_check.cpp holds one row against every refusal site of this file and pins
// their number.  Every refusal returns refuse(CODE, "message") on the spot, in the order the header states.
#include "arg_checks.h"

#include "../../../include/pbrs_numeric.h"

namespace pbrs {
namespace {

Refusal refuse(int code, const char* message) { return Refusal{code, message}; }
constexpr uint64_t kMaxPixels = 1ull << 28;

}  // namespace

Refusal check_dof(const pbrs_dof_params* p, const float* rgb, const float* depth, const float* rgb_out) {
    if (!p || !rgb || !depth || !rgb_out) return refuse(PBRS_E_INVALID, "null dof params, rgb, depth or rgb_out");
    if (rgb_out == rgb) return refuse(PBRS_E_INVALID, "the dof output must not be its input: a gather reads its neighbours");
    if (p->w == 0 || p->h == 0) return refuse(PBRS_E_INVALID, "empty image");
    if (p->max_radius < 1u || p->max_radius > PBRS_DOF_MAX_RADIUS) return refuse(PBRS_E_INVALID, "the dof max_radius must be 1 .. 16");
    if (p->flags != 0u) return refuse(PBRS_E_INVALID, "unknown dof flag bits");
    if (p->reserved[0] != 0u || p->reserved[1] != 0u) return refuse(PBRS_E_INVALID, "the dof reserved words must be 0");
    if (!pn_isfinite(p->focus) || !(p->focus > 0.0f)) return refuse(PBRS_E_INVALID, "the dof focus must be finite and > 0");
    if (!pn_isfinite(p->scale) || !(p->scale >= 0.0f)) return refuse(PBRS_E_INVALID, "the dof scale must be finite and >= 0");
    if ((uint64_t)p->w * p->h > kMaxPixels) return refuse(PBRS_E_LIMIT, "more than 2^28 pixels");
    return Refusal{};
}

}  // namespace pbrs

extern "C" void pbrsf_dof_params_default(uint32_t w, uint32_t h, pbrs_dof_params* out) {
    if (!out) return;
    *out = pbrs_dof_params{};
    out->w = w, out->h = h;
    out->max_radius = 8u;
    out->focus = 1.0f, out->scale = 0.0f;
}
