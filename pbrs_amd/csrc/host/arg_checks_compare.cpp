// host/arg_checks_compare.cpp — check_compare of arg_checks.h and the filler pbrsx_compare_params_default (include/pbrs_gpu.h, "image
// comparison"), in a file of their own like arg_checks_display.cpp: tests/compare_check.cpp holds one row against every refusal site of
// this file and pins their number.  Every refusal returns refuse(CODE, "message") on the spot.
#include "arg_checks.h"

#include "../../../include/pbrs_numeric.h"

namespace pbrs {
namespace {

Refusal refuse(int code, const char* message) { return Refusal{code, message}; }
constexpr uint64_t kMaxPixels = 1ull << 28;
bool positive_finite(float x) { return pn_isfinite(x) && x > 0.0f; }

}  // namespace

Refusal check_compare(const pbrs_compare_params* p, const float* a, const float* b, const pbrs_compare_maps* maps, const pbrs_compare_result* result) {
    if (!p || !a || !b || !result) return refuse(PBRS_E_INVALID, "null compare params, image, reference or result");
    if (p->w == 0 || p->h == 0) return refuse(PBRS_E_INVALID, "empty image");
    if (p->transform > PBRS_COMPARE_REINHARD) return refuse(PBRS_E_INVALID, "unknown compare transform");
    if (p->flags & ~PBRS_COMPARE_SSIM) return refuse(PBRS_E_INVALID, "unknown compare flag bits");
    if (!positive_finite(p->rel_epsilon)) return refuse(PBRS_E_INVALID, "the compare rel_epsilon must be finite and > 0");
    if (!positive_finite(p->peak)) return refuse(PBRS_E_INVALID, "the compare peak must be finite and > 0");
    if (maps) {  // NULL, or any of its pointers NULL: not wanted
        const float *e = maps->error_out, *s = maps->ssim_out;
        if (s && !(p->flags & PBRS_COMPARE_SSIM)) return refuse(PBRS_E_INVALID, "the compare ssim map needs PBRS_COMPARE_SSIM");
        if (e && (e == a || e == b)) return refuse(PBRS_E_INVALID, "the compare error map cannot be an image's plane");
        if (s && (s == a || s == b)) return refuse(PBRS_E_INVALID, "the compare ssim map cannot be an image's plane");
        if (e && e == s) return refuse(PBRS_E_INVALID, "the compare maps cannot share a plane");
    }
    if ((uint64_t)p->w * p->h > kMaxPixels) return refuse(PBRS_E_LIMIT, "more than 2^28 pixels");
    return Refusal{};
}

}  // namespace pbrs

extern "C" void pbrsx_compare_params_default(uint32_t w, uint32_t h, pbrs_compare_params* out) {
    if (!out) return;
    *out = pbrs_compare_params{};
    out->w = w, out->h = h;
    out->transform = PBRS_COMPARE_REINHARD, out->flags = PBRS_COMPARE_SSIM;
    out->rel_epsilon = 1e-2f, out->peak = 1.0f;
}
