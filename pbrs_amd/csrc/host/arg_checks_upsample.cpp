// host/arg_checks_upsample.cpp — check_upsample of arg_checks.h and the filler pbrs_upsample_params_default (include/pbrs_gpu.h, "guided
// upsampling"), in a file of their own like arg_checks_display.cpp: tests/upsample_check.cpp holds one row against every refusal site of
// this file and pins their number.  Every refusal returns refuse(CODE, "message") on the spot.
#include "arg_checks.h"

#include "../../../include/pbrs_numeric.h"

namespace pbrs {
namespace {

Refusal refuse(int code, const char* message) { return Refusal{code, message}; }
constexpr uint64_t kMaxPixels = 1ull << 28;
bool positive_finite(float x) { return pn_isfinite(x) && x > 0.0f; }
bool nonnegative_finite(float x) { return pn_isfinite(x) && x >= 0.0f; }

// `plane` (not null) is rgb_lo or one of the eight guide planes.
bool is_an_input(const void* plane, const float* rgb_lo, const pbrs_denoise_guides* lo, const pbrs_denoise_guides* hi) {
    const void* in[] = {rgb_lo, lo->albedo, lo->normal, lo->depth, lo->instance, hi->albedo, hi->normal, hi->depth, hi->instance};
    for (const void* q : in)
        if (q == plane) return true;
    return false;
}

}  // namespace

Refusal check_upsample(const pbrs_upsample_params* p, const float* rgb_lo, const pbrs_denoise_guides* lo, const pbrs_denoise_guides* hi,
                       const float* out, const float* weight_out) {
    if (!p || !rgb_lo || !lo || !hi || !out) return refuse(PBRS_E_INVALID, "null upsample params, image, guides or output");
    if (p->w == 0 || p->h == 0) return refuse(PBRS_E_INVALID, "empty image");
    if (p->factor < PBRS_UPSAMPLE_MIN_FACTOR || p->factor > PBRS_UPSAMPLE_MAX_FACTOR) return refuse(PBRS_E_INVALID, "the upsample factor must be 2 .. 4");
    if (p->radius == 0 || p->radius > PBRS_UPSAMPLE_MAX_RADIUS) return refuse(PBRS_E_INVALID, "the upsample radius must be 1 .. 2");
    if (!positive_finite(p->sigma_normal) || !positive_finite(p->sigma_depth)) return refuse(PBRS_E_INVALID, "an upsample sigma must be finite and > 0");
    if (!nonnegative_finite(p->albedo_floor)) return refuse(PBRS_E_INVALID, "the albedo floor must be finite and >= 0");
    if (!nonnegative_finite(p->min_weight)) return refuse(PBRS_E_INVALID, "the upsample min_weight must be finite and >= 0");
    if (p->flags & ~(PBRS_UPSAMPLE_DEMODULATE | PBRS_UPSAMPLE_ID_STOP)) return refuse(PBRS_E_INVALID, "unknown upsample flag bits");
    if (!lo->albedo != !hi->albedo || !lo->normal != !hi->normal || !lo->depth != !hi->depth || !lo->instance != !hi->instance)
        return refuse(PBRS_E_INVALID, "a guide given at only one of the two resolutions");
    if ((p->flags & PBRS_UPSAMPLE_DEMODULATE) && !lo->albedo) return refuse(PBRS_E_INVALID, "PBRS_UPSAMPLE_DEMODULATE without the albedo guides");
    if ((p->flags & PBRS_UPSAMPLE_ID_STOP) && !lo->instance) return refuse(PBRS_E_INVALID, "PBRS_UPSAMPLE_ID_STOP without the instance guides");
    if (is_an_input(out, rgb_lo, lo, hi)) return refuse(PBRS_E_INVALID, "the upsampled image cannot be written over an input plane");
    if (weight_out && (weight_out == out || is_an_input(weight_out, rgb_lo, lo, hi)))
        return refuse(PBRS_E_INVALID, "weight_out cannot be the output's or an input's plane");
    if ((uint64_t)p->w * p->h > kMaxPixels) return refuse(PBRS_E_LIMIT, "more than 2^28 pixels");
    return Refusal{};
}

}  // namespace pbrs

extern "C" void pbrs_upsample_params_default(uint32_t w, uint32_t h, uint32_t factor, pbrs_upsample_params* out) {
    if (!out) return;
    *out = pbrs_upsample_params{};
    out->w = w, out->h = h, out->factor = factor;
    out->radius = 1u;
    out->sigma_normal = 0.3f, out->sigma_depth = 0.2f, out->albedo_floor = 1e-3f;
    out->min_weight = 1e-3f;
}
