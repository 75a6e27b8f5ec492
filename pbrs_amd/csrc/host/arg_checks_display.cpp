// host/arg_checks_display.cpp — check_display of arg_checks.h and the filler pbrs_display_params_default (include/pbrs_gpu.h, "display
// transform"), in a file of their own like arg_checks_clip.cpp: tests/display_check.cpp holds one row against every refusal site of this
// file and pins their number.  Every refusal returns refuse(CODE, "message") on the spot.
#include "arg_checks.h"

#include "../../../include/pbrs_numeric.h"

namespace pbrs {
namespace {

Refusal refuse(int code, const char* message) { return Refusal{code, message}; }
constexpr uint64_t kMaxPixels = 1ull << 28;
bool positive_finite(float x) { return pn_isfinite(x) && x > 0.0f; }

}  // namespace

Refusal check_display(const pbrs_display_params* p, const float* rgb, const pbrs_display_io* io, const uint32_t* rgba8_out) {
    (void)io;  // NULL or any of its pointers NULL: all allowed
    if (!p || !rgb || !rgba8_out) return refuse(PBRS_E_INVALID, "null display params, image or output");
    if (p->w == 0 || p->h == 0) return refuse(PBRS_E_INVALID, "empty image");
    if (p->curve > PBRS_CURVE_ACES) return refuse(PBRS_E_INVALID, "unknown display curve");
    if (p->encode > PBRS_ENCODE_SRGB) return refuse(PBRS_E_INVALID, "unknown display encode");
    if (p->quantize > PBRS_QUANT_DITHER) return refuse(PBRS_E_INVALID, "unknown display quantize");
    if (p->flags & ~PBRS_DISPLAY_AUTO_EXPOSURE) return refuse(PBRS_E_INVALID, "unknown display flag bits");
    if (!positive_finite(p->exposure)) return refuse(PBRS_E_INVALID, "the display exposure must be finite and > 0");
    if (!(p->white > 0.0f)) return refuse(PBRS_E_INVALID, "the display white must be > 0 (+inf: plain Reinhard)");
    if (p->flags & PBRS_DISPLAY_AUTO_EXPOSURE) {
        if (!positive_finite(p->key)) return refuse(PBRS_E_INVALID, "the display key must be finite and > 0");
        if (!positive_finite(p->min_exposure) || !positive_finite(p->max_exposure) || p->min_exposure > p->max_exposure)
            return refuse(PBRS_E_INVALID, "the display exposure limits must be finite with 0 < min <= max");
        if (!(p->adapt > 0.0f && p->adapt <= 1.0f)) return refuse(PBRS_E_INVALID, "the display adapt must be in (0, 1]");
        if (p->low_q16 >= p->high_q16 || p->high_q16 > 65536u) return refuse(PBRS_E_INVALID, "the display ranks need low_q16 < high_q16 <= 65536");
    }
    if (static_cast<const void*>(rgba8_out) == static_cast<const void*>(rgb)) return refuse(PBRS_E_INVALID, "the display output cannot be the image's plane");
    if ((uint64_t)p->w * p->h > kMaxPixels) return refuse(PBRS_E_LIMIT, "more than 2^28 pixels");
    return Refusal{};
}

}  // namespace pbrs

extern "C" void pbrs_display_params_default(uint32_t w, uint32_t h, pbrs_display_params* out) {
    if (!out) return;
    *out = pbrs_display_params{};
    out->w = w, out->h = h;
    out->curve = PBRS_CURVE_ACES, out->encode = PBRS_ENCODE_SRGB, out->quantize = PBRS_QUANT_ROUND;
    out->exposure = 1.0f, out->key = 0.18f, out->white = pn_inf();
    out->min_exposure = 9.5367431640625e-7f, out->max_exposure = 1048576.0f;  // 2^-20, 2^20
    out->adapt = 1.0f;
    out->low_q16 = 6554u, out->high_q16 = 62259u;  // 10 % and 95 %
}
