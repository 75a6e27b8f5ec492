// host/arg_checks_bloom.cpp — check_bloom of arg_checks.h and the filler pbrsb_bloom_params_default (include/pbrs_gpu.h, "bloom"), in
// a file of their own like arg_checks_despeckle.cpp: tests/bloom_check.cpp holds one row against every refusal site of this file and
// pins their number.  Every refusal returns refuse(CODE, "message") on the spot.
#include "arg_checks.h"

#include "../../../include/pbrs_numeric.h"

namespace pbrs {
namespace {

Refusal refuse(int code, const char* message) { return Refusal{code, message}; }
constexpr uint64_t kMaxPixels = 1ull << 28;

}  // namespace

Refusal check_bloom(const pbrs_bloom_params* p, const float* rgb, const float* rgb_out) {
    if (!p || !rgb || !rgb_out) return refuse(PBRS_E_INVALID, "null bloom params, rgb or rgb_out");
    if (p->w == 0 || p->h == 0) return refuse(PBRS_E_INVALID, "empty image");
    if (p->levels < 1u || p->levels > PBRS_BLOOM_MAX_LEVELS) return refuse(PBRS_E_INVALID, "the bloom levels must be 1 .. 8");
    if (p->flags & ~PBRS_BLOOM_MIX) return refuse(PBRS_E_INVALID, "unknown bloom flag bits");
    if (!pn_isfinite(p->threshold) || !(p->threshold >= 0.0f)) return refuse(PBRS_E_INVALID, "the bloom threshold must be finite and >= 0");
    if (!pn_isfinite(p->knee) || !(p->knee >= 0.0f && p->knee <= 1.0f)) return refuse(PBRS_E_INVALID, "the bloom knee must be in [0, 1]");
    if (!pn_isfinite(p->strength) || !(p->strength >= 0.0f)) return refuse(PBRS_E_INVALID, "the bloom strength must be finite and >= 0");
    if (!pn_isfinite(p->spread) || !(p->spread >= 0.0f && p->spread <= 1.0f)) return refuse(PBRS_E_INVALID, "the bloom spread must be in [0, 1]");
    if ((p->flags & PBRS_BLOOM_MIX) && p->strength > 1.0f) return refuse(PBRS_E_INVALID, "PBRS_BLOOM_MIX takes a strength <= 1");
    if ((uint64_t)p->w * p->h > kMaxPixels) return refuse(PBRS_E_LIMIT, "more than 2^28 pixels");
    return Refusal{};
}

}  // namespace pbrs

extern "C" void pbrsb_bloom_params_default(uint32_t w, uint32_t h, pbrs_bloom_params* out) {
    if (!out) return;
    *out = pbrs_bloom_params{};
    out->w = w, out->h = h;
    out->levels = 6u;
    out->threshold = 1.0f, out->knee = 0.5f;
    out->strength = 0.05f, out->spread = 0.6f;
}
