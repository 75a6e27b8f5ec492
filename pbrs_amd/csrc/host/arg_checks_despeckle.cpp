// host/arg_checks_despeckle.cpp — check_despeckle of arg_checks.h and the filler pbrsi_despeckle_params_default (include/pbrs_gpu.h,
// "despeckle"), in a file of their own like arg_checks_compare.cpp: tests/despeckle_check.cpp holds one row against every refusal site
// of this file and pins their number.  Every refusal returns refuse(CODE, "message") on the spot.
#include "arg_checks.h"

#include "../../../include/pbrs_numeric.h"

namespace pbrs {
namespace {

Refusal refuse(int code, const char* message) { return Refusal{code, message}; }
constexpr uint64_t kMaxPixels = 1ull << 28;

}  // namespace

Refusal check_despeckle(const pbrs_despeckle_params* p, const pbrs_despeckle_io* io) {
    if (!p || !io || !io->rgb_in || !io->rgb_out) return refuse(PBRS_E_INVALID, "null despeckle params, io, rgb_in or rgb_out");
    if (p->w == 0 || p->h == 0) return refuse(PBRS_E_INVALID, "empty image");
    if (p->radius < 1u || p->radius > PBRS_DESPECKLE_MAX_RADIUS) return refuse(PBRS_E_INVALID, "the despeckle radius must be 1 or 2");
    if (p->rank < 1u || p->rank > PBRS_DESPECKLE_MAX_RANK) return refuse(PBRS_E_INVALID, "the despeckle rank must be 1 .. 4");
    if (!pn_isfinite(p->gain) || !(p->gain >= 1.0f)) return refuse(PBRS_E_INVALID, "the despeckle gain must be finite and >= 1");
    if (!pn_isfinite(p->floor) || !(p->floor >= 0.0f)) return refuse(PBRS_E_INVALID, "the despeckle floor must be finite and >= 0");
    if (p->flags) return refuse(PBRS_E_INVALID, "unknown despeckle flag bits");
    if ((io->variance_in == nullptr) != (io->variance_out == nullptr)) return refuse(PBRS_E_INVALID, "the despeckle variance planes come as a pair");
    if (io->rgb_out == io->rgb_in) return refuse(PBRS_E_INVALID, "despeckle reads neighbours: rgb_out cannot be rgb_in");
    // every output plane against every other plane of the call; variance_out == variance_in is the one pair that may meet
    const void* const in[] = {io->rgb_in, io->variance_in};
    const void* const out[] = {io->rgb_out, io->variance_out, io->mask_out, io->removed_out};
    for (int i = 0; i < 4; ++i) {
        if (!out[i]) continue;
        for (int j = 0; j < 2; ++j)
            if (out[i] == in[j] && !(i == 1 && j == 1)) return refuse(PBRS_E_INVALID, "a despeckle output plane cannot be an input plane");
        for (int j = i + 1; j < 4; ++j)
            if (out[i] == out[j]) return refuse(PBRS_E_INVALID, "the despeckle output planes cannot share a plane");
    }
    if ((uint64_t)p->w * p->h > kMaxPixels) return refuse(PBRS_E_LIMIT, "more than 2^28 pixels");
    return Refusal{};
}

}  // namespace pbrs

extern "C" void pbrsi_despeckle_params_default(uint32_t w, uint32_t h, pbrs_despeckle_params* out) {
    if (!out) return;
    *out = pbrs_despeckle_params{};
    out->w = w, out->h = h;
    out->radius = 1u, out->rank = 2u;
    out->gain = 2.0f, out->floor = 0.0f;
}
