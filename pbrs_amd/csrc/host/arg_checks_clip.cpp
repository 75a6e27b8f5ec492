// host/arg_checks_clip.cpp — check_temporal_clip of arg_checks.h, in a file of its own: tests/arg_checks_check.cpp holds one row against
// every refusal site of arg_checks.cpp and pins their number, and tests/history_clip_check.cpp does the same for this file.  Every
// refusal returns refuse(CODE, "message") on the spot.
#include "arg_checks.h"

#include "../../../include/pbrs_numeric.h"

namespace pbrs {
namespace {

Refusal refuse(int code, const char* message) { return Refusal{code, message}; }

}  // namespace

Refusal check_temporal_clip(const pbrs_temporal_params* p, const pbrs_camera* cam, const pbrs_camera* cam_prev, const pbrs_temporal_frame* f,
                            const pbrs_temporal_guides* prev, const pbrs_temporal_history* hin, const pbrs_temporal_history* hout,
                            const pbrs_instance_motion* motion, uint32_t n_motion, const pbrs_history_clip_params* clip) {
    const Refusal r = check_temporal_motion(p, cam, cam_prev, f, prev, hin, hout, motion, n_motion);
    if (r.code || !clip) return r;
    if (clip->radius == 0 || clip->radius > PBRS_CLIP_MAX_RADIUS) return refuse(PBRS_E_INVALID, "the history clip radius must be 1 .. 3");
    if (!pn_isfinite(clip->gamma) || !(clip->gamma > 0.0f)) return refuse(PBRS_E_INVALID, "the history clip gamma must be finite and > 0");
    if (!(clip->clip_history >= 1.0f)) return refuse(PBRS_E_INVALID, "clip_history must be >= 1 (+inf: never shortened)");
    if (clip->flags) return refuse(PBRS_E_INVALID, "unknown history clip flag bits");
    if (hout->rgb == f->rgb) return refuse(PBRS_E_INVALID, "history clipping gathers a halo of frame.rgb: history_out.rgb cannot be that plane");
    return Refusal{};
}

}  // namespace pbrs
