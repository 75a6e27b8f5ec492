// host/arg_checks.h — the argument checks of the C ABI's render and image-space entry points (include/pbrs_gpu.h): plain C++, no HIP
// header and no pbrs_ctx, so that tests/arg_checks_check.cpp runs every refusal on a CPU under AddressSanitizer.
//
// A check reads its arguments and nothing else: it dereferences the parameter structs and the selection of check_matte_mask, never an
// image plane.  It returns the first refusal in the order of its source lines, or `{PBRS_OK, nullptr}`.  pbrs_gpu.hip turns a refusal
// into the entry point's return code and pbrs_last_error (`fail`) before it touches the device.
#pragma once
#include <cstdint>

#include "../../../include/pbrs_gpu.h"

namespace pbrs {

struct Refusal {
    int code = PBRS_OK;             // PBRS_OK, or the code the entry point returns
    const char* message = nullptr;  // ... and its pbrs_last_error
};

constexpr uint32_t kMaxDepth = 64;  // bounces a render may ask for (check_params); sizes the per-bounce counters of pbrs_gpu.hip

// ---- renders ----
// What check_params needs to know of the context.
struct SceneState {
    bool has_scene = false;
    bool has_vis_records = false;  // every material names its pbrs_material::vis_bxdf record (normal_visualizer)
};
Refusal check_params(const SceneState& s, const pbrs_camera* cam, const pbrs_render_params* p);

// What a render is to produce beside the image, as far as check_targets cares.
struct WantedOutputs {
    bool aovs = false, variance = false, passes = false;
    bool matte = false;                               // a matte, with:
    const pbrs_matte_params* matte_params = nullptr;  // ... its parameters (required)
    bool matte_ids_and_coverage = false;              // ... both required buffers are given
};
// `p` has passed check_params.
Refusal check_targets(const pbrs_render_params* p, const WantedOutputs& t);
// A filtered render of the tile `p` (which has passed check_params) through `f` (not null).  The traced region, the tile plus its
// halo, is the caller's to compute and to pass through check_params again.
Refusal check_filter(const pbrs_render_params* p, const pbrs_pixel_filter* f);

// ---- image operations ----
Refusal check_denoise(const pbrs_denoise_params* p, const float* rgb_in, const pbrs_denoise_guides* g, const float* rgb_out);
// The variance-guided denoiser's parameters as the plain one's: sigma_luminance in the place of sigma_color (one layout).
pbrs_denoise_params plain_params(const pbrs_denoise_var_params& p);
Refusal check_denoise_var(const pbrs_denoise_var_params* p, const float* rgb_in, const pbrs_denoise_var_guides* g, const float* rgb_out);
Refusal check_matte_mask(uint32_t w, uint32_t h, uint32_t slots, const uint32_t* ids, const float* coverage, const uint32_t* select, uint32_t n_select,
                         const float* mask_out);
Refusal check_combine(uint32_t w, uint32_t h, const float* direct, const float* indirect, const float* rgb_out);
// `instance`: this frame's instance ids, which a motion table is indexed by.
Refusal check_motion_table(const pbrs_instance_motion* motion, uint32_t n_motion, const uint32_t* instance);
Refusal check_temporal(const pbrs_temporal_params* p, const pbrs_camera* cam, const pbrs_camera* cam_prev, const pbrs_temporal_frame* f,
                       const pbrs_temporal_guides* prev, const pbrs_temporal_history* hin, const pbrs_temporal_history* hout);
// check_temporal, then check_motion_table with the frame's instance ids: pbrs_temporal_accumulate_motion*.
Refusal check_temporal_motion(const pbrs_temporal_params* p, const pbrs_camera* cam, const pbrs_camera* cam_prev, const pbrs_temporal_frame* f,
                              const pbrs_temporal_guides* prev, const pbrs_temporal_history* hin, const pbrs_temporal_history* hout,
                              const pbrs_instance_motion* motion, uint32_t n_motion);
// check_temporal_motion, then the clip's own list (host/arg_checks_clip.cpp); clip == NULL is check_temporal_motion:
// pbrs_temporal_accumulate_clip*.
Refusal check_temporal_clip(const pbrs_temporal_params* p, const pbrs_camera* cam, const pbrs_camera* cam_prev, const pbrs_temporal_frame* f,
                            const pbrs_temporal_guides* prev, const pbrs_temporal_history* hin, const pbrs_temporal_history* hout,
                            const pbrs_instance_motion* motion, uint32_t n_motion, const pbrs_history_clip_params* clip);
Refusal check_motion_vectors(uint32_t w, uint32_t h, const pbrs_camera* cam, const pbrs_camera* cam_prev, const float* depth, const uint32_t* instance,
                             const pbrs_instance_motion* motion, uint32_t n_motion, const float* motion_out);
Refusal check_spatial_variance(const pbrs_spatial_variance_params* p, const float* moments, const float* length, const pbrs_spatial_variance_guides* g,
                               const float* variance_in, const float* variance_out);
// pbrs_display* (host/arg_checks_display.cpp, beside the filler pbrs_display_params_default).  `io` and its pointers may be NULL; the
// fields only the auto exposure reads are checked only with PBRS_DISPLAY_AUTO_EXPOSURE.
Refusal check_display(const pbrs_display_params* p, const float* rgb, const pbrs_display_io* io, const uint32_t* rgba8_out);
// pbrs_upsample* (host/arg_checks_upsample.cpp, beside the filler pbrs_upsample_params_default).  `weight_out` may be NULL; a guide of
// `lo` and `hi` counts when both give it.
Refusal check_upsample(const pbrs_upsample_params* p, const float* rgb_lo, const pbrs_denoise_guides* lo, const pbrs_denoise_guides* hi,
                       const float* out, const float* weight_out);
// pbrsx_compare* (host/arg_checks_compare.cpp, beside the filler pbrsx_compare_params_default).  `maps` and its pointers may be NULL;
// `a` may be `b`.
Refusal check_compare(const pbrs_compare_params* p, const float* a, const float* b, const pbrs_compare_maps* maps, const pbrs_compare_result* result);
// pbrsi_despeckle* (host/arg_checks_despeckle.cpp, beside the filler pbrsi_despeckle_params_default).  The optional planes of `io`
// may be NULL; the result, which may be NULL too, is not a plane and is not looked at.
Refusal check_despeckle(const pbrs_despeckle_params* p, const pbrs_despeckle_io* io);
// pbrsb_bloom* (host/arg_checks_bloom.cpp, beside the filler pbrsb_bloom_params_default).  `rgb_out` may be `rgb`.
Refusal check_bloom(const pbrs_bloom_params* p, const float* rgb, const float* rgb_out);
// pbrsf_dof* (host/arg_checks_dof.cpp, beside the filler pbrsf_dof_params_default).  `rgb_out` must not be `rgb`; coc_out, which may
// be NULL, is not looked at.
Refusal check_dof(const pbrs_dof_params* p, const float* rgb, const float* depth, const float* rgb_out);
// pbrsm_motion_blur* (host/arg_checks_motion_blur.cpp, beside the filler pbrsm_motion_blur_params_default).  `rgb_out` must not be
// `rgb`; velocity_out, which may be NULL, is not looked at.
Refusal check_motion_blur(const pbrs_motion_blur_params* p, const float* rgb, const float* depth, const float* motion, const float* rgb_out);

}  // namespace pbrs
