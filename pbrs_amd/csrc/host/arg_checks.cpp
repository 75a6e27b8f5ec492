// host/arg_checks.cpp — see arg_checks.h.  Every refusal returns refuse(CODE, "message") on the spot: tests/arg_checks_check.cpp counts
// these sites per function and holds one row against each.
#include "arg_checks.h"

#include "../../../include/pbrs_numeric.h"

namespace pbrs {
namespace {

Refusal refuse(int code, const char* message) { return Refusal{code, message}; }
constexpr uint64_t kMaxPixels = 1ull << 28;

}  // namespace

Refusal check_params(const SceneState& s, const pbrs_camera* cam, const pbrs_render_params* p) {
    if (!cam || !p) return refuse(PBRS_E_INVALID, "null camera or params");
    if (!s.has_scene) return refuse(PBRS_E_NO_SCENE, "no scene uploaded");
    if (p->w == 0 || p->h == 0) return refuse(PBRS_E_INVALID, "empty tile");
    if (p->band_count > 1) {
        if (p->band_rows == 0 || p->band_index >= p->band_count) return refuse(PBRS_E_INVALID, "bad row-band parameters");
        uint64_t vr = p->h - 1;
        uint64_t last = p->y0 + ((vr / p->band_rows) * p->band_count + p->band_index) * (uint64_t)p->band_rows + vr % p->band_rows;
        if (p->x0 + p->w > cam->width || last >= cam->height) return refuse(PBRS_E_INVALID, "row bands outside the film");
    } else if (p->x0 + p->w > cam->width || p->y0 + p->h > cam->height) {
        return refuse(PBRS_E_INVALID, "tile outside the film");
    }
    if (p->strata_x == 0 || p->strata_y == 0) return refuse(PBRS_E_INVALID, "zero strata");
    if (p->max_depth > kMaxDepth) return refuse(PBRS_E_LIMIT, "max_depth above 64");
    if (p->integrator > PBRS_INTEGRATOR_NORMALS) return refuse(PBRS_E_INVALID, "unknown integrator");
    if (p->integrator >= PBRS_INTEGRATOR_MATERIALS && (p->strata_x != 1 || p->strata_y != 1))
        return refuse(PBRS_E_INVALID, "a visualiser takes one un-jittered ray per pixel (strata 1 x 1)");
    if (p->integrator == PBRS_INTEGRATOR_NORMALS && !s.has_vis_records)
        return refuse(PBRS_E_INVALID, "the scene's materials carry no pbrs_material::vis_bxdf records");
    if ((uint64_t)p->w * p->h > kMaxPixels) return refuse(PBRS_E_LIMIT, "tile above 2^28 pixels");
    return Refusal{};
}

Refusal check_targets(const pbrs_render_params* p, const WantedOutputs& t) {
    // a render that traces no camera ray has no first hits to report
    const bool no_camera_ray = p->integrator <= PBRS_INTEGRATOR_DIRECT && p->max_depth == 0;
    if ((t.aovs || t.variance) && no_camera_ray)
        return refuse(PBRS_E_INVALID, "AOVs requested from a render that traces no camera ray (max_depth 0)");
    if (t.passes) {
        if (p->integrator != PBRS_INTEGRATOR_PATH)
            return refuse(PBRS_E_INVALID, "light passes need the path integrator (the direct integrator has its own depth semantics, the visualisers bypass the film)");
        if (p->max_depth == 0) return refuse(PBRS_E_INVALID, "light passes requested from a render that traces no camera ray (max_depth 0)");
    }
    if (!t.matte) return Refusal{};
    const pbrs_matte_params* mp = t.matte_params;
    if (!mp) return refuse(PBRS_E_INVALID, "a matte without pbrs_matte_params");
    if (mp->key != PBRS_MATTE_INSTANCE && mp->key != PBRS_MATTE_MATERIAL) return refuse(PBRS_E_INVALID, "unknown matte key");
    if (mp->slots == 0 || mp->slots > PBRS_MATTE_MAX_SLOTS) return refuse(PBRS_E_INVALID, "matte slots must be 1 .. 8");
    if (!t.matte_ids_and_coverage) return refuse(PBRS_E_INVALID, "a matte needs ids and coverage");
    if (no_camera_ray) return refuse(PBRS_E_INVALID, "a matte requested from a render that traces no camera ray (max_depth 0)");
    return Refusal{};
}

Refusal check_filter(const pbrs_render_params* p, const pbrs_pixel_filter* f) {
    if (p->band_count > 1) return refuse(PBRS_E_INVALID, "a filtered render takes a rectangular tile, not interleaved row bands");
    if (p->integrator >= PBRS_INTEGRATOR_MATERIALS) return refuse(PBRS_E_INVALID, "the visualisers bypass the film: no pixel filter");
    if (f->kind > PBRS_FILTER_LANCZOS) return refuse(PBRS_E_INVALID, "unknown pixel filter kind");
    for (int a = 0; a < 2; ++a)
        if (!pn_isfinite(f->radius[a]) || !(f->radius[a] > 0.0f)) return refuse(PBRS_E_INVALID, "a pixel filter radius must be finite and > 0");
    const uint32_t n_params = f->kind == PBRS_FILTER_MITCHELL ? 2u : (f->kind == PBRS_FILTER_GAUSSIAN || f->kind == PBRS_FILTER_LANCZOS) ? 1u : 0u;
    if ((n_params > 0 && !pn_isfinite(f->a)) || (n_params > 1 && !pn_isfinite(f->b)))
        return refuse(PBRS_E_INVALID, "non-finite pixel filter parameter");
    if (f->radius[0] > PBRS_FILTER_MAX_RADIUS || f->radius[1] > PBRS_FILTER_MAX_RADIUS)
        return refuse(PBRS_E_LIMIT, "pixel filter radius above 4 (the halo's LDS budget)");
    return Refusal{};
}

Refusal check_denoise(const pbrs_denoise_params* p, const float* rgb_in, const pbrs_denoise_guides* g, const float* rgb_out) {
    if (!p || !rgb_in || !rgb_out || !g) return refuse(PBRS_E_INVALID, "null denoise params, image or guides");
    if (p->w == 0 || p->h == 0) return refuse(PBRS_E_INVALID, "empty image");
    if (p->iterations == 0 || p->iterations > PBRS_DENOISE_MAX_ITERATIONS) return refuse(PBRS_E_INVALID, "denoise iterations must be 1 .. 6");
    const float sigma[3] = {p->sigma_color, p->sigma_normal, p->sigma_depth};
    for (float s : sigma)
        if (!pn_isfinite(s) || !(s > 0.0f)) return refuse(PBRS_E_INVALID, "a denoise sigma must be finite and > 0");
    if (!pn_isfinite(p->albedo_floor) || !(p->albedo_floor >= 0.0f)) return refuse(PBRS_E_INVALID, "the albedo floor must be finite and >= 0");
    if (p->flags & ~(PBRS_DENOISE_DEMODULATE | PBRS_DENOISE_ID_STOP)) return refuse(PBRS_E_INVALID, "unknown denoise flag bits");
    if ((p->flags & PBRS_DENOISE_DEMODULATE) && !g->albedo) return refuse(PBRS_E_INVALID, "PBRS_DENOISE_DEMODULATE without an albedo guide");
    if ((p->flags & PBRS_DENOISE_ID_STOP) && !g->instance) return refuse(PBRS_E_INVALID, "PBRS_DENOISE_ID_STOP without an instance guide");
    if ((uint64_t)p->w * p->h > kMaxPixels) return refuse(PBRS_E_LIMIT, "more than 2^28 pixels");
    return Refusal{};
}

pbrs_denoise_params plain_params(const pbrs_denoise_var_params& p) {
    return {p.w, p.h, p.iterations, p.flags, p.sigma_luminance, p.sigma_normal, p.sigma_depth, p.albedo_floor};
}

Refusal check_denoise_var(const pbrs_denoise_var_params* p, const float* rgb_in, const pbrs_denoise_var_guides* g, const float* rgb_out) {
    if (!p || !rgb_in || !rgb_out || !g) return refuse(PBRS_E_INVALID, "null denoise params, image or guides");
    if (!g->variance) return refuse(PBRS_E_INVALID, "the variance-guided denoiser needs guides.variance");
    // the rest is the plain denoiser's list
    const pbrs_denoise_params q = plain_params(*p);
    const pbrs_denoise_guides gq{g->albedo, g->normal, g->depth, g->instance};
    return check_denoise(&q, rgb_in, &gq, rgb_out);
}

Refusal check_matte_mask(uint32_t w, uint32_t h, uint32_t slots, const uint32_t* ids, const float* coverage, const uint32_t* select, uint32_t n_select,
                         const float* mask_out) {
    if (!ids || !coverage || !mask_out) return refuse(PBRS_E_INVALID, "null matte layers or mask");
    if (w == 0 || h == 0) return refuse(PBRS_E_INVALID, "empty image");
    if (slots == 0 || slots > PBRS_MATTE_MAX_SLOTS) return refuse(PBRS_E_INVALID, "matte slots must be 1 .. 8");
    if (n_select > PBRS_MATTE_MAX_SELECT) return refuse(PBRS_E_INVALID, "more than PBRS_MATTE_MAX_SELECT selected ids");
    if (n_select && !select) return refuse(PBRS_E_INVALID, "null selection");
    for (uint32_t i = 1; i < n_select; ++i)
        if (select[i - 1] >= select[i]) return refuse(PBRS_E_INVALID, "the selected ids must be strictly ascending");
    if ((uint64_t)w * h > kMaxPixels) return refuse(PBRS_E_LIMIT, "more than 2^28 pixels");
    return Refusal{};
}

Refusal check_combine(uint32_t w, uint32_t h, const float* direct, const float* indirect, const float* rgb_out) {
    if (!direct || !indirect || !rgb_out) return refuse(PBRS_E_INVALID, "null light passes or output");
    if (w == 0 || h == 0) return refuse(PBRS_E_INVALID, "empty image");
    if ((uint64_t)w * h > kMaxPixels) return refuse(PBRS_E_LIMIT, "more than 2^28 pixels");
    return Refusal{};
}

Refusal check_motion_table(const pbrs_instance_motion* motion, uint32_t n_motion, const uint32_t* instance) {
    if (!motion && n_motion) return refuse(PBRS_E_INVALID, "n_motion without a motion table");
    if (!motion) return Refusal{};
    if (n_motion == 0) return refuse(PBRS_E_INVALID, "a motion table of 0 records");
    if (!instance) return refuse(PBRS_E_INVALID, "a motion table without this frame's instance ids");
    if (n_motion > (1u << 24)) return refuse(PBRS_E_LIMIT, "more than 2^24 motion records");
    return Refusal{};
}

Refusal check_temporal(const pbrs_temporal_params* p, const pbrs_camera* cam, const pbrs_camera* cam_prev, const pbrs_temporal_frame* f,
                       const pbrs_temporal_guides* prev, const pbrs_temporal_history* hin, const pbrs_temporal_history* hout) {
    if (!p || !cam || !f || !hout) return refuse(PBRS_E_INVALID, "null temporal params, camera, frame or history_out");
    if (!f->rgb || !f->depth) return refuse(PBRS_E_INVALID, "the temporal frame needs rgb and depth");
    if (!hout->rgb || !hout->moments || !hout->length) return refuse(PBRS_E_INVALID, "history_out with a null plane");
    if (p->w == 0 || p->h == 0) return refuse(PBRS_E_INVALID, "empty image");
    if (p->flags & ~PBRS_TEMPORAL_ID_TEST) return refuse(PBRS_E_INVALID, "unknown temporal flag bits");
    if ((p->flags & PBRS_TEMPORAL_ID_TEST) && !f->instance) return refuse(PBRS_E_INVALID, "PBRS_TEMPORAL_ID_TEST without instance ids");
    if (!pn_isfinite(p->max_history) || !(p->max_history >= 1.0f)) return refuse(PBRS_E_INVALID, "max_history must be finite and >= 1");
    const float tol[2] = {p->depth_tolerance, p->normal_tolerance};
    for (float t : tol)
        if (!pn_isfinite(t) || !(t > 0.0f)) return refuse(PBRS_E_INVALID, "a temporal tolerance must be finite and > 0");
    if (!pn_isfinite(p->min_temporal) || !(p->min_temporal >= 2.0f)) return refuse(PBRS_E_INVALID, "min_temporal must be finite and >= 2");
    if (cam->width != p->w || cam->height != p->h) return refuse(PBRS_E_INVALID, "the camera's size is not w x h");
    if (hin) {
        if (!hin->rgb || !hin->moments || !hin->length) return refuse(PBRS_E_INVALID, "history_in with a null plane");
        if (!cam_prev || !prev || !prev->depth) return refuse(PBRS_E_INVALID, "history_in without the previous camera or the previous depth");
        if (cam_prev->width != p->w || cam_prev->height != p->h) return refuse(PBRS_E_INVALID, "the previous camera's size is not w x h");
        if (!f->normal != !prev->normal || !f->instance != !prev->instance)
            return refuse(PBRS_E_INVALID, "a normal or an instance guide given for only one of the two frames");
        if (hin->rgb == hout->rgb || hin->moments == hout->moments || hin->length == hout->length)
            return refuse(PBRS_E_INVALID, "temporal accumulation cannot run in place: history_out shares a plane with history_in");
    }
    if ((uint64_t)p->w * p->h > kMaxPixels) return refuse(PBRS_E_LIMIT, "more than 2^28 pixels");
    return Refusal{};
}

Refusal check_temporal_motion(const pbrs_temporal_params* p, const pbrs_camera* cam, const pbrs_camera* cam_prev, const pbrs_temporal_frame* f,
                              const pbrs_temporal_guides* prev, const pbrs_temporal_history* hin, const pbrs_temporal_history* hout,
                              const pbrs_instance_motion* motion, uint32_t n_motion) {
    const Refusal r = check_temporal(p, cam, cam_prev, f, prev, hin, hout);
    return r.code ? r : check_motion_table(motion, n_motion, f->instance);
}

Refusal check_motion_vectors(uint32_t w, uint32_t h, const pbrs_camera* cam, const pbrs_camera* cam_prev, const float* depth, const uint32_t* instance,
                             const pbrs_instance_motion* motion, uint32_t n_motion, const float* motion_out) {
    if (!cam || !cam_prev || !depth || !motion_out) return refuse(PBRS_E_INVALID, "null cameras, depth or motion_out");
    if (w == 0 || h == 0) return refuse(PBRS_E_INVALID, "empty image");
    if (cam->width != w || cam->height != h || cam_prev->width != w || cam_prev->height != h)
        return refuse(PBRS_E_INVALID, "a camera's size is not w x h");
    const Refusal r = check_motion_table(motion, n_motion, instance);
    if (r.code) return r;
    if ((uint64_t)w * h > kMaxPixels) return refuse(PBRS_E_LIMIT, "more than 2^28 pixels");
    return Refusal{};
}

Refusal check_spatial_variance(const pbrs_spatial_variance_params* p, const float* moments, const float* length, const pbrs_spatial_variance_guides* g,
                               const float* variance_in, const float* variance_out) {
    if (!p || !moments || !length || !variance_in || !variance_out)
        return refuse(PBRS_E_INVALID, "null spatial variance params, moments, length, variance_in or variance_out");
    if (p->w == 0 || p->h == 0) return refuse(PBRS_E_INVALID, "empty image");
    if (p->radius == 0 || p->radius > PBRS_SPATIAL_MAX_RADIUS) return refuse(PBRS_E_INVALID, "the spatial variance radius must be 1 .. 3");
    if (p->flags & ~(PBRS_SPATIAL_ID_STOP | PBRS_SPATIAL_ONLY_UNKNOWN)) return refuse(PBRS_E_INVALID, "unknown spatial variance flag bits");
    if ((p->flags & PBRS_SPATIAL_ID_STOP) && !(g && g->instance)) return refuse(PBRS_E_INVALID, "PBRS_SPATIAL_ID_STOP without instance ids");
    const float sig[2] = {p->sigma_normal, p->sigma_depth};
    for (float s : sig)
        if (!pn_isfinite(s) || !(s > 0.0f)) return refuse(PBRS_E_INVALID, "a spatial variance sigma must be finite and > 0");
    if (!pn_isfinite(p->min_temporal) || !(p->min_temporal >= 1.0f)) return refuse(PBRS_E_INVALID, "min_temporal must be finite and >= 1");
    if (variance_out == moments || variance_out == length)
        return refuse(PBRS_E_INVALID, "the spatial variance estimate cannot write over the moments or the length");
    if ((uint64_t)p->w * p->h > kMaxPixels) return refuse(PBRS_E_LIMIT, "more than 2^28 pixels");
    return Refusal{};
}

}  // namespace pbrs
