// tests/arg_checks_check.cpp — the argument checks of the render and image-space entry points (pbrs_amd/csrc/host/arg_checks.h) on a
// CPU: a program of its own that tests/test_arg_checks.py compiles with -fsanitize=address,undefined and runs.
//
//   usage: arg_checks_check <path of host/arg_checks.cpp>
//
// Every check starts from a valid baseline; image planes are addresses that are never dereferenced, the one array a check does read (the
// selection of check_matte_mask) is a heap block of exactly its size.  Checked:
//   refusals     one row per `return refuse(` site of the source: the baseline with one defect, the code and the message.  The rows are
//                compared with the sites function by function: a site without a row, or a row without a site, fails
//   baselines    each check accepts its baseline, and the baseline with every optional argument absent
//   precedence   arguments with two defects give the earlier refusal; a check that calls another hands its refusal on
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
#include <map>
#include <regex>
#include <sstream>
#include <string>
#include <vector>

#include "../pbrs_amd/csrc/host/arg_checks.h"

using namespace pbrs;

namespace {

[[noreturn]] void die(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::fprintf(stderr, "FAIL: ");
    std::vfprintf(stderr, fmt, ap);
    std::fprintf(stderr, "\n");
    va_end(ap);
    std::exit(1);
}
#define REQUIRE(cond, ...) \
    do {                   \
        if (!(cond)) die(__VA_ARGS__); \
    } while (0)

// Planes: distinct non-null addresses, never read.
float kF[32];
uint32_t kU[8];
const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();
constexpr uint32_t kBig = 16385;  // kBig^2 > 2^28

pbrs_camera camera(uint32_t w, uint32_t h) {
    pbrs_camera c{};
    c.width = w, c.height = h;
    return c;
}

// ---- the baselines: every argument of a check by value, `run` the call ----
struct Params {
    SceneState s{true, true};
    pbrs_camera cam = camera(32, 32);
    pbrs_render_params p{};
    bool null_cam = false;
    Params() {
        p.w = 13, p.h = 7, p.strata_x = 2, p.strata_y = 2, p.max_depth = 4, p.integrator = PBRS_INTEGRATOR_PATH;
    }
    Refusal run() const { return check_params(s, null_cam ? nullptr : &cam, &p); }
};
struct Targets {
    pbrs_render_params p = Params().p;
    pbrs_matte_params mp{PBRS_MATTE_INSTANCE, 4};
    WantedOutputs t{true, true, true, true, &mp, true};
    Targets() = default;
    Targets(const Targets& o) : p(o.p), mp(o.mp), t(o.t) { if (o.t.matte_params) t.matte_params = &mp; }
    Refusal run() const { return check_targets(&p, t); }
};
struct Filter {
    pbrs_render_params p = Params().p;
    pbrs_pixel_filter f{PBRS_FILTER_GAUSSIAN, {2.0f, 1.5f}, 2.0f, 0.0f, 0};
    Refusal run() const { return check_filter(&p, &f); }
};
struct Denoise {
    pbrs_denoise_params p{13, 7, 3, PBRS_DENOISE_DEMODULATE | PBRS_DENOISE_ID_STOP, 1.0f, 0.5f, 0.25f, 0.01f};
    const float* rgb_in = kF;
    pbrs_denoise_guides g{kF + 1, kF + 2, kF + 3, kU};
    bool null_guides = false;
    float* rgb_out = kF + 4;
    Refusal run() const { return check_denoise(&p, rgb_in, null_guides ? nullptr : &g, rgb_out); }
};
struct DenoiseVar {
    pbrs_denoise_var_params p{13, 7, 3, PBRS_DENOISE_DEMODULATE | PBRS_DENOISE_ID_STOP, 4.0f, 0.5f, 0.25f, 0.01f};
    const float* rgb_in = kF;
    pbrs_denoise_var_guides g{kF + 1, kF + 2, kF + 3, kU, kF + 5};
    bool null_guides = false;
    float* rgb_out = kF + 4;
    Refusal run() const { return check_denoise_var(&p, rgb_in, null_guides ? nullptr : &g, rgb_out); }
};
struct MatteMask {
    uint32_t w = 13, h = 7, slots = 4;
    const uint32_t* ids = kU;
    const float* coverage = kF;
    std::vector<uint32_t> select{1, 5, 9};  // a heap block of exactly n_select words
    bool null_select = false;
    uint32_t n_select = 3;
    float* mask = kF + 1;
    Refusal run() const { return check_matte_mask(w, h, slots, ids, coverage, null_select ? nullptr : select.data(), n_select, mask); }
};
struct Combine {
    uint32_t w = 13, h = 7;
    const float *direct = kF, *indirect = kF + 1;
    float* out = kF;  // the sum may land on a layer
    Refusal run() const { return check_combine(w, h, direct, indirect, out); }
};
const pbrs_instance_motion* const kTable = reinterpret_cast<const pbrs_instance_motion*>(kF);  // never read
struct MotionTable {
    const pbrs_instance_motion* motion = kTable;
    uint32_t n = 2;
    const uint32_t* instance = kU;
    Refusal run() const { return check_motion_table(motion, n, instance); }
};
struct Temporal {
    pbrs_temporal_params p{13, 7, PBRS_TEMPORAL_ID_TEST, 5.0f, 0.1f, 0.2f, 4.0f, 0};
    pbrs_camera cam = camera(13, 7), cam_prev = camera(13, 7);
    pbrs_temporal_frame f{kF, kF + 1, kF + 2, kF + 3, kU};
    pbrs_temporal_guides prev{kF + 4, kF + 5, kU + 1};
    pbrs_temporal_history hin{kF + 6, kF + 7, kF + 8}, hout{kF + 9, kF + 10, kF + 11};
    bool null_frame = false, null_prev = false, null_hin = false, null_cam_prev = false;
    const pbrs_instance_motion* motion = kTable;
    uint32_t n_motion = 2;
    Refusal run() const {
        return check_temporal(&p, &cam, null_cam_prev ? nullptr : &cam_prev, null_frame ? nullptr : &f, null_prev ? nullptr : &prev, null_hin ? nullptr : &hin, &hout);
    }
    Refusal run_motion() const {
        return check_temporal_motion(&p, &cam, null_cam_prev ? nullptr : &cam_prev, null_frame ? nullptr : &f, null_prev ? nullptr : &prev,
                                     null_hin ? nullptr : &hin, &hout, motion, n_motion);
    }
};
struct MotionVectors {
    uint32_t w = 13, h = 7;
    pbrs_camera cam = camera(13, 7), cam_prev = camera(13, 7);
    const float* depth = kF;
    const uint32_t* instance = kU;
    const pbrs_instance_motion* motion = kTable;
    uint32_t n_motion = 2;
    float* out = kF + 1;
    Refusal run() const { return check_motion_vectors(w, h, &cam, &cam_prev, depth, instance, motion, n_motion, out); }
};
struct Spatial {
    pbrs_spatial_variance_params p{13, 7, 2, PBRS_SPATIAL_ID_STOP | PBRS_SPATIAL_ONLY_UNKNOWN, 0.5f, 0.25f, 4.0f, 0};
    const float *moments = kF, *length = kF + 1;
    pbrs_spatial_variance_guides g{kF + 2, kF + 3, kU};
    bool null_guides = false;
    const float* vin = kF + 4;
    float* vout = kF + 4;  // in place is allowed
    Refusal run() const { return check_spatial_variance(&p, moments, length, null_guides ? nullptr : &g, vin, vout); }
};

// ---- one row per refusal site ----
struct Row {
    const char* check;  // the function of arg_checks.cpp whose site this is
    int code;
    const char* message;
    std::function<Refusal()> call;
};
template <class Args, class Mutate>
Row row(const char* check, int code, const char* message, Mutate mutate) {
    return Row{check, code, message, [mutate] {
                   Args a;
                   mutate(a);
                   return a.run();
               }};
}
void big(pbrs_camera& c) { c.width = c.height = kBig; }

const std::vector<Row>& rows() {
    static const std::vector<Row> r = {
        row<Params>("check_params", PBRS_E_INVALID, "null camera or params", [](Params& a) { a.null_cam = true; }),
        row<Params>("check_params", PBRS_E_NO_SCENE, "no scene uploaded", [](Params& a) { a.s.has_scene = false; }),
        row<Params>("check_params", PBRS_E_INVALID, "empty tile", [](Params& a) { a.p.w = 0; }),
        row<Params>("check_params", PBRS_E_INVALID, "bad row-band parameters", [](Params& a) { a.p.band_count = 2, a.p.band_rows = 0; }),
        row<Params>("check_params", PBRS_E_INVALID, "row bands outside the film",
                    [](Params& a) { a.p.band_count = 2, a.p.band_rows = 4, a.p.band_index = 1, a.cam.height = 14; }),  // the last row is row 14
        row<Params>("check_params", PBRS_E_INVALID, "tile outside the film", [](Params& a) { a.p.x0 = 20; }),
        row<Params>("check_params", PBRS_E_INVALID, "zero strata", [](Params& a) { a.p.strata_y = 0; }),
        row<Params>("check_params", PBRS_E_LIMIT, "max_depth above 64", [](Params& a) { a.p.max_depth = 65; }),
        row<Params>("check_params", PBRS_E_INVALID, "unknown integrator", [](Params& a) { a.p.integrator = PBRS_INTEGRATOR_NORMALS + 1; }),
        row<Params>("check_params", PBRS_E_INVALID, "a visualiser takes one un-jittered ray per pixel (strata 1 x 1)",
                    [](Params& a) { a.p.integrator = PBRS_INTEGRATOR_MATERIALS; }),
        row<Params>("check_params", PBRS_E_INVALID, "the scene's materials carry no pbrs_material::vis_bxdf records",
                    [](Params& a) { a.p.integrator = PBRS_INTEGRATOR_NORMALS, a.p.strata_x = a.p.strata_y = 1, a.s.has_vis_records = false; }),
        row<Params>("check_params", PBRS_E_LIMIT, "tile above 2^28 pixels", [](Params& a) { a.p.w = a.p.h = kBig, big(a.cam); }),

        row<Targets>("check_targets", PBRS_E_INVALID, "AOVs requested from a render that traces no camera ray (max_depth 0)",
                     [](Targets& a) { a.p.max_depth = 0, a.t.aovs = false; }),  // the variance alone
        row<Targets>("check_targets", PBRS_E_INVALID,
                     "light passes need the path integrator (the direct integrator has its own depth semantics, the visualisers bypass the film)",
                     [](Targets& a) { a.p.integrator = PBRS_INTEGRATOR_DIRECT; }),
        row<Targets>("check_targets", PBRS_E_INVALID, "light passes requested from a render that traces no camera ray (max_depth 0)",
                     [](Targets& a) { a.p.max_depth = 0, a.t.aovs = a.t.variance = false; }),
        row<Targets>("check_targets", PBRS_E_INVALID, "a matte without pbrs_matte_params", [](Targets& a) { a.t.matte_params = nullptr; }),
        row<Targets>("check_targets", PBRS_E_INVALID, "unknown matte key", [](Targets& a) { a.mp.key = PBRS_MATTE_MATERIAL + 1; }),
        row<Targets>("check_targets", PBRS_E_INVALID, "matte slots must be 1 .. 8", [](Targets& a) { a.mp.slots = PBRS_MATTE_MAX_SLOTS + 1; }),
        row<Targets>("check_targets", PBRS_E_INVALID, "a matte needs ids and coverage", [](Targets& a) { a.t.matte_ids_and_coverage = false; }),
        row<Targets>("check_targets", PBRS_E_INVALID, "a matte requested from a render that traces no camera ray (max_depth 0)",
                     [](Targets& a) { a.p.max_depth = 0, a.t.aovs = a.t.variance = a.t.passes = false; }),

        row<Filter>("check_filter", PBRS_E_INVALID, "a filtered render takes a rectangular tile, not interleaved row bands",
                    [](Filter& a) { a.p.band_count = 2, a.p.band_rows = 4; }),
        row<Filter>("check_filter", PBRS_E_INVALID, "the visualisers bypass the film: no pixel filter", [](Filter& a) { a.p.integrator = PBRS_INTEGRATOR_MATERIALS; }),
        row<Filter>("check_filter", PBRS_E_INVALID, "unknown pixel filter kind", [](Filter& a) { a.f.kind = PBRS_FILTER_LANCZOS + 1; }),
        row<Filter>("check_filter", PBRS_E_INVALID, "a pixel filter radius must be finite and > 0", [](Filter& a) { a.f.radius[1] = 0.0f; }),
        row<Filter>("check_filter", PBRS_E_INVALID, "non-finite pixel filter parameter", [](Filter& a) { a.f.a = kNaN; }),
        row<Filter>("check_filter", PBRS_E_LIMIT, "pixel filter radius above 4 (the halo's LDS budget)", [](Filter& a) { a.f.radius[0] = 4.5f; }),

        row<Denoise>("check_denoise", PBRS_E_INVALID, "null denoise params, image or guides", [](Denoise& a) { a.rgb_in = nullptr; }),
        row<Denoise>("check_denoise", PBRS_E_INVALID, "empty image", [](Denoise& a) { a.p.h = 0; }),
        row<Denoise>("check_denoise", PBRS_E_INVALID, "denoise iterations must be 1 .. 6", [](Denoise& a) { a.p.iterations = 0; }),
        row<Denoise>("check_denoise", PBRS_E_INVALID, "a denoise sigma must be finite and > 0", [](Denoise& a) { a.p.sigma_normal = kNaN; }),
        row<Denoise>("check_denoise", PBRS_E_INVALID, "the albedo floor must be finite and >= 0", [](Denoise& a) { a.p.albedo_floor = -1.0f; }),
        row<Denoise>("check_denoise", PBRS_E_INVALID, "unknown denoise flag bits", [](Denoise& a) { a.p.flags |= 0x100u; }),
        row<Denoise>("check_denoise", PBRS_E_INVALID, "PBRS_DENOISE_DEMODULATE without an albedo guide", [](Denoise& a) { a.g.albedo = nullptr; }),
        row<Denoise>("check_denoise", PBRS_E_INVALID, "PBRS_DENOISE_ID_STOP without an instance guide", [](Denoise& a) { a.g.instance = nullptr; }),
        row<Denoise>("check_denoise", PBRS_E_LIMIT, "more than 2^28 pixels", [](Denoise& a) { a.p.w = a.p.h = kBig; }),

        row<DenoiseVar>("check_denoise_var", PBRS_E_INVALID, "null denoise params, image or guides", [](DenoiseVar& a) { a.null_guides = true; }),
        row<DenoiseVar>("check_denoise_var", PBRS_E_INVALID, "the variance-guided denoiser needs guides.variance", [](DenoiseVar& a) { a.g.variance = nullptr; }),

        row<MatteMask>("check_matte_mask", PBRS_E_INVALID, "null matte layers or mask", [](MatteMask& a) { a.coverage = nullptr; }),
        row<MatteMask>("check_matte_mask", PBRS_E_INVALID, "empty image", [](MatteMask& a) { a.w = 0; }),
        row<MatteMask>("check_matte_mask", PBRS_E_INVALID, "matte slots must be 1 .. 8", [](MatteMask& a) { a.slots = 0; }),
        row<MatteMask>("check_matte_mask", PBRS_E_INVALID, "more than PBRS_MATTE_MAX_SELECT selected ids", [](MatteMask& a) { a.n_select = PBRS_MATTE_MAX_SELECT + 1; }),
        row<MatteMask>("check_matte_mask", PBRS_E_INVALID, "null selection", [](MatteMask& a) { a.null_select = true; }),
        row<MatteMask>("check_matte_mask", PBRS_E_INVALID, "the selected ids must be strictly ascending", [](MatteMask& a) { a.select[2] = a.select[1]; }),
        row<MatteMask>("check_matte_mask", PBRS_E_LIMIT, "more than 2^28 pixels", [](MatteMask& a) { a.w = a.h = kBig; }),

        row<Combine>("check_combine", PBRS_E_INVALID, "null light passes or output", [](Combine& a) { a.indirect = nullptr; }),
        row<Combine>("check_combine", PBRS_E_INVALID, "empty image", [](Combine& a) { a.h = 0; }),
        row<Combine>("check_combine", PBRS_E_LIMIT, "more than 2^28 pixels", [](Combine& a) { a.w = a.h = kBig; }),

        row<MotionTable>("check_motion_table", PBRS_E_INVALID, "n_motion without a motion table", [](MotionTable& a) { a.motion = nullptr; }),
        row<MotionTable>("check_motion_table", PBRS_E_INVALID, "a motion table of 0 records", [](MotionTable& a) { a.n = 0; }),
        row<MotionTable>("check_motion_table", PBRS_E_INVALID, "a motion table without this frame's instance ids", [](MotionTable& a) { a.instance = nullptr; }),
        row<MotionTable>("check_motion_table", PBRS_E_LIMIT, "more than 2^24 motion records", [](MotionTable& a) { a.n = (1u << 24) + 1u; }),

        row<Temporal>("check_temporal", PBRS_E_INVALID, "null temporal params, camera, frame or history_out", [](Temporal& a) { a.null_frame = true; }),
        row<Temporal>("check_temporal", PBRS_E_INVALID, "the temporal frame needs rgb and depth", [](Temporal& a) { a.f.depth = nullptr; }),
        row<Temporal>("check_temporal", PBRS_E_INVALID, "history_out with a null plane", [](Temporal& a) { a.hout.length = nullptr; }),
        row<Temporal>("check_temporal", PBRS_E_INVALID, "empty image", [](Temporal& a) { a.p.h = 0; }),
        row<Temporal>("check_temporal", PBRS_E_INVALID, "unknown temporal flag bits", [](Temporal& a) { a.p.flags |= 2u; }),
        row<Temporal>("check_temporal", PBRS_E_INVALID, "PBRS_TEMPORAL_ID_TEST without instance ids", [](Temporal& a) { a.f.instance = nullptr; }),
        row<Temporal>("check_temporal", PBRS_E_INVALID, "max_history must be finite and >= 1", [](Temporal& a) { a.p.max_history = 0.5f; }),
        row<Temporal>("check_temporal", PBRS_E_INVALID, "a temporal tolerance must be finite and > 0", [](Temporal& a) { a.p.normal_tolerance = 0.0f; }),
        row<Temporal>("check_temporal", PBRS_E_INVALID, "min_temporal must be finite and >= 2", [](Temporal& a) { a.p.min_temporal = 1.0f; }),
        row<Temporal>("check_temporal", PBRS_E_INVALID, "the camera's size is not w x h", [](Temporal& a) { a.cam.width = 14; }),
        row<Temporal>("check_temporal", PBRS_E_INVALID, "history_in with a null plane", [](Temporal& a) { a.hin.moments = nullptr; }),
        row<Temporal>("check_temporal", PBRS_E_INVALID, "history_in without the previous camera or the previous depth", [](Temporal& a) { a.null_prev = true; }),
        row<Temporal>("check_temporal", PBRS_E_INVALID, "the previous camera's size is not w x h", [](Temporal& a) { a.cam_prev.height = 8; }),
        row<Temporal>("check_temporal", PBRS_E_INVALID, "a normal or an instance guide given for only one of the two frames", [](Temporal& a) { a.prev.normal = nullptr; }),
        row<Temporal>("check_temporal", PBRS_E_INVALID, "temporal accumulation cannot run in place: history_out shares a plane with history_in",
                      [](Temporal& a) { a.hout.moments = a.hin.moments; }),
        row<Temporal>("check_temporal", PBRS_E_LIMIT, "more than 2^28 pixels", [](Temporal& a) { a.p.w = a.p.h = kBig, big(a.cam), big(a.cam_prev); }),

        row<MotionVectors>("check_motion_vectors", PBRS_E_INVALID, "null cameras, depth or motion_out", [](MotionVectors& a) { a.depth = nullptr; }),
        row<MotionVectors>("check_motion_vectors", PBRS_E_INVALID, "empty image", [](MotionVectors& a) { a.w = 0; }),
        row<MotionVectors>("check_motion_vectors", PBRS_E_INVALID, "a camera's size is not w x h", [](MotionVectors& a) { a.cam_prev.width = 14; }),
        row<MotionVectors>("check_motion_vectors", PBRS_E_LIMIT, "more than 2^28 pixels", [](MotionVectors& a) { a.w = a.h = kBig, big(a.cam), big(a.cam_prev); }),

        row<Spatial>("check_spatial_variance", PBRS_E_INVALID, "null spatial variance params, moments, length, variance_in or variance_out",
                     [](Spatial& a) { a.moments = nullptr; }),
        row<Spatial>("check_spatial_variance", PBRS_E_INVALID, "empty image", [](Spatial& a) { a.p.w = 0; }),
        row<Spatial>("check_spatial_variance", PBRS_E_INVALID, "the spatial variance radius must be 1 .. 3", [](Spatial& a) { a.p.radius = PBRS_SPATIAL_MAX_RADIUS + 1; }),
        row<Spatial>("check_spatial_variance", PBRS_E_INVALID, "unknown spatial variance flag bits", [](Spatial& a) { a.p.flags |= 0x100u; }),
        row<Spatial>("check_spatial_variance", PBRS_E_INVALID, "PBRS_SPATIAL_ID_STOP without instance ids", [](Spatial& a) { a.null_guides = true; }),
        row<Spatial>("check_spatial_variance", PBRS_E_INVALID, "a spatial variance sigma must be finite and > 0", [](Spatial& a) { a.p.sigma_depth = kInf; }),
        row<Spatial>("check_spatial_variance", PBRS_E_INVALID, "min_temporal must be finite and >= 1", [](Spatial& a) { a.p.min_temporal = 0.5f; }),
        row<Spatial>("check_spatial_variance", PBRS_E_INVALID, "the spatial variance estimate cannot write over the moments or the length",
                     [](Spatial& a) { a.vout = const_cast<float*>(a.length); }),
        row<Spatial>("check_spatial_variance", PBRS_E_LIMIT, "more than 2^28 pixels", [](Spatial& a) { a.p.w = a.p.h = kBig; }),
    };
    return r;
}

const char* code_name(int code) {
    return code == PBRS_E_INVALID ? "PBRS_E_INVALID" : code == PBRS_E_LIMIT ? "PBRS_E_LIMIT" : code == PBRS_E_NO_SCENE ? "PBRS_E_NO_SCENE" : "?";
}

void expect(const char* what, const Refusal& r, int code, const char* message) {
    REQUIRE(r.code == code && (code == PBRS_OK ? r.message == nullptr : r.message && std::strcmp(r.message, message) == 0), "%s: got %d \"%s\", expected %d \"%s\"", what,
            r.code, r.message ? r.message : "(accepted)", code, message ? message : "(accepted)");
}

void check_refusals(const char* source_path) {
    for (const Row& row : rows()) expect((std::string(row.check) + " row \"" + row.message + "\"").c_str(), row.call(), row.code, row.message);
    // the `return refuse(` sites of the source, function by function, against the rows
    std::ifstream in(source_path);
    REQUIRE(in.good(), "cannot read %s", source_path);
    std::stringstream ss;
    ss << in.rdbuf();
    const std::string text = ss.str();
    const std::regex head("\nRefusal (check_[a-z_]+)\\("), site("return refuse\\(\\s*(PBRS_E_[A-Z_]+),\\s*\"([^\"]*)\"\\)");
    size_t sites = 0, checks = 0;
    for (auto f = std::sregex_iterator(text.begin(), text.end(), head); f != std::sregex_iterator(); ++f, ++checks) {
        const std::string name = (*f)[1];
        const size_t a = (size_t)f->position(), b = text.find("\n}\n", a);
        REQUIRE(b != std::string::npos, "%s: no end of the function", name.c_str());
        const std::string body = text.substr(a, b - a);
        size_t of_check = 0, rows_of_check = 0;
        for (auto it = std::sregex_iterator(body.begin(), body.end(), site); it != std::sregex_iterator(); ++it, ++of_check) {
            const std::string code = (*it)[1], msg = (*it)[2];
            size_t found = 0;
            for (const Row& row : rows()) found += name == row.check && msg == row.message && code == code_name(row.code);
            REQUIRE(found == 1, "%s refuses with \"%s\" (%s): %zu rows for it", name.c_str(), msg.c_str(), code.c_str(), found);
        }
        for (const Row& row : rows()) rows_of_check += name == row.check;
        REQUIRE(of_check == rows_of_check, "%s: %zu refusal sites, %zu rows", name.c_str(), of_check, rows_of_check);
        sites += of_check;
    }
    // no site outside the functions found, or in a form the pattern does not read
    size_t plain = 0;
    for (size_t at = text.find("return refuse("); at != std::string::npos; at = text.find("return refuse(", at + 1)) ++plain;
    REQUIRE(plain == sites, "%zu `return refuse(` in the source, %zu read as sites", plain, sites);
    REQUIRE(sites == rows().size(), "%zu refusal sites, %zu rows", sites, rows().size());
    std::printf("refusals: %zu rows, %zu sites, %zu checks\n", rows().size(), sites, checks);
}

template <class Args, class Mutate>
Refusal with(Mutate mutate) {
    Args a;
    mutate(a);
    return a.run();
}

void check_baselines() {
    const auto ok = [](const char* what, const Refusal& r) { expect(what, r, PBRS_OK, nullptr); };
    ok("check_params", Params().run());
    ok("check_params, row bands", with<Params>([](Params& a) { a.p.band_count = 2, a.p.band_rows = 4, a.p.band_index = 1, a.cam.height = 15; }));
    ok("check_params, normals visualiser", with<Params>([](Params& a) { a.p.integrator = PBRS_INTEGRATOR_NORMALS, a.p.strata_x = a.p.strata_y = 1; }));
    ok("check_params, 2^28 pixels", with<Params>([](Params& a) { a.p.w = a.p.h = 16384, a.cam.width = a.cam.height = 16384; }));
    ok("check_targets", Targets().run());
    ok("check_targets, nothing wanted", with<Targets>([](Targets& a) { a.t = WantedOutputs{}, a.p.max_depth = 0; }));
    ok("check_filter", Filter().run());
    ok("check_filter, a box ignores its parameters", with<Filter>([](Filter& a) { a.f.kind = PBRS_FILTER_BOX, a.f.a = a.f.b = kNaN; }));
    ok("check_denoise", Denoise().run());
    ok("check_denoise, no guides", with<Denoise>([](Denoise& a) { a.g = pbrs_denoise_guides{}, a.p.flags = 0; }));
    ok("check_denoise_var", DenoiseVar().run());
    ok("check_denoise_var, the variance alone", with<DenoiseVar>([](DenoiseVar& a) { a.g = pbrs_denoise_var_guides{nullptr, nullptr, nullptr, nullptr, kF}, a.p.flags = 0; }));
    ok("check_matte_mask", MatteMask().run());
    ok("check_matte_mask, empty selection", with<MatteMask>([](MatteMask& a) { a.null_select = true, a.n_select = 0; }));
    ok("check_combine", Combine().run());
    ok("check_motion_table", MotionTable().run());
    ok("check_motion_table, no table", with<MotionTable>([](MotionTable& a) { a.motion = nullptr, a.n = 0, a.instance = nullptr; }));
    ok("check_temporal", Temporal().run());
    ok("check_temporal_motion", Temporal().run_motion());
    const auto first_frame = [](Temporal& a) {
        a.null_hin = a.null_prev = a.null_cam_prev = true, a.p.flags = 0;
        a.f.variance = a.f.normal = nullptr, a.f.instance = nullptr;
        a.motion = nullptr, a.n_motion = 0;
    };
    ok("check_temporal, no history", with<Temporal>(first_frame));
    {
        Temporal a;
        first_frame(a);
        ok("check_temporal_motion, no history", a.run_motion());
    }
    ok("check_motion_vectors", MotionVectors().run());
    ok("check_motion_vectors, no table", with<MotionVectors>([](MotionVectors& a) { a.instance = nullptr, a.motion = nullptr, a.n_motion = 0; }));
    ok("check_spatial_variance", Spatial().run());
    ok("check_spatial_variance, no guides", with<Spatial>([](Spatial& a) { a.null_guides = true, a.p.flags = 0; }));
    std::printf("baselines accepted\n");
}

void check_precedence() {
    expect("check_params: no scene before an empty tile", with<Params>([](Params& a) { a.s.has_scene = false, a.p.w = 0; }), PBRS_E_NO_SCENE, "no scene uploaded");
    expect("check_denoise: a null image before an empty one", with<Denoise>([](Denoise& a) { a.rgb_in = nullptr, a.p.w = 0; }), PBRS_E_INVALID,
           "null denoise params, image or guides");
    expect("check_denoise: the iterations before a sigma before the pixel limit",
           with<Denoise>([](Denoise& a) { a.p.iterations = 7, a.p.sigma_depth = kNaN, a.p.w = a.p.h = kBig; }), PBRS_E_INVALID, "denoise iterations must be 1 .. 6");
    expect("check_denoise_var: the variance before the plain list", with<DenoiseVar>([](DenoiseVar& a) { a.g.variance = nullptr, a.p.w = 0; }), PBRS_E_INVALID,
           "the variance-guided denoiser needs guides.variance");
    expect("check_denoise_var hands on the plain list", with<DenoiseVar>([](DenoiseVar& a) { a.p.sigma_luminance = 0.0f; }), PBRS_E_INVALID,
           "a denoise sigma must be finite and > 0");
    expect("check_temporal: the flags before the camera's size", with<Temporal>([](Temporal& a) { a.p.flags |= 4u, a.cam.width = 14; }), PBRS_E_INVALID,
           "unknown temporal flag bits");
    {
        Temporal a;
        a.p.max_history = kNaN, a.motion = nullptr;
        expect("check_temporal_motion: the temporal list before the table", a.run_motion(), PBRS_E_INVALID, "max_history must be finite and >= 1");
        Temporal b;
        b.motion = nullptr;
        expect("check_temporal_motion hands on the table's refusal", b.run_motion(), PBRS_E_INVALID, "n_motion without a motion table");
    }
    expect("check_motion_vectors: the table before the pixel limit",
           with<MotionVectors>([](MotionVectors& a) { a.n_motion = 0, a.w = a.h = kBig, big(a.cam), big(a.cam_prev); }), PBRS_E_INVALID, "a motion table of 0 records");
    std::printf("precedence holds\n");
}

}  // namespace

int main(int argc, char** argv) {
    REQUIRE(argc == 2, "usage: arg_checks_check <path of host/arg_checks.cpp>");
    check_refusals(argv[1]);
    check_baselines();
    check_precedence();
    std::printf("ok\n");
    return 0;
}
