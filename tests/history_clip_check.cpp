// tests/history_clip_check.cpp — check_temporal_clip (pbrs_amd/csrc/host/arg_checks.h, arg_checks_clip.cpp), the argument check of
// pbrs_temporal_accumulate_clip[_device], on a CPU: a program of its own that tests/test_history_clip_checks.py compiles with
// -fsanitize=address,undefined and runs, in the manner of tests/arg_checks_check.cpp.
//
//   usage: history_clip_check <path of host/arg_checks_clip.cpp>
//
// The call starts from a valid baseline; image planes are addresses that are never dereferenced.  Checked:
//   refusals     one row per refusal the header lists: the baseline with one defect, the code and the message; every `return refuse(`
//                site of the source has at least one row, and no row names a message the source does not have
//   accepted     the baseline, the edges of the ranges, +inf as clip_history, the first frame of a sequence
//   precedence   the motion call's refusal before the clip's; clip == NULL is check_temporal_motion, whatever else is given
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
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
const pbrs_instance_motion* const kTable = reinterpret_cast<const pbrs_instance_motion*>(kF);  // never read

pbrs_camera camera(uint32_t w, uint32_t h) {
    pbrs_camera c{};
    c.width = w, c.height = h;
    return c;
}

// The baseline: every argument of the check by value, `run` the call.
struct Clip {
    pbrs_temporal_params p{13, 7, PBRS_TEMPORAL_ID_TEST, 5.0f, 0.1f, 0.2f, 4.0f, 0};
    pbrs_camera cam = camera(13, 7), cam_prev = camera(13, 7);
    pbrs_temporal_frame f{kF, kF + 1, kF + 2, kF + 3, kU};
    pbrs_temporal_guides prev{kF + 4, kF + 5, kU + 1};
    pbrs_temporal_history hin{kF + 6, kF + 7, kF + 8}, hout{kF + 9, kF + 10, kF + 11};
    bool first_frame = false, null_clip = false;
    const pbrs_instance_motion* motion = kTable;
    uint32_t n_motion = 2;
    pbrs_history_clip_params clip{2, 1.5f, 4.0f, 0};
    Refusal run() const {
        return check_temporal_clip(&p, &cam, first_frame ? nullptr : &cam_prev, &f, first_frame ? nullptr : &prev, first_frame ? nullptr : &hin, &hout, motion,
                                   n_motion, null_clip ? nullptr : &clip);
    }
};

struct Row {
    int code;
    const char* message;
    std::function<void(Clip&)> mutate;
};

const char* const kRadius = "the history clip radius must be 1 .. 3";
const char* const kGamma = "the history clip gamma must be finite and > 0";
const char* const kLength = "clip_history must be >= 1 (+inf: never shortened)";
const char* const kFlags = "unknown history clip flag bits";
const char* const kAlias = "history clipping gathers a halo of frame.rgb: history_out.rgb cannot be that plane";

const std::vector<Row>& rows() {
    static const std::vector<Row> r = {
        {PBRS_E_INVALID, kRadius, [](Clip& a) { a.clip.radius = 0; }},
        {PBRS_E_INVALID, kRadius, [](Clip& a) { a.clip.radius = PBRS_CLIP_MAX_RADIUS + 1; }},
        {PBRS_E_INVALID, kGamma, [](Clip& a) { a.clip.gamma = 0.0f; }},
        {PBRS_E_INVALID, kGamma, [](Clip& a) { a.clip.gamma = kInf; }},
        {PBRS_E_INVALID, kGamma, [](Clip& a) { a.clip.gamma = kNaN; }},
        {PBRS_E_INVALID, kLength, [](Clip& a) { a.clip.clip_history = 0.5f; }},
        {PBRS_E_INVALID, kLength, [](Clip& a) { a.clip.clip_history = kNaN; }},
        {PBRS_E_INVALID, kFlags, [](Clip& a) { a.clip.flags = 1u; }},
        {PBRS_E_INVALID, kAlias, [](Clip& a) { a.hout.rgb = const_cast<float*>(a.f.rgb); }},
    };
    return r;
}

void expect(const char* what, const Refusal& r, int code, const char* message) {
    REQUIRE(r.code == code && (code == PBRS_OK ? r.message == nullptr : r.message && std::strcmp(r.message, message) == 0), "%s: got %d \"%s\", expected %d \"%s\"", what,
            r.code, r.message ? r.message : "(accepted)", code, message ? message : "(accepted)");
}

template <class Mutate>
Refusal with(Mutate mutate) {
    Clip a;
    mutate(a);
    return a.run();
}

void check_refusals(const char* source_path) {
    for (const Row& row : rows()) expect(row.message, with(row.mutate), row.code, row.message);
    std::ifstream in(source_path);
    REQUIRE(in.good(), "cannot read %s", source_path);
    std::stringstream ss;
    ss << in.rdbuf();
    const std::string text = ss.str();
    const std::regex site("return refuse\\(\\s*(PBRS_E_[A-Z_]+),\\s*\"([^\"]*)\"\\)");
    size_t sites = 0;
    std::vector<std::string> seen;
    for (auto it = std::sregex_iterator(text.begin(), text.end(), site); it != std::sregex_iterator(); ++it, ++sites) {
        const std::string code = (*it)[1], msg = (*it)[2];
        size_t found = 0;
        for (const Row& row : rows()) found += msg == row.message && code == "PBRS_E_INVALID" && row.code == PBRS_E_INVALID;
        REQUIRE(found >= 1, "the source refuses with \"%s\" (%s): no row for it", msg.c_str(), code.c_str());
        seen.push_back(msg);
    }
    for (const Row& row : rows()) {
        size_t found = 0;
        for (const std::string& m : seen) found += m == row.message;
        REQUIRE(found == 1, "a row expects \"%s\": %zu sites refuse with it", row.message, found);
    }
    size_t plain = 0;
    for (size_t at = text.find("return refuse("); at != std::string::npos; at = text.find("return refuse(", at + 1)) ++plain;
    REQUIRE(plain == sites, "%zu `return refuse(` in the source, %zu read as sites", plain, sites);
    std::printf("refusals: %zu rows, %zu sites\n", rows().size(), sites);
}

void check_accepted() {
    const auto ok = [](const char* what, const Refusal& r) { expect(what, r, PBRS_OK, nullptr); };
    ok("the baseline", Clip().run());
    ok("radius 1", with([](Clip& a) { a.clip.radius = 1; }));
    ok("radius 3", with([](Clip& a) { a.clip.radius = PBRS_CLIP_MAX_RADIUS; }));
    ok("clip_history 1", with([](Clip& a) { a.clip.clip_history = 1.0f; }));
    ok("clip_history +inf", with([](Clip& a) { a.clip.clip_history = kInf; }));
    ok("no motion table", with([](Clip& a) { a.motion = nullptr, a.n_motion = 0; }));
    ok("the first frame of a sequence", with([](Clip& a) { a.first_frame = true; }));
    ok("history_out.rgb on the frame's plane without a clip (the motion call tolerates it)",
       with([](Clip& a) { a.hout.rgb = const_cast<float*>(a.f.rgb), a.null_clip = true; }));
    std::printf("accepted calls pass\n");
}

void check_precedence() {
    expect("the temporal list before the clip", with([](Clip& a) { a.p.max_history = kNaN, a.clip.radius = 0; }), PBRS_E_INVALID,
           "max_history must be finite and >= 1");
    expect("the motion table before the clip", with([](Clip& a) { a.n_motion = 0, a.clip.gamma = kNaN; }), PBRS_E_INVALID, "a motion table of 0 records");
    expect("the table's limit before the clip", with([](Clip& a) { a.n_motion = (1u << 24) + 1u, a.clip.flags = 2u; }), PBRS_E_LIMIT,
           "more than 2^24 motion records");
    expect("the radius before gamma", with([](Clip& a) { a.clip.radius = 9, a.clip.gamma = -1.0f; }), PBRS_E_INVALID, kRadius);
    expect("the flags before the aliasing", with([](Clip& a) { a.clip.flags = 4u, a.hout.rgb = const_cast<float*>(a.f.rgb); }), PBRS_E_INVALID, kFlags);
    expect("a null clip hands on the motion call's refusal", with([](Clip& a) { a.null_clip = true, a.p.w = 0; }), PBRS_E_INVALID, "empty image");
    {
        Clip a;  // a null clip is check_temporal_motion on the same arguments
        a.null_clip = true;
        const Refusal r = a.run(), m = check_temporal_motion(&a.p, &a.cam, &a.cam_prev, &a.f, &a.prev, &a.hin, &a.hout, a.motion, a.n_motion);
        REQUIRE(r.code == m.code && r.message == m.message && r.code == PBRS_OK, "a null clip is not the motion call");
    }
    std::printf("precedence holds\n");
}

}  // namespace

int main(int argc, char** argv) {
    REQUIRE(argc == 2, "usage: history_clip_check <path of host/arg_checks_clip.cpp>");
    check_refusals(argv[1]);
    check_accepted();
    check_precedence();
    std::printf("ok\n");
    return 0;
}
