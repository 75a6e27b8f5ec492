// tests/motion_blur_check.cpp — check_motion_blur and pbrsm_motion_blur_params_default (pbrs_amd/csrc/host/arg_checks.h,
// arg_checks_motion_blur.cpp), the argument check and the filler of pbrsm_motion_blur[_device], on a CPU: a program of its own that
// tests/test_motion_blur_checks.py compiles with -fsanitize=address,undefined and runs, in the manner of tests/dof_check.cpp.
//
//   usage: motion_blur_check <path of host/arg_checks_motion_blur.cpp>
//
// The call starts from a valid baseline; planes are addresses that are never dereferenced.  Checked:
//   refusals     one row per refusal the header lists, and per boundary value on its refusing side: the baseline with one defect, the
//                code and the message; every `return refuse(` site of the source has at least one row, and no row names a message the
//                source does not have
//   accepted     the baseline, the filler's defaults and its bytes, each boundary value on its accepting side, 2^28 pixels
//   precedence   the order of the refusals, as the header states it
#include <cmath>
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
float kF[4];
const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();
const float kMax = std::numeric_limits<float>::max(), kDenorm = std::numeric_limits<float>::denorm_min();

pbrs_motion_blur_params defaults(uint32_t w, uint32_t h) {
    pbrs_motion_blur_params p;
    std::memset(&p, 0xAB, sizeof p);  // the filler writes every byte
    pbrsm_motion_blur_params_default(w, h, &p);
    return p;
}

// The baseline: every argument of the check by value, `run` the call.
struct Call {
    pbrs_motion_blur_params p = defaults(13, 7);
    const float* rgb = kF;
    const float* depth = kF + 1;
    const float* motion = kF + 2;
    float* rgb_out = kF + 3;
    bool null_params = false;
    Refusal run() const { return check_motion_blur(null_params ? nullptr : &p, rgb, depth, motion, rgb_out); }
};

struct Row {
    int code;
    const char* message;
    std::function<void(Call&)> mutate;
};

const char* const kNull = "null motion blur params, rgb, depth, motion or rgb_out";
const char* const kInPlace = "the motion blur output must not be its input: a gather reads its neighbours";
const char* const kEmpty = "empty image";
const char* const kRadius = "the motion blur max_radius must be 1 .. 16";
const char* const kTaps = "the motion blur taps must be 2 .. 64";
const char* const kFlags = "unknown motion blur flag bits";
const char* const kReserved = "the motion blur reserved word must be 0";
const char* const kShutter = "the motion blur shutter must be finite and 0 .. 1";
const char* const kZRel = "the motion blur z_rel must be finite and > 0";
const char* const kPixels = "more than 2^28 pixels";

const std::vector<Row>& rows() {
    static const std::vector<Row> r = {
        {PBRS_E_INVALID, kNull, [](Call& c) { c.null_params = true; }},
        {PBRS_E_INVALID, kNull, [](Call& c) { c.rgb = nullptr; }},
        {PBRS_E_INVALID, kNull, [](Call& c) { c.depth = nullptr; }},
        {PBRS_E_INVALID, kNull, [](Call& c) { c.motion = nullptr; }},
        {PBRS_E_INVALID, kNull, [](Call& c) { c.rgb_out = nullptr; }},
        {PBRS_E_INVALID, kInPlace, [](Call& c) { c.rgb_out = const_cast<float*>(c.rgb); }},
        {PBRS_E_INVALID, kEmpty, [](Call& c) { c.p.w = 0; }},
        {PBRS_E_INVALID, kEmpty, [](Call& c) { c.p.h = 0; }},
        {PBRS_E_INVALID, kRadius, [](Call& c) { c.p.max_radius = 0; }},
        {PBRS_E_INVALID, kRadius, [](Call& c) { c.p.max_radius = PBRS_MOTION_BLUR_MAX_RADIUS + 1u; }},
        {PBRS_E_INVALID, kRadius, [](Call& c) { c.p.max_radius = 0xFFFFFFFFu; }},
        {PBRS_E_INVALID, kTaps, [](Call& c) { c.p.taps = 0; }},
        {PBRS_E_INVALID, kTaps, [](Call& c) { c.p.taps = 1; }},
        {PBRS_E_INVALID, kTaps, [](Call& c) { c.p.taps = PBRS_MOTION_BLUR_MAX_TAPS + 1u; }},
        {PBRS_E_INVALID, kTaps, [](Call& c) { c.p.taps = 0xFFFFFFFFu; }},
        {PBRS_E_INVALID, kFlags, [](Call& c) { c.p.flags = 2u; }},
        {PBRS_E_INVALID, kFlags, [](Call& c) { c.p.flags = PBRS_MOTION_BLUR_JITTER | 2u; }},
        {PBRS_E_INVALID, kFlags, [](Call& c) { c.p.flags = 0x80000000u; }},
        {PBRS_E_INVALID, kReserved, [](Call& c) { c.p.reserved = 1u; }},
        {PBRS_E_INVALID, kReserved, [](Call& c) { c.p.reserved = 0x80000000u; }},
        {PBRS_E_INVALID, kShutter, [](Call& c) { c.p.shutter = -kDenorm; }},
        {PBRS_E_INVALID, kShutter, [](Call& c) { c.p.shutter = -1.0f; }},
        {PBRS_E_INVALID, kShutter, [](Call& c) { c.p.shutter = std::nextafter(1.0f, 2.0f); }},
        {PBRS_E_INVALID, kShutter, [](Call& c) { c.p.shutter = 2.0f; }},
        {PBRS_E_INVALID, kShutter, [](Call& c) { c.p.shutter = kInf; }},
        {PBRS_E_INVALID, kShutter, [](Call& c) { c.p.shutter = -kInf; }},
        {PBRS_E_INVALID, kShutter, [](Call& c) { c.p.shutter = kNaN; }},
        {PBRS_E_INVALID, kZRel, [](Call& c) { c.p.z_rel = 0.0f; }},
        {PBRS_E_INVALID, kZRel, [](Call& c) { c.p.z_rel = -0.0f; }},
        {PBRS_E_INVALID, kZRel, [](Call& c) { c.p.z_rel = -kDenorm; }},
        {PBRS_E_INVALID, kZRel, [](Call& c) { c.p.z_rel = -1.0f; }},
        {PBRS_E_INVALID, kZRel, [](Call& c) { c.p.z_rel = kInf; }},
        {PBRS_E_INVALID, kZRel, [](Call& c) { c.p.z_rel = -kInf; }},
        {PBRS_E_INVALID, kZRel, [](Call& c) { c.p.z_rel = kNaN; }},
        {PBRS_E_LIMIT, kPixels, [](Call& c) { c.p.w = 1u << 15, c.p.h = (1u << 13) + 1u; }},
        {PBRS_E_LIMIT, kPixels, [](Call& c) { c.p.w = (1u << 28) + 1u, c.p.h = 1; }},
        {PBRS_E_LIMIT, kPixels, [](Call& c) { c.p.w = 0xFFFFFFFFu, c.p.h = 0xFFFFFFFFu; }},
    };
    return r;
}

void expect(const char* what, const Refusal& r, int code, const char* message) {
    REQUIRE(r.code == code && (code == PBRS_OK ? r.message == nullptr : r.message && std::strcmp(r.message, message) == 0), "%s: got %d \"%s\", expected %d \"%s\"", what,
            r.code, r.message ? r.message : "(accepted)", code, message ? message : "(accepted)");
}

template <class Mutate>
Refusal with(Mutate mutate) {
    Call c;
    mutate(c);
    return c.run();
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
        for (const Row& row : rows()) found += msg == row.message && code == (row.code == PBRS_E_LIMIT ? "PBRS_E_LIMIT" : "PBRS_E_INVALID");
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
    ok("the baseline", Call().run());
    {
        const pbrs_motion_blur_params d = defaults(1920, 1080);
        REQUIRE(d.w == 1920 && d.h == 1080 && d.max_radius == 16 && d.taps == 16 && d.flags == 0 && d.shutter == 0.5f && d.z_rel == 0.05f && d.reserved == 0,
                "pbrsm_motion_blur_params_default does not fill the documented values");
        // w, h, max_radius, taps, flags, 0.5f, 0.05f, 0: the filler's 32 bytes
        const uint32_t words[8] = {1920u, 1080u, 16u, 16u, 0u, 0x3F000000u, 0x3D4CCCCDu, 0u};
        REQUIRE(sizeof d == sizeof words && std::memcmp(&d, words, sizeof d) == 0, "pbrsm_motion_blur_params_default does not write the documented bytes");
        pbrsm_motion_blur_params_default(3, 4, nullptr);  // does nothing
        ok("the defaults", check_motion_blur(&d, kF, kF + 1, kF + 2, kF + 3));
    }
    for (uint32_t radius = 1; radius <= PBRS_MOTION_BLUR_MAX_RADIUS; ++radius) ok("a radius", with([&](Call& c) { c.p.max_radius = radius; }));
    for (uint32_t taps = 2; taps <= PBRS_MOTION_BLUR_MAX_TAPS; ++taps) ok("a number of taps", with([&](Call& c) { c.p.taps = taps; }));
    ok("the jitter flag", with([](Call& c) { c.p.flags = PBRS_MOTION_BLUR_JITTER; }));
    ok("shutter +0", with([](Call& c) { c.p.shutter = 0.0f; }));
    ok("shutter -0", with([](Call& c) { c.p.shutter = -0.0f; }));
    ok("the smallest shutter above 0", with([](Call& c) { c.p.shutter = kDenorm; }));
    ok("shutter 1", with([](Call& c) { c.p.shutter = 1.0f; }));
    ok("the smallest z_rel", with([](Call& c) { c.p.z_rel = kDenorm; }));
    ok("the largest z_rel", with([](Call& c) { c.p.z_rel = kMax; }));
    ok("the depth in the output's place is the caller's business", with([](Call& c) { c.depth = c.rgb_out; }));
    ok("one pixel", with([](Call& c) { c.p.w = 1, c.p.h = 1; }));
    ok("2^28 pixels", with([](Call& c) { c.p.w = 1u << 14, c.p.h = 1u << 14; }));
    ok("2^28 pixels in one row", with([](Call& c) { c.p.w = 1u << 28, c.p.h = 1; }));
    std::printf("accepted calls pass\n");
}

void check_precedence() {
    expect("null before in place", with([](Call& c) { c.motion = nullptr, c.rgb_out = const_cast<float*>(c.rgb); }), PBRS_E_INVALID, kNull);
    expect("in place before empty", with([](Call& c) { c.rgb_out = const_cast<float*>(c.rgb), c.p.w = 0; }), PBRS_E_INVALID, kInPlace);
    expect("empty before the radius", with([](Call& c) { c.p.h = 0, c.p.max_radius = 17; }), PBRS_E_INVALID, kEmpty);
    expect("the radius before the taps", with([](Call& c) { c.p.max_radius = 0, c.p.taps = 1; }), PBRS_E_INVALID, kRadius);
    expect("the taps before the flags", with([](Call& c) { c.p.taps = 65, c.p.flags = 4u; }), PBRS_E_INVALID, kTaps);
    expect("the flags before the reserved word", with([](Call& c) { c.p.flags = 4u, c.p.reserved = 1u; }), PBRS_E_INVALID, kFlags);
    expect("the reserved word before the shutter", with([](Call& c) { c.p.reserved = 1u, c.p.shutter = kNaN; }), PBRS_E_INVALID, kReserved);
    expect("the shutter before z_rel", with([](Call& c) { c.p.shutter = 2.0f, c.p.z_rel = -1.0f; }), PBRS_E_INVALID, kShutter);
    expect("z_rel before the limit", with([](Call& c) { c.p.z_rel = kNaN, c.p.w = c.p.h = 1u << 15; }), PBRS_E_INVALID, kZRel);
    std::printf("precedence holds\n");
}

}  // namespace

int main(int argc, char** argv) {
    REQUIRE(argc == 2, "usage: motion_blur_check <path of host/arg_checks_motion_blur.cpp>");
    check_refusals(argv[1]);
    check_accepted();
    check_precedence();
    std::printf("ok\n");
    return 0;
}
