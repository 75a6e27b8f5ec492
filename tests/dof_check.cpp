// tests/dof_check.cpp — check_dof and pbrsf_dof_params_default (pbrs_amd/csrc/host/arg_checks.h, arg_checks_dof.cpp), the argument
// check and the filler of pbrsf_dof[_device], on a CPU: a program of its own that tests/test_dof_checks.py compiles with
// -fsanitize=address,undefined and runs, in the manner of tests/bloom_check.cpp.
//
//   usage: dof_check <path of host/arg_checks_dof.cpp>
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
float kF[3];
const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();
const float kMax = std::numeric_limits<float>::max(), kDenorm = std::numeric_limits<float>::denorm_min();

pbrs_dof_params defaults(uint32_t w, uint32_t h) {
    pbrs_dof_params p;
    std::memset(&p, 0xAB, sizeof p);  // the filler writes every byte
    pbrsf_dof_params_default(w, h, &p);
    return p;
}

// The baseline: every argument of the check by value, `run` the call.
struct Call {
    pbrs_dof_params p = defaults(13, 7);
    const float* rgb = kF;
    const float* depth = kF + 1;
    float* rgb_out = kF + 2;
    bool null_params = false;
    Call() { p.scale = 2.0f; }
    Refusal run() const { return check_dof(null_params ? nullptr : &p, rgb, depth, rgb_out); }
};

struct Row {
    int code;
    const char* message;
    std::function<void(Call&)> mutate;
};

const char* const kNull = "null dof params, rgb, depth or rgb_out";
const char* const kInPlace = "the dof output must not be its input: a gather reads its neighbours";
const char* const kEmpty = "empty image";
const char* const kRadius = "the dof max_radius must be 1 .. 16";
const char* const kFlags = "unknown dof flag bits";
const char* const kReserved = "the dof reserved words must be 0";
const char* const kFocus = "the dof focus must be finite and > 0";
const char* const kScale = "the dof scale must be finite and >= 0";
const char* const kPixels = "more than 2^28 pixels";

const std::vector<Row>& rows() {
    static const std::vector<Row> r = {
        {PBRS_E_INVALID, kNull, [](Call& c) { c.null_params = true; }},
        {PBRS_E_INVALID, kNull, [](Call& c) { c.rgb = nullptr; }},
        {PBRS_E_INVALID, kNull, [](Call& c) { c.depth = nullptr; }},
        {PBRS_E_INVALID, kNull, [](Call& c) { c.rgb_out = nullptr; }},
        {PBRS_E_INVALID, kInPlace, [](Call& c) { c.rgb_out = const_cast<float*>(c.rgb); }},
        {PBRS_E_INVALID, kEmpty, [](Call& c) { c.p.w = 0; }},
        {PBRS_E_INVALID, kEmpty, [](Call& c) { c.p.h = 0; }},
        {PBRS_E_INVALID, kRadius, [](Call& c) { c.p.max_radius = 0; }},
        {PBRS_E_INVALID, kRadius, [](Call& c) { c.p.max_radius = PBRS_DOF_MAX_RADIUS + 1u; }},
        {PBRS_E_INVALID, kRadius, [](Call& c) { c.p.max_radius = 0xFFFFFFFFu; }},
        {PBRS_E_INVALID, kFlags, [](Call& c) { c.p.flags = 1u; }},
        {PBRS_E_INVALID, kFlags, [](Call& c) { c.p.flags = 0x80000000u; }},
        {PBRS_E_INVALID, kReserved, [](Call& c) { c.p.reserved[0] = 1u; }},
        {PBRS_E_INVALID, kReserved, [](Call& c) { c.p.reserved[1] = 0x80000000u; }},
        {PBRS_E_INVALID, kFocus, [](Call& c) { c.p.focus = 0.0f; }},
        {PBRS_E_INVALID, kFocus, [](Call& c) { c.p.focus = -0.0f; }},
        {PBRS_E_INVALID, kFocus, [](Call& c) { c.p.focus = -kDenorm; }},
        {PBRS_E_INVALID, kFocus, [](Call& c) { c.p.focus = -1.0f; }},
        {PBRS_E_INVALID, kFocus, [](Call& c) { c.p.focus = kInf; }},
        {PBRS_E_INVALID, kFocus, [](Call& c) { c.p.focus = -kInf; }},
        {PBRS_E_INVALID, kFocus, [](Call& c) { c.p.focus = kNaN; }},
        {PBRS_E_INVALID, kScale, [](Call& c) { c.p.scale = -kDenorm; }},
        {PBRS_E_INVALID, kScale, [](Call& c) { c.p.scale = -1.0f; }},
        {PBRS_E_INVALID, kScale, [](Call& c) { c.p.scale = kInf; }},
        {PBRS_E_INVALID, kScale, [](Call& c) { c.p.scale = -kInf; }},
        {PBRS_E_INVALID, kScale, [](Call& c) { c.p.scale = kNaN; }},
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
        const pbrs_dof_params d = defaults(1920, 1080);
        REQUIRE(d.w == 1920 && d.h == 1080 && d.max_radius == 8 && d.flags == 0 && d.focus == 1.0f && d.scale == 0.0f && d.reserved[0] == 0 && d.reserved[1] == 0,
                "pbrsf_dof_params_default does not fill the documented values");
        // w, h, max_radius, flags, 1.0f, +0.0f, 0, 0: the filler's 32 bytes
        const uint32_t words[8] = {1920u, 1080u, 8u, 0u, 0x3F800000u, 0u, 0u, 0u};
        REQUIRE(sizeof d == sizeof words && std::memcmp(&d, words, sizeof d) == 0, "pbrsf_dof_params_default does not write the documented bytes");
        pbrsf_dof_params_default(3, 4, nullptr);  // does nothing
        ok("the defaults", check_dof(&d, kF, kF + 1, kF + 2));
    }
    for (uint32_t radius = 1; radius <= PBRS_DOF_MAX_RADIUS; ++radius) ok("a radius", with([&](Call& c) { c.p.max_radius = radius; }));
    ok("the smallest focus", with([](Call& c) { c.p.focus = kDenorm; }));
    ok("the largest focus", with([](Call& c) { c.p.focus = kMax; }));
    ok("scale +0", with([](Call& c) { c.p.scale = 0.0f; }));
    ok("scale -0", with([](Call& c) { c.p.scale = -0.0f; }));
    ok("the smallest scale above 0", with([](Call& c) { c.p.scale = kDenorm; }));
    ok("the largest scale", with([](Call& c) { c.p.scale = kMax; }));
    ok("the depth in the output's place is the caller's business", with([](Call& c) { c.depth = c.rgb_out; }));
    ok("one pixel", with([](Call& c) { c.p.w = 1, c.p.h = 1; }));
    ok("2^28 pixels", with([](Call& c) { c.p.w = 1u << 14, c.p.h = 1u << 14; }));
    ok("2^28 pixels in one row", with([](Call& c) { c.p.w = 1u << 28, c.p.h = 1; }));
    std::printf("accepted calls pass\n");
}

void check_precedence() {
    expect("null before in place", with([](Call& c) { c.depth = nullptr, c.rgb_out = const_cast<float*>(c.rgb); }), PBRS_E_INVALID, kNull);
    expect("in place before empty", with([](Call& c) { c.rgb_out = const_cast<float*>(c.rgb), c.p.w = 0; }), PBRS_E_INVALID, kInPlace);
    expect("empty before the radius", with([](Call& c) { c.p.h = 0, c.p.max_radius = 17; }), PBRS_E_INVALID, kEmpty);
    expect("the radius before the flags", with([](Call& c) { c.p.max_radius = 0, c.p.flags = 4u; }), PBRS_E_INVALID, kRadius);
    expect("the flags before the reserved words", with([](Call& c) { c.p.flags = 4u, c.p.reserved[0] = 1u; }), PBRS_E_INVALID, kFlags);
    expect("the reserved words before the focus", with([](Call& c) { c.p.reserved[1] = 1u, c.p.focus = kNaN; }), PBRS_E_INVALID, kReserved);
    expect("the focus before the scale", with([](Call& c) { c.p.focus = 0.0f, c.p.scale = -1.0f; }), PBRS_E_INVALID, kFocus);
    expect("the scale before the limit", with([](Call& c) { c.p.scale = kNaN, c.p.w = c.p.h = 1u << 15; }), PBRS_E_INVALID, kScale);
    std::printf("precedence holds\n");
}

}  // namespace

int main(int argc, char** argv) {
    REQUIRE(argc == 2, "usage: dof_check <path of host/arg_checks_dof.cpp>");
    check_refusals(argv[1]);
    check_accepted();
    check_precedence();
    std::printf("ok\n");
    return 0;
}
