// tests/bloom_check.cpp — check_bloom and pbrsb_bloom_params_default (pbrs_amd/csrc/host/arg_checks.h, arg_checks_bloom.cpp), the
// argument check and the filler of pbrsb_bloom[_device], on a CPU: a program of its own that tests/test_bloom_checks.py compiles with
// -fsanitize=address,undefined and runs, in the manner of tests/despeckle_check.cpp.
//
//   usage: bloom_check <path of host/arg_checks_bloom.cpp>
//
// The call starts from a valid baseline; planes are addresses that are never dereferenced.  Checked:
//   refusals     one row per refusal the header lists, and per boundary value on its refusing side: the baseline with one defect, the
//                code and the message; every `return refuse(` site of the source has at least one row, and no row names a message the
//                source does not have
//   accepted     the baseline, the filler's defaults and its bytes, each boundary value on its accepting side, in place, 2^28 pixels
//   precedence   the order of the refusals
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
float kF[2];
const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();
const float kMax = std::numeric_limits<float>::max(), kDenorm = std::numeric_limits<float>::denorm_min();

pbrs_bloom_params defaults(uint32_t w, uint32_t h) {
    pbrs_bloom_params p;
    std::memset(&p, 0xAB, sizeof p);  // the filler writes every byte
    pbrsb_bloom_params_default(w, h, &p);
    return p;
}

// The baseline: every argument of the check by value, `run` the call.
struct Call {
    pbrs_bloom_params p = defaults(13, 7);
    const float* rgb = kF;
    float* rgb_out = kF + 1;
    bool null_params = false;
    Refusal run() const { return check_bloom(null_params ? nullptr : &p, rgb, rgb_out); }
};

struct Row {
    int code;
    const char* message;
    std::function<void(Call&)> mutate;
};

const char* const kNull = "null bloom params, rgb or rgb_out";
const char* const kEmpty = "empty image";
const char* const kLevels = "the bloom levels must be 1 .. 8";
const char* const kFlags = "unknown bloom flag bits";
const char* const kThreshold = "the bloom threshold must be finite and >= 0";
const char* const kKnee = "the bloom knee must be in [0, 1]";
const char* const kStrength = "the bloom strength must be finite and >= 0";
const char* const kSpread = "the bloom spread must be in [0, 1]";
const char* const kMix = "PBRS_BLOOM_MIX takes a strength <= 1";
const char* const kPixels = "more than 2^28 pixels";

const std::vector<Row>& rows() {
    static const std::vector<Row> r = {
        {PBRS_E_INVALID, kNull, [](Call& c) { c.null_params = true; }},
        {PBRS_E_INVALID, kNull, [](Call& c) { c.rgb = nullptr; }},
        {PBRS_E_INVALID, kNull, [](Call& c) { c.rgb_out = nullptr; }},
        {PBRS_E_INVALID, kEmpty, [](Call& c) { c.p.w = 0; }},
        {PBRS_E_INVALID, kEmpty, [](Call& c) { c.p.h = 0; }},
        {PBRS_E_INVALID, kLevels, [](Call& c) { c.p.levels = 0; }},
        {PBRS_E_INVALID, kLevels, [](Call& c) { c.p.levels = PBRS_BLOOM_MAX_LEVELS + 1u; }},
        {PBRS_E_INVALID, kLevels, [](Call& c) { c.p.levels = 0xFFFFFFFFu; }},
        {PBRS_E_INVALID, kFlags, [](Call& c) { c.p.flags = 2u; }},
        {PBRS_E_INVALID, kFlags, [](Call& c) { c.p.flags = PBRS_BLOOM_MIX | 0x80000000u; }},
        {PBRS_E_INVALID, kThreshold, [](Call& c) { c.p.threshold = -kDenorm; }},
        {PBRS_E_INVALID, kThreshold, [](Call& c) { c.p.threshold = -1.0f; }},
        {PBRS_E_INVALID, kThreshold, [](Call& c) { c.p.threshold = kInf; }},
        {PBRS_E_INVALID, kThreshold, [](Call& c) { c.p.threshold = -kInf; }},
        {PBRS_E_INVALID, kThreshold, [](Call& c) { c.p.threshold = kNaN; }},
        {PBRS_E_INVALID, kKnee, [](Call& c) { c.p.knee = -kDenorm; }},
        {PBRS_E_INVALID, kKnee, [](Call& c) { c.p.knee = std::nextafter(1.0f, 2.0f); }},
        {PBRS_E_INVALID, kKnee, [](Call& c) { c.p.knee = kInf; }},
        {PBRS_E_INVALID, kKnee, [](Call& c) { c.p.knee = kNaN; }},
        {PBRS_E_INVALID, kStrength, [](Call& c) { c.p.strength = -kDenorm; }},
        {PBRS_E_INVALID, kStrength, [](Call& c) { c.p.strength = -1.0f; }},
        {PBRS_E_INVALID, kStrength, [](Call& c) { c.p.strength = kInf; }},
        {PBRS_E_INVALID, kStrength, [](Call& c) { c.p.strength = kNaN; }},
        {PBRS_E_INVALID, kSpread, [](Call& c) { c.p.spread = -kDenorm; }},
        {PBRS_E_INVALID, kSpread, [](Call& c) { c.p.spread = std::nextafter(1.0f, 2.0f); }},
        {PBRS_E_INVALID, kSpread, [](Call& c) { c.p.spread = -kInf; }},
        {PBRS_E_INVALID, kSpread, [](Call& c) { c.p.spread = kNaN; }},
        {PBRS_E_INVALID, kMix, [](Call& c) { c.p.flags = PBRS_BLOOM_MIX, c.p.strength = std::nextafter(1.0f, 2.0f); }},
        {PBRS_E_INVALID, kMix, [](Call& c) { c.p.flags = PBRS_BLOOM_MIX, c.p.strength = kMax; }},
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
        const pbrs_bloom_params d = defaults(1920, 1080);
        REQUIRE(d.w == 1920 && d.h == 1080 && d.levels == 6 && d.flags == 0 && d.threshold == 1.0f && d.knee == 0.5f && d.strength == 0.05f && d.spread == 0.6f,
                "pbrsb_bloom_params_default does not fill the documented values");
        // w, h, levels, flags, 1.0f, 0.5f, 0.05f, 0.6f: the filler's 32 bytes
        const uint32_t words[8] = {1920u, 1080u, 6u, 0u, 0x3F800000u, 0x3F000000u, 0x3D4CCCCDu, 0x3F19999Au};
        REQUIRE(sizeof d == sizeof words && std::memcmp(&d, words, sizeof d) == 0, "pbrsb_bloom_params_default does not write the documented bytes");
        pbrsb_bloom_params_default(3, 4, nullptr);  // does nothing
        ok("the defaults", check_bloom(&d, kF, kF + 1));
    }
    for (uint32_t levels = 1; levels <= PBRS_BLOOM_MAX_LEVELS; ++levels) ok("a level count", with([&](Call& c) { c.p.levels = levels; }));
    ok("the flag", with([](Call& c) { c.p.flags = PBRS_BLOOM_MIX; }));
    ok("threshold +0", with([](Call& c) { c.p.threshold = 0.0f; }));
    ok("threshold -0", with([](Call& c) { c.p.threshold = -0.0f; }));
    ok("the smallest threshold above 0", with([](Call& c) { c.p.threshold = kDenorm; }));
    ok("the largest threshold", with([](Call& c) { c.p.threshold = kMax; }));
    ok("knee 0", with([](Call& c) { c.p.knee = 0.0f; }));
    ok("knee -0", with([](Call& c) { c.p.knee = -0.0f; }));
    ok("knee 1", with([](Call& c) { c.p.knee = 1.0f; }));
    ok("strength 0", with([](Call& c) { c.p.strength = 0.0f; }));
    ok("the largest strength without the flag", with([](Call& c) { c.p.strength = kMax; }));
    ok("strength 1 with the flag", with([](Call& c) { c.p.flags = PBRS_BLOOM_MIX, c.p.strength = 1.0f; }));
    ok("strength 0 with the flag", with([](Call& c) { c.p.flags = PBRS_BLOOM_MIX, c.p.strength = 0.0f; }));
    ok("spread 0", with([](Call& c) { c.p.spread = 0.0f; }));
    ok("spread 1", with([](Call& c) { c.p.spread = 1.0f; }));
    ok("in place", with([](Call& c) { c.rgb_out = const_cast<float*>(c.rgb); }));
    ok("one pixel", with([](Call& c) { c.p.w = 1, c.p.h = 1; }));
    ok("2^28 pixels", with([](Call& c) { c.p.w = 1u << 14, c.p.h = 1u << 14; }));
    ok("2^28 pixels in one row", with([](Call& c) { c.p.w = 1u << 28, c.p.h = 1; }));
    std::printf("accepted calls pass\n");
}

void check_precedence() {
    expect("null before empty", with([](Call& c) { c.rgb = nullptr, c.p.w = 0; }), PBRS_E_INVALID, kNull);
    expect("empty before the levels", with([](Call& c) { c.p.h = 0, c.p.levels = 9; }), PBRS_E_INVALID, kEmpty);
    expect("the levels before the flags", with([](Call& c) { c.p.levels = 0, c.p.flags = 4u; }), PBRS_E_INVALID, kLevels);
    expect("the flags before the threshold", with([](Call& c) { c.p.flags = 4u, c.p.threshold = kNaN; }), PBRS_E_INVALID, kFlags);
    expect("the threshold before the knee", with([](Call& c) { c.p.threshold = -1.0f, c.p.knee = 2.0f; }), PBRS_E_INVALID, kThreshold);
    expect("the knee before the strength", with([](Call& c) { c.p.knee = kNaN, c.p.strength = kNaN; }), PBRS_E_INVALID, kKnee);
    expect("the strength before the spread", with([](Call& c) { c.p.strength = -1.0f, c.p.spread = 2.0f; }), PBRS_E_INVALID, kStrength);
    expect("the spread before the flag's strength", with([](Call& c) { c.p.spread = 2.0f, c.p.flags = PBRS_BLOOM_MIX, c.p.strength = 2.0f; }), PBRS_E_INVALID, kSpread);
    expect("the flag's strength before the limit", with([](Call& c) { c.p.flags = PBRS_BLOOM_MIX, c.p.strength = 2.0f, c.p.w = c.p.h = 1u << 15; }), PBRS_E_INVALID, kMix);
    std::printf("precedence holds\n");
}

}  // namespace

int main(int argc, char** argv) {
    REQUIRE(argc == 2, "usage: bloom_check <path of host/arg_checks_bloom.cpp>");
    check_refusals(argv[1]);
    check_accepted();
    check_precedence();
    std::printf("ok\n");
    return 0;
}
