// tests/display_check.cpp — check_display and pbrs_display_params_default (pbrs_amd/csrc/host/arg_checks.h, arg_checks_display.cpp), the
// argument check and the filler of pbrs_display[_device], on a CPU: a program of its own that tests/test_display_checks.py compiles
// with -fsanitize=address,undefined and runs, in the manner of tests/history_clip_check.cpp.
//
//   usage: display_check <path of host/arg_checks_display.cpp>
//
// The call starts from a valid baseline with the auto exposure on; image planes are addresses that are never dereferenced.  Checked:
//   refusals     one row per refusal the header lists: the baseline with one defect, the code and the message; every `return refuse(`
//                site of the source has at least one row, and no row names a message the source does not have
//   accepted     the baseline, the filler's defaults, the edges of the ranges, +inf as white, no io and an io of NULLs
//   auto only    key, the exposure limits, adapt and the ranks are not read without PBRS_DISPLAY_AUTO_EXPOSURE
//   precedence   the order of the refusals
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
float kF[8];
uint32_t kU[8];
const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

pbrs_display_params defaults(uint32_t w, uint32_t h) {
    pbrs_display_params p;
    std::memset(&p, 0xAB, sizeof p);  // the filler writes every byte
    pbrs_display_params_default(w, h, &p);
    return p;
}

// The baseline: every argument of the check by value, `run` the call.
struct Call {
    pbrs_display_params p = defaults(13, 7);
    const float* rgb = kF;
    uint32_t* out = kU;
    pbrs_display_io io{kF + 1, kF + 2, kU + 1};
    bool null_params = false, null_io = false;
    Call() { p.flags = PBRS_DISPLAY_AUTO_EXPOSURE; }
    Refusal run() const { return check_display(null_params ? nullptr : &p, rgb, null_io ? nullptr : &io, out); }
};

struct Row {
    int code;
    const char* message;
    std::function<void(Call&)> mutate;
};

const char* const kNull = "null display params, image or output";
const char* const kEmpty = "empty image";
const char* const kCurve = "unknown display curve";
const char* const kEncode = "unknown display encode";
const char* const kQuantize = "unknown display quantize";
const char* const kFlags = "unknown display flag bits";
const char* const kExposure = "the display exposure must be finite and > 0";
const char* const kWhite = "the display white must be > 0 (+inf: plain Reinhard)";
const char* const kKey = "the display key must be finite and > 0";
const char* const kLimits = "the display exposure limits must be finite with 0 < min <= max";
const char* const kAdapt = "the display adapt must be in (0, 1]";
const char* const kRanks = "the display ranks need low_q16 < high_q16 <= 65536";
const char* const kAlias = "the display output cannot be the image's plane";
const char* const kPixels = "more than 2^28 pixels";

const std::vector<Row>& rows() {
    static const std::vector<Row> r = {
        {PBRS_E_INVALID, kNull, [](Call& a) { a.null_params = true; }},
        {PBRS_E_INVALID, kNull, [](Call& a) { a.rgb = nullptr; }},
        {PBRS_E_INVALID, kNull, [](Call& a) { a.out = nullptr; }},
        {PBRS_E_INVALID, kEmpty, [](Call& a) { a.p.w = 0; }},
        {PBRS_E_INVALID, kEmpty, [](Call& a) { a.p.h = 0; }},
        {PBRS_E_INVALID, kCurve, [](Call& a) { a.p.curve = PBRS_CURVE_ACES + 1; }},
        {PBRS_E_INVALID, kEncode, [](Call& a) { a.p.encode = PBRS_ENCODE_SRGB + 1; }},
        {PBRS_E_INVALID, kQuantize, [](Call& a) { a.p.quantize = PBRS_QUANT_DITHER + 1; }},
        {PBRS_E_INVALID, kFlags, [](Call& a) { a.p.flags = 2u; }},
        {PBRS_E_INVALID, kFlags, [](Call& a) { a.p.flags = 0x80000001u; }},
        {PBRS_E_INVALID, kExposure, [](Call& a) { a.p.exposure = 0.0f; }},
        {PBRS_E_INVALID, kExposure, [](Call& a) { a.p.exposure = -1.0f; }},
        {PBRS_E_INVALID, kExposure, [](Call& a) { a.p.exposure = kInf; }},
        {PBRS_E_INVALID, kExposure, [](Call& a) { a.p.exposure = kNaN; }},
        {PBRS_E_INVALID, kWhite, [](Call& a) { a.p.white = 0.0f; }},
        {PBRS_E_INVALID, kWhite, [](Call& a) { a.p.white = -2.0f; }},
        {PBRS_E_INVALID, kWhite, [](Call& a) { a.p.white = kNaN; }},
        {PBRS_E_INVALID, kKey, [](Call& a) { a.p.key = 0.0f; }},
        {PBRS_E_INVALID, kKey, [](Call& a) { a.p.key = kInf; }},
        {PBRS_E_INVALID, kKey, [](Call& a) { a.p.key = kNaN; }},
        {PBRS_E_INVALID, kLimits, [](Call& a) { a.p.min_exposure = 0.0f; }},
        {PBRS_E_INVALID, kLimits, [](Call& a) { a.p.min_exposure = kNaN; }},
        {PBRS_E_INVALID, kLimits, [](Call& a) { a.p.max_exposure = kInf; }},
        {PBRS_E_INVALID, kLimits, [](Call& a) { a.p.max_exposure = -1.0f; }},
        {PBRS_E_INVALID, kLimits, [](Call& a) { a.p.min_exposure = 2.0f, a.p.max_exposure = 1.0f; }},
        {PBRS_E_INVALID, kAdapt, [](Call& a) { a.p.adapt = 0.0f; }},
        {PBRS_E_INVALID, kAdapt, [](Call& a) { a.p.adapt = 1.5f; }},
        {PBRS_E_INVALID, kAdapt, [](Call& a) { a.p.adapt = kNaN; }},
        {PBRS_E_INVALID, kRanks, [](Call& a) { a.p.low_q16 = a.p.high_q16; }},
        {PBRS_E_INVALID, kRanks, [](Call& a) { a.p.low_q16 = 70000u, a.p.high_q16 = 60000u; }},
        {PBRS_E_INVALID, kRanks, [](Call& a) { a.p.high_q16 = 65537u; }},
        {PBRS_E_INVALID, kAlias, [](Call& a) { a.out = reinterpret_cast<uint32_t*>(const_cast<float*>(a.rgb)); }},
        {PBRS_E_LIMIT, kPixels, [](Call& a) { a.p.w = 1u << 15, a.p.h = (1u << 13) + 1u; }},
    };
    return r;
}

void expect(const char* what, const Refusal& r, int code, const char* message) {
    REQUIRE(r.code == code && (code == PBRS_OK ? r.message == nullptr : r.message && std::strcmp(r.message, message) == 0), "%s: got %d \"%s\", expected %d \"%s\"", what,
            r.code, r.message ? r.message : "(accepted)", code, message ? message : "(accepted)");
}

template <class Mutate>
Refusal with(Mutate mutate) {
    Call a;
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
        const pbrs_display_params d = defaults(1920, 1080);  // the documented defaults, and they pass with and without the auto exposure
        REQUIRE(d.w == 1920 && d.h == 1080 && d.curve == PBRS_CURVE_ACES && d.encode == PBRS_ENCODE_SRGB && d.quantize == PBRS_QUANT_ROUND && d.flags == 0 &&
                    d.exposure == 1.0f && d.key == 0.18f && d.white == kInf && d.min_exposure == 0x1p-20f && d.max_exposure == 0x1p20f && d.adapt == 1.0f &&
                    d.low_q16 == 6554u && d.high_q16 == 62259u && d.pad[0] == 0 && d.pad[1] == 0,
                "pbrs_display_params_default does not fill the documented values");
        pbrs_display_params_default(3, 4, nullptr);  // does nothing
        ok("the defaults", check_display(&d, kF, nullptr, kU));
    }
    ok("no io", with([](Call& a) { a.null_io = true; }));
    ok("an io of NULLs", with([](Call& a) { a.io = pbrs_display_io{}; }));
    ok("exposure_out on exposure_in", with([](Call& a) { a.io.exposure_out = const_cast<float*>(a.io.exposure_in); }));
    ok("every curve, encode and quantize", with([](Call& a) { a.p.curve = PBRS_CURVE_NONE, a.p.encode = PBRS_ENCODE_SQRT, a.p.quantize = PBRS_QUANT_TRUNC; }));
    ok("reinhard, dither", with([](Call& a) { a.p.curve = PBRS_CURVE_REINHARD, a.p.quantize = PBRS_QUANT_DITHER; }));
    ok("white +inf", with([](Call& a) { a.p.white = kInf; }));
    ok("a finite white", with([](Call& a) { a.p.white = 4.0f; }));
    ok("min_exposure == max_exposure", with([](Call& a) { a.p.min_exposure = a.p.max_exposure = 2.0f; }));
    ok("adapt 1", with([](Call& a) { a.p.adapt = 1.0f; }));
    ok("a small adapt", with([](Call& a) { a.p.adapt = 0x1p-20f; }));
    ok("all ranks", with([](Call& a) { a.p.low_q16 = 0, a.p.high_q16 = 65536u; }));
    ok("2^28 pixels", with([](Call& a) { a.p.w = 1u << 14, a.p.h = 1u << 14; }));
    std::printf("accepted calls pass\n");
}

void check_auto_only() {
    // without the flag, what only the auto exposure reads may hold anything
    const Refusal r = with([](Call& a) {
        a.p.flags = 0;
        a.p.key = kNaN, a.p.min_exposure = -1.0f, a.p.max_exposure = kInf, a.p.adapt = 7.0f, a.p.low_q16 = 9u, a.p.high_q16 = 3u;
    });
    expect("the auto exposure's fields without the flag", r, PBRS_OK, nullptr);
    // ... while exposure and white are read either way
    expect("exposure without the flag", with([](Call& a) { a.p.flags = 0, a.p.exposure = kNaN; }), PBRS_E_INVALID, kExposure);
    expect("white without the flag", with([](Call& a) { a.p.flags = 0, a.p.white = 0.0f; }), PBRS_E_INVALID, kWhite);
    std::printf("auto-only fields are ignored without the flag\n");
}

void check_precedence() {
    expect("null before empty", with([](Call& a) { a.rgb = nullptr, a.p.w = 0; }), PBRS_E_INVALID, kNull);
    expect("empty before the curve", with([](Call& a) { a.p.h = 0, a.p.curve = 9; }), PBRS_E_INVALID, kEmpty);
    expect("the curve before the encode", with([](Call& a) { a.p.curve = 9, a.p.encode = 9; }), PBRS_E_INVALID, kCurve);
    expect("the flags before the exposure", with([](Call& a) { a.p.flags = 4u, a.p.exposure = 0.0f; }), PBRS_E_INVALID, kFlags);
    expect("white before the key", with([](Call& a) { a.p.white = kNaN, a.p.key = kNaN; }), PBRS_E_INVALID, kWhite);
    expect("the key before the ranks", with([](Call& a) { a.p.key = -1.0f, a.p.high_q16 = 0; }), PBRS_E_INVALID, kKey);
    expect("the ranks before the aliasing", with([](Call& a) { a.p.high_q16 = 0, a.out = reinterpret_cast<uint32_t*>(const_cast<float*>(a.rgb)); }), PBRS_E_INVALID,
           kRanks);
    expect("the aliasing before the limit", with([](Call& a) { a.out = reinterpret_cast<uint32_t*>(const_cast<float*>(a.rgb)), a.p.w = a.p.h = 1u << 15; }),
           PBRS_E_INVALID, kAlias);
    std::printf("precedence holds\n");
}

}  // namespace

int main(int argc, char** argv) {
    REQUIRE(argc == 2, "usage: display_check <path of host/arg_checks_display.cpp>");
    check_refusals(argv[1]);
    check_accepted();
    check_auto_only();
    check_precedence();
    std::printf("ok\n");
    return 0;
}
