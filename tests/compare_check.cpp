// tests/compare_check.cpp — check_compare and pbrsx_compare_params_default (pbrs_amd/csrc/host/arg_checks.h, arg_checks_compare.cpp), the
// argument check and the filler of pbrsx_compare[_device], on a CPU: a program of its own that tests/test_compare_checks.py compiles
// with -fsanitize=address,undefined and runs, in the manner of tests/display_check.cpp.
//
//   usage: compare_check <path of host/arg_checks_compare.cpp>
//
// The call starts from a valid baseline with SSIM on and both maps; image planes are addresses that are never dereferenced.  Checked:
//   refusals     one row per refusal the header lists: the baseline with one defect, the code and the message; every `return refuse(`
//                site of the source has at least one row, and no row names a message the source does not have
//   accepted     the baseline, the filler's defaults and its bytes, both transforms, no maps and maps of NULLs, a == b, 2^28 pixels
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
pbrs_compare_result kResult;
const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

pbrs_compare_params defaults(uint32_t w, uint32_t h) {
    pbrs_compare_params p;
    std::memset(&p, 0xAB, sizeof p);  // the filler writes every byte
    pbrsx_compare_params_default(w, h, &p);
    return p;
}

// The baseline: every argument of the check by value, `run` the call.
struct Call {
    pbrs_compare_params p = defaults(13, 7);
    const float* a = kF;
    const float* b = kF + 1;
    pbrs_compare_maps maps{kF + 2, kF + 3};
    const pbrs_compare_result* result = &kResult;
    bool null_params = false, null_maps = false;
    Refusal run() const { return check_compare(null_params ? nullptr : &p, a, b, null_maps ? nullptr : &maps, result); }
};

struct Row {
    int code;
    const char* message;
    std::function<void(Call&)> mutate;
};

const char* const kNull = "null compare params, image, reference or result";
const char* const kEmpty = "empty image";
const char* const kTransform = "unknown compare transform";
const char* const kFlags = "unknown compare flag bits";
const char* const kEpsilon = "the compare rel_epsilon must be finite and > 0";
const char* const kPeak = "the compare peak must be finite and > 0";
const char* const kNeedsSsim = "the compare ssim map needs PBRS_COMPARE_SSIM";
const char* const kErrorAlias = "the compare error map cannot be an image's plane";
const char* const kSsimAlias = "the compare ssim map cannot be an image's plane";
const char* const kShared = "the compare maps cannot share a plane";
const char* const kPixels = "more than 2^28 pixels";

const std::vector<Row>& rows() {
    static const std::vector<Row> r = {
        {PBRS_E_INVALID, kNull, [](Call& c) { c.null_params = true; }},
        {PBRS_E_INVALID, kNull, [](Call& c) { c.a = nullptr; }},
        {PBRS_E_INVALID, kNull, [](Call& c) { c.b = nullptr; }},
        {PBRS_E_INVALID, kNull, [](Call& c) { c.result = nullptr; }},
        {PBRS_E_INVALID, kEmpty, [](Call& c) { c.p.w = 0; }},
        {PBRS_E_INVALID, kEmpty, [](Call& c) { c.p.h = 0; }},
        {PBRS_E_INVALID, kTransform, [](Call& c) { c.p.transform = PBRS_COMPARE_REINHARD + 1; }},
        {PBRS_E_INVALID, kTransform, [](Call& c) { c.p.transform = 0xFFFFFFFFu; }},
        {PBRS_E_INVALID, kFlags, [](Call& c) { c.p.flags = 2u; }},
        {PBRS_E_INVALID, kFlags, [](Call& c) { c.p.flags = 0x80000001u; }},
        {PBRS_E_INVALID, kEpsilon, [](Call& c) { c.p.rel_epsilon = 0.0f; }},
        {PBRS_E_INVALID, kEpsilon, [](Call& c) { c.p.rel_epsilon = -1e-2f; }},
        {PBRS_E_INVALID, kEpsilon, [](Call& c) { c.p.rel_epsilon = kInf; }},
        {PBRS_E_INVALID, kEpsilon, [](Call& c) { c.p.rel_epsilon = kNaN; }},
        {PBRS_E_INVALID, kPeak, [](Call& c) { c.p.peak = 0.0f; }},
        {PBRS_E_INVALID, kPeak, [](Call& c) { c.p.peak = -1.0f; }},
        {PBRS_E_INVALID, kPeak, [](Call& c) { c.p.peak = kInf; }},
        {PBRS_E_INVALID, kPeak, [](Call& c) { c.p.peak = kNaN; }},
        {PBRS_E_INVALID, kNeedsSsim, [](Call& c) { c.p.flags = 0; }},
        {PBRS_E_INVALID, kErrorAlias, [](Call& c) { c.maps.error_out = const_cast<float*>(c.a); }},
        {PBRS_E_INVALID, kErrorAlias, [](Call& c) { c.maps.error_out = const_cast<float*>(c.b); }},
        {PBRS_E_INVALID, kSsimAlias, [](Call& c) { c.maps.ssim_out = const_cast<float*>(c.a); }},
        {PBRS_E_INVALID, kSsimAlias, [](Call& c) { c.maps.ssim_out = const_cast<float*>(c.b); }},
        {PBRS_E_INVALID, kShared, [](Call& c) { c.maps.ssim_out = c.maps.error_out; }},
        {PBRS_E_LIMIT, kPixels, [](Call& c) { c.p.w = 1u << 15, c.p.h = (1u << 13) + 1u; }},
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
        const pbrs_compare_params d = defaults(1920, 1080);
        REQUIRE(d.w == 1920 && d.h == 1080 && d.transform == PBRS_COMPARE_REINHARD && d.flags == PBRS_COMPARE_SSIM && d.rel_epsilon == 1e-2f && d.peak == 1.0f &&
                    d.pad[0] == 0 && d.pad[1] == 0,
                "pbrsx_compare_params_default does not fill the documented values");
        // w, h, transform, flags, 1e-2f, 1.0f, two zero words: the filler's 32 bytes
        const uint32_t words[8] = {1920u, 1080u, 1u, 1u, 0x3C23D70Au, 0x3F800000u, 0u, 0u};
        REQUIRE(sizeof d == sizeof words && std::memcmp(&d, words, sizeof d) == 0, "pbrsx_compare_params_default does not write the documented bytes");
        pbrsx_compare_params_default(3, 4, nullptr);  // does nothing
        ok("the defaults", check_compare(&d, kF, kF + 1, nullptr, &kResult));
    }
    ok("no maps", with([](Call& c) { c.null_maps = true; }));
    ok("maps of NULLs", with([](Call& c) { c.maps = pbrs_compare_maps{}; }));
    ok("only the error map", with([](Call& c) { c.maps.ssim_out = nullptr; }));
    ok("only the ssim map", with([](Call& c) { c.maps.error_out = nullptr; }));
    ok("no ssim, the error map", with([](Call& c) { c.p.flags = 0, c.maps.ssim_out = nullptr; }));
    ok("no ssim, no maps", with([](Call& c) { c.p.flags = 0, c.null_maps = true; }));
    ok("linear", with([](Call& c) { c.p.transform = PBRS_COMPARE_LINEAR; }));
    ok("the image against itself", with([](Call& c) { c.b = c.a; }));
    ok("a large peak and a small epsilon", with([](Call& c) { c.p.peak = 65504.0f, c.p.rel_epsilon = 0x1p-100f; }));
    ok("2^28 pixels", with([](Call& c) { c.p.w = 1u << 14, c.p.h = 1u << 14; }));
    std::printf("accepted calls pass\n");
}

void check_precedence() {
    expect("null before empty", with([](Call& c) { c.a = nullptr, c.p.w = 0; }), PBRS_E_INVALID, kNull);
    expect("empty before the transform", with([](Call& c) { c.p.h = 0, c.p.transform = 9; }), PBRS_E_INVALID, kEmpty);
    expect("the transform before the flags", with([](Call& c) { c.p.transform = 9, c.p.flags = 4u; }), PBRS_E_INVALID, kTransform);
    expect("the flags before rel_epsilon", with([](Call& c) { c.p.flags = 4u, c.p.rel_epsilon = 0.0f; }), PBRS_E_INVALID, kFlags);
    expect("rel_epsilon before the peak", with([](Call& c) { c.p.rel_epsilon = kNaN, c.p.peak = kNaN; }), PBRS_E_INVALID, kEpsilon);
    expect("the peak before the maps", with([](Call& c) { c.p.peak = 0.0f, c.p.flags = 0; }), PBRS_E_INVALID, kPeak);
    expect("the missing flag before the aliasing", with([](Call& c) { c.p.flags = 0, c.maps.error_out = const_cast<float*>(c.a); }), PBRS_E_INVALID, kNeedsSsim);
    expect("the error map before the ssim map", with([](Call& c) { c.maps.error_out = const_cast<float*>(c.a), c.maps.ssim_out = const_cast<float*>(c.b); }),
           PBRS_E_INVALID, kErrorAlias);
    expect("an image's plane before the shared plane", with([](Call& c) { c.maps.error_out = c.maps.ssim_out = const_cast<float*>(c.b); }), PBRS_E_INVALID,
           kErrorAlias);
    expect("the aliasing before the limit", with([](Call& c) { c.maps.ssim_out = c.maps.error_out, c.p.w = c.p.h = 1u << 15; }), PBRS_E_INVALID, kShared);
    std::printf("precedence holds\n");
}

}  // namespace

int main(int argc, char** argv) {
    REQUIRE(argc == 2, "usage: compare_check <path of host/arg_checks_compare.cpp>");
    check_refusals(argv[1]);
    check_accepted();
    check_precedence();
    std::printf("ok\n");
    return 0;
}
