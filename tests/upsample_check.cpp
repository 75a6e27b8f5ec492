// tests/upsample_check.cpp — check_upsample and pbrs_upsample_params_default (pbrs_amd/csrc/host/arg_checks.h, arg_checks_upsample.cpp),
// the argument check and the filler of pbrs_upsample[_device], on a CPU: a program of its own that tests/test_upsample_checks.py compiles
// with -fsanitize=address,undefined and runs, in the manner of tests/display_check.cpp.
//
//   usage: upsample_check <path of host/arg_checks_upsample.cpp>
//
// The call starts from a valid baseline with every guide pair and both flags; image planes are addresses that are never dereferenced.
// Checked:
//   refusals     one row per refusal the header lists: the baseline with one defect, the code and the message; every `return refuse(`
//                site of the source has at least one row, and no row names a message the source does not have
//   accepted     the baseline, the filler's defaults, the edges of the ranges, no guides, each pair alone, no weight_out
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
float kF[16];
uint32_t kU[4];
const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

pbrs_upsample_params defaults(uint32_t w, uint32_t h, uint32_t factor) {
    pbrs_upsample_params p;
    std::memset(&p, 0xAB, sizeof p);  // the filler writes every byte
    pbrs_upsample_params_default(w, h, factor, &p);
    return p;
}

// The baseline: every argument of the check by value, `run` the call.
struct Call {
    pbrs_upsample_params p = defaults(13, 7, 2);
    const float* rgb_lo = kF;
    pbrs_denoise_guides lo{kF + 1, kF + 2, kF + 3, kU};
    pbrs_denoise_guides hi{kF + 4, kF + 5, kF + 6, kU + 1};
    float* out = kF + 7;
    float* weight_out = kF + 8;
    bool null_params = false, null_lo = false, null_hi = false;
    Call() { p.flags = PBRS_UPSAMPLE_DEMODULATE | PBRS_UPSAMPLE_ID_STOP; }
    Refusal run() const { return check_upsample(null_params ? nullptr : &p, rgb_lo, null_lo ? nullptr : &lo, null_hi ? nullptr : &hi, out, weight_out); }
};

struct Row {
    int code;
    const char* message;
    std::function<void(Call&)> mutate;
};

const char* const kNull = "null upsample params, image, guides or output";
const char* const kEmpty = "empty image";
const char* const kFactor = "the upsample factor must be 2 .. 4";
const char* const kRadius = "the upsample radius must be 1 .. 2";
const char* const kSigma = "an upsample sigma must be finite and > 0";
const char* const kFloor = "the albedo floor must be finite and >= 0";
const char* const kMinWeight = "the upsample min_weight must be finite and >= 0";
const char* const kFlags = "unknown upsample flag bits";
const char* const kPair = "a guide given at only one of the two resolutions";
const char* const kDemodulate = "PBRS_UPSAMPLE_DEMODULATE without the albedo guides";
const char* const kIdStop = "PBRS_UPSAMPLE_ID_STOP without the instance guides";
const char* const kAlias = "the upsampled image cannot be written over an input plane";
const char* const kWeightAlias = "weight_out cannot be the output's or an input's plane";
const char* const kPixels = "more than 2^28 pixels";

float* plane(const void* p) { return static_cast<float*>(const_cast<void*>(p)); }

const std::vector<Row>& rows() {
    static const std::vector<Row> r = {
        {PBRS_E_INVALID, kNull, [](Call& a) { a.null_params = true; }},
        {PBRS_E_INVALID, kNull, [](Call& a) { a.rgb_lo = nullptr; }},
        {PBRS_E_INVALID, kNull, [](Call& a) { a.null_lo = true; }},
        {PBRS_E_INVALID, kNull, [](Call& a) { a.null_hi = true; }},
        {PBRS_E_INVALID, kNull, [](Call& a) { a.out = nullptr; }},
        {PBRS_E_INVALID, kEmpty, [](Call& a) { a.p.w = 0; }},
        {PBRS_E_INVALID, kEmpty, [](Call& a) { a.p.h = 0; }},
        {PBRS_E_INVALID, kFactor, [](Call& a) { a.p.factor = 0; }},
        {PBRS_E_INVALID, kFactor, [](Call& a) { a.p.factor = 1; }},
        {PBRS_E_INVALID, kFactor, [](Call& a) { a.p.factor = 5; }},
        {PBRS_E_INVALID, kRadius, [](Call& a) { a.p.radius = 0; }},
        {PBRS_E_INVALID, kRadius, [](Call& a) { a.p.radius = 3; }},
        {PBRS_E_INVALID, kSigma, [](Call& a) { a.p.sigma_normal = 0.0f; }},
        {PBRS_E_INVALID, kSigma, [](Call& a) { a.p.sigma_normal = kNaN; }},
        {PBRS_E_INVALID, kSigma, [](Call& a) { a.p.sigma_depth = -1.0f; }},
        {PBRS_E_INVALID, kSigma, [](Call& a) { a.p.sigma_depth = kInf; }},
        {PBRS_E_INVALID, kFloor, [](Call& a) { a.p.albedo_floor = -1e-3f; }},
        {PBRS_E_INVALID, kFloor, [](Call& a) { a.p.albedo_floor = kInf; }},
        {PBRS_E_INVALID, kFloor, [](Call& a) { a.p.albedo_floor = kNaN; }},
        {PBRS_E_INVALID, kMinWeight, [](Call& a) { a.p.min_weight = -1.0f; }},
        {PBRS_E_INVALID, kMinWeight, [](Call& a) { a.p.min_weight = kInf; }},
        {PBRS_E_INVALID, kMinWeight, [](Call& a) { a.p.min_weight = kNaN; }},
        {PBRS_E_INVALID, kFlags, [](Call& a) { a.p.flags = 4u; }},
        {PBRS_E_INVALID, kFlags, [](Call& a) { a.p.flags = 0x80000003u; }},
        {PBRS_E_INVALID, kPair, [](Call& a) { a.lo.albedo = nullptr; }},
        {PBRS_E_INVALID, kPair, [](Call& a) { a.hi.normal = nullptr; }},
        {PBRS_E_INVALID, kPair, [](Call& a) { a.lo.depth = nullptr; }},
        {PBRS_E_INVALID, kPair, [](Call& a) { a.hi.instance = nullptr; }},
        {PBRS_E_INVALID, kPair, [](Call& a) { a.p.flags = 0, a.hi.albedo = nullptr; }},  // a pair is a pair whatever the flags read
        {PBRS_E_INVALID, kDemodulate, [](Call& a) { a.lo.albedo = a.hi.albedo = nullptr; }},
        {PBRS_E_INVALID, kIdStop, [](Call& a) { a.lo.instance = a.hi.instance = nullptr; }},
        {PBRS_E_INVALID, kAlias, [](Call& a) { a.out = plane(a.rgb_lo); }},
        {PBRS_E_INVALID, kAlias, [](Call& a) { a.out = plane(a.lo.albedo); }},
        {PBRS_E_INVALID, kAlias, [](Call& a) { a.out = plane(a.lo.normal); }},
        {PBRS_E_INVALID, kAlias, [](Call& a) { a.out = plane(a.lo.depth); }},
        {PBRS_E_INVALID, kAlias, [](Call& a) { a.out = plane(a.lo.instance); }},
        {PBRS_E_INVALID, kAlias, [](Call& a) { a.out = plane(a.hi.albedo); }},
        {PBRS_E_INVALID, kAlias, [](Call& a) { a.out = plane(a.hi.normal); }},
        {PBRS_E_INVALID, kAlias, [](Call& a) { a.out = plane(a.hi.depth); }},
        {PBRS_E_INVALID, kAlias, [](Call& a) { a.out = plane(a.hi.instance); }},
        {PBRS_E_INVALID, kWeightAlias, [](Call& a) { a.weight_out = a.out; }},
        {PBRS_E_INVALID, kWeightAlias, [](Call& a) { a.weight_out = plane(a.rgb_lo); }},
        {PBRS_E_INVALID, kWeightAlias, [](Call& a) { a.weight_out = plane(a.hi.depth); }},
        {PBRS_E_INVALID, kWeightAlias, [](Call& a) { a.weight_out = plane(a.lo.instance); }},
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
        const pbrs_upsample_params d = defaults(1920, 1080, 3);  // the documented defaults, and they pass without any guide
        REQUIRE(d.w == 1920 && d.h == 1080 && d.factor == 3 && d.radius == 1 && d.flags == 0 && d.sigma_normal == 0.3f && d.sigma_depth == 0.2f &&
                    d.albedo_floor == 1e-3f && d.min_weight == 1e-3f && d.pad[0] == 0 && d.pad[1] == 0 && d.pad[2] == 0,
                "pbrs_upsample_params_default does not fill the documented values");
        pbrs_upsample_params_default(3, 4, 2, nullptr);  // does nothing
        const pbrs_denoise_guides none{};
        ok("the defaults", check_upsample(&d, kF, &none, &none, kF + 7, nullptr));
    }
    ok("no weight_out", with([](Call& a) { a.weight_out = nullptr; }));
    ok("every factor and radius", with([](Call& a) { a.p.factor = 4, a.p.radius = 2; }));
    ok("factor 3", with([](Call& a) { a.p.factor = 3; }));
    ok("the albedo pair alone", with([](Call& a) {
           a.p.flags = PBRS_UPSAMPLE_DEMODULATE;
           a.lo.normal = a.hi.normal = a.lo.depth = a.hi.depth = nullptr, a.lo.instance = a.hi.instance = nullptr;
       }));
    ok("the instance pair alone", with([](Call& a) {
           a.p.flags = PBRS_UPSAMPLE_ID_STOP;
           a.lo.normal = a.hi.normal = a.lo.depth = a.hi.depth = a.lo.albedo = a.hi.albedo = nullptr;
       }));
    ok("pairs given and their flags off", with([](Call& a) { a.p.flags = 0; }));
    ok("a floor and a min_weight of 0", with([](Call& a) { a.p.albedo_floor = 0.0f, a.p.min_weight = 0.0f; }));
    ok("a huge min_weight", with([](Call& a) { a.p.min_weight = 1e30f; }));
    ok("a 1 x 1 image", with([](Call& a) { a.p.w = a.p.h = 1; }));
    ok("2^28 pixels", with([](Call& a) { a.p.w = 1u << 14, a.p.h = 1u << 14; }));
    std::printf("accepted calls pass\n");
}

void check_precedence() {
    expect("null before empty", with([](Call& a) { a.rgb_lo = nullptr, a.p.w = 0; }), PBRS_E_INVALID, kNull);
    expect("empty before the factor", with([](Call& a) { a.p.h = 0, a.p.factor = 9; }), PBRS_E_INVALID, kEmpty);
    expect("the factor before the radius", with([](Call& a) { a.p.factor = 9, a.p.radius = 9; }), PBRS_E_INVALID, kFactor);
    expect("the radius before the sigmas", with([](Call& a) { a.p.radius = 0, a.p.sigma_depth = 0.0f; }), PBRS_E_INVALID, kRadius);
    expect("the sigmas before the floor", with([](Call& a) { a.p.sigma_normal = kNaN, a.p.albedo_floor = kNaN; }), PBRS_E_INVALID, kSigma);
    expect("the floor before min_weight", with([](Call& a) { a.p.albedo_floor = -1.0f, a.p.min_weight = -1.0f; }), PBRS_E_INVALID, kFloor);
    expect("min_weight before the flags", with([](Call& a) { a.p.min_weight = kNaN, a.p.flags = 8u; }), PBRS_E_INVALID, kMinWeight);
    expect("the flags before the pairs", with([](Call& a) { a.p.flags = 8u, a.lo.depth = nullptr; }), PBRS_E_INVALID, kFlags);
    expect("the pairs before the flags' guides", with([](Call& a) { a.lo.albedo = nullptr, a.lo.instance = a.hi.instance = nullptr; }), PBRS_E_INVALID, kPair);
    expect("demodulation before the id stop", with([](Call& a) { a.lo.albedo = a.hi.albedo = nullptr, a.lo.instance = a.hi.instance = nullptr; }),
           PBRS_E_INVALID, kDemodulate);
    expect("the id stop before the aliasing", with([](Call& a) { a.lo.instance = a.hi.instance = nullptr, a.out = plane(a.rgb_lo); }), PBRS_E_INVALID, kIdStop);
    expect("out before weight_out", with([](Call& a) { a.out = plane(a.rgb_lo), a.weight_out = plane(a.rgb_lo); }), PBRS_E_INVALID, kAlias);
    expect("the aliasing before the limit", with([](Call& a) { a.weight_out = a.out, a.p.w = a.p.h = 1u << 15; }), PBRS_E_INVALID, kWeightAlias);
    std::printf("precedence holds\n");
}

}  // namespace

int main(int argc, char** argv) {
    REQUIRE(argc == 2, "usage: upsample_check <path of host/arg_checks_upsample.cpp>");
    check_refusals(argv[1]);
    check_accepted();
    check_precedence();
    std::printf("ok\n");
    return 0;
}
