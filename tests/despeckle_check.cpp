// tests/despeckle_check.cpp — check_despeckle and pbrsi_despeckle_params_default (pbrs_amd/csrc/host/arg_checks.h,
// arg_checks_despeckle.cpp), the argument check and the filler of pbrsi_despeckle[_device], on a CPU: a program of its own that
// tests/test_despeckle_checks.py compiles with -fsanitize=address,undefined and runs, in the manner of tests/compare_check.cpp.
//
//   usage: despeckle_check <path of host/arg_checks_despeckle.cpp>
//
// The call starts from a valid baseline with every optional plane; planes are addresses that are never dereferenced.  Checked:
//   refusals     one row per refusal the header lists, and per boundary value on its refusing side: the baseline with one defect, the
//                code and the message; every `return refuse(` site of the source has at least one row, and no row names a message the
//                source does not have
//   accepted     the baseline, the filler's defaults and its bytes, each boundary value on its accepting side, every subset of the
//                optional planes, the variance in place, 2^28 pixels
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
float kF[8];
uint32_t kU[2];
const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();
const float kMax = std::numeric_limits<float>::max(), kDenorm = std::numeric_limits<float>::denorm_min();

pbrs_despeckle_params defaults(uint32_t w, uint32_t h) {
    pbrs_despeckle_params p;
    std::memset(&p, 0xAB, sizeof p);  // the filler writes every byte
    pbrsi_despeckle_params_default(w, h, &p);
    return p;
}

// The baseline: every argument of the check by value, `run` the call.
struct Call {
    pbrs_despeckle_params p = defaults(13, 7);
    pbrs_despeckle_io io{kF, kF + 1, kF + 2, kF + 3, kU, kF + 4};
    bool null_params = false, null_io = false;
    Refusal run() const { return check_despeckle(null_params ? nullptr : &p, null_io ? nullptr : &io); }
};

struct Row {
    int code;
    const char* message;
    std::function<void(Call&)> mutate;
};

const char* const kNull = "null despeckle params, io, rgb_in or rgb_out";
const char* const kEmpty = "empty image";
const char* const kRadius = "the despeckle radius must be 1 or 2";
const char* const kRank = "the despeckle rank must be 1 .. 4";
const char* const kGain = "the despeckle gain must be finite and >= 1";
const char* const kFloor = "the despeckle floor must be finite and >= 0";
const char* const kFlags = "unknown despeckle flag bits";
const char* const kPair = "the despeckle variance planes come as a pair";
const char* const kInPlace = "despeckle reads neighbours: rgb_out cannot be rgb_in";
const char* const kInput = "a despeckle output plane cannot be an input plane";
const char* const kShared = "the despeckle output planes cannot share a plane";
const char* const kPixels = "more than 2^28 pixels";

float* out_of(const float* p) { return const_cast<float*>(p); }

const std::vector<Row>& rows() {
    static const std::vector<Row> r = {
        {PBRS_E_INVALID, kNull, [](Call& c) { c.null_params = true; }},
        {PBRS_E_INVALID, kNull, [](Call& c) { c.null_io = true; }},
        {PBRS_E_INVALID, kNull, [](Call& c) { c.io.rgb_in = nullptr; }},
        {PBRS_E_INVALID, kNull, [](Call& c) { c.io.rgb_out = nullptr; }},
        {PBRS_E_INVALID, kEmpty, [](Call& c) { c.p.w = 0; }},
        {PBRS_E_INVALID, kEmpty, [](Call& c) { c.p.h = 0; }},
        {PBRS_E_INVALID, kRadius, [](Call& c) { c.p.radius = 0; }},
        {PBRS_E_INVALID, kRadius, [](Call& c) { c.p.radius = 3; }},
        {PBRS_E_INVALID, kRadius, [](Call& c) { c.p.radius = 0xFFFFFFFFu; }},
        {PBRS_E_INVALID, kRank, [](Call& c) { c.p.rank = 0; }},
        {PBRS_E_INVALID, kRank, [](Call& c) { c.p.rank = 5; }},
        {PBRS_E_INVALID, kRank, [](Call& c) { c.p.rank = 0x80000001u; }},
        {PBRS_E_INVALID, kGain, [](Call& c) { c.p.gain = std::nextafter(1.0f, 0.0f); }},
        {PBRS_E_INVALID, kGain, [](Call& c) { c.p.gain = 0.0f; }},
        {PBRS_E_INVALID, kGain, [](Call& c) { c.p.gain = -2.0f; }},
        {PBRS_E_INVALID, kGain, [](Call& c) { c.p.gain = kInf; }},
        {PBRS_E_INVALID, kGain, [](Call& c) { c.p.gain = kNaN; }},
        {PBRS_E_INVALID, kFloor, [](Call& c) { c.p.floor = -kDenorm; }},
        {PBRS_E_INVALID, kFloor, [](Call& c) { c.p.floor = -1.0f; }},
        {PBRS_E_INVALID, kFloor, [](Call& c) { c.p.floor = kInf; }},
        {PBRS_E_INVALID, kFloor, [](Call& c) { c.p.floor = -kInf; }},
        {PBRS_E_INVALID, kFloor, [](Call& c) { c.p.floor = kNaN; }},
        {PBRS_E_INVALID, kFlags, [](Call& c) { c.p.flags = 1u; }},
        {PBRS_E_INVALID, kFlags, [](Call& c) { c.p.flags = 0x80000000u; }},
        {PBRS_E_INVALID, kPair, [](Call& c) { c.io.variance_in = nullptr; }},
        {PBRS_E_INVALID, kPair, [](Call& c) { c.io.variance_out = nullptr; }},
        {PBRS_E_INVALID, kInPlace, [](Call& c) { c.io.rgb_out = out_of(c.io.rgb_in); }},
        {PBRS_E_INVALID, kInput, [](Call& c) { c.io.rgb_out = out_of(c.io.variance_in); }},
        {PBRS_E_INVALID, kInput, [](Call& c) { c.io.variance_out = out_of(c.io.rgb_in); }},
        {PBRS_E_INVALID, kInput, [](Call& c) { c.io.mask_out = reinterpret_cast<uint32_t*>(out_of(c.io.rgb_in)); }},
        {PBRS_E_INVALID, kInput, [](Call& c) { c.io.mask_out = reinterpret_cast<uint32_t*>(out_of(c.io.variance_in)); }},
        {PBRS_E_INVALID, kInput, [](Call& c) { c.io.removed_out = out_of(c.io.rgb_in); }},
        {PBRS_E_INVALID, kInput, [](Call& c) { c.io.removed_out = out_of(c.io.variance_in); }},
        {PBRS_E_INVALID, kShared, [](Call& c) { c.io.variance_out = c.io.rgb_out; }},
        {PBRS_E_INVALID, kShared, [](Call& c) { c.io.mask_out = reinterpret_cast<uint32_t*>(c.io.rgb_out); }},
        {PBRS_E_INVALID, kShared, [](Call& c) { c.io.removed_out = c.io.rgb_out; }},
        {PBRS_E_INVALID, kShared, [](Call& c) { c.io.mask_out = reinterpret_cast<uint32_t*>(c.io.variance_out); }},
        {PBRS_E_INVALID, kShared, [](Call& c) { c.io.removed_out = c.io.variance_out; }},
        {PBRS_E_INVALID, kShared, [](Call& c) { c.io.removed_out = reinterpret_cast<float*>(c.io.mask_out); }},
        // in place on the variance, and another output on the same plane
        {PBRS_E_INVALID, kShared, [](Call& c) { c.io.variance_out = out_of(c.io.variance_in), c.io.removed_out = c.io.variance_out; }},
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
        const pbrs_despeckle_params d = defaults(1920, 1080);
        REQUIRE(d.w == 1920 && d.h == 1080 && d.radius == 1 && d.rank == 2 && d.gain == 2.0f && d.floor == 0.0f && d.flags == 0 && d.pad == 0,
                "pbrsi_despeckle_params_default does not fill the documented values");
        // w, h, radius, rank, 2.0f, +0.0f, flags, pad: the filler's 32 bytes
        const uint32_t words[8] = {1920u, 1080u, 1u, 2u, 0x40000000u, 0u, 0u, 0u};
        REQUIRE(sizeof d == sizeof words && std::memcmp(&d, words, sizeof d) == 0, "pbrsi_despeckle_params_default does not write the documented bytes");
        pbrsi_despeckle_params_default(3, 4, nullptr);  // does nothing
        const pbrs_despeckle_io io{kF, kF + 1, nullptr, nullptr, nullptr, nullptr};
        ok("the defaults", check_despeckle(&d, &io));
    }
    for (uint32_t radius = 1; radius <= PBRS_DESPECKLE_MAX_RADIUS; ++radius) ok("a radius", with([&](Call& c) { c.p.radius = radius; }));
    for (uint32_t rank = 1; rank <= PBRS_DESPECKLE_MAX_RANK; ++rank) ok("a rank", with([&](Call& c) { c.p.rank = rank; }));
    ok("gain 1", with([](Call& c) { c.p.gain = 1.0f; }));
    ok("the largest gain", with([](Call& c) { c.p.gain = kMax; }));
    ok("floor +0", with([](Call& c) { c.p.floor = 0.0f; }));
    ok("floor -0", with([](Call& c) { c.p.floor = -0.0f; }));
    ok("the smallest floor above 0", with([](Call& c) { c.p.floor = kDenorm; }));
    ok("the largest floor", with([](Call& c) { c.p.floor = kMax; }));
    for (unsigned subset = 0; subset < 8; ++subset)  // every subset of {the variance pair, the mask, the removed energy}
        ok("a subset of the optional planes", with([&](Call& c) {
               if (!(subset & 1u)) c.io.variance_in = nullptr, c.io.variance_out = nullptr;
               if (!(subset & 2u)) c.io.mask_out = nullptr;
               if (!(subset & 4u)) c.io.removed_out = nullptr;
           }));
    ok("the variance in place", with([](Call& c) { c.io.variance_out = out_of(c.io.variance_in); }));
    ok("one pixel", with([](Call& c) { c.p.w = 1, c.p.h = 1; }));
    ok("2^28 pixels", with([](Call& c) { c.p.w = 1u << 14, c.p.h = 1u << 14; }));
    ok("2^28 pixels in one row", with([](Call& c) { c.p.w = 1u << 28, c.p.h = 1; }));
    std::printf("accepted calls pass\n");
}

void check_precedence() {
    expect("null before empty", with([](Call& c) { c.io.rgb_in = nullptr, c.p.w = 0; }), PBRS_E_INVALID, kNull);
    expect("empty before the radius", with([](Call& c) { c.p.h = 0, c.p.radius = 9; }), PBRS_E_INVALID, kEmpty);
    expect("the radius before the rank", with([](Call& c) { c.p.radius = 0, c.p.rank = 0; }), PBRS_E_INVALID, kRadius);
    expect("the rank before the gain", with([](Call& c) { c.p.rank = 5, c.p.gain = 0.5f; }), PBRS_E_INVALID, kRank);
    expect("the gain before the floor", with([](Call& c) { c.p.gain = kNaN, c.p.floor = kNaN; }), PBRS_E_INVALID, kGain);
    expect("the floor before the flags", with([](Call& c) { c.p.floor = -1.0f, c.p.flags = 4u; }), PBRS_E_INVALID, kFloor);
    expect("the flags before the pair", with([](Call& c) { c.p.flags = 4u, c.io.variance_out = nullptr; }), PBRS_E_INVALID, kFlags);
    expect("the pair before the aliasing", with([](Call& c) { c.io.variance_in = nullptr, c.io.rgb_out = out_of(c.io.rgb_in); }), PBRS_E_INVALID, kPair);
    expect("rgb in place before the other planes", with([](Call& c) { c.io.rgb_out = out_of(c.io.rgb_in), c.io.removed_out = c.io.variance_out; }), PBRS_E_INVALID,
           kInPlace);
    expect("the aliasing before the limit", with([](Call& c) { c.io.removed_out = c.io.rgb_out, c.p.w = c.p.h = 1u << 15; }), PBRS_E_INVALID, kShared);
    std::printf("precedence holds\n");
}

}  // namespace

int main(int argc, char** argv) {
    REQUIRE(argc == 2, "usage: despeckle_check <path of host/arg_checks_despeckle.cpp>");
    check_refusals(argv[1]);
    check_accepted();
    check_precedence();
    std::printf("ok\n");
    return 0;
}
