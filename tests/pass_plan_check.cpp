// tests/pass_plan_check.cpp — the pass driver's decisions (pbrs_amd/csrc/host/pass_plan.h) on a CPU: a program of its own that
// tests/test_pass_plan.py compiles with -fsanitize=address,undefined and runs.
//
// Checked:
//   layout      path_layout at sizes around every rounding step: aligned regions in the stated order, no overlap, room for every
//               column, and the total the driver allocated before the table existed (stated here once, as a closed form)
//   counters    the six regions tile the counter block, and every index run_pass forms stays inside its own region
//   pass size   properties over a grid of inputs, and literal rows: what auto_samples_per_pass of pbrs_gpu.hip answered, before it
//               became samples_per_pass, for the same inputs
//   bounce plan literal expectations for every integrator x split_queue x split_decision x order x bounce
//   shape       the grids of a pass against the expressions run_pass used to compute inline
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>

#include "../pbrs_amd/csrc/host/pass_plan.h"

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

using u64 = unsigned long long;

// ---- layout ----
// What ensure_work allocated before path_layout: eleven one-float4 columns, three of two float4 in two aligned halves, and the rest.
size_t align256(size_t b) { return (b + 255) / 256 * 256; }
size_t closed_form_total(size_t n) {
    const size_t v16 = align256(n * 16);
    const size_t n_tiles = n / 16384 + 1;
    const size_t sort_bytes = align256(n_tiles * 16 * 4) + align256((16 + 1) * 8);
    return (6 + 1 + 1 + 3) * v16 + 3 * 2 * v16 + align256(2 * n) + align256(n * 4) + align256(n * 4) + sort_bytes + align256(n) + align256(2 * n * 4) + align256(n * 4);
}

void check_layout() {
    static_assert(N_PATH_COLUMNS == 22, "q[2][3], hit, L, nee[3], sr[3], occ, nee queue, perm, cls, slow, tile_hist, class_range, rng_hi0");
    static_assert(kPathBytesPerSlot == 295, "the bytes a path holds");
    // the order of the columns, by the first of each group
    REQUIRE(COL_Q == 0 && COL_HIT == 6 && COL_L == 7 && COL_NEE == 8 && COL_SR == 11 && COL_OCC == 14 && COL_NEEQ == 15 && COL_PERM == 16 && COL_CLS == 17 &&
                COL_SLOW == 18 && COL_TILE_HIST == 19 && COL_CLASS_RANGE == 20 && COL_RNG_HI0 == 21,
            "the columns are not in the allocation's order");
    const char* names[N_PATH_COLUMNS] = {"q[0][0]", "q[0][1]", "q[0][2]", "q[1][0]", "q[1][1]", "q[1][2]", "hit", "L", "nee[0]", "nee[1]", "nee[2]",
                                         "sr[0]", "sr[1]", "sr[2]", "occ", "nee queue", "perm", "cls", "slow", "tile_hist", "class_range", "rng_hi0"};
    // bytes per slot of each column, stated here on their own: float4 records, two shadow rays per path, bytes and words
    const size_t per_slot[N_PATH_COLUMNS] = {16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 32, 32, 32, 2, 4, 4, 1, 8, 0, 0, 4};
    for (uint32_t i = 0; i < N_PATH_COLUMNS; ++i) {
        REQUIRE(!std::strcmp(kPathColumns[i].name, names[i]), "column %u is %s, not %s", i, kPathColumns[i].name, names[i]);
        REQUIRE((size_t)kPathColumns[i].elem * kPathColumns[i].per_slot == per_slot[i], "%s: %u x %u bytes per slot", names[i], kPathColumns[i].elem,
                kPathColumns[i].per_slot);
    }
    const size_t sizes[] = {1, 63, 64, 255, 256, 257, 273, 16383, 16384, 16385, 3u * (1u << 20) + 5, (1u << 28) - 1};
    for (size_t n : sizes) {
        const PathLayout l = path_layout(n);
        const size_t n_tiles = n / 16384 + 1;
        size_t at = 0, parts = 0, sort_tables = 0;
        for (uint32_t i = 0; i < N_PATH_COLUMNS; ++i) {
            REQUIRE(l.offset[i] % 256 == 0, "n = %zu: %s starts at %zu", n, names[i], l.offset[i]);
            REQUIRE(l.offset[i] == at, "n = %zu: %s starts at %zu, the region before it ends at %zu", n, names[i], l.offset[i], at);
            const size_t need = i == COL_TILE_HIST ? n_tiles * 16 * 4 : i == COL_CLASS_RANGE ? 17 * 8 : per_slot[i] * n;
            REQUIRE(l.bytes[i] >= need, "n = %zu: %s holds %zu bytes, its elements need %zu", n, names[i], l.bytes[i], need);
            if (per_slot[i]) parts += kPathColumns[i].parts;
            else sort_tables += l.bytes[i];
            at += l.bytes[i];
        }
        REQUIRE(l.total == at, "n = %zu: total %zu, the last region ends at %zu", n, l.total, at);
        REQUIRE(l.total == closed_form_total(n), "n = %zu: total %zu, the closed form gives %zu", n, l.total, closed_form_total(n));
        // occ[1] = occ[0] + n lies in occ's region (ensure_work forms it); the region holds both bytes of every path
        REQUIRE(l.bytes[COL_OCC] >= 2 * n, "n = %zu: occ[1] leaves occ's region", n);
        // beyond 295 bytes per path: the two sort tables, and below 256 bytes of rounding per separately rounded part of a per-path column
        const size_t slack = l.total - 295 * n;
        REQUIRE(l.total >= 295 * n && slack <= sort_tables + 255 * parts, "n = %zu: %zu bytes beyond the paths' own, at most %zu expected", n, slack,
                sort_tables + 255 * parts);
    }
    std::printf("layout: %zu sizes, %u columns, 295 bytes per path\n", sizeof sizes / sizeof *sizes, (unsigned)N_PATH_COLUMNS);
}

// ---- counters ----
void check_counters() {
    const CounterLayout& l = kCounters;
    const uint32_t H = 8 * 32;  // heads x words between them
    REQUIRE(kHeadWords == H && kMaxDepth == 64, "the sizes this check was written for");
    // the regions in their order, each up to the next one's start: disjoint and tiling the block by construction, if the starts ascend
    const uint32_t start[7] = {l.act, l.ns, l.slows, l.xhead, l.shead, l.shead2, l.words};
    REQUIRE(start[0] == 0, "the block starts with a gap");
    for (int i = 0; i < 6; ++i) REQUIRE(start[i] < start[i + 1], "region %d is empty or out of order", i);
    REQUIRE(l.words == (4 + 3 * H) * (64 + 2), "%u words, not the %u of the block as it was", l.words, (4 + 3 * H) * (64 + 2));
    REQUIRE(l.ns % 2 == 0, "ns is not 8-byte aligned");
    auto inside = [&](int region, uint64_t word, const char* what, uint32_t b) {
        REQUIRE(word >= start[region] && word < start[region + 1], "bounce %u: %s at word %llu leaves [%u, %u)", b, what, (u64)word, start[region], start[region + 1]);
    };
    for (uint32_t b = 0; b < kMaxDepth; ++b) {
        if (b) inside(0, l.act + b, "act + b", b);  // (bounce 0 reads no count)
        inside(0, l.act + b + 1, "act + b + 1", b);
        inside(1, l.ns + 2 * b, "ns + b, low half", b);
        inside(1, l.ns + 2 * b + 1, "ns + b, high half", b);
        inside(2, l.slows + b, "slows + b", b);
        const uint32_t heads[3] = {l.xhead, l.shead, l.shead2};
        for (int k = 0; k < 3; ++k) {
            inside(3 + k, heads[k] + (uint64_t)b * H, "first head", b);
            inside(3 + k, heads[k] + (uint64_t)b * H + 7 * 32, "last head", b);
            inside(3 + k, heads[k] + (uint64_t)b * H + H - 1, "last head word", b);
        }
    }
    // k_sum_bounce_counts reads act[b] and ns[b] for b < n_bounces <= kMaxDepth: covered above
    std::printf("counters: 6 regions tile %u words, %u bounces inside\n", l.words, kMaxDepth);
}

// ---- pass size ----
constexpr long long kNoQuery = -1;
constexpr u64 GiB = 1ull << 30, MiB = 1ull << 20;
uint32_t size_of(u64 P, u64 spp, uint32_t req, bool direct, u64 held, u64 held_direct, long long free_b) {
    return samples_per_pass(P, spp, req, direct, held, held_direct, free_b == kNoQuery ? std::nullopt : std::optional<uint64_t>((uint64_t)free_b));
}
u64 ceil_div(u64 a, u64 b) { return (a + b - 1) / b; }
// spp in the fewest passes of at most `cap` samples, all equal but the last
u64 equal_passes(u64 spp, u64 cap) {
    if (cap >= spp) return spp;
    return ceil_div(spp, ceil_div(spp, cap));
}

struct SizeRow {
    u64 P, spp;
    int direct;
    u64 held, held_direct;
    long long free_b;
    uint32_t K;
};
// auto_samples_per_pass of pbrs_gpu.hip as it was (the free-memory query replaced by a parameter) for these inputs
const SizeRow kSizeRows[] = {
    // no answer from the query: the 240 Mi rule alone
    {1048576, 256, 0, 0, 0, kNoQuery, 128},  // 240 per pass would be 240 + 16: 128 + 128
    {1048576, 4096, 0, 0, 0, kNoQuery, 228},
    {2073600, 256, 0, 0, 0, kNoQuery, 86},
    {6144, 4096, 0, 0, 0, kNoQuery, 4096},
    {4194304, 64, 0, 0, 0, kNoQuery, 32},
    {12582912, 255, 0, 0, 0, kNoQuery, 20},
    {4196352, 1024, 0, 0, 0, kNoQuery, 57},
    {91, 9, 0, 0, 0, kNoQuery, 9},
    {1, 1, 0, 0, 0, kNoQuery, 1},
    // a tile at and above the target: one sample per pass
    {251658240, 16, 0, 0, 0, kNoQuery, 1},
    {251674624, 16, 0, 0, 0, kNoQuery, 1},
    {268419072, 4, 0, 0, 0, kNoQuery, 1},
    // no memory free, or little: the floor of 4 Mi paths
    {1048576, 256, 0, 0, 0, 0, 4},
    {1048576, 256, 0, 0, 0, (long long)(4 * GiB), 4},
    {1048576, 256, 1, 0, 0, (long long)(4 * GiB), 4},
    {2073600, 4096, 0, 0, 0, 0, 2},
    {2073600, 4096, 1, 0, 0, (long long)(4 * GiB), 2},
    {4194304, 1024, 0, 0, 0, (long long)(4 * GiB), 1},
    {6144, 4096, 0, 0, 0, 0, 586},
    {6144, 4096, 1, 0, 0, (long long)(4 * GiB), 586},
    // a quarter of the free memory, without and with the D column
    {1048576, 256, 0, 0, 0, (long long)(64 * GiB), 52},
    {1048576, 256, 1, 0, 0, (long long)(64 * GiB), 52},
    {2073600, 4096, 0, 0, 0, (long long)(64 * GiB), 28},
    {2073600, 4096, 1, 0, 0, (long long)(64 * GiB), 26},
    {2073600, 4096, 0, 0, 0, (long long)(283 * GiB), 121},
    {2073600, 4096, 1, 0, 0, (long long)(283 * GiB), 114},
    {4194304, 1024, 0, 0, 0, (long long)(64 * GiB), 13},
    {4194304, 1024, 1, 0, 0, (long long)(283 * GiB), 57},
    {1048576, 256, 0, 0, 0, (long long)(283 * GiB), 128},
    {6144, 4096, 1, 0, 0, (long long)(64 * GiB), 4096},
    // what the context holds counts as free: 100 Mi slots in its pass sets, 1 GiB in its D columns (those only with light passes)
    {1048576, 256, 0, 100 * MiB, 1 * GiB, 0, 24},
    {1048576, 256, 1, 100 * MiB, 1 * GiB, 0, 24},
    {1048576, 256, 0, 100 * MiB, 1 * GiB, (long long)(4 * GiB), 26},
    {1048576, 256, 1, 100 * MiB, 1 * GiB, (long long)(64 * GiB), 64},
    {2073600, 4096, 0, 100 * MiB, 1 * GiB, (long long)(64 * GiB), 40},
    {2073600, 4096, 1, 100 * MiB, 1 * GiB, (long long)(64 * GiB), 39},
    {2073600, 4096, 1, 100 * MiB, 1 * GiB, (long long)(4 * GiB), 14},
    {4194304, 1024, 0, 100 * MiB, 1 * GiB, (long long)(4 * GiB), 7},
    {4194304, 1024, 1, 100 * MiB, 1 * GiB, (long long)(4 * GiB), 6},
    {4194304, 1024, 0, 100 * MiB, 1 * GiB, (long long)(64 * GiB), 20},
    {4194304, 1024, 1, 100 * MiB, 1 * GiB, (long long)(64 * GiB), 19},
    {6144, 4096, 0, 100 * MiB, 1 * GiB, 0, 4096},
};

void check_pass_size() {
    const u64 Ps[] = {1, 91, 6144, 1 * MiB, 2073600, 4 * MiB, 4 * MiB + 2048, 12 * MiB, 240 * MiB, 240 * MiB + 16384, (1ull << 28) - 16384};
    const u64 spps[] = {1, 2, 4, 9, 16, 64, 255, 256, 257, 1024, 4096};
    const uint32_t reqs[] = {0, 1, 3, 64, 300};
    const u64 helds[] = {0, 1 * MiB, 100 * MiB}, held_directs[] = {0, 16 * MiB, 1 * GiB};
    const long long frees[] = {kNoQuery, 0, (long long)(1 * GiB), (long long)(4 * GiB), (long long)(5 * GiB), (long long)(16 * GiB), (long long)(64 * GiB),
                               (long long)(200 * GiB), (long long)(283 * GiB)};
    size_t points = 0;
    for (u64 P : Ps)
        for (u64 spp : spps)
            for (uint32_t req : reqs)
                for (int direct = 0; direct < 2; ++direct)
                    for (u64 held : helds)
                        for (u64 hd : held_directs) {
                            u64 passes_before = ~0ull;
                            for (long long fr : frees) {
                                const u64 K = size_of(P, spp, req, direct != 0, held, hd, fr);
                                ++points;
                                REQUIRE(K >= 1 && K <= spp, "%llu px, %llu spp, request %u, free %lld: %llu samples per pass", P, spp, req, fr, K);
                                if (req) {
                                    REQUIRE(K == (req < spp ? req : spp), "%llu spp, request %u: %llu samples per pass", spp, req, K);
                                    continue;
                                }
                                // equal passes: K is the smallest size that renders spp in as many passes as K does
                                const u64 passes = ceil_div(spp, K);
                                REQUIRE(K == ceil_div(spp, passes), "%llu px, %llu spp, free %lld: %llu passes of %llu are not equal ones", P, spp, fr, passes, K);
                                // between the floor of 4 Mi paths and the target of 240 Mi, which a failed query gives alone
                                const u64 hi = equal_passes(spp, P >= 240 * MiB ? 1 : 240 * MiB / P), lo = equal_passes(spp, P >= 4 * MiB ? 1 : 4 * MiB / P);
                                REQUIRE(K >= lo && K <= hi, "%llu px, %llu spp, free %lld: %llu outside [%llu, %llu]", P, spp, fr, K, lo, hi);
                                if (fr == kNoQuery) REQUIRE(K == hi, "%llu px, %llu spp, no query: %llu, the 240 Mi rule gives %llu", P, spp, K, hi);
                                // more free memory never means more passes (`frees` ascends behind the failed query)
                                if (fr != kNoQuery) {
                                    REQUIRE(passes <= passes_before, "%llu px, %llu spp: %llu passes at %lld free bytes, fewer with less", P, spp, passes, fr);
                                    passes_before = passes;
                                }
                                // the D columns count only for a render with light passes
                                if (!direct) REQUIRE(K == size_of(P, spp, req, false, held, 0, fr), "the D columns moved a render without light passes");
                            }
                        }
    size_t rows = 0;
    bool floor_row = false, one_row = false, halves_row = false, direct_rows[2] = {false, false};
    for (const SizeRow& r : kSizeRows) {
        const uint32_t K = size_of(r.P, r.spp, 0, r.direct != 0, r.held, r.held_direct, r.free_b);
        REQUIRE(K == r.K, "row %zu (%llu px, %llu spp, direct %d, held %llu + %llu, free %lld): %u, expected %u", rows, r.P, r.spp, r.direct, r.held, r.held_direct,
                r.free_b, K, r.K);
        ++rows;
        direct_rows[r.direct] = true;
        floor_row = floor_row || (r.free_b != kNoQuery && r.P * r.K <= 4 * MiB && r.P * (r.K + 1) > 4 * MiB);
        one_row = one_row || (r.P > 240 * MiB && r.K == 1);
        halves_row = halves_row || (r.spp == 256 && r.K == 128);
    }
    REQUIRE(floor_row && one_row && halves_row && direct_rows[0] && direct_rows[1], "a kind of literal row is missing");
    std::printf("pass size: %zu grid points, %zu literal rows\n", points, rows);
}

// ---- bounce plan ----
struct Expect {
    uint32_t split;
    IntegratorChoice::Order order;
    uint32_t n_classes, last, zero_dropped, sorted;
};
bool same(const BouncePlan& b, const Expect& e, const uint32_t (&ranges)[2]) {
    return b.split == e.split && b.order == e.order && b.n_classes == e.n_classes && b.last == e.last && b.zero_dropped == e.zero_dropped && b.sorted == e.sorted &&
           b.shade_range[0] == ranges[0] && b.shade_range[1] == ranges[1];
}

void check_bounce_plan() {
    const auto NO = IntegratorChoice::NO_ORDER, SORT = IntegratorChoice::CLASS_SORT, MAJOR = IntegratorChoice::CLASS_MAJOR;
    static_assert(PBRS_QSPLIT_ON == 1u && PBRS_QSPLIT_ENV == 2u, "the flags k_extend reads");
    static_assert(PBRS_INTEGRATOR_PATH == 0 && PBRS_INTEGRATOR_DIRECT == 1 && PBRS_INTEGRATOR_MATERIALS == 2 && PBRS_INTEGRATOR_NORMALS == 3, "the four integrators");
    // two choices: two launches over ranges of their own (the classes before class 5, and class 5), and one launch over the queue
    IntegratorChoice own, whole;
    own.last_class = 5, own.n_shade = 2, own.shade[0].range = 16, own.shade[1].range = 5;
    whole.last_class = 0, whole.n_shade = 1;
    // which combinations split: [integrator][split_queue][split_decision] — the path integrator with split_queue, undecided or decided for
    const bool splits[4][2][3] = {{{false, false, false}, {true, true, false}},
                                  {{false, false, false}, {false, false, false}},
                                  {{false, false, false}, {false, false, false}},
                                  {{false, false, false}, {false, false, false}}};
    // a queue that is not split: [order], whatever the bounce — sixteen classes, the choice's last class, nothing zeroed
    const Expect plain_own[3] = {{0, NO, 16, 5, 0, 0}, {0, SORT, 16, 5, 0, 1}, {0, MAJOR, 16, 5, 0, 1}};
    const Expect plain_whole[3] = {{0, NO, 16, 0, 0, 0}, {0, SORT, 16, 0, 0, 1}, {0, MAJOR, 16, 0, 0, 1}};
    // a split queue: [bounce], whatever the choice's order — class-major over two classes, the kept paths (class 1) last; the environment
    // flag and the zeroing of the dropped paths at bounce 0 only
    const Expect split[3] = {{3, MAJOR, 2, 1, 1, 1}, {1, MAJOR, 2, 1, 0, 1}, {1, MAJOR, 2, 1, 0, 1}};
    const uint32_t own_ranges[2] = {16, 5}, no_ranges[2] = {0, 0}, kept_ranges[2] = {1, 0};
    const IntegratorChoice::Order orders[3] = {NO, SORT, MAJOR};
    size_t n = 0;
    for (uint32_t integ = 0; integ < 4; ++integ)
        for (int sq = 0; sq < 2; ++sq)
            for (int dec = 0; dec < 3; ++dec)
                for (int o = 0; o < 3; ++o)
                    for (uint32_t b = 0; b < 3; ++b) {
                        own.order = whole.order = orders[o];
                        const bool s = splits[integ][sq][dec];
                        const BouncePlan with_own = bounce_plan(integ, sq != 0, own, dec, b), with_whole = bounce_plan(integ, sq != 0, whole, dec, b);
                        // a launch with a range of its own keeps it; one without covers the kept paths of a split queue, range 1
                        REQUIRE(same(with_own, s ? split[b] : plain_own[o], own_ranges), "integrator %u, split_queue %d, decision %d, order %d, bounce %u: ranges of their own",
                                integ, sq, dec, o, b);
                        REQUIRE(same(with_whole, s ? split[b] : plain_whole[o], s ? kept_ranges : no_ranges),
                                "integrator %u, split_queue %d, decision %d, order %d, bounce %u: one launch over the queue", integ, sq, dec, o, b);
                        ++n;
                    }
    // the bounces of a pass
    for (uint32_t depth : {0u, 1u, 2u, 5u, 64u}) {
        REQUIRE(bounce_count(PBRS_INTEGRATOR_PATH, depth) == depth, "path, depth %u", depth);
        REQUIRE(bounce_count(PBRS_INTEGRATOR_DIRECT, depth) == (depth ? 2u : 0u), "direct, depth %u", depth);
        REQUIRE(bounce_count(PBRS_INTEGRATOR_MATERIALS, depth) == 1u && bounce_count(PBRS_INTEGRATOR_NORMALS, depth) == 1u, "visualisers, depth %u", depth);
    }
    std::printf("bounce plan: %zu combinations, two choices each\n", n);
}

// ---- shape ----
void check_shape() {
    const uint32_t sizes[] = {1, 256, 257, 4096 * 256 + 1, (1u << 28) - 1};
    for (uint32_t N : sizes) {
        // what run_pass computed inline
        const uint32_t grid = (N + 256 - 1) / 256;
        const uint32_t sgrid = grid < 4096 ? grid : 4096;
        const uint32_t pgrid = grid < 1536 ? grid : 1536;
        const uint32_t slow = pgrid < 64 ? pgrid : 64;
        const uint32_t n_tiles = (N + 16384 - 1) / 16384;
        const PassShape s = pass_shape(N, 1);
        REQUIRE(s.n_slots == N && s.grid == grid && s.sgrid == sgrid && s.pgrid == pgrid && s.slow_grid == slow && s.n_tiles == n_tiles,
                "N = %u: %u slots, grids %u %u %u %u, %u tiles", N, s.n_slots, s.grid, s.sgrid, s.pgrid, s.slow_grid, s.n_tiles);
        // the sort tables of a layout for these slots hold the pass's tiles
        REQUIRE(path_tiles(N) >= n_tiles, "N = %u: %u tiles in a layout of %zu", N, n_tiles, path_tiles(N));
    }
    // pixels x samples: the product alone counts
    const PassShape a = pass_shape(91, 3), b = pass_shape(273, 1);
    REQUIRE(a.n_slots == 273 && a.grid == b.grid && a.sgrid == b.sgrid && a.pgrid == b.pgrid && a.slow_grid == b.slow_grid && a.n_tiles == b.n_tiles, "91 x 3 against 273 x 1");
    std::printf("shape: %zu sizes\n", sizeof sizes / sizeof *sizes);
}

}  // namespace

int main() {
    check_layout();
    check_counters();
    check_pass_size();
    check_bounce_plan();
    check_shape();
    std::printf("ok\n");
    return 0;
}
