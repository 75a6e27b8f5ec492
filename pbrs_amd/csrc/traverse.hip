// traverse.hip — the traversal kernels: every k_extend and k_shadow a scene's plan can name, in tables by key, and k_intersect_rays.
// (The units of the library: kernel_tables.h.)
#include <hip/hip_runtime.h>

#include <utility>

#include "kernel_tables.h"

// The traversal probes' sums (device/probes.h): defined here, once, in the unit that holds every kernel that adds to them and the
// entry points that read them.
#ifdef PBRS_PROBE_TIME
__device__ unsigned long long g_trav_time[2][8];
#endif
#ifdef PBRS_PROBE_TRAV
__device__ unsigned long long g_trav_probe[2][24];
#endif
#define PBRS_TRAVERSAL_PROBES_DEFINED
#include "device/extend.h"
#include "device/intersect.h"
#include "device/shadow.h"

using namespace pbrs;

namespace {

// The traversal kernels, one per valid key (host/kernel_choice.h: extend_key_ok, shadow_key_ok), in tables filled at compile time.
template <uint32_t K>
extend_fn_t extend_fn_of() {  // (no constant expression: the entry kernels are handed out under k_extend's pointer type)
    if constexpr (K >= kTraversalKeys) {
        if constexpr (extend_entry_ok(K - kTraversalKeys)) return reinterpret_cast<extend_fn_t>(static_cast<extend_entry_fn_t>(&k_extend<false, K - kTraversalKeys, EntryArgs>));
        else return nullptr;
    } else if constexpr (extend_key_ok(K)) return &k_extend<(K & kStatsKey) != 0u, (K & ~kStatsKey)>;
    else return nullptr;
}
template <uint32_t K>
constexpr shadow_fn_t shadow_fn_of() {
    if constexpr (shadow_key_ok(K)) return &k_shadow<(K & kStatsKey) != 0u, (K & ~kStatsKey)>;
    else return nullptr;
}
template <uint32_t... K>
const extend_fn_t* extend_table(std::integer_sequence<uint32_t, K...>) {
    static const extend_fn_t t[sizeof...(K)] = {extend_fn_of<K>()...};
    return t;
}
template <uint32_t... K>
const shadow_fn_t* shadow_table(std::integer_sequence<uint32_t, K...>) {
    static const shadow_fn_t t[sizeof...(K)] = {shadow_fn_of<K>()...};
    return t;
}

}  // namespace

namespace pbrs {

const extend_fn_t* extend_fns() { return extend_table(std::make_integer_sequence<uint32_t, kExtendKeys>{}); }
const shadow_fn_t* shadow_fns() { return shadow_table(std::make_integer_sequence<uint32_t, kTraversalKeys>{}); }
intersect_fn_t intersect_fn(bool wide_any) { return wide_any ? &k_intersect_rays<true> : &k_intersect_rays<false>; }

}  // namespace pbrs

extern "C" {

#ifdef PBRS_PROBE_TIME
// developer probe: reads and clears the traversal loops' cycle sums by region ([0]: k_extend, [1]: k_shadow; device/probes.h)
int pbrs_debug_trav_time(unsigned long long* out16) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_trav_time), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
    unsigned long long zero[16] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_trav_time), zero, sizeof zero) == hipSuccess ? 0 : -1;
}
#endif
#ifdef PBRS_PROBE_TRAV
// developer probe: reads and clears the traversal loops' event counts ([0]: k_extend, [1]: k_shadow; device/probes.h)
int pbrs_debug_trav_probe(unsigned long long* out48) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out48, HIP_SYMBOL(g_trav_probe), 48 * sizeof(unsigned long long)) != hipSuccess) return -1;
    unsigned long long zero[48] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_trav_probe), zero, sizeof zero) == hipSuccess ? 0 : -1;
}
#endif

}  // extern "C"
