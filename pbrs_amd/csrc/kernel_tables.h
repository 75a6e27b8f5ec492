// kernel_tables.h — how pbrs_gpu.hip reaches the kernels that other translation units of libpbrs_gpu.so instantiate (internal; the
// library's interface is include/pbrs_gpu.h).
//
//   pbrs_gpu.hip   the context, scene upload, the pass driver, the render entry points, the image operations, the developer entry points,
//                  with the kernels only they launch (device/kernels.h and the image headers)
//   traverse.hip   every k_extend and k_shadow a scene's plan can name, k_intersect_rays, the traversal probes' sums and their readers
//   shade.hip      every k_shade a scene's plan can name, the shade probe's sums and their reader, and k_bsdf_eval (pbrs_bsdf_eval): the
//                  unit that owns device/bsdf.h's callers
//
// A kernel is instantiated in ONE unit, and the library is built without device linking: pbrs_gpu.hip launches these kernels, and sets
// their attributes, through the host pointers their owners hand out here.  Everything declared here has hidden visibility.
#pragma once
#include <cstdint>

#include "device/path_state.h"
#include "host/kernel_choice.h"

#pragma GCC visibility push(hidden)
namespace pbrs {

typedef void (*extend_fn_t)(DevScene, PathState, uint32_t, const uint32_t*, uint32_t, uint32_t*, GlobalCounters*, const uint32_t*, uint32_t*, uint32_t*, uint32_t);
// k_extend<.., EntryArgs>: the same arguments and the entry table's.  extend_fns() hands these out as extend_fn_t; cast back before the launch.
typedef void (*extend_entry_fn_t)(DevScene, PathState, uint32_t, const uint32_t*, uint32_t, uint32_t*, GlobalCounters*, const uint32_t*, uint32_t*, uint32_t*, uint32_t, EntryArgs);
typedef void (*shadow_fn_t)(DevScene, PathState, const uint32_t*, uint32_t*, GlobalCounters*, const uint32_t*, uint32_t*, uint32_t*);
typedef void (*shade_fn_t)(DevScene, PathState, RenderConst, uint32_t, const uint32_t*, uint32_t, uint32_t*, uint32_t*, unsigned long long*, uint32_t, const uint2*,
                           const uint32_t*);
typedef void (*intersect_fn_t)(DevScene, uint32_t, const float4*, const float4*, const float*, pbrs_hit_record*, uint8_t*, uint32_t*);
typedef void (*bsdf_eval_fn_t)(DevScene, uint32_t, uint32_t, const uint32_t*, uint32_t*);

// traverse.hip: the traversal kernels, one per valid key (host/kernel_choice.h: extend_key_ok, shadow_key_ok; null elsewhere), kTraversalKeys
// each — and behind k_extend's, at entry_key(k), the entry variants of the keys that have one (extend_entry_ok; kExtendKeys in all); and k_intersect_rays, its occlusion queries through the four-wide any-hit walk or through the binary one.
const extend_fn_t* extend_fns();
const shadow_fn_t* shadow_fns();
intersect_fn_t intersect_fn(bool wide_any);

// shade.hip: the k_shade instantiation a key names (host/kernel_choice.h, PBRS_SHADE_KERNELS), or null.
shade_fn_t shade_fn(const ShadeKey& key);
// ... and k_bsdf_eval (device/bsdf_probe.h): specialised as the PBRS_SHADE_LAMBERT variants are, or with the Fourier lobe as the
// PBRS_SHADE_FOURIER variants carry it, or neither; null for both at once (no k_shade is both).
bsdf_eval_fn_t bsdf_eval_fn(bool lambert, bool fourier);

}  // namespace pbrs
#pragma GCC visibility pop
