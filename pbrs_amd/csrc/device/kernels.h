// device/kernels.h — the wavefront stages.
//
//   raygen      src/main.rs:197-203 + geometry/src/camera.rs:65-77
//   extend      tlas/src/bvh.rs:77-103 (closest hit)            -> hit record per path
//   shade       src/pathintegrator.rs:19-71 + src/directlighting.rs:58-222 minus the occlusion calls
//   shadow      tlas/src/bvh.rs:105-113 (any hit) + the radiance add of pathintegrator.rs:35
//   accumulate  src/main.rs:205-208 (in-order f32 sum over samples, then * 1/spp)
//
// One lane owns one path vertex (k_shade) or one ray (k_extend / k_shadow).  What a path carries from bounce to bounce
// travels as DENSE records at the path's position in the bounce's queue — k_shade writes the next ray where the
// compaction puts the path, k_extend writes the hit next to it, k_shade reads both back — so every access of the
// traversal kernels and all but one of k_shade's is a full-width coalesced 16-byte-per-lane stream.  Only the radiance
// accumulator stays at a fixed address per path (slot = k * P + pixel: k_accumulate sums the samples of a pixel in
// order).  The `break`s of the bounce loop (pathintegrator.rs:25-27, :48-50, :67-69) become "not appended to the next
// queue", compacted with __ballot + mbcnt prefixes summed per block in LDS (two atomics per block).
#pragma once
// The stages stand in a header each, and a translation unit of the library includes only the ones whose kernels it launches (a kernel
// that is no template is emitted by every unit that includes its header): shade.h in shade.hip; extend.h, shadow.h and intersect.h in
// traverse.hip; raygen.h, class_sort.h, accumulate.h and dev_kernels.h in pbrs_gpu.hip.  What they share is path_state.h.  This file
// includes all of them, for a tool that wants the whole pipeline; no unit of the library includes it.
#include "path_state.h"
#include "raygen.h"
#include "extend.h"
#include "shade.h"
#include "class_sort.h"
#include "shadow.h"
#include "accumulate.h"
#include "intersect.h"
#include "dev_kernels.h"
