// device/split_planes.h — the two split planes an inner BLAS node carries in the spare bits of its `b` word, and the one expression that
// turns a stored number back into a coordinate.  Plain C++ / HIP, no other header of the device code: host/scene_prepare.cpp chooses the
// numbers with these functions and device/traverse.h (ClosestWalk::cull_children) reads them with the same ones.
//
// For an inner node X split on axis k, with left child L (node i + 1) and right child R (node X.a), both inside X's box:
//     down(qd) <= R.min[k]      a plane no point of R lies below, counted up from X.min[k]
//     up(qu)   >= L.max[k]      a plane no point of L lies above, counted down from X.max[k]
// in steps of 2^-14 of X's own extent on k.  The host takes the largest q for which the inequality holds when it evaluates the very
// expression below — the device evaluates the same one on the same bits (one RN subtraction, an exact scaling by a power of two, one
// fused multiply-add), so the inequality needs no rounding argument.  q = 0 gives X.min[k] / X.max[k] themselves: always valid, and a
// word of zeros culls nothing (traverse.h).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PBRS_SP_FN __host__ __device__ static inline
#else
#define PBRS_SP_FN static inline
#endif

#define PBRS_PLANE_BITS 14u
#define PBRS_PLANE_MAX ((1u << PBRS_PLANE_BITS) - 1u)
#define PBRS_PLANE_DOWN_SHIFT 2u  // bits 2 .. 15 of an inner BLAS node's b (bits 0 .. 1: the split axis; bit 31: PBRS_LEAF_FLAG)
#define PBRS_PLANE_UP_SHIFT 16u   // bits 16 .. 29

PBRS_SP_FN float pbrs_plane_step(float lo, float hi) { return (hi - lo) * 0x1p-14f; }
PBRS_SP_FN float pbrs_plane_down(uint32_t q, float step, float lo) { return __builtin_fmaf((float)q, step, lo); }
PBRS_SP_FN float pbrs_plane_up(uint32_t q, float step, float hi) { return __builtin_fmaf(-(float)q, step, hi); }
PBRS_SP_FN uint32_t pbrs_plane_qd(uint32_t b) { return (b >> PBRS_PLANE_DOWN_SHIFT) & PBRS_PLANE_MAX; }
PBRS_SP_FN uint32_t pbrs_plane_qu(uint32_t b) { return (b >> PBRS_PLANE_UP_SHIFT) & PBRS_PLANE_MAX; }
PBRS_SP_FN uint32_t pbrs_plane_pack(uint32_t qd, uint32_t qu) { return qd << PBRS_PLANE_DOWN_SHIFT | qu << PBRS_PLANE_UP_SHIFT; }
