// device/entry_nodes.h — per-pixel entry nodes of the camera rays: the record k_entry_nodes writes and k_extend<.., EntryArgs> reads, the
// camera direction both k_raygen and the pre-pass evaluate, the beam test and the refinement that chooses a pixel's entries.  Plain C++ /
// HIP like device/split_planes.h, no other header of the device code: tests/entry_nodes_check.cpp runs the same functions on a CPU.
//
// What it is for.  All camera rays share one origin and the samples of a pixel differ by less than a pixel in direction, yet each of
// them walks the BLAS of the scene's deep mesh from its root and fails the same siblings on the way down.  Once per render, one lane per
// pixel walks down from the root with a test that is conservative for EVERY ray of the pixel and keeps the few deepest nodes (at most
// PBRS_ENTRY_MAX, in the order the walk reaches them) under which every leaf any of those rays can pass must lie.  The closest-hit walk
// of bounce 0 then tests the root as before and, where it passes, pushes the pixel's entries instead of the root.
//
// Why the walk's results keep their bits (checked against traverse.h, ClosestWalk::node_step / xfer_step / cull_children, and against
// the reference, shape/src/blas.rs:422-476, geometry/src/bvh.rs:84-99).  The ray is on the division-free box test (RaySpace::fast),
// whose quotient is RN division (traverse.h: proved by exhaustion), in an instance that is the identity or a pure translation.
//   1. Nesting.  The host gives a table only to a BLAS in which every child box lies inside its parent's (prepare_scene).  RN subtraction
//      and RN division are monotone, so a node's [t_low, hi_el] lies inside every ancestor's, and since the extent a lane tests with only
//      falls while it stays in one BLAS, a node whose ancestor would fail its box test fails its own.  A failed pop has no side effect.
//   2. The reference's result is fixed by the sequence of LEAVES whose own box test passes — in DFS order, the near child first by the
//      sign of d[axis] (blas.rs:456-466) — and by the extent each sees, which changes only in those leaves (blas.rs:468: lt = mt after
//      every passing node, mt changes in leaves alone).  Inner nodes only decide which leaves are reached.
//   3. Monotonicity.  The origin o is one float triple for every ray of the pixel (k_raygen writes cam.center; enter_instance moves it
//      by xf_apply with the instance's rows, or not at all), so a plane's numerator p - o is the same float for all of them.  For a
//      fixed numerator RN(n / d) is monotone in d on an interval that does not contain zero, so for lo <= d <= hi of one sign the
//      quotient lies between the quotients at lo and at hi.  pbrs_entry_beam takes, per axis, the smallest and the largest of the four
//      quotients (two planes x two ends): LB = max over the axes of the smallest <= the ray's lo_el, UB = min over the axes of the
//      largest >= the ray's hi_el.  A ray passes a node at extent +inf iff max(lo_el, 0) <= hi_el, which implies max(LB, 0) <= UB: a
//      node that fails the beam test fails the box test of every ray of the pixel at every extent.
//   4. The direction box.  dir = c + a x + b y (pbrs_camera_dir, the one expression k_raygen evaluates) with x in [col, col + 1] and
//      y in [row, row + 1]: every operation is RN and monotone in x and in y separately, whatever the other is, so each component's
//      range over the pixel is spanned by the four corners.  A component that is zero or changes sign gives no table for the pixel.
//   5. Covering.  pbrs_entry_refine starts at the root and only drops children whose beam test fails; it emits a node only after every
//      ancestor's other child was dropped or refined in its turn: every leaf a ray of the pixel can pass lies under an entry, entries
//      are disjoint subtrees, and they are emitted near child first with the sign of d[axis], which is the same for the whole pixel.
//   6. Consequence.  The walk from the root reaches the passing leaves in DFS order; pops of nodes above the entries either fail (no
//      side effect) or push their children and set lt = mt (which it is already, after the root).  Pushing the entries last-first
//      pops them, and below them everything, in the same DFS order; an entry whose ancestor the walk from the root would have failed
//      or culled (cull_children: "a child that is not pushed would have failed its own box test when popped") fails its own test by 1.
//      The root keeps its own test against the incoming extent t_max (blas.rs: the root sees ray.t_max, later nodes outer_hit.ray_t);
//      where it fails nothing is pushed, as today.  Each entry is tested against the mesh-local best, +inf for the first, as the
//      reference tests a non-root node.
// Rays outside all this (not on the division-free test, an instance that is rotated or scaled, another instance) push the root.
//
// Stack.  The entries of a pixel are pushed at once.  While entry i of n (i = 0 first) is walked, n - 1 - i entries wait below it and
// its subtree, whose root lies `depth` levels below the BLAS root, needs at most height - depth rows: the refinement is accepted only if
// (n - 1 - i) + (height - depth_i) + 1 <= rows for every entry, else it is repeated with a smaller fork budget, down to no table.
#pragma once
#include <stdint.h>

#include "../../../include/pbrs_gpu.h"

#if defined(__HIPCC__)
#define PBRS_EN_FN __host__ __device__ static inline
#else
#define PBRS_EN_FN static inline
#endif

#define PBRS_ENTRY_MAX 8u             // entries of a record: two uint4
#define PBRS_ENTRY_FORKS 3u           // fork budget: a path from the root to an entry passes at most this many forks (2^3 = PBRS_ENTRY_MAX)
#define PBRS_ENTRY_ROOT 0xfffffffeu   // in word 0: no table for this pixel, the walk pushes the root
#define PBRS_ENTRY_UNUSED 0xffffffffu // a slot not in use; the used ones come first; all eight unused: no ray of the pixel reaches the mesh
#define PBRS_ENTRY_NONE 0xffffffffu   // DevScene::entry_inst: the scene has no instance with a table

struct pbrs_entry_record {
    uint32_t e[PBRS_ENTRY_MAX];  // node indices in DevScene::nodes, in the order the walk reaches them
};

// Camera::shoot_ray (camera.rs:65-77): the direction of film position (x, y).  k_raygen calls this with the sample's position, the
// pre-pass with the corners of the pixel.
PBRS_EN_FN void pbrs_camera_dir(const pbrs_camera& cam, float x, float y, float d[3]) {
    for (int k = 0; k < 3; ++k) d[k] = cam.c[k] + cam.a[k] * x + cam.b[k] * y;
}

PBRS_EN_FN uint32_t pbrs_en_bits(float x) {
    union {
        float f;
        uint32_t u;
    } v;
    v.f = x;
    return v.u;
}
// The guarded range of the division-free box test: the same bounds as dir_in_range / origin_in_range of traverse.h, which the walk tests
// each ray with (that header says so too: change them together).  A pre-pass that were stricter than the walk would only give fewer
// pixels a table; one that were laxer would still be sound — the walk uses the table only for a ray that passes ITS test (RaySpace::fast),
// and the beam test needs no more of the corners than finite non-zero quotients of one sign.
PBRS_EN_FN bool pbrs_en_dir_in_range(float x) { return ((pbrs_en_bits(x) >> 23) & 0xffu) - (127u - 40u) <= 80u; }
PBRS_EN_FN bool pbrs_en_origin_in_range(float x) {
    const uint32_t u = pbrs_en_bits(x) & 0x7fffffffu;
    return u == 0u || (u >> 23) - (127u - 60u) <= 100u;
}

// The component ranges of the directions of pixel (col, row); false where the pixel gets no table (a component that is zero, changes
// sign or leaves the guarded range at a corner).
struct pbrs_dir_box {
    float lo[3], hi[3];
};
PBRS_EN_FN bool pbrs_entry_dir_box(const pbrs_camera& cam, uint32_t col, uint32_t row, pbrs_dir_box& B) {
    bool ok = true;
    for (int i = 0; i < 4; ++i) {
        float d[3];
        pbrs_camera_dir(cam, (float)(col + (uint32_t)(i & 1)), (float)(row + (uint32_t)(i >> 1)), d);
        for (int k = 0; k < 3; ++k) {
            ok = ok && pbrs_en_dir_in_range(d[k]);
            B.lo[k] = i == 0 || d[k] < B.lo[k] ? d[k] : B.lo[k];
            B.hi[k] = i == 0 || d[k] > B.hi[k] ? d[k] : B.hi[k];
        }
    }
    for (int k = 0; k < 3; ++k) ok = ok && ((B.lo[k] > 0.0f) == (B.hi[k] > 0.0f));  // (in range: neither is zero)
    return ok;
}

// The beam test (3. above): false only if no ray from `o` with a direction inside `B` passes the node's box at any extent.
PBRS_EN_FN bool pbrs_entry_beam(const pbrs_node& n, const float o[3], const pbrs_dir_box& B) {
    float lb = 0.0f, ub = 0.0f;
    for (int k = 0; k < 3; ++k) {
        const float n0 = n.min[k] - o[k], n1 = n.max[k] - o[k];
        const float q[4] = {n0 / B.lo[k], n0 / B.hi[k], n1 / B.lo[k], n1 / B.hi[k]};  // IEEE divisions, correctly rounded: the walk's quotients
        float mn = q[0], mx = q[0];
        for (int i = 1; i < 4; ++i) mn = q[i] < mn ? q[i] : mn, mx = q[i] > mx ? q[i] : mx;
        lb = k == 0 || mn > lb ? mn : lb;
        ub = k == 0 || mx < ub ? mx : ub;
    }
    return (lb > 0.0f ? lb : 0.0f) <= ub;
}

// The entries of a pixel with fork budget `forks` <= PBRS_ENTRY_FORKS (5. above), `root` the BLAS root in `nodes`:
//   follow the chain while exactly one child may pass; at a fork spend one unit of the budget and refine both children, the rays' near
//   child first; with no budget left the fork node itself is the entry; a leaf is an entry; a node neither child of which may pass is dropped.
// Returns the number of entries, written to rec.e[0 ..] with their depths below the root in depth[]; the other slots are PBRS_ENTRY_UNUSED.
PBRS_EN_FN uint32_t pbrs_entry_refine(const pbrs_node* nodes, uint32_t root, const float o[3], const pbrs_dir_box& B, uint32_t forks, pbrs_entry_record& rec,
                                      uint32_t depth[PBRS_ENTRY_MAX]) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < PBRS_ENTRY_MAX; ++i) rec.e[i] = PBRS_ENTRY_UNUSED, depth[i] = 0u;
    if (!pbrs_entry_beam(nodes[root], o, B)) return 0u;
    // far children of the forks on the way down, waiting for their turn: at most one per unit of the budget
    uint32_t pend_node[PBRS_ENTRY_FORKS], pend_depth[PBRS_ENTRY_FORKS], pend_forks[PBRS_ENTRY_FORKS], np = 0;
    uint32_t x = root, dx = 0u, fx = forks < PBRS_ENTRY_FORKS ? forks : PBRS_ENTRY_FORKS;
    for (;;) {
        // x has passed the beam test
        const pbrs_node X = nodes[x];
        bool emit = (X.b & PBRS_LEAF_FLAG) != 0u, drop = false;
        if (!emit) {
            const uint32_t left = x + 1u, right = X.a;
            const bool pl = pbrs_entry_beam(nodes[left], o, B), pr = pbrs_entry_beam(nodes[right], o, B);
            if (pl != pr) {
                x = pl ? left : right;
                ++dx;
                continue;
            }
            if (!pl) drop = true;
            else if (fx == 0u) emit = true;
            else {
                const bool left_first = B.lo[X.b & 3u] > 0.0f;  // ClosestWalk::node_step: dk > 0 (the sign is the pixel's)
                --fx;
                pend_node[np] = left_first ? right : left, pend_depth[np] = dx + 1u, pend_forks[np] = fx;
                ++np;
                x = left_first ? left : right;
                ++dx;
                continue;
            }
        }
        if (emit && !drop) rec.e[n] = x, depth[n] = dx, ++n;
        if (np == 0u) break;
        --np;
        x = pend_node[np], dx = pend_depth[np], fx = pend_forks[np];
    }
    return n;
}

// The stack bound (above): may a lane with `rows` free rows at the BLAS root push these n entries at once?
PBRS_EN_FN bool pbrs_entry_fits(uint32_t n, const uint32_t depth[PBRS_ENTRY_MAX], uint32_t height, uint32_t rows) {
    for (uint32_t i = 0; i < n; ++i)
        if ((n - 1u - i) + (height > depth[i] ? height - depth[i] : 1u) + 1u > rows) return false;
    return true;
}

// A pixel's record: the refinement with the largest fork budget that fits the stack; the root sentinel where none does.
// Returns the number of entries, or PBRS_ENTRY_ROOT.
PBRS_EN_FN uint32_t pbrs_entry_record_of(const pbrs_node* nodes, uint32_t root, const float o[3], const pbrs_dir_box& B, uint32_t max_forks, uint32_t height,
                                         uint32_t rows, pbrs_entry_record& rec) {
    uint32_t depth[PBRS_ENTRY_MAX];
    for (uint32_t f = max_forks < PBRS_ENTRY_FORKS ? max_forks : PBRS_ENTRY_FORKS;; --f) {
        const uint32_t n = pbrs_entry_refine(nodes, root, o, B, f, rec, depth);
        if (pbrs_entry_fits(n, depth, height, rows)) return n;
        if (f == 0u) break;
    }
    for (uint32_t i = 0; i < PBRS_ENTRY_MAX; ++i) rec.e[i] = PBRS_ENTRY_UNUSED;
    rec.e[0] = PBRS_ENTRY_ROOT;
    return PBRS_ENTRY_ROOT;
}
