// device/wide.h — four-wide BVH nodes for the BLAS walk of k_shadow (AnyWalkW, traverse.h; the closest-hit walk over them was retired).
//
// What the reference's traversal DEFINES, for a ray on the division-free box test (no NaN quotients, traverse.h), is small:
//   * closest hit in a mesh (shape/src/blas.rs:422-476): the leaves are taken in the order of the near-first depth-first walk
//     (the child the ray enters first along the split axis, `ray.dir[axis] > 0`); a leaf's triangles are tested iff the leaf's
//     OWN box passes the reference's test against the best hit of that moment (after the root: the root is tested against the
//     incoming extent).  Every slab bound is a correctly rounded — monotone — function of the box coordinate and a child's box
//     lies inside its parent's, so a leaf's box passing implies that all its ancestors passed earlier, against larger extents:
//     the tests of the inner nodes only prune, they decide nothing.
//   * any hit (:478-495): occluded iff some leaf whose own box passes (fixed extent) holds a triangle that passes; order free.
// So inner nodes may be pruned with ANY test that never rejects a box the reference's test accepts, in ANY grouping.  The walks
// below take the reference's binary tree two levels at a time: a wide node holds the boxes of up to four grandchildren (or a
// child, where it is a leaf) of an inner node X, in left-first order, tested together with pn_slab_filter (include/pbrs_numeric.h:
// f32 products by the rounded reciprocals, bounds widened by 2^-21 — proved and tested never to reject what the reference
// accepts); the children that pass are visited in the reference's order (three split axes per wide node: X's and its two
// children's).  A leaf that comes up gets the reference's exact test (slab_rs): in a closest-hit walk at ITS turn, with the best hit
// of that moment, before its triangles are tested — the sequence of (leaf, extent) pairs whose triangles are tested, hence every hit,
// every tie-break and the final result, is the reference's.  In the any-hit walk (AnyWalkW, traverse.h) a leaf of one to four triangles
// is named by a reference that carries the triangles themselves (PBRS_WREF_PACKED, device/scene.h) and the order is the other way
// round: the triangles first, the leaf's box — found through tri_leaf below — only for a leaf one of whose triangles has passed, and
// only when the lane's walk is retired (AnyWalkW::settle).  The answer is the OR, over the leaves reached, of (box passes AND some
// triangle passes); the conjunction commutes, the triangle predicate is pure arithmetic on a ray inside the guarded range (no side
// effect, no state carried from leaf to leaf, a fixed extent), and reaching MORE leaves than the reference does is harmless because
// each still has to pass its own box: no bit of the answer changes.  A ray that leaves every leaf without a passing triangle — most
// shadow rays of an open scene — never pays for a leaf's box.  Leaves of more than four triangles (coincident centroids), empty leaves
// and leaves beyond the reference's triangle field keep the node form and are verified first, as before.  Measured on C4's terrain (tools/trav_stats): 54 box tests in 54 dependent steps per bounce ray become 54
// tests in 14 steps + 2.4 exact leaf tests; shadow rays 61 -> 16 steps.
//
// Rays outside the guarded range (a zero / denormal / huge direction or origin component, in the world or inside an instance)
// never take this path: the wide kernels hand them to the binary-walk kernels through a list (kernels.h, slow list).
#pragma once
#include "scene.h"   // pbrs_wnode, PBRS_WREF_*, PBRS_WIDE_*
#include "shapes.h"  // included by traverse.h once RaySpace exists

// pbrs_wnode, PBRS_WREF_* and the PBRS_WIDE_* constants: device/scene.h (the host builds the nodes: host/scene_prepare.cpp)

// DevScene::tri_leaf: the leaf node of triangle record `t` (behind the wide nodes, in their allocation)
PD uint32_t tri_leaf(const DevScene& S, uint32_t t) { return reinterpret_cast<const uint32_t*>(S.wnodes + S.n_wnodes)[t]; }

struct WideRay {
    f3 r32;       // RN(1 / d) per component: the correctly rounded reciprocals of the direction (-RaySpace::nr)
    uint32_t nb;  // byte offsets of the planes met first on each axis, one per byte: axis * 16 (+ 48 where the direction is negative)
    PD void set(const RaySpace& C) {
        r32 = -C.nr;
        nb = (C.d.x > 0.0f ? 0u : 48u) | (C.d.y > 0.0f ? 16u : 64u) << 8 | (C.d.z > 0.0f ? 32u : 80u) << 16;
    }
    PD uint32_t nx() const { return nb & 0xffu; }
    PD uint32_t ny() const { return (nb >> 8) & 0xffu; }
    PD uint32_t nz() const { return nb >> 16; }
};

struct WideTest {
    uint32_t pass;  // bit s: slot s passed the filter
    uint32_t child[4];  // as stored: axis bits included
    PD int axis_x() const { return (int)((child[0] >> PBRS_WREF_AXIS_SHIFT) & 3u); }
    PD int axis_left() const { return (int)((child[0] >> (PBRS_WREF_AXIS_SHIFT + 2)) & 3u); }
    PD int axis_right() const { return (int)((child[2] >> PBRS_WREF_AXIS_SHIFT) & 3u); }
};
// The four slots of wide node `wi` against the ray (C: origin; W: reciprocals, plane choice) within `t_max`.  One uniform base
// and 32-bit byte offsets per lane (wide nodes are indexed below 2^24: pbrs_upload_scene).
PD WideTest wide_test(const pbrs_wnode* nodes, uint32_t wi, const RaySpace& C, const WideRay& W, float t_max) {
    const char* base = reinterpret_cast<const char*>(nodes);
    const uint32_t at = wi * (uint32_t)sizeof(pbrs_wnode);
    const float4 nx = *reinterpret_cast<const float4*>(base + (at + W.nx())), ny = *reinterpret_cast<const float4*>(base + (at + W.ny())),
                 nz = *reinterpret_cast<const float4*>(base + (at + W.nz()));
    const float4 fx = *reinterpret_cast<const float4*>(base + (at + (48u - W.nx()))), fy = *reinterpret_cast<const float4*>(base + (at + (80u - W.ny()))),
                 fz = *reinterpret_cast<const float4*>(base + (at + (112u - W.nz())));
    const uint4 ch = *reinterpret_cast<const uint4*>(base + (at + 96u));
    WideTest t;
    t.child[0] = ch.x, t.child[1] = ch.y, t.child[2] = ch.z, t.child[3] = ch.w;
    // (scalar operations: the packed forms v_pk_add_f32 / v_pk_mul_f32 for two slots at a time were measured slower — C4 k_shadow
    // 236 -> 292 ms per frame, the register allocator spilling the ray's origin around them)
    const uint32_t p0 = pn_slab_filter(nx.x, ny.x, nz.x, fx.x, fy.x, fz.x, C.o.x, C.o.y, C.o.z, W.r32.x, W.r32.y, W.r32.z, t_max) ? 1u : 0u;
    const uint32_t p1 = pn_slab_filter(nx.y, ny.y, nz.y, fx.y, fy.y, fz.y, C.o.x, C.o.y, C.o.z, W.r32.x, W.r32.y, W.r32.z, t_max) ? 2u : 0u;
    const uint32_t p2 = pn_slab_filter(nx.z, ny.z, nz.z, fx.z, fy.z, fz.z, C.o.x, C.o.y, C.o.z, W.r32.x, W.r32.y, W.r32.z, t_max) ? 4u : 0u;
    const uint32_t p3 = pn_slab_filter(nx.w, ny.w, nz.w, fx.w, fy.w, fz.w, C.o.x, C.o.y, C.o.z, W.r32.x, W.r32.y, W.r32.z, t_max) ? 8u : 0u;
    t.pass = p0 | p1 | p2 | p3;  // (a slot not in use never passes: its box is inverted)
    // the links are wanted here, with the planes: left to itself the compiler sinks their load behind the test of `pass` — a second
    // memory latency on the dependent chain of every node step that goes on (C4 k_shadow 219 -> 228 ms per frame)
    asm volatile("" : "+v"(t.child[0]), "+v"(t.child[1]), "+v"(t.child[2]), "+v"(t.child[3]));
    return t;
}

// The survivors of a node step in visiting order (r[0] first) with their pass bits, by selects only — the obvious loop over
// positions with a four-way pick compiles into nested exec-mask branches, a couple of hundred scalar and vector instructions.
struct WideOrder {
    uint32_t r[4], p[4];
};
// Any order gives an any-hit walk the same answer; the side of X the ray enters first goes first (finds an occluder sooner)
PD WideOrder wide_order_any(const WideTest& t, f3 d) {
    const bool sx = !(comp(d, t.axis_x()) > 0.0f);
    const uint32_t q0 = t.pass & 1u, q1 = (t.pass >> 1) & 1u, q2 = (t.pass >> 2) & 1u, q3 = (t.pass >> 3) & 1u;
    WideOrder o;
    o.r[0] = sx ? t.child[3] : t.child[0], o.r[1] = sx ? t.child[2] : t.child[1], o.r[2] = sx ? t.child[1] : t.child[2], o.r[3] = sx ? t.child[0] : t.child[3];
    o.p[0] = sx ? q3 : q0, o.p[1] = sx ? q2 : q1, o.p[2] = sx ? q1 : q2, o.p[3] = sx ? q0 : q3;
    return o;
}
// Pushes every survivor but the first (the stack pops them in visiting order) and returns the first; at least one survives.
PD uint32_t wide_push(const WideOrder& o, LaneStack stk, int& sp) {
    const uint32_t any01 = o.p[0] | o.p[1], any012 = any01 | o.p[2];
    if (o.p[3] & any012) stk.put(sp, o.r[3]);
    if (o.p[2] & any01) stk.put(sp + (int)o.p[3], o.r[2]);
    if (o.p[1] & o.p[0]) stk.put(sp + (int)(o.p[3] + o.p[2]), o.r[1]);
    sp += (int)(o.p[0] + o.p[1] + o.p[2] + o.p[3]) - 1;
    return o.p[0] ? o.r[0] : o.p[1] ? o.r[1] : o.p[2] ? o.r[2] : o.r[3];
}
