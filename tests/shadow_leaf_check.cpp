// tests/shadow_leaf_check.cpp — leaf references that carry their triangles (pbrs_amd/csrc/device/scene.h, PBRS_WREF_PACKED; written by
// host/scene_prepare.cpp, pack_wide_leaves), the tri_leaf table, and the order of the four-wide any-hit walk's leaf step
// (device/traverse.h, AnyWalkW: the triangles first, the leaf's own box only once one of them has passed), on a CPU: a program of its
// own that tests/test_shadow_leaf.py compiles with -fsanitize=address,undefined and runs.
//
// Scenes come from pbrs_host_scene_build, one mesh each under an identity instance and a second, translated one (a TLAS of two: scanned,
// so the scene gets wide nodes), each mesh deep enough for PBRS_WIDE_MIN_LEVELS:
//   terrain     the C4 family's height field (pbrs_amd/scenes.py, heightfield_mesh with seed 4) at nx = 16, nz = 32: 1 024 triangles
//   flat        a grid at height 0
//   overlap     long triangles whose boxes overlap heavily
//   nested      the terrain and 13 nested triangles whose centroids coincide: a leaf of 13
//   tiny, huge  a grid on whole numbers, every coordinate scaled (exactly) by 2^-60 / 2^34
// Checked, per scene, on prepare_scene's output before and after pack_wide_leaves:
//   references  walking the wide tree beside the binary one: a reference to a leaf of 1 .. 4 triangles is packed and decodes to that
//               leaf's range, inside [0, n_triangles); every other leaf (more triangles; forged on copies: none, or a first triangle
//               beyond the field) keeps the node form; axis bits, inner references and unused slots are untouched
//   tri_leaf    names, for every triangle of a BLAS leaf, a leaf whose range holds it
//   layout      the constants' relations (the header's static_asserts compile into this program) and the extremes of the field, on a
//               forged leaf at triangle 2^24 - 1
// and on the terrain, for at least 10^5 rays (from the surface upward, grazing along it, through leaf-box corners, with t_max equal to
// a leaf box's entry distance): a restatement of the wide walk run verify-first and triangles-first, and of the binary walk, must agree
// ray for ray.  Natural boxes may never let a triangle pass outside its leaf's box, so the comparison runs again on a copy of the arrays
// in which the leaf boxes are shrunk (the wide slots keep the natural ones: the filter may pass more than the exact test, never less):
// the defined answer is still box AND triangle, and the branch "triangle passed, box failed" must have been taken.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/pbrs_host.h"
#include "../include/pbrs_numeric.h"
#include "../pbrs_amd/csrc/host/scene_prepare.h"

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

struct Rng {  // SplitMix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    float uniform(float a, float b) { return a + (b - a) * (float)((double)(next() >> 11) * (1.0 / 9007199254740992.0)); }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

// ---- meshes ----
struct Mesh {
    std::vector<float> pos, nrm, uv;
    std::vector<uint32_t> idx;
    void vertex(float x, float y, float z) {
        pos.insert(pos.end(), {x, y, z});
        nrm.insert(nrm.end(), {0.0f, 1.0f, 0.0f});
        uv.insert(uv.end(), {0.0f, 0.0f});
    }
    void triangle(const float a[3], const float b[3], const float c[3]) {
        const uint32_t v = (uint32_t)(pos.size() / 3);
        vertex(a[0], a[1], a[2]), vertex(b[0], b[1], b[2]), vertex(c[0], c[1], c[2]);
        idx.insert(idx.end(), {v, v + 1u, v + 2u});
    }
    template <class F>
    void grid(uint32_t nx, uint32_t nz, F at) {
        const uint32_t base = (uint32_t)(pos.size() / 3);
        for (uint32_t i = 0; i <= nx; ++i)
            for (uint32_t j = 0; j <= nz; ++j) {
                float p[3];
                at(i, j, p);
                vertex(p[0], p[1], p[2]);
            }
        for (uint32_t i = 0; i < nx; ++i)
            for (uint32_t j = 0; j < nz; ++j) {
                const uint32_t v00 = base + i * (nz + 1) + j, v01 = v00 + 1, v10 = v00 + nz + 1, v11 = v10 + 1;
                idx.insert(idx.end(), {v00, v01, v10, v10, v01, v11});
            }
    }
};

Mesh terrain_mesh(uint32_t nx, uint32_t nz) {
    // the draws of numpy's RandomState(4) in heightfield_mesh's order: fx, fz, phase x, phase z, weight
    static const double w[6][5] = {{13.604358068164121, 8.566786990108668, 6.111556079054741, 4.491321348791744, 0.7884101772180896},
                                   {4.593073946964516, 13.715293457314901, 0.039145847961458174, 1.5895350623032367, 0.604354072683112},
                                   {11.35259506152503, 4.3722208952030375, 5.422346418112404, 6.1788886858983805, 0.41468956898328907},
                                   {9.16800732719431, 2.10783317201066, 2.428899003284019, 0.2774658271593975, 0.9696570773999651},
                                   {7.233759762557572, 13.387727681378752, 4.940506217774534, 5.443056192615438, 0.42121579504716367},
                                   {2.8993830441572843, 9.208912656533231, 1.055400356754345, 4.607963493079317, 0.5859107021064103}};
    const double sx = 200.0, sz = 400.0, amp = 12.0, two_pi = 6.283185307179586;
    Mesh m;
    m.grid(nx, nz, [&](uint32_t i, uint32_t j, float* p) {
        const double x = sx * (double)i / (double)nx, z = sz * (double)j / (double)nz;
        double y = 0.0;
        for (const auto& r : w) y += r[4] * std::sin(two_pi * r[0] * x / sx + r[2]) * std::sin(two_pi * r[1] * z / sz + r[3]);
        p[0] = (float)x, p[1] = (float)(amp * y / 3.0), p[2] = (float)z;
    });
    return m;
}
Mesh flat_mesh() {
    Mesh m;
    m.grid(16, 24, [](uint32_t i, uint32_t j, float* p) { p[0] = 0.37f * (float)i - 1.5f, p[1] = 0.0f, p[2] = 0.29f * (float)j - 1.0f; });
    return m;
}
Mesh overlap_mesh() {
    Mesh m;
    for (int i = 0; i < 640; ++i) {
        const float x = 0.1f * (float)i, z = 0.013f * (float)i;
        const float a[3] = {x, 0.0f, z}, b[3] = {x + 5.0f, 1.0f, z + 0.01f}, c[3] = {x + 2.5f, (float)(i % 3), z + 0.5f};
        m.triangle(a, b, c);
    }
    return m;
}
Mesh nested_mesh() {  // tests/test_gpu_traversal.py, test_leaf_with_many_triangles: 13 triangles around one midpoint, above the terrain
    Mesh m = terrain_mesh(16, 32);
    for (int k = 0; k < 13; ++k) {
        const float s = 0.25f * (float)(k + 1), t = 0.125f * (float)((k * 5) % 7) - 0.25f;
        const float a[3] = {100.0f - s, 40.0f - s, 200.0f - t * s}, b[3] = {100.0f + s, 40.0f - s, 200.0f - t * s}, c[3] = {100.0f, 40.0f + s, 200.0f + t * s};
        m.triangle(a, b, c);
    }
    return m;
}
Mesh whole_number_mesh() {  // coordinates 1 .. 33: scaled afterwards
    Mesh m;
    m.grid(16, 32, [](uint32_t i, uint32_t j, float* p) { p[0] = (float)(i + 1u), p[1] = (float)((i * 7u + j * 3u) % 5u + 1u), p[2] = (float)(j + 1u); });
    return m;
}

// ---- a scene: the mesh under an identity instance and a translated one, flattened, scaled, checked, prepared and packed ----
struct Scene {
    std::string name;
    pbrs_host_scene* hs = nullptr;
    pbrs_scene_desc d{};
    std::vector<pbrs_node> tlas, blas;
    std::vector<pbrs_tri_verts> tv;
    PreparedScene P;               // as pbrs_upload_scene uploads it: after pack_wide_leaves
    std::vector<pbrs_wnode> wide0;  // P.wide as prepare_scene left it
    uint32_t root = 0, wroot = 0, packed = 0;
    ~Scene() {
        if (hs) pbrs_host_scene_free(hs);
    }
};

void build(Scene& sc, const char* name, const Mesh& mesh, float scale) {
    sc.name = name;
    pbrs_mesh_spec ms{};
    ms.n_vertices = (uint32_t)(mesh.pos.size() / 3);
    ms.n_triangles = (uint32_t)(mesh.idx.size() / 3);
    ms.positions = mesh.pos.data(), ms.normals = mesh.nrm.data(), ms.uvs = mesh.uv.data(), ms.indices = mesh.idx.data();
    pbrs_shape_spec shape{};
    shape.kind = PBRS_SHAPE_MESH;
    pbrs_material_spec mat{};
    mat.kind = PBRS_MTL_LAMBERTIAN;
    mat.p[0] = mat.p[1] = mat.p[2] = 0.5f;
    pbrs_instance_spec inst[2] = {};
    for (pbrs_instance_spec& in : inst)
        for (int i = 0; i < 4; ++i) in.forward[5 * i] = in.inverse[5 * i] = 1.0f;
    inst[1].forward[13] = 8.0f, inst[1].inverse[13] = -8.0f;  // [col][row]: 8 up (small: the huge scene stays inside the guarded range)
    pbrs_scene_spec spec{};
    spec.n_meshes = 1, spec.meshes = &ms;
    spec.n_shapes = 1, spec.shapes = &shape;
    spec.n_materials = 1, spec.materials = &mat;
    spec.n_instances = 2, spec.instances = inst;
    spec.camera.width = spec.camera.height = 8;
    spec.camera.fov_y_rad = 0.8f;
    spec.camera.target[2] = -1.0f, spec.camera.up[1] = 1.0f;
    spec.env_kind = PBRS_ENV_CONSTANT;
    REQUIRE(pbrs_host_scene_build(&spec, &sc.hs) == PBRS_OK, "%s: pbrs_host_scene_build: %s", name, pbrs_host_last_error());
    sc.d = *pbrs_host_scene_desc(sc.hs);
    sc.tlas.assign(sc.d.tlas_nodes, sc.d.tlas_nodes + sc.d.n_tlas_nodes);
    sc.blas.assign(sc.d.blas_nodes, sc.d.blas_nodes + sc.d.n_blas_nodes);
    sc.tv.assign(sc.d.tri_verts, sc.d.tri_verts + sc.d.n_triangles);
    for (std::vector<pbrs_node>* v : {&sc.tlas, &sc.blas})
        for (pbrs_node& n : *v)
            for (int a = 0; a < 3; ++a) n.min[a] *= scale, n.max[a] *= scale;  // a power of two: exact
    for (pbrs_tri_verts& t : sc.tv)
        for (int a = 0; a < 3; ++a) t.p0[a] *= scale, t.p1[a] *= scale, t.p2[a] *= scale;
    sc.d.tlas_nodes = sc.tlas.data(), sc.d.blas_nodes = sc.blas.data(), sc.d.tri_verts = sc.tv.data();
    const SceneCheck chk = check_scene(sc.d);
    REQUIRE(chk.code == PBRS_OK, "%s: check_scene: %s", name, chk.message);
    sc.P = prepare_scene(sc.d, chk.levels, DevOverrides{});
    REQUIRE(sc.P.S.fast_slab != 0u && sc.P.S.n_flat == 2u, "%s: fast_slab %u, %u scanned leaves", name, sc.P.S.fast_slab, sc.P.S.n_flat);
    REQUIRE(!sc.P.wide.empty() && sc.P.facts.wide_ok, "%s: the scene got no wide nodes (%u levels)", name, sc.P.wide_levels);
    REQUIRE(sc.P.S.n_wnodes == sc.P.wide.size(), "%s: n_wnodes %u, %zu wide nodes", name, sc.P.S.n_wnodes, sc.P.wide.size());
    REQUIRE(sc.P.tri_leaf.size() == sc.d.n_triangles, "%s: tri_leaf has %zu entries for %u triangles", name, sc.P.tri_leaf.size(), sc.d.n_triangles);
    sc.wide0 = sc.P.wide;
    sc.packed = pack_wide_leaves(sc.P);
    REQUIRE(sc.P.wide.size() == sc.wide0.size(), "%s: packing changed the number of wide nodes", name);
    sc.root = sc.P.inst[0].blas_root;
    sc.wroot = sc.P.inst[0].pad[1];
    REQUIRE(sc.P.inst[0].shape_kind == PBRS_SHAPE_MESH && sc.wroot != PBRS_WREF_NONE, "%s: instance 0 is the mesh, with a wide root", name);
}

// ---- the references ----
bool is_packed(uint32_t ref) { return ref != PBRS_WREF_NONE && (ref & PBRS_WREF_LEAF) && (ref & PBRS_WREF_PACKED); }
uint32_t packed_first(uint32_t ref) { return ref & PBRS_WREF_TRI; }
uint32_t packed_count(uint32_t ref) { return ((ref >> PBRS_WREF_COUNT_SHIFT) & (PBRS_WREF_COUNT_MAX - 1u)) + 1u; }

struct RefCount {
    uint32_t leaves = 0, packed = 0, many = 0;
};
// wide node wi stands for the inner node x of P.nodes (build_wide's slots, restated)
void check_refs(const Scene& sc, uint32_t wi, uint32_t x, RefCount& rc) {
    const std::vector<pbrs_node>& n = sc.P.nodes;
    REQUIRE(wi < sc.P.wide.size(), "%s: wide index %u out of %zu", sc.name.c_str(), wi, sc.P.wide.size());
    const pbrs_wnode &w = sc.P.wide[wi], &w0 = sc.wide0[wi];
    REQUIRE(std::memcmp(w.lo, w0.lo, sizeof w.lo) == 0 && std::memcmp(w.hi, w0.hi, sizeof w.hi) == 0, "%s: wide node %u: packing touched the planes", sc.name.c_str(), wi);
    const uint32_t child[2] = {x + 1u, n[x].a};
    uint32_t slot_node[4] = {0, 0, 0, 0};
    bool used[4] = {false, false, false, false};
    for (uint32_t s = 0; s < 2; ++s) {
        const pbrs_node& ch = n[child[s]];
        if (ch.b & PBRS_LEAF_FLAG) slot_node[2 * s] = child[s], used[2 * s] = true;
        else slot_node[2 * s] = child[s] + 1u, slot_node[2 * s + 1] = ch.a, used[2 * s] = used[2 * s + 1] = true;
    }
    for (uint32_t k = 0; k < 4; ++k) {
        if (!used[k]) {
            REQUIRE(w.child[k] == PBRS_WREF_NONE, "%s: wide node %u slot %u: unused slot names %08x", sc.name.c_str(), wi, k, w.child[k]);
            continue;
        }
        const uint32_t above = ~(PBRS_WREF_INDEX);  // leaf bit and axis bits
        REQUIRE(((w.child[k] ^ w0.child[k]) & above) == 0u, "%s: wide node %u slot %u: packing changed the bits above the index: %08x -> %08x", sc.name.c_str(), wi, k,
                w0.child[k], w.child[k]);
        const pbrs_node& leaf = n[slot_node[k]];
        if (!(leaf.b & PBRS_LEAF_FLAG)) {
            REQUIRE(w.child[k] == w0.child[k] && !(w.child[k] & PBRS_WREF_LEAF), "%s: wide node %u slot %u: inner reference %08x -> %08x", sc.name.c_str(), wi, k, w0.child[k],
                    w.child[k]);
            check_refs(sc, w.child[k] & PBRS_WREF_INDEX, slot_node[k], rc);
            continue;
        }
        ++rc.leaves;
        REQUIRE((w0.child[k] & PBRS_WREF_INDEX) == slot_node[k], "%s: wide node %u slot %u: prepare_scene's reference %08x, node %u", sc.name.c_str(), wi, k, w0.child[k], slot_node[k]);
        const uint32_t cnt = leaf.b & ~PBRS_LEAF_FLAG;
        const bool should_pack = cnt >= 1u && cnt <= PBRS_WREF_COUNT_MAX && leaf.a <= PBRS_WREF_TRI;
        REQUIRE(is_packed(w.child[k]) == should_pack, "%s: wide node %u slot %u: leaf %u of %u triangles from %u has reference %08x", sc.name.c_str(), wi, k, slot_node[k], cnt,
                leaf.a, w.child[k]);
        if (!should_pack) {
            REQUIRE(w.child[k] == w0.child[k], "%s: wide node %u slot %u: a leaf that keeps the node form was rewritten", sc.name.c_str(), wi, k);
            rc.many += cnt > PBRS_WREF_COUNT_MAX ? 1u : 0u;
            continue;
        }
        ++rc.packed;
        const uint32_t first = packed_first(w.child[k]), count = packed_count(w.child[k]);
        REQUIRE(first == leaf.a && count == cnt, "%s: wide node %u slot %u: decodes to [%u, +%u), the leaf holds [%u, +%u)", sc.name.c_str(), wi, k, first, count, leaf.a, cnt);
        REQUIRE((uint64_t)first + count <= sc.d.n_triangles, "%s: wide node %u slot %u: [%u, +%u) leaves the %u triangles", sc.name.c_str(), wi, k, first, count, sc.d.n_triangles);
        for (uint32_t j = 0; j < count; ++j)
            REQUIRE(sc.P.tri_leaf[first + j] == slot_node[k], "%s: tri_leaf[%u] = %u, the packed leaf is node %u", sc.name.c_str(), first + j, sc.P.tri_leaf[first + j], slot_node[k]);
    }
}

void check_tri_leaf(const Scene& sc) {
    const std::vector<pbrs_node>& n = sc.P.nodes;
    std::vector<uint32_t> holders(sc.d.n_triangles, 0u);
    for (uint32_t i = sc.root; i < n.size(); ++i)
        if (n[i].b & PBRS_LEAF_FLAG)
            for (uint32_t t = n[i].a; t < n[i].a + (n[i].b & ~PBRS_LEAF_FLAG); ++t) ++holders[t];
    for (uint32_t t = 0; t < sc.d.n_triangles; ++t) {
        const uint32_t li = sc.P.tri_leaf[t];
        if (holders[t] == 0u) {
            REQUIRE(li == 0xffffffffu, "%s: tri_leaf[%u] = %u for a triangle no leaf holds", sc.name.c_str(), t, li);
            continue;
        }
        REQUIRE(li >= sc.root && li < n.size() && (n[li].b & PBRS_LEAF_FLAG), "%s: tri_leaf[%u] = %u is not a BLAS leaf", sc.name.c_str(), t, li);
        REQUIRE(t >= n[li].a && t < n[li].a + (n[li].b & ~PBRS_LEAF_FLAG), "%s: tri_leaf[%u] = %u, whose range is [%u, +%u)", sc.name.c_str(), t, li, n[li].a,
                n[li].b & ~PBRS_LEAF_FLAG);
    }
}

// the leaves that must keep the node form, forged on copies of a prepared scene; and the extremes of the triangle field
void check_forged(const Scene& sc) {
    // the first reference to a packable leaf
    uint32_t at_w = 0, at_k = 0, leaf = 0xffffffffu;
    for (uint32_t wi = 0; wi < sc.P.wide.size() && leaf == 0xffffffffu; ++wi)
        for (uint32_t k = 0; k < 4; ++k)
            if (is_packed(sc.P.wide[wi].child[k])) {
                at_w = wi, at_k = k, leaf = sc.wide0[wi].child[k] & PBRS_WREF_INDEX;
                break;
            }
    REQUIRE(leaf != 0xffffffffu, "%s: no packed reference", sc.name.c_str());
    auto repack = [&](uint32_t a, uint32_t cnt, size_t table) {
        PreparedScene Q = sc.P;
        Q.wide = sc.wide0;
        Q.nodes[leaf].a = a;
        Q.nodes[leaf].b = PBRS_LEAF_FLAG | cnt;
        if (table) {
            Q.tri_leaf.assign(table, 0xffffffffu);
            for (uint32_t j = 0; j < cnt && (size_t)a + j < table; ++j) Q.tri_leaf[a + j] = leaf;
        }
        pack_wide_leaves(Q);
        return Q.wide[at_w].child[at_k];
    };
    const uint32_t old_form = sc.wide0[at_w].child[at_k];
    REQUIRE(repack(sc.P.nodes[leaf].a, 0u, 0) == old_form, "%s: an empty leaf was packed", sc.name.c_str());
    REQUIRE(repack(sc.P.nodes[leaf].a, 5u, sc.P.tri_leaf.size() + 8u) == old_form, "%s: a leaf of five triangles was packed", sc.name.c_str());
    const size_t field = (size_t)1 << PBRS_WREF_TRI_BITS;
    REQUIRE(repack((uint32_t)field, 1u, field + 4u) == old_form, "%s: a leaf at triangle 2^24 was packed", sc.name.c_str());
    const uint32_t last = repack((uint32_t)field - 1u, 1u, field + 4u);
    REQUIRE(is_packed(last) && packed_first(last) == field - 1u && packed_count(last) == 1u && ((last ^ old_form) & ~PBRS_WREF_INDEX) == 0u,
            "%s: a leaf at triangle 2^24 - 1 has reference %08x", sc.name.c_str(), last);
    const uint32_t four = repack((uint32_t)field - 4u, 4u, field + 4u);
    REQUIRE(is_packed(four) && packed_first(four) == field - 4u && packed_count(four) == 4u, "%s: four triangles up to 2^24 - 1: reference %08x", sc.name.c_str(), four);
    // a triangle that tri_leaf gives to another leaf (a description whose leaves share a record): the node form
    {
        PreparedScene Q = sc.P;
        Q.wide = sc.wide0;
        Q.tri_leaf[Q.nodes[leaf].a] = leaf + 1u;
        pack_wide_leaves(Q);
        REQUIRE(Q.wide[at_w].child[at_k] == old_form, "%s: a leaf whose triangle the table gives to another leaf was packed", sc.name.c_str());
    }
}

void check_layout_constants() {
    REQUIRE((PBRS_WREF_LEAF | (15u << PBRS_WREF_AXIS_SHIFT) | PBRS_WREF_PACKED | (3u << PBRS_WREF_COUNT_SHIFT) | PBRS_WREF_TRI) == 0xffffffffu, "the fields do not fill the word");
    REQUIRE((PBRS_WREF_PACKED & (3u << PBRS_WREF_COUNT_SHIFT)) == 0u && (PBRS_WREF_PACKED & PBRS_WREF_TRI) == 0u && ((3u << PBRS_WREF_COUNT_SHIFT) & PBRS_WREF_TRI) == 0u,
            "the fields overlap");
    REQUIRE(PBRS_WREF_TRI >= (1u << 24) - 1u, "a mesh of 2^24 triangles does not fit the field");
    REQUIRE(sizeof(DevScene) % 8u == 0u && offsetof(DevScene, n_wnodes) + sizeof(uint32_t) == sizeof(DevScene), "n_wnodes is not the structure's last word");
}

// ---- the walks (device/traverse.h: RaySpace, qdiv, slab_rs; device/wide.h: wide_test, wide_order_any, wide_push; AnyWalkW) ----
struct Ray {
    float o[3], d[3], nr[3], r32[3], t_max;
};
Ray make_ray(const float o[3], const float d[3], float t_max) {
    Ray r;
    for (int a = 0; a < 3; ++a) r.o[a] = o[a], r.d[a] = d[a], r.nr[a] = -(1.0f / d[a]), r.r32[a] = 1.0f / d[a];
    r.t_max = t_max;
    return r;
}
bool in_range(const Ray& r) {  // the guarded range of the division-free test: the wide walk takes no other ray
    for (int a = 0; a < 3; ++a) {
        const uint32_t e = (pn_bits(r.d[a]) >> 23) & 0xffu, u = pn_bits(r.o[a]) & 0x7fffffffu;
        if (!(e - (127u - 40u) <= 80u) || !(u == 0u || (u >> 23) - (127u - 60u) <= 100u)) return false;
    }
    return true;
}
float qdiv(float nn, float d, float nr) {
    const float q0 = nn * nr;
    const float e = __builtin_fmaf(d, q0, nn);
    return __builtin_fmaf(e, nr, q0);
}
bool slab(const pbrs_node& n, const Ray& R, float* entry = nullptr) {
    float t0[3], t1[3];
    for (int a = 0; a < 3; ++a) t0[a] = qdiv(R.o[a] - n.min[a], R.d[a], R.nr[a]), t1[a] = qdiv(R.o[a] - n.max[a], R.d[a], R.nr[a]);
    const float lo_el = std::fmax(std::fmax(std::fmin(t0[0], t1[0]), std::fmin(t0[1], t1[1])), std::fmin(t0[2], t1[2]));
    const float hi_el = std::fmin(std::fmin(std::fmax(t0[0], t1[0]), std::fmax(t0[1], t1[1])), std::fmax(t0[2], t1[2]));
    const float t_low = std::fmax(lo_el, 0.0f);
    if (entry) *entry = t_low;
    return t_low <= std::fmin(hi_el, R.t_max);
}
// any one deterministic predicate serves (every walk runs the same one): pure arithmetic on the ray and the record
bool tri_pred(const pbrs_tri_verts& tv, const Ray& R) {
    double e1[3], e2[3], p[3], s[3], q[3];
    for (int a = 0; a < 3; ++a) e1[a] = (double)tv.p1[a] - tv.p0[a], e2[a] = (double)tv.p2[a] - tv.p0[a], s[a] = (double)R.o[a] - tv.p0[a];
    p[0] = R.d[1] * e2[2] - R.d[2] * e2[1], p[1] = R.d[2] * e2[0] - R.d[0] * e2[2], p[2] = R.d[0] * e2[1] - R.d[1] * e2[0];
    const double det = e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2];
    if (det == 0.0 || !(det == det)) return false;
    const double u = (s[0] * p[0] + s[1] * p[1] + s[2] * p[2]) / det;
    if (!(u >= 0.0 && u <= 1.0)) return false;
    q[0] = s[1] * e1[2] - s[2] * e1[1], q[1] = s[2] * e1[0] - s[0] * e1[2], q[2] = s[0] * e1[1] - s[1] * e1[0];
    const double v = (R.d[0] * q[0] + R.d[1] * q[1] + R.d[2] * q[2]) / det;
    if (!(v >= 0.0 && u + v <= 1.0)) return false;
    const float t = (float)((e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) / det);
    return t > 1e-4f && t < R.t_max;
}

struct Arrays {  // what the walks read
    const std::vector<pbrs_node>* nodes;
    const std::vector<pbrs_wnode>* wide;
    const std::vector<uint32_t>* tri_leaf;
    const std::vector<pbrs_tri_verts>* tv;
    uint32_t root, wroot;
};
struct Tally {
    uint64_t leaves = 0, tris = 0, boxes = 0, tri_passed_box_failed = 0;
};

// the binary any-hit walk: the definition — some leaf whose own box passes holds a triangle that passes
bool walk_binary(const Arrays& A, const Ray& R) {
    std::vector<uint32_t> stack = {A.root};
    while (!stack.empty()) {
        const uint32_t ni = stack.back();
        stack.pop_back();
        const pbrs_node& X = (*A.nodes)[ni];
        if (!slab(X, R)) continue;
        if (!(X.b & PBRS_LEAF_FLAG)) {
            const bool left_first = R.d[X.b & 3u] > 0.0f;
            stack.push_back(left_first ? X.a : ni + 1u);
            stack.push_back(left_first ? ni + 1u : X.a);
            continue;
        }
        for (uint32_t j = 0; j < (X.b & ~PBRS_LEAF_FLAG); ++j)
            if (tri_pred((*A.tv)[X.a + j], R)) return true;
    }
    return false;
}

// the four-wide walk inside the mesh; triangles_first: AnyWalkW's leaf step, else the one it replaces (every leaf verified first)
bool walk_wide(const Arrays& A, const Ray& R, bool triangles_first, Tally& tally) {
    const std::vector<pbrs_node>& nodes = *A.nodes;
    if (!slab(nodes[A.root], R)) return false;  // xfer_step: the root's own test
    std::vector<uint32_t> stack = {A.wroot};
    while (!stack.empty()) {
        const uint32_t e = stack.back();
        stack.pop_back();
        if (e & PBRS_WREF_LEAF) {
            ++tally.leaves;
            uint32_t first, count;
            bool verified = false;
            if (e & PBRS_WREF_PACKED) {
                first = packed_first(e), count = packed_count(e);
                if (!triangles_first) {  // the old order, through the table
                    ++tally.boxes;
                    if (!slab(nodes[(*A.tri_leaf)[first]], R)) continue;
                    verified = true;
                }
            } else {  // the node form: leaf_wave's prologue
                const pbrs_node& leaf = nodes[e & PBRS_WREF_INDEX];
                ++tally.boxes;
                if (!slab(leaf, R)) continue;
                first = leaf.a, count = leaf.b & ~PBRS_LEAF_FLAG;
                verified = true;
            }
            for (uint32_t j = 0; j < count; ++j) {
                ++tally.tris;
                if (!tri_pred((*A.tv)[first + j], R)) continue;
                if (verified) return true;
                ++tally.boxes;
                if (slab(nodes[(*A.tri_leaf)[first + j]], R)) return true;
                ++tally.tri_passed_box_failed;
                break;  // the leaf contributes nothing: its other triangles are skipped
            }
            continue;
        }
        const pbrs_wnode& w = (*A.wide)[e & PBRS_WREF_INDEX];
        bool pass[4];
        for (uint32_t k = 0; k < 4; ++k) {
            float nearp[3], farp[3];
            for (int a = 0; a < 3; ++a) nearp[a] = R.d[a] > 0.0f ? w.lo[a][k] : w.hi[a][k], farp[a] = R.d[a] > 0.0f ? w.hi[a][k] : w.lo[a][k];
            pass[k] = pn_slab_filter(nearp[0], nearp[1], nearp[2], farp[0], farp[1], farp[2], R.o[0], R.o[1], R.o[2], R.r32[0], R.r32[1], R.r32[2], R.t_max) != 0;
        }
        const bool sx = !(R.d[(w.child[0] >> PBRS_WREF_AXIS_SHIFT) & 3u] > 0.0f);
        for (uint32_t v = 4; v-- > 0;) {  // visiting order: slots 0..3, or 3..0; pushed last-first
            const uint32_t k = sx ? 3u - v : v;
            if (!pass[k]) continue;
            const uint32_t axis_bits = k == 0 ? 15u << PBRS_WREF_AXIS_SHIFT : k == 2 ? 3u << PBRS_WREF_AXIS_SHIFT : 0u;
            stack.push_back(w.child[k] & ~axis_bits);
        }
    }
    return false;
}

// ---- rays over the terrain ----
std::vector<Ray> make_rays(const Scene& sc, uint32_t per_kind) {
    std::vector<Ray> rays;
    Rng rng{0x5ade0001ull};
    const pbrs_node& box = sc.P.nodes[sc.root];
    float ext[3], mid[3];
    for (int a = 0; a < 3; ++a) ext[a] = box.max[a] - box.min[a], mid[a] = 0.5f * (box.max[a] + box.min[a]);
    const float size = std::fmax(ext[0], std::fmax(ext[1], ext[2])), inf = INFINITY;
    std::vector<uint32_t> leaves;
    for (uint32_t i = sc.root; i < sc.P.nodes.size(); ++i)
        if (sc.P.nodes[i].b & PBRS_LEAF_FLAG) leaves.push_back(i);
    auto add = [&](const float* o, const float* d, float t_max) {
        const Ray r = make_ray(o, d, t_max);
        if (in_range(r)) rays.push_back(r);
    };
    auto surface_point = [&](float* o) {
        const pbrs_tri_verts& t = sc.tv[rng.below((uint32_t)sc.tv.size())];
        float u = rng.uniform(0.0f, 1.0f), v = rng.uniform(0.0f, 1.0f);
        if (u + v > 1.0f) u = 1.0f - u, v = 1.0f - v;
        for (int a = 0; a < 3; ++a) o[a] = t.p0[a] + u * (t.p1[a] - t.p0[a]) + v * (t.p2[a] - t.p0[a]);
    };
    for (uint32_t i = 0; i < per_kind; ++i) {  // from the surface upward: towards the sky, most leave unoccluded
        float o[3], d[3] = {rng.uniform(-1.0f, 1.0f), rng.uniform(0.05f, 1.0f), rng.uniform(-1.0f, 1.0f)};
        surface_point(o);
        add(o, d, (i & 3u) ? inf : rng.uniform(0.02f, 1.0f) * size);
    }
    for (uint32_t i = 0; i < per_kind; ++i) {  // grazing along it: nearly horizontal, from a little above the surface
        float o[3], d[3] = {rng.uniform(-1.0f, 1.0f), rng.uniform(-0.08f, 0.08f), rng.uniform(-1.0f, 1.0f)};
        surface_point(o);
        o[1] += rng.uniform(0.0f, 0.5f);
        add(o, d, (i & 1u) ? inf : rng.uniform(0.02f, 1.0f) * size);
    }
    for (uint32_t i = 0; i < per_kind; ++i) {  // through a corner of a leaf's box, from outside the mesh
        const pbrs_node& leaf = sc.P.nodes[leaves[rng.below((uint32_t)leaves.size())]];
        float o[3], d[3], c[3];
        const uint32_t pick = rng.below(8);
        for (int a = 0; a < 3; ++a) c[a] = (pick >> a) & 1u ? leaf.max[a] : leaf.min[a];
        for (int a = 0; a < 3; ++a) o[a] = mid[a] + rng.uniform(-1.0f, 1.0f) * size;
        o[1] = box.max[1] + rng.uniform(0.1f, 0.6f) * size;
        for (int a = 0; a < 3; ++a) d[a] = (c[a] - o[a]) / size;
        add(o, d, (i & 1u) ? inf : 2.0f * size);
    }
    for (uint32_t i = 0; i < per_kind; ++i) {  // t_max equal to the distance at which the ray enters a leaf's box
        const pbrs_node& leaf = sc.P.nodes[leaves[rng.below((uint32_t)leaves.size())]];
        float o[3], d[3];
        for (int a = 0; a < 3; ++a) o[a] = mid[a] + rng.uniform(-0.7f, 0.7f) * ext[a];
        o[1] = box.max[1] + rng.uniform(0.05f, 0.5f) * size;
        for (int a = 0; a < 3; ++a) d[a] = (leaf.min[a] + rng.uniform(0.0f, 1.0f) * (leaf.max[a] - leaf.min[a]) - o[a]) / size;
        Ray probe = make_ray(o, d, inf);
        float entry = 0.0f;
        if (!in_range(probe) || !slab(leaf, probe, &entry) || !(entry > 0.0f)) continue;
        add(o, d, (i % 3u) == 0u ? entry : (i % 3u) == 1u ? std::nextafterf(entry, inf) : std::nextafterf(entry, 0.0f));
    }
    return rays;
}

struct Outcome {
    uint64_t rays = 0, occluded = 0;
    Tally first, verify;
};
Outcome compare(const Scene& sc, const Arrays& A, const std::vector<Ray>& rays, const char* what) {
    Outcome out;
    for (const Ray& r : rays) {
        const bool def = walk_binary(A, r);
        const bool a = walk_wide(A, r, false, out.verify), b = walk_wide(A, r, true, out.first);
        REQUIRE(a == def && b == def, "%s, %s: ray %zu: the binary walk says %d, the wide walk %d verify-first and %d triangles-first", sc.name.c_str(), what,
                (size_t)(&r - rays.data()), (int)def, (int)a, (int)b);
        ++out.rays;
        out.occluded += def ? 1u : 0u;
    }
    return out;
}

void run_walks(const Scene& sc) {
    const std::vector<Ray> rays = make_rays(sc, 30000);
    REQUIRE(rays.size() >= 100000, "%s: %zu rays", sc.name.c_str(), rays.size());
    const Arrays natural{&sc.P.nodes, &sc.P.wide, &sc.P.tri_leaf, &sc.tv, sc.root, sc.wroot};
    const Outcome n = compare(sc, natural, rays, "natural boxes");
    REQUIRE(n.occluded * 10u >= n.rays && (n.rays - n.occluded) * 10u >= 3u * n.rays, "%s: %llu of %llu rays occluded", sc.name.c_str(), (unsigned long long)n.occluded,
            (unsigned long long)n.rays);
    REQUIRE(n.first.leaves >= n.verify.leaves && n.first.tris >= n.verify.tris && n.first.boxes < n.verify.boxes, "%s: triangles-first tests %llu leaf boxes, verify-first %llu",
            sc.name.c_str(), (unsigned long long)n.first.boxes, (unsigned long long)n.verify.boxes);
    std::printf("%s walks, natural boxes: rays %llu, occluded %llu, leaves per ray %.2f, leaf box tests per ray %.2f -> %.2f, triangle tests per ray %.2f -> %.2f, "
                "triangle passed and box failed %llu\n",
                sc.name.c_str(), (unsigned long long)n.rays, (unsigned long long)n.occluded, (double)n.first.leaves / n.rays, (double)n.verify.boxes / n.rays,
                (double)n.first.boxes / n.rays, (double)n.verify.tris / n.rays, (double)n.first.tris / n.rays, (unsigned long long)n.first.tri_passed_box_failed);
    // leaf boxes shrunk to the middle half on x and z (still inside their parents; the wide slots keep the natural boxes)
    std::vector<pbrs_node> shrunk = sc.P.nodes;
    for (uint32_t i = sc.root; i < shrunk.size(); ++i)
        if (shrunk[i].b & PBRS_LEAF_FLAG)
            for (int a = 0; a < 3; a += 2) {
                const float lo = shrunk[i].min[a], hi = shrunk[i].max[a], q = 0.25f * (hi - lo);
                shrunk[i].min[a] = lo + q, shrunk[i].max[a] = hi - q;
            }
    const Arrays forged{&shrunk, &sc.P.wide, &sc.P.tri_leaf, &sc.tv, sc.root, sc.wroot};
    const Outcome s = compare(sc, forged, rays, "shrunk boxes");
    REQUIRE(s.first.tri_passed_box_failed > 0u, "%s: shrunk boxes: the branch 'triangle passed, box failed' was never taken", sc.name.c_str());
    REQUIRE(s.occluded > 0u && s.occluded < n.occluded, "%s: shrunk boxes: %llu rays occluded, %llu with natural boxes", sc.name.c_str(), (unsigned long long)s.occluded,
            (unsigned long long)n.occluded);
    std::printf("%s walks, shrunk boxes: rays %llu, occluded %llu, triangle passed and box failed %llu\n", sc.name.c_str(), (unsigned long long)s.rays,
                (unsigned long long)s.occluded, (unsigned long long)s.first.tri_passed_box_failed);
}

void run(const char* name, const Mesh& mesh, float scale, bool many, bool walks) {
    Scene sc;
    build(sc, name, mesh, scale);
    RefCount rc;
    check_refs(sc, sc.wroot, sc.root, rc);
    REQUIRE(rc.packed == sc.packed && rc.packed > 0u, "%s: %u packed references found, pack_wide_leaves reported %u", name, rc.packed, sc.packed);
    REQUIRE((rc.many > 0u) == many, "%s: %u leaves of more than four triangles", name, rc.many);
    check_tri_leaf(sc);
    check_forged(sc);
    std::printf("%s: triangles %u, wide nodes %zu, leaves %u, packed %u, many-triangle leaves %u\n", name, sc.d.n_triangles, sc.P.wide.size(), rc.leaves, rc.packed, rc.many);
    if (walks) run_walks(sc);
}

}  // namespace

int main() {
    check_layout_constants();
    run("terrain", terrain_mesh(16, 32), 1.0f, false, true);
    run("flat", flat_mesh(), 1.0f, false, false);
    run("overlap", overlap_mesh(), 1.0f, false, false);
    run("nested", nested_mesh(), 1.0f, true, false);
    run("tiny", whole_number_mesh(), 0x1p-60f, false, false);
    run("huge", whole_number_mesh(), 0x1p34f, false, false);
    std::printf("ok\n");
    return 0;
}
