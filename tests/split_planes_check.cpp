// tests/split_planes_check.cpp — the split planes of the inner BLAS nodes (pbrs_amd/csrc/device/split_planes.h, chosen by
// host/scene_prepare.cpp) and the cull the closest-hit walk makes with them (device/traverse.h, ClosestWalk::cull_children), on a CPU:
// a program of its own that tests/test_split_planes.py compiles with -fsanitize=address,undefined and runs.
//
// Scenes come from pbrs_host_scene_build (the reference's half-area builder), one mesh each under an identity instance:
//   five        5 triangles: one inner node
//   overlap     long triangles whose boxes overlap heavily on the split axis
//   flat        a grid at height 0: zero extent on y
//   tiny, huge  a grid on whole numbers, every node and vertex coordinate then scaled (exactly) by 2^-60 / 2^34: coordinates from 2^-60, up to 2^39
//   terrain     the C4 family's height field (pbrs_amd/scenes.py, heightfield_mesh with seed 4) at nx = 64, nz = 128
// Checked, per scene:
//   planes   for every inner BLAS node X on axis k: down(qd) <= R.min[k] and up(qu) >= L.max[k], evaluated with the header's own
//            expressions; each q is the largest that does (or 0); leaves and TLAS nodes carry 0; the packed word leaves bits 0, 1, 30, 31 alone
//   walk     a restatement of the mesh-local closest-hit walk (near-first, box tests at pop time, the division-free quotient) runs
//            every ray twice, without and with the cull: (t, prim) must be identical, and every child the cull drops must fail its
//            own box test against the best hit of that moment (an upper bound of every extent it could be popped with).
//            Rays: from the surface (triangle centroids and vertices) and from outside, random and axis-near directions, all sign
//            combinations, origins exactly on a stored plane, and a few outside the guarded range (never culled).
// Prints pops and failed pops per ray, before and after.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/pbrs_host.h"
#include "../pbrs_amd/csrc/device/split_planes.h"
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
    // (nx x nz) cells, vertex (i, j) at `at(i, j)`
    template <class F>
    void grid(uint32_t nx, uint32_t nz, F at) {
        for (uint32_t i = 0; i <= nx; ++i)
            for (uint32_t j = 0; j <= nz; ++j) {
                float p[3];
                at(i, j, p);
                vertex(p[0], p[1], p[2]);
            }
        for (uint32_t i = 0; i < nx; ++i)
            for (uint32_t j = 0; j < nz; ++j) {
                const uint32_t v00 = i * (nz + 1) + j, v01 = v00 + 1, v10 = v00 + nz + 1, v11 = v10 + 1;
                idx.insert(idx.end(), {v00, v01, v10, v10, v01, v11});
            }
    }
};

Mesh five_mesh() {
    Mesh m;
    for (int i = 0; i < 5; ++i) {
        const float x = (float)i * 1.5f - 3.0f, a[3] = {x, 0.1f * (float)i, -1.0f}, b[3] = {x + 1.0f, 0.3f, 1.0f}, c[3] = {x + 0.5f, 1.0f + 0.2f * (float)i, 0.25f};
        m.triangle(a, b, c);
    }
    return m;
}
Mesh overlap_mesh() {
    Mesh m;
    for (int i = 0; i < 48; ++i) {
        const float x = 0.1f * (float)i, z = 0.013f * (float)i;
        const float a[3] = {x, 0.0f, z}, b[3] = {x + 5.0f, 1.0f, z + 0.01f}, c[3] = {x + 2.5f, (float)(i % 3), z + 0.5f};
        m.triangle(a, b, c);
    }
    return m;
}
Mesh flat_mesh() {
    Mesh m;
    m.grid(9, 7, [](uint32_t i, uint32_t j, float* p) { p[0] = 0.37f * (float)i - 1.5f, p[1] = 0.0f, p[2] = 0.29f * (float)j - 1.0f; });
    return m;
}
Mesh whole_number_mesh() {  // coordinates 1 .. 33: scaled afterwards
    Mesh m;
    m.grid(16, 32, [](uint32_t i, uint32_t j, float* p) { p[0] = (float)(i + 1u), p[1] = (float)((i * 7u + j * 3u) % 5u + 1u), p[2] = (float)(j + 1u); });
    return m;
}
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

// ---- a scene: the mesh under an identity instance, flattened, its node and vertex coordinates scaled, checked and prepared ----
struct Scene {
    std::string name;
    pbrs_host_scene* hs = nullptr;
    pbrs_scene_desc d{};
    std::vector<pbrs_node> tlas, blas;
    std::vector<pbrs_tri_verts> tv;
    PreparedScene P;
    float scale = 1.0f;
    uint32_t root = 0;
    ~Scene() {
        if (hs) pbrs_host_scene_free(hs);
    }
};

void build(Scene& sc, const char* name, const Mesh& mesh, float scale) {
    sc.name = name;
    sc.scale = scale;
    pbrs_mesh_spec ms{};
    ms.n_vertices = (uint32_t)(mesh.pos.size() / 3);
    ms.n_triangles = (uint32_t)(mesh.idx.size() / 3);
    ms.positions = mesh.pos.data(), ms.normals = mesh.nrm.data(), ms.uvs = mesh.uv.data(), ms.indices = mesh.idx.data();
    pbrs_shape_spec shape{};
    shape.kind = PBRS_SHAPE_MESH;
    pbrs_material_spec mat{};
    mat.kind = PBRS_MTL_LAMBERTIAN;
    mat.p[0] = mat.p[1] = mat.p[2] = 0.5f;
    pbrs_instance_spec inst{};
    for (int i = 0; i < 4; ++i) inst.forward[5 * i] = inst.inverse[5 * i] = 1.0f;
    pbrs_scene_spec spec{};
    spec.n_meshes = 1, spec.meshes = &ms;
    spec.n_shapes = 1, spec.shapes = &shape;
    spec.n_materials = 1, spec.materials = &mat;
    spec.n_instances = 1, spec.instances = &inst;
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
    REQUIRE(sc.P.S.fast_slab != 0u, "%s: the scene's coordinates are outside the guarded range", name);
    REQUIRE(sc.P.node_planes.size() == sc.P.nodes.size(), "%s: one plane word per node", name);
    REQUIRE(sc.P.inst[0].shape_kind == PBRS_SHAPE_MESH, "%s: instance 0 is the mesh", name);
    sc.root = sc.P.inst[0].blas_root;
}

// ---- the planes ----
struct PlaneCount {
    uint32_t inner = 0, with_planes = 0;
};
PlaneCount check_planes(const Scene& sc) {
    const std::vector<pbrs_node>& n = sc.P.nodes;
    PlaneCount c;
    for (size_t i = 0; i < n.size(); ++i) {
        const uint32_t w = sc.P.node_planes[i];
        REQUIRE((w & 0xc0000003u) == 0u, "%s: node %zu: plane word %08x touches the axis or flag bits", sc.name.c_str(), i, w);
        const bool blas_inner = i >= sc.root && !(n[i].b & PBRS_LEAF_FLAG);
        if (!blas_inner) {
            REQUIRE(w == 0u, "%s: node %zu is a leaf or a TLAS node and carries planes %08x", sc.name.c_str(), i, w);
            continue;
        }
        ++c.inner;
        c.with_planes += w != 0u ? 1u : 0u;
        const pbrs_node &X = n[i], &L = n[i + 1], &R = n[X.a];
        const uint32_t k = X.b & 3u, qd = pbrs_plane_qd(w), qu = pbrs_plane_qu(w);
        REQUIRE(pbrs_plane_pack(qd, qu) == w, "%s: node %zu: pack / unpack", sc.name.c_str(), i);
        const float step = pbrs_plane_step(X.min[k], X.max[k]);
        REQUIRE(pbrs_plane_down(qd, step, X.min[k]) <= R.min[k], "%s: node %zu: down(%u) = %a above R.min = %a", sc.name.c_str(), i, qd,
                (double)pbrs_plane_down(qd, step, X.min[k]), (double)R.min[k]);
        REQUIRE(pbrs_plane_up(qu, step, X.max[k]) >= L.max[k], "%s: node %zu: up(%u) = %a below L.max = %a", sc.name.c_str(), i, qu,
                (double)pbrs_plane_up(qu, step, X.max[k]), (double)L.max[k]);
        REQUIRE(pbrs_plane_down(0u, step, X.min[k]) == X.min[k] && pbrs_plane_up(0u, step, X.max[k]) == X.max[k], "%s: node %zu: q = 0 is the box", sc.name.c_str(), i);
        if (qd != 0u && qd < PBRS_PLANE_MAX) REQUIRE(!(pbrs_plane_down(qd + 1u, step, X.min[k]) <= R.min[k]), "%s: node %zu: qd = %u is not the largest", sc.name.c_str(), i, qd);
        if (qu != 0u && qu < PBRS_PLANE_MAX) REQUIRE(!(pbrs_plane_up(qu + 1u, step, X.max[k]) >= L.max[k]), "%s: node %zu: qu = %u is not the largest", sc.name.c_str(), i, qu);
    }
    return c;
}

// ---- the walk (device/traverse.h: RaySpace, qdiv, slab_rs, ClosestWalk::node_step inside one BLAS) ----
struct Ray {
    float o[3], d[3], nr[3];
    bool fast;
};
bool dir_in_range(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    const uint32_t e = (u >> 23) & 0xffu;
    return e - (127u - 40u) <= 80u;
}
bool origin_in_range(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    u &= 0x7fffffffu;
    return u == 0u || (u >> 23) - (127u - 60u) <= 100u;
}
Ray make_ray(const float o[3], const float d[3]) {
    Ray r;
    r.fast = true;
    for (int a = 0; a < 3; ++a) {
        r.o[a] = o[a], r.d[a] = d[a];
        r.fast = r.fast && dir_in_range(d[a]) && origin_in_range(o[a]);
    }
    for (int a = 0; a < 3; ++a) r.nr[a] = r.fast ? -(1.0f / d[a]) : 0.0f;
    return r;
}
float qdiv(float nn, float d, float nr) {
    const float q0 = nn * nr;
    const float e = __builtin_fmaf(d, q0, nn);
    return __builtin_fmaf(e, nr, q0);
}
bool slab(const pbrs_node& n, const Ray& R, float t_max, float& t_low, float& hi_el) {
    float t0[3], t1[3];
    for (int a = 0; a < 3; ++a) {
        if (R.fast) t0[a] = qdiv(R.o[a] - n.min[a], R.d[a], R.nr[a]), t1[a] = qdiv(R.o[a] - n.max[a], R.d[a], R.nr[a]);
        else t0[a] = (n.min[a] - R.o[a]) / R.d[a], t1[a] = (n.max[a] - R.o[a]) / R.d[a];
    }
    const float lo_el = std::fmax(std::fmax(std::fmin(t0[0], t1[0]), std::fmin(t0[1], t1[1])), std::fmin(t0[2], t1[2]));
    hi_el = std::fmin(std::fmin(std::fmax(t0[0], t1[0]), std::fmax(t0[1], t1[1])), std::fmax(t0[2], t1[2]));
    t_low = std::fmax(lo_el, 0.0f);
    return t_low <= std::fmin(hi_el, t_max);
}
// any one deterministic triangle test serves (both walks run the same one); in double, so that it works at 2^-60 and at 2^39
bool tri_hit(const pbrs_tri_verts& tv, const Ray& R, float t_max, float& t_out) {
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
    if (!(t >= 0.0f && t < t_max)) return false;
    t_out = t;
    return true;
}

struct Tally {
    uint64_t rays = 0, pops = 0, failed = 0, culled = 0, tris = 0;
};
struct Found {
    float t;
    uint32_t prim;
};
Found walk(const Scene& sc, const Ray& R, bool cull, Tally& tally) {
    const std::vector<pbrs_node>& nodes = sc.P.nodes;
    std::vector<uint32_t> stack = {sc.root};
    const float inf = INFINITY;
    float lt = inf, mt = inf;  // the root against the incoming extent, every later node against the mesh-local best
    uint32_t prim = 0xffffffffu;
    ++tally.rays;
    while (!stack.empty()) {
        const uint32_t ni = stack.back();
        stack.pop_back();
        ++tally.pops;
        const pbrs_node& X = nodes[ni];
        float t_low = 0.0f, hi_el = 0.0f;
        if (!slab(X, R, lt, t_low, hi_el)) {
            ++tally.failed;
            continue;
        }
        if (!(X.b & PBRS_LEAF_FLAG)) {
            const uint32_t k = X.b & 3u;
            const float dk = R.d[k];
            const bool left_first = dk > 0.0f;
            const uint32_t left = ni + 1u, right = X.a, far = left_first ? right : left, near = left_first ? left : right;
            bool keep_near = true, keep_far = true;
            if (cull && R.fast) {  // ClosestWalk::cull_children
                const uint32_t w = X.b | sc.P.node_planes[ni];  // as uploaded
                const float step = pbrs_plane_step(X.min[k], X.max[k]);
                const float pd = pbrs_plane_down(pbrs_plane_qd(w), step, X.min[k]), pu = pbrs_plane_up(pbrs_plane_qu(w), step, X.max[k]);
                const bool pos = dk > 0.0f;
                const float e_near = qdiv(R.o[k] - (pos ? pu : pd), dk, R.nr[k]), e_far = qdiv(R.o[k] - (pos ? pd : pu), dk, R.nr[k]);
                const float T = std::fmin(hi_el, mt);
                keep_near = !(e_near < t_low);
                keep_far = !(e_far > T);
                // a dropped child fails its own test against mt of now, hence against any later (smaller) extent
                float a, b;
                if (!keep_near) REQUIRE(!slab(nodes[near], R, mt, a, b), "%s: node %u: the culled near child %u passes its box test", sc.name.c_str(), ni, near);
                if (!keep_far) REQUIRE(!slab(nodes[far], R, mt, a, b), "%s: node %u: the culled far child %u passes its box test", sc.name.c_str(), ni, far);
                tally.culled += (keep_near ? 0u : 1u) + (keep_far ? 0u : 1u);
            }
            if (keep_far) stack.push_back(far);
            if (keep_near) stack.push_back(near);
            lt = mt;
        } else {
            const uint32_t cnt = X.b & ~PBRS_LEAF_FLAG;
            for (uint32_t j = 0; j < cnt; ++j) {  // every triangle sees the extent from before the leaf; strictly smaller replaces
                float t;
                ++tally.tris;
                if (tri_hit(sc.tv[X.a + j], R, lt, t) && t < mt) mt = t, prim = X.a + j;
            }
            lt = mt;
        }
    }
    return Found{mt, prim};
}

// ---- rays ----
void add(std::vector<Ray>& rays, const float o[3], float dx, float dy, float dz) {
    const float d[3] = {dx, dy, dz};
    rays.push_back(make_ray(o, d));
}
std::vector<Ray> make_rays(const Scene& sc, uint32_t want) {
    std::vector<Ray> rays;
    Rng rng{0x5eed0000ull + sc.tv.size()};
    const pbrs_node& box = sc.P.nodes[sc.root];
    float ext[3], mid[3];
    for (int a = 0; a < 3; ++a) ext[a] = box.max[a] - box.min[a], mid[a] = 0.5f * (box.max[a] + box.min[a]);
    const float size = std::fmax(ext[0], std::fmax(ext[1], ext[2]));
    auto random_dir = [&](float* d) {
        do {
            for (int a = 0; a < 3; ++a) d[a] = rng.uniform(-1.0f, 1.0f);
        } while (d[0] * d[0] + d[1] * d[1] + d[2] * d[2] < 0.01f);
    };
    auto axis_near = [&](float* d) {  // one component of size 1, two small ones; every sign
        const uint32_t major = rng.below(3);
        for (uint32_t a = 0; a < 3; ++a) d[a] = (rng.below(2) ? 1.0f : -1.0f) * (a == major ? 1.0f : rng.uniform(1e-7f, 1e-3f));
    };
    const uint32_t per_kind = want / 5u;
    // from the surface: triangle centroids and vertices
    for (uint32_t i = 0; i < 2u * per_kind; ++i) {
        const pbrs_tri_verts& t = sc.tv[rng.below((uint32_t)sc.tv.size())];
        float o[3], d[3];
        for (int a = 0; a < 3; ++a) o[a] = (i & 1u) ? t.p0[a] : (t.p0[a] + t.p1[a] + t.p2[a]) * (1.0f / 3.0f);
        if (i & 2u) axis_near(d);
        else random_dir(d);
        add(rays, o, d[0], d[1], d[2]);
    }
    // from outside, towards the mesh and past it
    for (uint32_t i = 0; i < per_kind; ++i) {
        float o[3], d[3], to[3];
        for (int a = 0; a < 3; ++a) o[a] = mid[a] + rng.uniform(-1.5f, 1.5f) * size, to[a] = box.min[a] + rng.uniform(0.0f, 1.0f) * ext[a];
        for (int a = 0; a < 3; ++a) d[a] = (to[a] - o[a]) / size;
        if (i % 3u == 2u) axis_near(d);
        add(rays, o, d[0], d[1], d[2]);
    }
    // origins exactly on a stored plane of some inner node, the other two coordinates inside its box
    std::vector<uint32_t> inner;
    for (uint32_t i = sc.root; i < sc.P.nodes.size(); ++i)
        if (!(sc.P.nodes[i].b & PBRS_LEAF_FLAG)) inner.push_back(i);
    for (uint32_t i = 0; i < per_kind; ++i) {
        const uint32_t ni = inner[rng.below((uint32_t)inner.size())];
        const pbrs_node& X = sc.P.nodes[ni];
        const uint32_t k = X.b & 3u, w = sc.P.node_planes[ni];
        const float step = pbrs_plane_step(X.min[k], X.max[k]);
        float o[3], d[3];
        for (int a = 0; a < 3; ++a) o[a] = X.min[a] + rng.uniform(0.0f, 1.0f) * (X.max[a] - X.min[a]);
        o[k] = (i & 1u) ? pbrs_plane_down(pbrs_plane_qd(w), step, X.min[k]) : pbrs_plane_up(pbrs_plane_qu(w), step, X.max[k]);
        if (i & 2u) axis_near(d);
        else random_dir(d);
        add(rays, o, d[0], d[1], d[2]);
    }
    // outside the guarded range: a zero, a denormal and a 2^41 direction component (the literal divisions: never culled)
    for (uint32_t i = 0; i < per_kind; ++i) {
        const pbrs_tri_verts& t = sc.tv[rng.below((uint32_t)sc.tv.size())];
        float o[3], d[3];
        for (int a = 0; a < 3; ++a) o[a] = t.p1[a];
        random_dir(d);
        d[rng.below(3)] = i % 3u == 0u ? 0.0f : i % 3u == 1u ? 1e-42f : 0x1p41f;
        add(rays, o, d[0], d[1], d[2]);
    }
    return rays;
}

void run(const char* name, const Mesh& mesh, float scale, uint32_t n_rays) {
    Scene sc;
    build(sc, name, mesh, scale);
    const PlaneCount pc = check_planes(sc);
    REQUIRE(pc.inner > 0u, "%s: no inner node", name);
    const std::vector<Ray> rays = make_rays(sc, n_rays);
    Tally plain, culled, slow;
    uint64_t hits = 0, fast = 0;
    for (const Ray& r : rays) {
        Tally& with = r.fast ? culled : slow;
        Tally scratch;
        const Found a = walk(sc, r, false, r.fast ? plain : scratch), b = walk(sc, r, true, with);
        uint32_t ta, tb;
        std::memcpy(&ta, &a.t, 4), std::memcpy(&tb, &b.t, 4);
        REQUIRE(ta == tb && a.prim == b.prim, "%s: ray %zu: (t, prim) = (%a, %u) without the cull, (%a, %u) with it", name, (size_t)(&r - rays.data()), (double)a.t, a.prim,
                (double)b.t, b.prim);
        hits += a.prim != 0xffffffffu ? 1u : 0u;
        fast += r.fast ? 1u : 0u;
    }
    REQUIRE(slow.culled == 0u, "%s: a ray on the literal divisions was culled", name);
    REQUIRE(plain.tris == culled.tris, "%s: triangle tests differ: %llu without the cull, %llu with it", name, (unsigned long long)plain.tris, (unsigned long long)culled.tris);
    REQUIRE(culled.pops + culled.culled == plain.pops && culled.failed + culled.culled == plain.failed, "%s: every culled child is one failed pop less", name);
    const double n = (double)fast;
    std::printf("%s: inner nodes %u (with planes %u), rays %zu (guarded range %llu, hits %llu), pops per ray %.2f -> %.2f, failed pops per ray %.2f -> %.2f, culled at push %.2f\n", name,
                pc.inner, pc.with_planes, rays.size(), (unsigned long long)fast, (unsigned long long)hits, plain.pops / n, culled.pops / n, plain.failed / n, culled.failed / n,
                culled.culled / n);
}

}  // namespace

int main() {
    run("five", five_mesh(), 1.0f, 2000);
    run("overlap", overlap_mesh(), 1.0f, 3000);
    run("flat", flat_mesh(), 1.0f, 3000);
    run("tiny", whole_number_mesh(), 0x1p-60f, 3000);
    run("huge", whole_number_mesh(), 0x1p34f, 3000);
    run("terrain", terrain_mesh(64, 128), 1.0f, 5000);
    std::printf("ok\n");
    return 0;
}
