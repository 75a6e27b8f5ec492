// tests/light_skip_check.cpp — the light a shadow ray was aimed at (pbrs_amd/csrc/device/scene.h, PBRS_SKIP_*; links set by
// host/scene_prepare.cpp, prepare_scene and write_light_links; read by device/shade.h, light_skip_tag, and device/traverse.h, AnyWalk::skip),
// on a CPU: a program of its own that tests/test_light_skip.py compiles with -fsanitize=address,undefined and runs.
//
// Scenes come from pbrs_host_scene_build, the four scene families of pbrs_amd/scenes.py at small size:
//   c1        a Lambertian sphere and a sphere light; beside them a bit-identical second instance of the light's sphere (a duplicate)
//             and a larger sphere around the light (for the forged links)
//   cornell   six wall meshes, a translated sphere, two triangle lights (IsolatedTriangle instances: no links)
//   terrain   the C4 family's height field at nx = 16, nz = 32 under a translation, a floor mesh, four sphere lights: a scanned TLAS
//   lights    24 objects (translated spheres, cuboids) and 24 lights — spheres, triangles, a disk and a quad — a TLAS walked as a tree
// Checked, per scene, on prepare_scene's output:
//   links     every link names an analytic instance of the light's kind whose shape parameters are the light's bit for bit and whose
//             matrices are the identity, and the first such; a light without such an instance has none; the flat-leaf half names the leaf
//             copy of that instance (0 where the TLAS is not scanned); write_light_links puts the halves into its copy's padding words and
//             leaves the description alone
//   walks     a restatement of the any-hit walk — scanned (a mask of the leaf copies whose box passes) and as a tree — with and without
//             the skip gives the same answer on at least 10^5 rays per scene: light samples from surface points (t_max = 0.999, as
//             limited_ray_to builds them), and rays with axis-parallel, denormal and huge components
//   tags      no ray is tagged whose linked instance's own test passes (the restated tag function is the walk's own visit function)
//   forged    with every light linked in turn to every analytic instance of the scene — the larger enclosing sphere and the duplicate
//             among them — and to nothing, the answers still agree: which instance a light is linked to is only a guess
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

// ---- scene specs ----
struct Mesh {
    std::vector<float> pos, nrm, uv;
    std::vector<uint32_t> idx;
    void vertex(float x, float y, float z) {
        pos.insert(pos.end(), {x, y, z});
        nrm.insert(nrm.end(), {0.0f, 1.0f, 0.0f});
        uv.insert(uv.end(), {0.0f, 0.0f});
    }
    void quad(const float a[3], const float b[3], const float c[3], const float d[3]) {
        const uint32_t v = (uint32_t)(pos.size() / 3);
        vertex(a[0], a[1], a[2]), vertex(b[0], b[1], b[2]), vertex(c[0], c[1], c[2]), vertex(d[0], d[1], d[2]);
        idx.insert(idx.end(), {v, v + 1u, v + 2u, v + 2u, v + 1u, v + 3u});
    }
};
Mesh quad_mesh(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz, float dx, float dy, float dz) {
    Mesh m;
    const float a[3] = {ax, ay, az}, b[3] = {bx, by, bz}, c[3] = {cx, cy, cz}, d[3] = {dx, dy, dz};
    m.quad(a, b, c, d);
    return m;
}
Mesh terrain_mesh(uint32_t nx, uint32_t nz) {  // pbrs_amd/scenes.py, heightfield_mesh: a sum of six sine products over 200 x 400
    static const double w[6][5] = {{13.6, 8.57, 6.11, 4.49, 0.79}, {4.59, 13.7, 0.04, 1.59, 0.60}, {11.4, 4.37, 5.42, 6.18, 0.41},
                                   {9.17, 2.11, 2.43, 0.28, 0.97}, {7.23, 13.4, 4.94, 5.44, 0.42}, {2.90, 9.21, 1.06, 4.61, 0.59}};
    Mesh m;
    for (uint32_t i = 0; i <= nx; ++i)
        for (uint32_t j = 0; j <= nz; ++j) {
            const double x = 200.0 * i / nx, z = 400.0 * j / nz;
            double y = 0.0;
            for (const auto& r : w) y += r[4] * std::sin(6.283185307179586 * r[0] * x / 200.0 + r[2]) * std::sin(6.283185307179586 * r[1] * z / 400.0 + r[3]);
            m.vertex((float)x, (float)(4.0 * y), (float)z);
        }
    for (uint32_t i = 0; i < nx; ++i)
        for (uint32_t j = 0; j < nz; ++j) {
            const uint32_t v00 = i * (nz + 1) + j, v01 = v00 + 1, v10 = v00 + nz + 1, v11 = v10 + 1;
            m.idx.insert(m.idx.end(), {v00, v01, v10, v10, v01, v11});
        }
    return m;
}

struct Spec {  // what pbrs_host_scene_build takes, with its storage
    std::vector<Mesh> meshes;
    std::vector<pbrs_shape_spec> shapes;
    std::vector<pbrs_material_spec> materials;
    std::vector<pbrs_instance_spec> instances;
    std::vector<pbrs_area_light_spec> lights;
    uint32_t material(uint32_t kind, float v) {
        pbrs_material_spec m{};
        m.kind = kind;
        m.p[0] = m.p[1] = m.p[2] = v;
        materials.push_back(m);
        return (uint32_t)materials.size() - 1u;
    }
    uint32_t shape(uint32_t kind, std::initializer_list<float> p) {
        pbrs_shape_spec s{};
        s.kind = kind;
        int k = 0;
        for (float v : p) s.p[k++] = v;
        shapes.push_back(s);
        return (uint32_t)shapes.size() - 1u;
    }
    uint32_t mesh(const Mesh& m) {
        meshes.push_back(m);
        pbrs_shape_spec s{};
        s.kind = PBRS_SHAPE_MESH;
        s.mesh = (uint32_t)meshes.size() - 1u;
        shapes.push_back(s);
        return (uint32_t)shapes.size() - 1u;
    }
    void instance(uint32_t shape, uint32_t material, float tx = 0.0f, float ty = 0.0f, float tz = 0.0f) {
        pbrs_instance_spec in{};
        in.shape = shape, in.material = material;
        for (int i = 0; i < 4; ++i) in.forward[5 * i] = in.inverse[5 * i] = 1.0f;
        if (tx != 0.0f || ty != 0.0f || tz != 0.0f) {  // [col][row]
            in.forward[12] = tx, in.forward[13] = ty, in.forward[14] = tz;
            in.inverse[12] = -tx, in.inverse[13] = -ty, in.inverse[14] = -tz;
        }
        instances.push_back(in);
    }
    void light(uint32_t shape_index, bool with_instance = true) {  // a light of that (world-space) shape, and the instance that is the light
        pbrs_area_light_spec a{};
        a.emit[0] = a.emit[1] = a.emit[2] = 10.0f;
        a.shape = shapes[shape_index];
        lights.push_back(a);
        if (with_instance) instance(shape_index, material(PBRS_MTL_DIFFUSE_LIGHT, 10.0f));
    }
};

Spec c1_spec() {
    Spec s;
    const uint32_t grey = s.material(PBRS_MTL_LAMBERTIAN, 0.5f);
    s.instance(s.shape(PBRS_SHAPE_SPHERE, {0, 0, 0, 1.0f}), grey);
    s.instance(s.shape(PBRS_SHAPE_SPHERE, {0, 3, 0, 0.8f}), grey);  // around the light: a forged link's target
    const uint32_t ls = s.shape(PBRS_SHAPE_SPHERE, {0, 3, 0, 0.5f});
    s.light(ls);
    s.instance(s.shape(PBRS_SHAPE_SPHERE, {0, 3, 0, 0.5f}), grey);  // the duplicate
    return s;
}
Spec cornell_spec() {
    Spec s;
    const uint32_t white = s.material(PBRS_MTL_LAMBERTIAN, 0.73f);
    const float S = 555.0f;
    s.instance(s.mesh(quad_mesh(S, 0, 0, S, S, 0, S, 0, S, S, S, S)), white);
    s.instance(s.mesh(quad_mesh(0, 0, 0, 0, 0, S, 0, S, 0, 0, S, S)), white);
    s.instance(s.mesh(quad_mesh(0, 0, 0, S, 0, 0, 0, 0, S, S, 0, S)), white);
    s.instance(s.mesh(quad_mesh(0, S, 0, 0, S, S, S, S, 0, S, S, S)), white);
    s.instance(s.mesh(quad_mesh(0, 0, S, S, 0, S, 0, S, S, S, S, S)), white);
    s.instance(s.mesh(quad_mesh(0, 0, 0, 0, S, 0, S, 0, 0, S, S, 0)), white);
    s.instance(s.shape(PBRS_SHAPE_SPHERE, {0, 0, 0, 80.0f}), white, 370.0f, 80.5f, 160.0f);
    s.light(s.shape(PBRS_SHAPE_TRIANGLE, {343, 554, 332, 343, 554, 227, 213, 554, 227}));
    s.light(s.shape(PBRS_SHAPE_TRIANGLE, {213, 554, 227, 213, 554, 332, 343, 554, 332}));
    return s;
}
Spec terrain_spec() {
    Spec s;
    const uint32_t ground = s.material(PBRS_MTL_LAMBERTIAN, 0.5f);
    s.instance(s.mesh(terrain_mesh(16, 32)), ground, -100.0f, 0.0f, 0.0f);
    s.instance(s.mesh(quad_mesh(-400, -14, -100, 400, -14, -100, -400, -14, 600, 400, -14, 600)), ground);
    Rng rng{4};
    for (int k = 0; k < 4; ++k) s.light(s.shape(PBRS_SHAPE_SPHERE, {rng.uniform(-80, 80), rng.uniform(60, 90), rng.uniform(40, 360), rng.uniform(6, 12)}));
    return s;
}
Spec lights_spec() {
    Spec s;
    const uint32_t grey = s.material(PBRS_MTL_LAMBERTIAN, 0.5f);
    s.instance(s.mesh(quad_mesh(-60, 0, -20, 60, 0, -20, -60, 0, 140, 60, 0, 140)), grey);
    Rng rng{5};
    for (int k = 0; k < 24; ++k) {
        const float cx = -49.0f + 14.0f * (float)(k % 8) + rng.uniform(-2, 2), cz = 6.0f + 15.0f * (float)(k / 8) + rng.uniform(-2, 2), r = rng.uniform(2.5f, 4.5f);
        if (k % 2 == 0) s.instance(s.shape(PBRS_SHAPE_SPHERE, {0, 0, 0, r}), grey, cx, r + 0.01f, cz);
        else s.instance(s.shape(PBRS_SHAPE_CUBOID, {-r, 0, -r, r, 2 * r, r}), grey, cx, 0.01f, cz);
    }
    for (int k = 0; k < 24; ++k) {
        const float lx = -52.0f + 104.0f * ((float)(k % 8) + rng.uniform(0.1f, 0.9f)) / 8.0f, lz = 130.0f * ((float)(k / 8) + rng.uniform(0.1f, 0.9f)) / 8.0f, ly = rng.uniform(22, 40);
        const float e = rng.uniform(1.0f, 2.5f);
        if (k == 5) s.light(s.shape(PBRS_SHAPE_DISK, {lx, ly, lz, 0, -1, 0, e, 0, 0}));
        else if (k == 7) s.light(s.shape(PBRS_SHAPE_QUAD, {lx, ly, lz, e, 0, 0, 0, 0, e}));
        else if (k == 9) s.light(s.shape(PBRS_SHAPE_SPHERE, {lx, ly, lz, e}), false);  // a light no instance stands for
        else if (k % 2 == 0) s.light(s.shape(PBRS_SHAPE_SPHERE, {lx, ly, lz, 0.5f * e}));
        else s.light(s.shape(PBRS_SHAPE_TRIANGLE, {lx + e, ly, lz + e, lx + e, ly, lz, lx, ly, lz}));
    }
    return s;
}

struct Scene {
    std::string name;
    Spec spec;
    pbrs_host_scene* hs = nullptr;
    pbrs_scene_desc d{};
    PreparedScene P;
    ~Scene() {
        if (hs) pbrs_host_scene_free(hs);
    }
};
void build(Scene& sc, const char* name, Spec spec) {
    sc.name = name;
    sc.spec = std::move(spec);
    Spec& s = sc.spec;
    std::vector<pbrs_mesh_spec> ms(s.meshes.size());
    for (size_t i = 0; i < ms.size(); ++i) {
        const Mesh& m = s.meshes[i];
        ms[i].n_vertices = (uint32_t)(m.pos.size() / 3), ms[i].n_triangles = (uint32_t)(m.idx.size() / 3);
        ms[i].positions = m.pos.data(), ms[i].normals = m.nrm.data(), ms[i].uvs = m.uv.data(), ms[i].indices = m.idx.data();
    }
    pbrs_scene_spec spec_c{};
    spec_c.n_meshes = (uint32_t)ms.size(), spec_c.meshes = ms.data();
    spec_c.n_shapes = (uint32_t)s.shapes.size(), spec_c.shapes = s.shapes.data();
    spec_c.n_materials = (uint32_t)s.materials.size(), spec_c.materials = s.materials.data();
    spec_c.n_instances = (uint32_t)s.instances.size(), spec_c.instances = s.instances.data();
    spec_c.n_area_lights = (uint32_t)s.lights.size(), spec_c.area_lights = s.lights.data();
    spec_c.camera.width = spec_c.camera.height = 8;
    spec_c.camera.fov_y_rad = 0.8f;
    spec_c.camera.target[2] = -1.0f, spec_c.camera.up[1] = 1.0f;
    spec_c.env_kind = PBRS_ENV_CONSTANT;
    REQUIRE(pbrs_host_scene_build(&spec_c, &sc.hs) == PBRS_OK, "%s: pbrs_host_scene_build: %s", name, pbrs_host_last_error());
    sc.d = *pbrs_host_scene_desc(sc.hs);
    const SceneCheck chk = check_scene(sc.d);
    REQUIRE(chk.code == PBRS_OK, "%s: check_scene: %s", name, chk.message);
    sc.P = prepare_scene(sc.d, chk.levels, DevOverrides{});
}

// ---- the links ----
bool analytic(uint32_t kind) { return kind == PBRS_SHAPE_SPHERE || kind == PBRS_SHAPE_QUAD || kind == PBRS_SHAPE_DISK || kind == PBRS_SHAPE_CUBOID; }
bool matches(const pbrs_scene_desc& d, const pbrs_area_light& L, uint32_t i) {  // the rule, restated
    const pbrs_instance& in = d.instances[i];
    if (!analytic(in.shape_kind) || in.shape_kind != L.shape_kind) return false;
    static const float id[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
    if (std::memcmp(in.inv, id, sizeof id) != 0 || std::memcmp(in.fwd, id, sizeof id) != 0) return false;
    return std::memcmp(d.shapes[in.shape_index].p, L.p, (L.shape_kind == PBRS_SHAPE_SPHERE ? 4u : 9u) * sizeof(float)) == 0;
}
uint32_t check_links(const Scene& sc) {
    const pbrs_scene_desc& d = sc.d;
    const PreparedScene& P = sc.P;
    REQUIRE(P.light_link.size() == d.n_area_lights, "%s: %zu links for %u lights", sc.name.c_str(), P.light_link.size(), d.n_area_lights);
    uint32_t linked = 0;
    for (uint32_t l = 0; l < d.n_area_lights; ++l) {
        uint32_t first = 0xffffffffu;
        for (uint32_t i = d.n_instances; i-- > 0u;)
            if (matches(d, d.area_lights[l], i)) first = i;
        const uint32_t link = P.light_link[l], inst = link & PBRS_SKIP_INST_MASK, leaf = link >> PBRS_SKIP_FLAT_SHIFT;
        if (first == 0xffffffffu) {
            REQUIRE(link == 0u, "%s: light %u has link %08x and no instance that is the light", sc.name.c_str(), l, link);
            continue;
        }
        REQUIRE(inst == first + 1u, "%s: light %u is linked to instance %u - 1, the first instance that is the light is %u", sc.name.c_str(), l, inst, first);
        if (P.S.n_flat == 0u) {
            REQUIRE(leaf == 0u, "%s: light %u: flat leaf %u in a scene without leaf copies", sc.name.c_str(), l, leaf);
        } else {
            REQUIRE(leaf >= 1u && leaf <= P.S.n_flat && leaf <= 32u, "%s: light %u: flat leaf %u of %u", sc.name.c_str(), l, leaf, P.S.n_flat);
            const pbrs_node& n = P.nodes[P.S.flat_off + leaf - 1u];
            REQUIRE((n.b & PBRS_LEAF_FLAG) && n.a == first, "%s: light %u: flat leaf %u holds instance %u, not %u", sc.name.c_str(), l, leaf - 1u, n.a, first);
        }
        ++linked;
    }
    // the uploaded copy carries the halves; the description's records keep their padding
    std::vector<pbrs_area_light> copy(d.area_lights, d.area_lights + d.n_area_lights);
    write_light_links(P, copy);
    for (uint32_t l = 0; l < d.n_area_lights; ++l) {
        uint32_t w0, w1;
        std::memcpy(&w0, &copy[l].pad[0], 4), std::memcpy(&w1, &copy[l].pad[1], 4);
        REQUIRE(w0 == (P.light_link[l] & PBRS_SKIP_INST_MASK) && w1 == P.light_link[l] >> PBRS_SKIP_FLAT_SHIFT, "%s: light %u: padding words %08x %08x for link %08x",
                sc.name.c_str(), l, w0, w1, P.light_link[l]);
        REQUIRE(std::memcmp(&copy[l], &d.area_lights[l], offsetof(pbrs_area_light, pad)) == 0, "%s: light %u: the copy's record changed", sc.name.c_str(), l);
        REQUIRE(pn_bits(d.area_lights[l].pad[0]) == 0u && pn_bits(d.area_lights[l].pad[1]) == 0u, "%s: light %u: the description's padding was written", sc.name.c_str(), l);
    }
    return linked;
}

// ---- the walk (device/traverse.h, AnyWalk; device/shapes.h, analytic_occludes) ----
struct Ray {
    float o[3], d[3], t_max;
};
bool truncated(float t, float t_max) { return !(t < 1e-4f || t >= t_max); }
float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
bool slab(const float mn[3], const float mx[3], const float o[3], const float d[3], float t_max) {  // dmath.h, slab_test: the literal divisions
    float lo = -INFINITY, hi = INFINITY;
    for (int a = 0; a < 3; ++a) {
        const float t0 = (mn[a] - o[a]) / d[a], t1 = (mx[a] - o[a]) / d[a];
        const float l = t0 < t1 ? t0 : t1, h = t0 > t1 ? t0 : t1;
        lo = l > lo ? l : lo, hi = h < hi ? h : hi;
    }
    return (lo > 0.0f ? lo : 0.0f) <= (hi < t_max ? hi : t_max);
}
// the instance's own test: `inverse * ray`, then the shape's predicate — ONE function, called by the tag (k_shade's side) and by the visit
bool own_test(const pbrs_scene_desc& D, uint32_t i, const Ray& R) {
    const pbrs_instance& in = D.instances[i];
    float o[3], d[3];
    for (int r = 0; r < 3; ++r) {
        o[r] = in.inv[r][0] * R.o[0] + in.inv[r][1] * R.o[1] + in.inv[r][2] * R.o[2] + in.inv[r][3] * 1.0f;
        d[r] = in.inv[r][0] * R.d[0] + in.inv[r][1] * R.d[1] + in.inv[r][2] * R.d[2] + in.inv[r][3] * 0.0f;
    }
    const float* p = D.shapes[in.shape_index].p;
    switch (in.shape_kind) {
        case PBRS_SHAPE_SPHERE: {
            float f[3], g[3];
            for (int a = 0; a < 3; ++a) f[a] = o[a] - p[a];
            const float a2 = dot3(d, d), bp = -dot3(f, d);
            for (int a = 0; a < 3; ++a) g[a] = f[a] + bp / a2 * d[a];
            const float delta = p[3] * p[3] - dot3(g, g);
            if (delta < 0.0f) return false;
            const float c = dot3(f, f) - p[3] * p[3], q = bp + (bp < 0.0f ? -1.0f : 1.0f) * std::sqrt(delta * a2);
            return truncated(c / q, R.t_max) && truncated(q / a2, R.t_max);
        }
        case PBRS_SHAPE_CUBOID: return slab(p, p + 3, o, d, R.t_max);
        case PBRS_SHAPE_DISK: {
            float c[3], h[3];
            for (int a = 0; a < 3; ++a) c[a] = p[a] - o[a];
            const float t = dot3(c, p + 3) / dot3(d, p + 3);
            for (int a = 0; a < 3; ++a) h[a] = o[a] + t * d[a] - p[a];
            return dot3(h, h) <= dot3(p + 6, p + 6);
        }
        case PBRS_SHAPE_QUAD: {
            const float *su = p + 3, *sv = p + 6;
            const float n[3] = {su[1] * sv[2] - su[2] * sv[1], su[2] * sv[0] - su[0] * sv[2], su[0] * sv[1] - su[1] * sv[0]};
            float c[3], h[3];
            for (int a = 0; a < 3; ++a) c[a] = p[a] - o[a];
            const float t = dot3(c, n) / dot3(d, n);
            if (!truncated(t, R.t_max)) return false;
            for (int a = 0; a < 3; ++a) h[a] = o[a] + t * d[a] - p[a];
            const float u = dot3(h, su) / dot3(su, su), v = dot3(h, sv) / dot3(sv, sv);
            return 0.0f <= u && u <= 1.0f && 0.0f <= v && v <= 1.0f;
        }
        default: return false;
    }
}
// any one deterministic predicate serves for the triangles (both walks run the same one)
bool tri_pred(const float p0[3], const float p1[3], const float p2[3], const float o[3], const float dd[3], float t_max) {
    double e1[3], e2[3], p[3], s[3], q[3];
    for (int a = 0; a < 3; ++a) e1[a] = (double)p1[a] - p0[a], e2[a] = (double)p2[a] - p0[a], s[a] = (double)o[a] - p0[a];
    p[0] = dd[1] * e2[2] - dd[2] * e2[1], p[1] = dd[2] * e2[0] - dd[0] * e2[2], p[2] = dd[0] * e2[1] - dd[1] * e2[0];
    const double det = e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2];
    if (det == 0.0 || !(det == det)) return false;
    const double u = (s[0] * p[0] + s[1] * p[1] + s[2] * p[2]) / det;
    if (!(u >= 0.0 && u <= 1.0)) return false;
    q[0] = s[1] * e1[2] - s[2] * e1[1], q[1] = s[2] * e1[0] - s[0] * e1[2], q[2] = s[0] * e1[1] - s[1] * e1[0];
    const double v = (dd[0] * q[0] + dd[1] * q[1] + dd[2] * q[2]) / det;
    if (!(v >= 0.0 && u + v <= 1.0)) return false;
    const float t = (float)((e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) / det);
    return truncated(t, t_max);
}
struct Tally {
    uint64_t visits = 0;
};
bool visit(const Scene& sc, uint32_t i, const Ray& R, Tally& tally) {  // Instance::occludes
    ++tally.visits;
    const pbrs_instance& in = sc.d.instances[i];
    if (analytic(in.shape_kind)) return own_test(sc.d, i, R);
    float o[3], d[3];
    for (int r = 0; r < 3; ++r) {
        o[r] = in.inv[r][0] * R.o[0] + in.inv[r][1] * R.o[1] + in.inv[r][2] * R.o[2] + in.inv[r][3];
        d[r] = in.inv[r][0] * R.d[0] + in.inv[r][1] * R.d[1] + in.inv[r][2] * R.d[2];
    }
    if (in.shape_kind == PBRS_SHAPE_TRIANGLE) {
        const pbrs_tri_verts& t = sc.d.tri_verts[in.blas_root];
        return tri_pred(t.p0, t.p1, t.p2, o, d, R.t_max);
    }
    std::vector<uint32_t> stack = {sc.P.inst[i].blas_root};  // (absolute, in P.nodes)
    while (!stack.empty()) {
        const uint32_t ni = stack.back();
        stack.pop_back();
        const pbrs_node& X = sc.P.nodes[ni];
        if (!slab(X.min, X.max, o, d, R.t_max)) continue;
        if (!(X.b & PBRS_LEAF_FLAG)) {
            stack.push_back(X.a), stack.push_back(ni + 1u);
            continue;
        }
        for (uint32_t j = 0; j < (X.b & ~PBRS_LEAF_FLAG); ++j) {
            const pbrs_tri_verts& t = sc.d.tri_verts[X.a + j];
            if (tri_pred(t.p0, t.p1, t.p2, o, d, R.t_max)) return true;
        }
    }
    return false;
}
// k_shade's side: the word a ray carries for the light with link `link` (0: none)
uint32_t tag_of(const Scene& sc, uint32_t link, const Ray& R) {
    if (link == 0u) return 0u;
    return own_test(sc.d, (link & PBRS_SKIP_INST_MASK) - 1u, R) ? 0u : link;
}
bool scanned(const Scene& sc, const Ray& R) {  // AnyWalk::start: the leaf copies exist and the ray is on the division-free test
    if (sc.P.S.n_flat == 0u || sc.P.S.fast_slab == 0u) return false;
    for (int a = 0; a < 3; ++a) {
        const uint32_t e = (pn_bits(R.d[a]) >> 23) & 0xffu, u = pn_bits(R.o[a]) & 0x7fffffffu;
        if (!(e - (127u - 40u) <= 80u) || !(u == 0u || (u >> 23) - (127u - 60u) <= 100u)) return false;
    }
    return true;
}
// skip_tree: whether the tree walk honours the tag (k_shadow's walks of a TLAS that is not scanned do; the scanning kernels' tree rays do not)
bool walk(const Scene& sc, const Ray& R, uint32_t tag, Tally& tally) {
    const std::vector<pbrs_node>& n = sc.P.nodes;
    if (scanned(sc, R)) {
        uint32_t cand = 0;
        for (uint32_t k = 0; k < sc.P.S.n_flat; ++k)
            if (slab(n[sc.P.S.flat_off + k].min, n[sc.P.S.flat_off + k].max, R.o, R.d, R.t_max)) cand |= 1u << k;
        const uint32_t leaf = tag >> PBRS_SKIP_FLAT_SHIFT;
        if (leaf != 0u) cand &= ~(1u << (leaf - 1u));
        for (; cand; cand &= cand - 1u)
            if (visit(sc, n[sc.P.S.flat_off + (uint32_t)__builtin_ctz(cand)].a, R, tally)) return true;
        return false;
    }
    const uint32_t skip = tag & PBRS_SKIP_INST_MASK;
    std::vector<uint32_t> stack = {0u};
    while (!stack.empty()) {
        const uint32_t ni = stack.back();
        stack.pop_back();
        const pbrs_node& X = n[ni];
        if (!slab(X.min, X.max, R.o, R.d, R.t_max)) continue;
        if (!(X.b & PBRS_LEAF_FLAG)) {
            stack.push_back(X.a), stack.push_back(ni + 1u);
            continue;
        }
        if (X.a + 1u == skip) continue;
        if (visit(sc, X.a, R, tally)) return true;
    }
    return false;
}

// ---- rays ----
struct LightRay {
    Ray r;
    uint32_t light;
};
void light_point(const pbrs_area_light& L, Rng& rng, float out[3]) {
    const float* p = L.p;
    const float u = rng.uniform(0, 1), v = rng.uniform(0, 1);
    switch (L.shape_kind) {
        case PBRS_SHAPE_SPHERE: {
            const float z = 2.0f * v - 1.0f, s = std::sqrt(std::fmax(0.0f, 1.0f - z * z)), ph = 6.2831853f * u;
            out[0] = p[0] + p[3] * s * std::cos(ph), out[1] = p[1] + p[3] * s * std::sin(ph), out[2] = p[2] + p[3] * z;
            break;
        }
        case PBRS_SHAPE_DISK: {
            const float *nn = p + 3, *ra = p + 6;
            const float r2[3] = {nn[1] * ra[2] - nn[2] * ra[1], nn[2] * ra[0] - nn[0] * ra[2], nn[0] * ra[1] - nn[1] * ra[0]};
            const float rr = std::sqrt(u), ph = 6.2831853f * v;
            for (int a = 0; a < 3; ++a) out[a] = p[a] + rr * (std::cos(ph) * ra[a] + std::sin(ph) * r2[a]);
            break;
        }
        case PBRS_SHAPE_TRIANGLE: {
            const float uu = u + v > 1.0f ? 1.0f - u : u, vv = u + v > 1.0f ? 1.0f - v : v;
            for (int a = 0; a < 3; ++a) out[a] = p[a] + uu * (p[3 + a] - p[a]) + vv * (p[6 + a] - p[a]);
            break;
        }
        default:
            for (int a = 0; a < 3; ++a) out[a] = p[a] + u * p[3 + a] + v * p[6 + a];
    }
}
std::vector<LightRay> make_rays(const Scene& sc, uint32_t n_samples, uint32_t n_odd) {
    std::vector<LightRay> rays;
    Rng rng{0x11a75c1full};
    const pbrs_scene_desc& d = sc.d;
    const pbrs_node& world = sc.P.nodes[0];
    auto surface_point = [&](float o[3]) {  // on a triangle where the scene has meshes, else on the first instance's sphere; lifted by 0.001 as spawn_ray does
        if (d.n_triangles && rng.below(4) != 0u) {
            const pbrs_instance* in = nullptr;
            while (!in || in->shape_kind != PBRS_SHAPE_MESH) in = &d.instances[rng.below(d.n_instances)];
            const pbrs_tri_verts& t = d.tri_verts[rng.below(d.n_triangles)];
            float u = rng.uniform(0, 1), v = rng.uniform(0, 1), l[3];
            if (u + v > 1.0f) u = 1.0f - u, v = 1.0f - v;
            for (int a = 0; a < 3; ++a) l[a] = t.p0[a] + u * (t.p1[a] - t.p0[a]) + v * (t.p2[a] - t.p0[a]);
            for (int r = 0; r < 3; ++r) o[r] = in->fwd[r][0] * l[0] + in->fwd[r][1] * l[1] + in->fwd[r][2] * l[2] + in->fwd[r][3];
            o[1] += 0.001f;
        } else {
            for (int a = 0; a < 3; ++a) o[a] = world.min[a] + rng.uniform(0.0f, 1.0f) * (world.max[a] - world.min[a]);
        }
    };
    for (uint32_t i = 0; i < n_samples; ++i) {  // light samples: the ray limited_ray_to builds, just short of the sampled point
        LightRay lr;
        lr.light = rng.below(d.n_area_lights);
        float q[3];
        surface_point(lr.r.o);
        light_point(d.area_lights[lr.light], rng, q);
        for (int a = 0; a < 3; ++a) lr.r.d[a] = q[a] - lr.r.o[a];
        lr.r.t_max = 1.0f - 0.001f;
        rays.push_back(lr);
    }
    static const float odd[] = {0.0f, -0.0f, 1e-42f, -3e-40f, 1e30f, -2.5e33f, 1.0f, -1.0f};  // axis-parallel, denormal and huge components
    for (uint32_t i = 0; i < n_odd; ++i) {
        LightRay lr;
        lr.light = rng.below(d.n_area_lights);
        float q[3];
        surface_point(lr.r.o);
        light_point(d.area_lights[lr.light], rng, q);
        for (int a = 0; a < 3; ++a) lr.r.d[a] = q[a] - lr.r.o[a];
        const uint32_t axis = rng.below(3), what = rng.below(4);
        if (what == 0u) lr.r.d[axis] = odd[rng.below(8)], lr.r.d[(axis + 1u) % 3u] = odd[rng.below(4)];  // towards the light along one or two axes only
        else if (what == 1u) lr.r.d[axis] = odd[rng.below(8)];
        else if (what == 2u) lr.r.o[axis] = odd[rng.below(6)];
        else for (int a = 0; a < 3; ++a) lr.r.d[a] *= 0x1p100f;  // the whole direction huge: t_max scales the other way
        lr.r.t_max = what == 3u ? 0x1p-100f * 0.999f : (i & 1u) ? 0.999f : INFINITY;
        rays.push_back(lr);
    }
    return rays;
}

struct Outcome {
    uint64_t rays = 0, occluded = 0, tagged = 0, own_passes = 0, scanned = 0;
    Tally plain, skipping;
};
Outcome compare(const Scene& sc, const std::vector<uint32_t>& links, const std::vector<LightRay>& rays, const char* what) {
    Outcome out;
    for (const LightRay& lr : rays) {
        const uint32_t link = links[lr.light], tag = tag_of(sc, link, lr.r);
        if (link != 0u) {
            Tally t;
            const bool own = visit(sc, (link & PBRS_SKIP_INST_MASK) - 1u, lr.r, t);  // what the walk would find at the leaf
            REQUIRE(!(tag != 0u && own), "%s, %s: ray %zu is tagged and its linked instance's own test passes", sc.name.c_str(), what, (size_t)(&lr - rays.data()));
            out.own_passes += own ? 1u : 0u;
        }
        const bool a = walk(sc, lr.r, 0u, out.plain), b = walk(sc, lr.r, tag, out.skipping);
        REQUIRE(a == b, "%s, %s: ray %zu (light %u, link %08x, tag %08x): occluded %d without the skip, %d with it", sc.name.c_str(), what, (size_t)(&lr - rays.data()),
                lr.light, link, tag, (int)a, (int)b);
        ++out.rays;
        out.occluded += a ? 1u : 0u;
        out.tagged += tag ? 1u : 0u;
        out.scanned += scanned(sc, lr.r) ? 1u : 0u;
    }
    return out;
}

void run(const char* name, Spec spec, uint32_t want_links, bool want_flat) {
    Scene sc;
    build(sc, name, std::move(spec));
    REQUIRE((sc.P.S.n_flat != 0u) == want_flat, "%s: %u scanned leaves", name, sc.P.S.n_flat);
    const uint32_t linked = check_links(sc);
    REQUIRE(linked == want_links, "%s: %u lights are linked, %u expected", name, linked, want_links);
    const std::vector<LightRay> rays = make_rays(sc, 90000, 20000);
    REQUIRE(rays.size() >= 100000, "%s: %zu rays", name, rays.size());
    const Outcome o = compare(sc, sc.P.light_link, rays, "the host's links");
    std::printf("%s: instances %u, lights %u, linked %u, scanned leaves %u; rays %llu, scanned %llu, occluded %llu, tagged %llu, own test passes %llu, "
                "instance visits per ray %.3f -> %.3f\n",
                name, sc.d.n_instances, sc.d.n_area_lights, linked, sc.P.S.n_flat, (unsigned long long)o.rays, (unsigned long long)o.scanned, (unsigned long long)o.occluded,
                (unsigned long long)o.tagged, (unsigned long long)o.own_passes, (double)o.plain.visits / o.rays, (double)o.skipping.visits / o.rays);
    if (linked) REQUIRE(o.tagged > 0u && o.skipping.visits < o.plain.visits, "%s: no ray was tagged, or the skip saved no visit", name);
    else REQUIRE(o.tagged == 0u && o.skipping.visits == o.plain.visits, "%s: rays were tagged without a link", name);
    // forged links: every light to every analytic instance in turn (the enclosing sphere, the duplicate, instances far away), and to nothing
    std::vector<uint32_t> ana;
    for (uint32_t i = 0; i < sc.d.n_instances; ++i)
        if (analytic(sc.d.instances[i].shape_kind)) ana.push_back(i);
    const std::vector<LightRay> fewer(rays.begin(), rays.begin() + 8000), tail(rays.end() - 4000, rays.end());
    uint64_t forged_tagged = 0, forged_own = 0;
    for (size_t round = 0; round <= std::min<size_t>(ana.size(), 12); ++round) {
        std::vector<uint32_t> links(sc.d.n_area_lights, 0u);
        if (round > 0)
            for (uint32_t l = 0; l < sc.d.n_area_lights; ++l) {
                const uint32_t i = ana[(round - 1u + l) % ana.size()];
                uint32_t leaf = 0u;
                for (uint32_t k = sc.P.S.n_flat; k-- > 0u;)
                    if (sc.P.nodes[sc.P.S.flat_off + k].a == i) leaf = k + 1u;
                links[l] = (i + 1u) | leaf << PBRS_SKIP_FLAT_SHIFT;
            }
        for (const std::vector<LightRay>* set : {&fewer, &tail}) {
            const Outcome f = compare(sc, links, *set, "forged links");
            forged_tagged += f.tagged, forged_own += f.own_passes;
            if (round == 0) REQUIRE(f.tagged == 0u, "%s: rays tagged with no links at all", name);
        }
    }
    std::printf("%s forged: analytic instances %zu, tagged %llu, own test passes %llu\n", name, ana.size(), (unsigned long long)forged_tagged, (unsigned long long)forged_own);
    if (!ana.empty()) REQUIRE(forged_tagged > 0u, "%s: forged links tagged no ray", name);
}

}  // namespace

int main() {
    run("c1", c1_spec(), 1u, true);
    run("cornell", cornell_spec(), 0u, true);
    run("terrain", terrain_spec(), 4u, true);
    run("lights", lights_spec(), 14u, false);  // the 12 sphere lights at even k, the disk and the quad; not the triangles, not the sphere at k = 9
    std::printf("ok\n");
    return 0;
}
