// tests/entry_nodes_check.cpp — the entry nodes of the camera rays (pbrs_amd/csrc/device/entry_nodes.h; eligibility: host/scene_prepare.cpp)
// on a CPU: a program of its own that tests/test_entry_nodes.py compiles with -fsanitize=address,undefined and runs.
//
// Scenes: the C4 family's height field (pbrs_amd/scenes.py, heightfield_mesh with seed 4) under one instance, flattened by
// pbrs_host_scene_build, checked and prepared by the host code the library runs:
//   translated   64 x 128 cells, the terrain moved by (-100, 0, 0), C4's camera (at x = 0, looking along +z): the film's middle columns
//                straddle dir.x = 0
//   identity     the same terrain under the identity, the camera moved with it
//   above        a camera high above the terrain, looking straight down
//   inside       a camera inside the terrain's box
//   straddle     a camera that looks level along +z: the middle columns straddle dir.x = 0 and the middle rows dir.y = 0
//   full         512 x 1024 cells (C4's 1 048 576 triangles) at 1920 x 1080, 300 sampled pixels
// Checked, per scene, with the header's own functions:
//   lists      every pixel's record is in the walk's DFS order (near child first by the sign of the pixel's directions), its entries are
//              disjoint subtrees, and it meets the stack bound with the rows the upload reserves
//   covering   for the sampled pixels and rays at jitter 0, a random jitter and the largest float below 1 on both axes: every leaf whose own
//              box the ray passes at extent +inf lies under an entry of its pixel
//   walk       a restatement of the mesh-local closest-hit walk WITH the split-plane cull (device/traverse.h: node_step, cull_children,
//              xfer_step) gives the same (t, prim), bit for bit, and the same sequence of (leaf, extent) from the root and from the entries
//   forgeries  a list with an entry removed, or two swapped, where the ray passes leaves under them, makes that comparison fail
//   nesting    a box grown outside its parent's takes the table away from the scene
// Prints, per scene, the pops per camera ray (passing, failed) from the root and with fork budgets 0 .. 3.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../include/pbrs_host.h"
#include "../pbrs_amd/csrc/device/entry_nodes.h"
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
    float unit() { return (float)((double)(next() >> 40) * (1.0 / 16777216.0)); }  // [0, 1)
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

// ---- the terrain (tests/split_planes_check.cpp has the same generator) ----
struct Mesh {
    std::vector<float> pos, nrm, uv;
    std::vector<uint32_t> idx;
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
    for (uint32_t i = 0; i <= nx; ++i)
        for (uint32_t j = 0; j <= nz; ++j) {
            const double x = sx * (double)i / (double)nx, z = sz * (double)j / (double)nz;
            double y = 0.0;
            for (const auto& r : w) y += r[4] * std::sin(two_pi * r[0] * x / sx + r[2]) * std::sin(two_pi * r[1] * z / sz + r[3]);
            m.pos.insert(m.pos.end(), {(float)x, (float)(amp * y / 3.0), (float)z});
            m.nrm.insert(m.nrm.end(), {0.0f, 1.0f, 0.0f});
            m.uv.insert(m.uv.end(), {0.0f, 0.0f});
        }
    for (uint32_t i = 0; i < nx; ++i)
        for (uint32_t j = 0; j < nz; ++j) {
            const uint32_t v00 = i * (nz + 1) + j, v01 = v00 + 1, v10 = v00 + nz + 1, v11 = v10 + 1;
            m.idx.insert(m.idx.end(), {v00, v01, v10, v10, v01, v11});
        }
    return m;
}

struct View {
    uint32_t width, height;
    float from[3], target[3], up[3];
};
struct Scene {
    std::string name;
    pbrs_host_scene* hs = nullptr;
    pbrs_scene_desc d{};
    pbrs_camera cam{};
    PreparedScene P;
    uint32_t root = 0;
    std::vector<uint32_t> end;  // per node: one past the last node of its subtree (pre-order)
    float o[3];                 // the camera's origin in the instance's space
    ~Scene() {
        if (hs) pbrs_host_scene_free(hs);
    }
};

void build(Scene& sc, const char* name, const Mesh& mesh, const float move[3], const View& v) {
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
    pbrs_instance_spec inst{};
    for (int i = 0; i < 4; ++i) inst.forward[5 * i] = inst.inverse[5 * i] = 1.0f;
    for (int a = 0; a < 3; ++a) inst.forward[12 + a] = move[a], inst.inverse[12 + a] = -move[a];  // column 3: the translation
    pbrs_scene_spec spec{};
    spec.n_meshes = 1, spec.meshes = &ms;
    spec.n_shapes = 1, spec.shapes = &shape;
    spec.n_materials = 1, spec.materials = &mat;
    spec.n_instances = 1, spec.instances = &inst;
    spec.camera.width = v.width, spec.camera.height = v.height;
    spec.camera.fov_y_rad = 0.7853981633974483f;
    for (int a = 0; a < 3; ++a) spec.camera.from[a] = v.from[a], spec.camera.target[a] = v.target[a], spec.camera.up[a] = v.up[a];
    spec.env_kind = PBRS_ENV_CONSTANT;
    REQUIRE(pbrs_host_scene_build(&spec, &sc.hs) == PBRS_OK, "%s: pbrs_host_scene_build: %s", name, pbrs_host_last_error());
    sc.d = *pbrs_host_scene_desc(sc.hs);
    sc.cam = *pbrs_host_scene_camera(sc.hs);
    const SceneCheck chk = check_scene(sc.d);
    REQUIRE(chk.code == PBRS_OK, "%s: check_scene: %s", name, chk.message);
    sc.P = prepare_scene(sc.d, chk.levels, DevOverrides{});
    REQUIRE(sc.P.S.fast_slab != 0u, "%s: the scene's coordinates are outside the guarded range", name);
    REQUIRE(sc.P.S.entry_inst == 0u, "%s: the terrain's instance has no entry table (entry_inst %u)", name, sc.P.S.entry_inst);
    // (a scene of one instance stages its TLAS in LDS, PBRS_FEAT_LDS_TOP, whose kernels carry no entry variant: the facts are what is asked here)
    REQUIRE(sc.P.facts.entry_nodes, "%s: the scene's facts do not name the table", name);
    REQUIRE(sc.P.stack_depth == sc.P.entry_rows && sc.P.entry_rows >= sc.P.entry_height, "%s: one TLAS leaf: every stack row (%u) is free at the BLAS root (%u), height %u", name,
            sc.P.stack_depth, sc.P.entry_rows, sc.P.entry_height);
    const pbrs_instance& in = sc.P.inst[0];
    sc.root = in.blas_root;
    const std::vector<pbrs_node>& n = sc.P.nodes;
    sc.end.assign(n.size(), 0u);
    for (uint32_t i = (uint32_t)n.size(); i-- > sc.root;) sc.end[i] = (n[i].b & PBRS_LEAF_FLAG) ? i + 1u : sc.end[n[i].a];
    // enter_instance (device/traverse.h) for a ray on the division-free test: the identity leaves a non-zero origin alone, else xf_apply
    const float* c = sc.cam.center;
    const bool stays = (in.flags & PBRS_INSTANCE_IDENTITY) && c[0] != 0.0f && c[1] != 0.0f && c[2] != 0.0f;
    for (int r = 0; r < 3; ++r) sc.o[r] = stays ? c[r] : in.inv[r][0] * c[0] + in.inv[r][1] * c[1] + in.inv[r][2] * c[2] + in.inv[r][3] * 1.0f;
    REQUIRE(std::fabs(sc.o[0] - (c[0] - move[0])) < 1e-3f, "%s: the instance's inverse does not undo the move", name);
}

// ---- the walk (device/traverse.h: RaySpace, qdiv, slab_rs, ClosestWalk::node_step inside one BLAS, xfer_step's entry) ----
struct Ray {
    float o[3], d[3], nr[3];
    bool fast;
};
Ray make_ray(const float o[3], const float d[3]) {
    Ray r;
    r.fast = true;
    for (int a = 0; a < 3; ++a) {
        r.o[a] = o[a], r.d[a] = d[a];
        r.fast = r.fast && pbrs_en_dir_in_range(d[a]) && pbrs_en_origin_in_range(o[a]);
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
// any one deterministic triangle test serves (both walks run the same one)
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
    uint64_t rays = 0, passed = 0, failed = 0;
};
struct Found {
    float t = INFINITY;
    uint32_t prim = 0xffffffffu;
    std::vector<std::pair<uint32_t, uint32_t>> leaves;  // (leaf whose box test passed, bits of the extent its triangles saw), in order
    size_t deepest = 0;                                 // most stack entries in use
    bool same(const Found& b) const {
        uint32_t x, y;
        std::memcpy(&x, &t, 4), std::memcpy(&y, &b.t, 4);
        return x == y && prim == b.prim && leaves == b.leaves;
    }
};
// rec: the pixel's record, or null for the walk from the root
Found walk(const Scene& sc, const Ray& R, const pbrs_entry_record* rec, Tally& tally) {
    const std::vector<pbrs_node>& nodes = sc.P.nodes;
    std::vector<uint32_t> stack;
    const float inf = INFINITY;
    float lt = inf, mt = inf;  // the root against the incoming extent (a camera ray's: +inf), every later node against the mesh-local best
    Found f;
    ++tally.rays;
    if (rec && rec->e[0] != PBRS_ENTRY_ROOT && R.fast) {  // ClosestWalk::xfer_step, ENTRY
        float a, b;
        if (slab(nodes[sc.root], R, lt, a, b)) {
            ++tally.passed;
            for (int i = (int)PBRS_ENTRY_MAX - 1; i >= 0; --i)
                if (rec->e[i] != PBRS_ENTRY_UNUSED) stack.push_back(rec->e[i]);
            lt = mt;
        } else {
            ++tally.failed;
        }
    } else {
        stack.push_back(sc.root);
    }
    f.deepest = stack.size();
    while (!stack.empty()) {
        const uint32_t ni = stack.back();
        stack.pop_back();
        const pbrs_node& X = nodes[ni];
        float t_low = 0.0f, hi_el = 0.0f;
        if (!slab(X, R, lt, t_low, hi_el)) {
            ++tally.failed;
            continue;
        }
        ++tally.passed;
        if (!(X.b & PBRS_LEAF_FLAG)) {
            const uint32_t k = X.b & 3u;
            const float dk = R.d[k];
            const bool left_first = dk > 0.0f;
            const uint32_t left = ni + 1u, right = X.a, far = left_first ? right : left, near = left_first ? left : right;
            bool keep_near = true, keep_far = true;
            if (R.fast) {  // ClosestWalk::cull_children
                const uint32_t w = X.b | sc.P.node_planes[ni];  // as uploaded
                const float step = pbrs_plane_step(X.min[k], X.max[k]);
                const float pd = pbrs_plane_down(pbrs_plane_qd(w), step, X.min[k]), pu = pbrs_plane_up(pbrs_plane_qu(w), step, X.max[k]);
                const bool pos = dk > 0.0f;
                const float e_near = qdiv(R.o[k] - (pos ? pu : pd), dk, R.nr[k]), e_far = qdiv(R.o[k] - (pos ? pd : pu), dk, R.nr[k]);
                keep_near = !(e_near < t_low);
                keep_far = !(e_far > std::fmin(hi_el, mt));
            }
            if (keep_far) stack.push_back(far);
            if (keep_near) stack.push_back(near);
            f.deepest = std::max(f.deepest, stack.size());
            lt = mt;
        } else {
            uint32_t ltb;
            std::memcpy(&ltb, &lt, 4);
            f.leaves.emplace_back(ni, ltb);
            const uint32_t cnt = X.b & ~PBRS_LEAF_FLAG;
            for (uint32_t j = 0; j < cnt; ++j) {  // every triangle sees the extent from before the leaf; strictly smaller replaces
                float t;
                if (tri_hit(sc.d.tri_verts[X.a + j], R, lt, t) && t < mt) mt = t, f.prim = X.a + j;
            }
            lt = mt;
        }
    }
    f.t = mt;
    return f;
}

// every leaf whose own box the ray passes at extent +inf (its ancestors pass too: the boxes nest)
void passing_leaves(const Scene& sc, const Ray& R, std::vector<uint32_t>& out) {
    out.clear();
    std::vector<uint32_t> todo = {sc.root};
    while (!todo.empty()) {
        const uint32_t x = todo.back();
        todo.pop_back();
        float a, b;
        if (!slab(sc.P.nodes[x], R, INFINITY, a, b)) continue;
        if (sc.P.nodes[x].b & PBRS_LEAF_FLAG) out.push_back(x);
        else todo.push_back(sc.P.nodes[x].a), todo.push_back(x + 1u);
    }
}

uint32_t depth_of(const Scene& sc, uint32_t node) {
    uint32_t x = sc.root, dpt = 0;
    while (x != node) {
        REQUIRE(!(sc.P.nodes[x].b & PBRS_LEAF_FLAG), "%s: node %u is not below the root", sc.name.c_str(), node);
        x = node < sc.P.nodes[x].a ? x + 1u : sc.P.nodes[x].a;
        ++dpt;
    }
    return dpt;
}
uint32_t count(const pbrs_entry_record& r) {
    uint32_t n = 0;
    while (n < PBRS_ENTRY_MAX && r.e[n] != PBRS_ENTRY_UNUSED) ++n;
    for (uint32_t i = n; i < PBRS_ENTRY_MAX; ++i) REQUIRE(r.e[i] == PBRS_ENTRY_UNUSED, "a used slot behind an unused one");
    return n;
}
// DFS order, disjoint subtrees, the stack bound
void check_list(const Scene& sc, const pbrs_entry_record& r, const pbrs_dir_box& B, uint32_t col, uint32_t row) {
    const uint32_t n = count(r);
    uint32_t depth[PBRS_ENTRY_MAX] = {};
    for (uint32_t i = 0; i < n; ++i) {
        REQUIRE(r.e[i] >= sc.root && r.e[i] < sc.end[sc.root], "%s: pixel (%u, %u): entry %u is not a node of the BLAS", sc.name.c_str(), col, row, r.e[i]);
        depth[i] = depth_of(sc, r.e[i]);
    }
    REQUIRE(pbrs_entry_fits(n, depth, sc.P.entry_height, sc.P.entry_rows), "%s: pixel (%u, %u): the list does not fit the stack", sc.name.c_str(), col, row);
    for (uint32_t i = 0; i + 1 < n; ++i) {
        const uint32_t a = r.e[i], b = r.e[i + 1];
        REQUIRE(sc.end[a] <= b || sc.end[b] <= a, "%s: pixel (%u, %u): entries %u and %u overlap", sc.name.c_str(), col, row, a, b);
        uint32_t x = sc.root;  // down to the node that parts them: a under its near child
        for (;;) {
            const pbrs_node& X = sc.P.nodes[x];
            const uint32_t left = x + 1u, right = X.a;
            const bool a_left = a < right, b_left = b < right;
            if (a_left == b_left) {
                x = a_left ? left : right;
                continue;
            }
            const bool left_first = B.lo[X.b & 3u] > 0.0f;
            REQUIRE(a_left == left_first, "%s: pixel (%u, %u): entries %u, %u are not in the walk's order", sc.name.c_str(), col, row, a, b);
            break;
        }
    }
}

struct Totals {
    Tally root, budget[PBRS_ENTRY_FORKS + 1u];
    uint64_t pixels = 0, with = 0, empty = 0, sentinel = 0, entries = 0, rays = 0, hits = 0, slow = 0, removed = 0, swapped = 0;
    uint64_t beam_tests = 0;
    double depth_sum = 0.0;
};

void check_pixel(const Scene& sc, uint32_t col, uint32_t row, Rng& rng, Totals& T) {
    pbrs_dir_box B;
    pbrs_entry_record rec[PBRS_ENTRY_FORKS + 1u];
    const bool boxed = pbrs_entry_dir_box(sc.cam, col, row, B) && pbrs_en_origin_in_range(sc.o[0]) && pbrs_en_origin_in_range(sc.o[1]) && pbrs_en_origin_in_range(sc.o[2]);
    uint32_t n[PBRS_ENTRY_FORKS + 1u];
    for (uint32_t f = 0; f <= PBRS_ENTRY_FORKS; ++f) {
        if (boxed) n[f] = pbrs_entry_record_of(sc.P.nodes.data(), sc.root, sc.o, B, f, sc.P.entry_height, sc.P.entry_rows, rec[f]);
        else {
            n[f] = PBRS_ENTRY_ROOT;
            for (uint32_t i = 0; i < PBRS_ENTRY_MAX; ++i) rec[f].e[i] = PBRS_ENTRY_UNUSED;
            rec[f].e[0] = PBRS_ENTRY_ROOT;
        }
        if (n[f] != PBRS_ENTRY_ROOT) {
            REQUIRE(count(rec[f]) == n[f] && n[f] <= (1u << f), "%s: pixel (%u, %u): %u entries with fork budget %u", sc.name.c_str(), col, row, n[f], f);
            check_list(sc, rec[f], B, col, row);
        }
    }
    const pbrs_entry_record& full = rec[PBRS_ENTRY_FORKS];
    ++T.pixels;
    if (n[PBRS_ENTRY_FORKS] == PBRS_ENTRY_ROOT) ++T.sentinel;
    else if (n[PBRS_ENTRY_FORKS] == 0u) ++T.empty;
    else {
        ++T.with, T.entries += n[PBRS_ENTRY_FORKS];
        for (uint32_t i = 0; i < n[PBRS_ENTRY_FORKS]; ++i) T.depth_sum += depth_of(sc, full.e[i]);
    }
    const float below_one = std::nextafter(1.0f, 0.0f);
    const float jit[3][2] = {{0.0f, 0.0f}, {rng.unit(), rng.unit()}, {below_one, below_one}};
    std::vector<uint32_t> leaves;
    for (const auto& j : jit) {
        float d[3];
        pbrs_camera_dir(sc.cam, (float)col + j[0], (float)row + j[1], d);  // k_raygen: x = col + fract(jx)
        const Ray R = make_ray(sc.o, d);
        ++T.rays;
        if (!R.fast) ++T.slow;
        if (boxed) {
            for (int a = 0; a < 3; ++a) REQUIRE(B.lo[a] <= d[a] && d[a] <= B.hi[a], "%s: pixel (%u, %u): a direction leaves the pixel's box", sc.name.c_str(), col, row);
            REQUIRE(R.fast, "%s: pixel (%u, %u): a ray of a boxed pixel leaves the guarded range", sc.name.c_str(), col, row);
        }
        const Found base = walk(sc, R, nullptr, T.root);
        T.hits += base.prim != 0xffffffffu ? 1u : 0u;
        REQUIRE(base.deepest <= sc.P.entry_rows, "%s: the walk from the root needs %zu rows of %u", sc.name.c_str(), base.deepest, sc.P.entry_rows);
        passing_leaves(sc, R, leaves);
        for (uint32_t f = 0; f <= PBRS_ENTRY_FORKS; ++f) {
            if (n[f] != PBRS_ENTRY_ROOT)
                for (uint32_t leaf : leaves) {
                    bool under = false;
                    for (uint32_t i = 0; i < n[f]; ++i) under = under || (rec[f].e[i] <= leaf && leaf < sc.end[rec[f].e[i]]);
                    REQUIRE(under, "%s: pixel (%u, %u), fork budget %u: leaf %u passes the ray's box test and lies under no entry", sc.name.c_str(), col, row, f, leaf);
                }
            const Found e = walk(sc, R, &rec[f], T.budget[f]);
            REQUIRE(e.deepest <= sc.P.entry_rows, "%s: pixel (%u, %u): the walk from the entries needs %zu rows of %u", sc.name.c_str(), col, row, e.deepest, sc.P.entry_rows);
            REQUIRE(base.same(e), "%s: pixel (%u, %u), fork budget %u: (t, prim) = (%a, %u) from the root, (%a, %u) from the entries, leaves %zu / %zu", sc.name.c_str(), col, row, f,
                    (double)base.t, base.prim, (double)e.t, e.prim, base.leaves.size(), e.leaves.size());
        }
        // forgeries of the full list, where the ray passes leaves under the entries concerned: the comparison must notice
        if (n[PBRS_ENTRY_FORKS] != PBRS_ENTRY_ROOT && !base.leaves.empty()) {
            const uint32_t cnt = n[PBRS_ENTRY_FORKS];
            auto entry_of = [&](uint32_t leaf) {
                for (uint32_t i = 0; i < cnt; ++i)
                    if (full.e[i] <= leaf && leaf < sc.end[full.e[i]]) return i;
                return cnt;
            };
            Tally scratch;
            const uint32_t first = entry_of(base.leaves.front().first);
            pbrs_entry_record forged = full;  // the entry of the first leaf removed
            for (uint32_t i = first; i + 1 < PBRS_ENTRY_MAX; ++i) forged.e[i] = forged.e[i + 1];
            forged.e[PBRS_ENTRY_MAX - 1] = PBRS_ENTRY_UNUSED;
            REQUIRE(!base.same(walk(sc, R, &forged, scratch)), "%s: pixel (%u, %u): a list without entry %u passes", sc.name.c_str(), col, row, first);
            ++T.removed;
            for (size_t k = 1; k < base.leaves.size(); ++k) {
                const uint32_t a = entry_of(base.leaves[k - 1].first), b = entry_of(base.leaves[k].first);
                if (a == b) continue;
                forged = full;  // two entries that both hold a leaf the ray tests, swapped
                std::swap(forged.e[a], forged.e[b]);
                REQUIRE(!base.same(walk(sc, R, &forged, scratch)), "%s: pixel (%u, %u): a list with entries %u and %u swapped passes", sc.name.c_str(), col, row, a, b);
                ++T.swapped;
                break;
            }
        }
    }
}

// a child box grown outside its parent's: no table for the scene
void check_nesting_is_asked(const Scene& sc) {
    std::vector<pbrs_node> blas(sc.d.blas_nodes, sc.d.blas_nodes + sc.d.n_blas_nodes);
    uint32_t x = 0;  // a node a few levels down
    for (int i = 0; i < 5 && !(blas[x].b & PBRS_LEAF_FLAG); ++i) x = (i & 1) ? blas[x].a : x + 1u;
    REQUIRE(x != 0u, "%s: the BLAS is a single leaf", sc.name.c_str());
    blas[x].max[1] += 64.0f;
    pbrs_scene_desc d = sc.d;
    d.blas_nodes = blas.data();
    const SceneCheck chk = check_scene(d);
    REQUIRE(chk.code == PBRS_OK, "%s: check_scene of the grown box: %s", sc.name.c_str(), chk.message);
    const PreparedScene P = prepare_scene(d, chk.levels, DevOverrides{});
    REQUIRE(P.S.entry_inst == PBRS_ENTRY_NONE && !P.facts.entry_nodes && !choose_kernels(P.facts, DevOverrides{}).entry_extend,
            "%s: a BLAS with a box outside its parent's keeps its table", sc.name.c_str());
}

void run(const char* name, const Mesh& mesh, const float move[3], const View& v, uint32_t sample) {
    Scene sc;
    build(sc, name, mesh, move, v);
    check_nesting_is_asked(sc);
    Totals T;
    Rng rng{0xe27a0000ull + v.width};
    if (sample == 0u) {
        for (uint32_t row = 0; row < v.height; ++row)
            for (uint32_t col = 0; col < v.width; ++col) check_pixel(sc, col, row, rng, T);
    } else {
        for (uint32_t i = 0; i < sample; ++i) check_pixel(sc, rng.below(v.width), rng.below(v.height), rng, T);
    }
    REQUIRE(T.with > 0u && T.removed > 0u, "%s: no pixel with entries, or no forged list", name);
    std::printf("%s: BLAS height %u, stack rows %u, pixels %llu (with entries %llu, empty %llu, from the root %llu), entries per pixel with some %.2f at mean depth %.1f, "
                "rays %llu (hits %llu, outside the guarded range %llu), forged lists caught: removed %llu, swapped %llu\n",
                name, sc.P.entry_height, sc.P.entry_rows, (unsigned long long)T.pixels, (unsigned long long)T.with, (unsigned long long)T.empty, (unsigned long long)T.sentinel,
                (double)T.entries / (double)T.with, T.depth_sum / (double)T.entries, (unsigned long long)T.rays, (unsigned long long)T.hits, (unsigned long long)T.slow,
                (unsigned long long)T.removed, (unsigned long long)T.swapped);
    const double r = (double)T.rays;
    std::printf("%s: pops per camera ray (passing, failed): from the root %.2f (%.2f, %.2f)", name, (T.root.passed + T.root.failed) / r, T.root.passed / r, T.root.failed / r);
    for (uint32_t f = 0; f <= PBRS_ENTRY_FORKS; ++f)
        std::printf("; fork budget %u %.2f (%.2f, %.2f)", f, (T.budget[f].passed + T.budget[f].failed) / r, T.budget[f].passed / r, T.budget[f].failed / r);
    std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
    const bool full = argc > 1 && std::string(argv[1]) == "full";
    const float moved[3] = {-100.0f, 0.0f, 0.0f}, none[3] = {0.0f, 0.0f, 0.0f};
    const Mesh small = terrain_mesh(64, 128);
    if (!full) {
        run("translated", small, moved, View{96, 64, {0, 60, -90}, {0, 0, 160}, {0, 1, 0}}, 0);
        run("identity", small, none, View{96, 64, {100, 60, -90}, {100, 0, 160}, {0, 1, 0}}, 0);
        run("above", small, moved, View{64, 48, {3, 300, 190}, {3, 0, 190}, {0, 0, 1}}, 0);
        run("inside", small, moved, View{64, 48, {-20, 1.5f, 100}, {30, -2, 300}, {0, 1, 0}}, 0);
        run("straddle", small, moved, View{64, 48, {0, 30, -90}, {0, 30, 160}, {0, 1, 0}}, 0);
    } else {
        run("full", terrain_mesh(512, 1024), moved, View{1920, 1080, {0, 60, -90}, {0, 0, 160}, {0, 1, 0}}, 300);
    }
    std::printf("ok\n");
    return 0;
}
