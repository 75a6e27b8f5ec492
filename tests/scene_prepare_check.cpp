// tests/scene_prepare_check.cpp — the host-only steps of pbrs_upload_scene (pbrs_amd/csrc/host/scene_prepare.h, kernel_choice.h) on a
// CPU: a program of its own that tests/test_scene_prepare.py compiles with -fsanitize=address,undefined and runs.
//
//   usage: scene_prepare_check <path of host/scene_prepare.cpp>
//
// Scenes come from pbrs_host_scene_build; every array of a descriptor is then copied into a heap block of exactly its size, so that a
// read past an array's end is an AddressSanitizer error.  Checked:
//   refusals         one row per refusal of check_scene: a mutation, the code and the message; the rows are compared with the
//                    `return refuse(` sites of the source, so a refusal without a row fails
//   prepared layout  nodes, instance annotations, stack depth and the four-wide tree, each from the descriptor and recursions written here
//   kernel choice    choose_kernels over every combination of SceneFacts prepare_scene can produce, default overrides and each changed singly
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <regex>
#include <set>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include "../include/pbrs_host.h"
#include "../pbrs_amd/csrc/host/scene_prepare.h"
#include "kernel_choice_sweep.h"

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

uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// ---- a descriptor whose arrays are heap blocks of exactly their size ----
struct Owned {
    pbrs_scene_desc d;
    std::vector<void*> blocks;
    template <class T>
    void own(const T*& p, size_t n) {
        T* q = static_cast<T*>(std::malloc(n * sizeof(T)));
        if (n) std::memcpy(q, p, n * sizeof(T));
        blocks.push_back(q);
        p = q;
    }
    explicit Owned(const pbrs_scene_desc& src) : d(src) {
        own(d.tlas_nodes, d.n_tlas_nodes);
        own(d.instances, d.n_instances);
        own(d.shapes, d.n_shapes);
        own(d.meshes, d.n_meshes);
        own(d.blas_nodes, d.n_blas_nodes);
        own(d.tri_verts, d.n_triangles);
        own(d.tri_shade, d.n_triangles);
        own(d.materials, d.n_materials);
        own(d.bxdfs, d.n_bxdfs);
        own(d.area_lights, d.n_area_lights);
        own(d.delta_lights, d.n_delta_lights);
        own(d.textures, d.n_textures);
        own(d.tex_floats, d.n_tex_floats);
        own(d.tex_words, d.n_tex_words);
        own(d.fourier_tables, d.n_fourier_tables);
    }
    Owned(const Owned& o) : Owned(o.d) {}
    Owned& operator=(const Owned&) = delete;
    ~Owned() {
        for (void* p : blocks) std::free(p);
    }
};
template <class T>
T& mut(const T* p, size_t i) { return const_cast<T&>(p[i]); }

// ---- scenes ----
struct Grid {
    std::vector<float> pos, nrm, uv;
    std::vector<uint32_t> idx;
    pbrs_mesh_spec spec{};
    // n x n cells over [-1, 1]^2 in x and z, heights in (0.2, 0.3); `tiny`: one vertex at height 1e-30
    Grid(uint32_t n, bool tiny) {
        for (uint32_t j = 0; j <= n; ++j)
            for (uint32_t i = 0; i <= n; ++i) {
                const float x = ((float)i - 0.5f * (float)n) / (0.5f * (float)n), z = ((float)j - 0.5f * (float)n) / (0.5f * (float)n);
                float y = 0.25f + 0.05f * std::sin(3.0f * x) * std::cos(2.0f * z);
                if (tiny && i == n / 3 && j == n / 2) y = 1e-30f;
                pos.insert(pos.end(), {x, y, z});
                nrm.insert(nrm.end(), {0.0f, 1.0f, 0.0f});
                uv.insert(uv.end(), {(float)i / (float)n, (float)j / (float)n});
            }
        for (uint32_t j = 0; j < n; ++j)
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t a = j * (n + 1) + i, b = a + 1, c = a + n + 1, e = c + 1;
                idx.insert(idx.end(), {a, b, c, b, e, c});
            }
        spec.n_vertices = (n + 1) * (n + 1);
        spec.n_triangles = 2 * n * n;
        spec.positions = pos.data();
        spec.normals = nrm.data();
        spec.uvs = uv.data();
        spec.indices = idx.data();
    }
};

pbrs_instance_spec instance(uint32_t shape, uint32_t material, float tx, float ty, float tz, bool rotate) {
    pbrs_instance_spec s{};
    s.shape = shape;
    s.material = material;
    // column-major: m[4 * col + row].  rotate: a quarter turn about y (exact zeros and ones), then the translation
    const float R[3][3] = {{0.0f, 0.0f, 1.0f}, {0.0f, 1.0f, 0.0f}, {-1.0f, 0.0f, 0.0f}}, I[3][3] = {{1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}};
    const float t[3] = {tx, ty, tz};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            s.forward[4 * c + r] = rotate ? R[r][c] : I[r][c];
            s.inverse[4 * c + r] = rotate ? R[c][r] : I[r][c];
        }
    for (int r = 0; r < 3; ++r) {
        s.forward[12 + r] = t[r];
        float it = 0.0f;  // -(R^T t)
        for (int c = 0; c < 3; ++c) it += (rotate ? R[c][r] : I[r][c]) * t[c];
        s.inverse[12 + r] = -it;
    }
    s.forward[15] = s.inverse[15] = 1.0f;
    return s;
}

pbrs_material_spec material(uint32_t kind, float r, float g, float b) {
    pbrs_material_spec m{};
    m.kind = kind;
    m.p[0] = r, m.p[1] = g, m.p[2] = b;
    return m;
}

enum SceneKind { FIRST, WITH_QUAD, SPHERES, BIG_MESH, BIG_MESH_TINY, TEXTURED };

// materials of FIRST: 0, 1 Lambertian (one signature), 2 mirror, 3 emitter.  Instances: 0 the mesh translated, 1 the mesh rotated, 2 a
// sphere, 3 a cuboid, 4 a disk that emits.  BIG_MESH: instances 0 and 1 over a grid of 48 x 48 cells.
Owned build(SceneKind kind) {
    const bool first_like = kind == FIRST || kind == WITH_QUAD || kind == TEXTURED;
    Grid grid(first_like ? 16u : 48u, kind == BIG_MESH_TINY);
    std::vector<pbrs_shape_spec> shapes;
    std::vector<pbrs_material_spec> mats = {material(PBRS_MTL_LAMBERTIAN, 0.7f, 0.6f, 0.5f), material(PBRS_MTL_LAMBERTIAN, 0.2f, 0.3f, 0.8f),
                                            material(PBRS_MTL_MIRROR, 0.9f, 0.9f, 0.9f), material(PBRS_MTL_DIFFUSE_LIGHT, 4.0f, 4.0f, 4.0f)};
    std::vector<pbrs_instance_spec> inst;
    auto shape = [&](uint32_t k, std::initializer_list<float> p) {
        pbrs_shape_spec s{};
        s.kind = k;
        std::copy(p.begin(), p.end(), s.p);
        shapes.push_back(s);
        return (uint32_t)shapes.size() - 1u;
    };
    pbrs_shape_spec mesh_shape{};
    mesh_shape.kind = PBRS_SHAPE_MESH;
    if (kind == SPHERES) {
        const uint32_t s = shape(PBRS_SHAPE_SPHERE, {0.0f, 0.0f, 0.0f, 0.4f});
        for (int i = 0; i < 40; ++i) inst.push_back(instance(s, (uint32_t)(i % 3), (float)(i % 8) - 3.5f, (float)(i / 8) - 2.0f, -6.0f, false));
    } else {
        shapes.push_back(mesh_shape);
        inst.push_back(instance(0, 0, 0.5f, -1.0f, -4.0f, false));
        inst.push_back(instance(0, 1, -2.5f, -1.0f, -5.0f, true));  // (a lone instance has no scanned TLAS, and so no wide nodes)
        if (first_like) {
            inst.push_back(instance(shape(PBRS_SHAPE_SPHERE, {0.0f, 0.0f, 0.0f, 0.5f}), 2, 1.5f, 0.5f, -3.0f, false));
            inst.push_back(instance(shape(PBRS_SHAPE_CUBOID, {-0.3f, -0.3f, -0.3f, 0.3f, 0.3f, 0.3f}), 0, -1.0f, 0.5f, -3.0f, true));
            inst.push_back(instance(shape(PBRS_SHAPE_DISK, {0.0f, 2.0f, -4.0f, 0.0f, -1.0f, 0.0f, 0.5f, 0.0f, 0.0f}), 3, 0.0f, 0.0f, 0.0f, false));
        }
        if (kind == WITH_QUAD) inst.push_back(instance(shape(PBRS_SHAPE_QUAD, {-3.0f, -1.5f, -8.0f, 6.0f, 0.0f, 0.0f, 0.0f, 4.0f, 0.0f}), 1, 0.0f, 0.0f, 0.0f, false));
    }
    pbrs_area_light_spec area{};
    area.emit[0] = area.emit[1] = area.emit[2] = 5.0f;
    area.shape.kind = PBRS_SHAPE_SPHERE;
    area.shape.p[1] = 3.0f, area.shape.p[2] = -4.0f, area.shape.p[3] = 0.25f;
    pbrs_delta_light_spec point{};
    point.kind = PBRS_DELTA_POINT;
    point.v[0] = 2.0f, point.v[1] = 2.0f, point.v[2] = 0.0f;
    point.color[0] = point.color[1] = point.color[2] = 3.0f;
    point.world_radius = 10.0f;

    // TEXTURED: a Perlin and an Image texture, a Lambertian on each, one Fourier table and its material (none of them on an instance)
    std::vector<float> perlin_vec(256 * 3), texels(2 * 2 * 3, 0.5f);
    std::vector<uint32_t> perm(3 * 256);
    for (size_t i = 0; i < perlin_vec.size(); ++i) perlin_vec[i] = i % 3 == 0 ? 1.0f : 0.0f;
    for (size_t i = 0; i < perm.size(); ++i) perm[i] = (uint32_t)((i * 7u) % 256u);
    std::vector<pbrs_texture_spec> textures(2);
    textures[0].kind = PBRS_TEX_PERLIN, textures[0].freq = 2.0f, textures[0].data = perlin_vec.data(), textures[0].perm = perm.data();
    textures[1].kind = PBRS_TEX_IMAGE, textures[1].width = 2, textures[1].height = 2, textures[1].data = texels.data();
    const float mu[3] = {-1.0f, 0.0f, 1.0f}, cdf[9] = {0, 0.5f, 1, 0, 0.5f, 1, 0, 0.5f, 1}, coeffs[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
    int32_t off_len[18];
    for (int i = 0; i < 9; ++i) off_len[2 * i] = i, off_len[2 * i + 1] = 1;
    pbrs_fourier_table_spec table{};
    table.n_mu = 3, table.n_channels = 1, table.n_coeffs = 9, table.eta = 1.0f;
    table.mu = mu, table.cdf = cdf, table.offset_and_length = off_len, table.a = coeffs;

    pbrs_scene_spec spec{};
    if (kind == TEXTURED) {
        for (uint32_t t = 1; t <= 2; ++t) {
            mats.push_back(material(PBRS_MTL_LAMBERTIAN, 0.5f, 0.5f, 0.5f));
            mats.back().tex[0] = t;
        }
        mats.push_back(material(PBRS_MTL_FOURIER, 0.0f, 0.0f, 0.0f));
        spec.n_textures = 2, spec.textures = textures.data();
        spec.n_fourier_tables = 1, spec.fourier_tables = &table;
    }
    spec.n_meshes = kind == SPHERES ? 0u : 1u;
    spec.meshes = &grid.spec;
    spec.n_shapes = (uint32_t)shapes.size(), spec.shapes = shapes.data();
    spec.n_materials = (uint32_t)mats.size(), spec.materials = mats.data();
    spec.n_instances = (uint32_t)inst.size(), spec.instances = inst.data();
    spec.n_area_lights = 1, spec.area_lights = &area;
    spec.n_delta_lights = 1, spec.delta_lights = &point;
    spec.camera.width = spec.camera.height = 32;
    spec.camera.fov_y_rad = 0.8f;
    spec.camera.target[2] = -1.0f, spec.camera.up[1] = 1.0f;
    spec.env_kind = PBRS_ENV_CONSTANT;
    pbrs_host_scene* hs = nullptr;
    REQUIRE(pbrs_host_scene_build(&spec, &hs) == PBRS_OK, "pbrs_host_scene_build (scene %d): %s", (int)kind, pbrs_host_last_error());
    Owned o(*pbrs_host_scene_desc(hs));
    pbrs_host_scene_free(hs);
    return o;
}

// ---- refusals ----
struct Row {
    SceneKind scene;  // FIRST, or TEXTURED where the first scene has nothing to mutate
    int code;
    const char* message;
    std::function<void(pbrs_scene_desc&)> mutate;
};
uint32_t first_node(const pbrs_node* n, uint32_t count, bool leaf) {
    for (uint32_t i = 0; i < count; ++i)
        if (((n[i].b & PBRS_LEAF_FLAG) != 0u) == leaf) return i;
    die("no such node");
}
uint32_t texture_of_kind(const pbrs_scene_desc& d, uint32_t kind) {
    for (uint32_t i = 0; i < d.n_textures; ++i)
        if (d.textures[i].kind == kind) return i;
    die("no texture of kind %u", kind);
}
uint32_t mesh_instance(const pbrs_scene_desc& d) {
    for (uint32_t i = 0; i < d.n_instances; ++i)
        if (d.instances[i].shape_kind == PBRS_SHAPE_MESH) return i;
    die("no mesh instance");
}
const std::vector<Row>& rows() {
    static const std::vector<Row> r = {
        {FIRST, PBRS_E_INVALID, "scene without instances", [](pbrs_scene_desc& d) { d.n_instances = 0; }},
        {FIRST, PBRS_E_INVALID, "tlas leaf references a missing instance",
         [](pbrs_scene_desc& d) { mut(d.tlas_nodes, first_node(d.tlas_nodes, d.n_tlas_nodes, true)).a = d.n_instances; }},
        {FIRST, PBRS_E_INVALID, "tlas child out of range", [](pbrs_scene_desc& d) { mut(d.tlas_nodes, 0).a = d.n_tlas_nodes; }},
        {FIRST, PBRS_E_INVALID, "tlas nodes are not in pre-order", [](pbrs_scene_desc& d) { mut(d.tlas_nodes, 0).a = 0; }},
        {FIRST, PBRS_E_INVALID, "blas leaf range out of range",
         [](pbrs_scene_desc& d) { mut(d.blas_nodes, first_node(d.blas_nodes, d.n_blas_nodes, true)).a = d.n_triangles; }},
        {FIRST, PBRS_E_INVALID, "blas child out of range", [](pbrs_scene_desc& d) { mut(d.blas_nodes, 0).a = d.n_blas_nodes; }},
        {FIRST, PBRS_E_INVALID, "blas nodes are not in pre-order", [](pbrs_scene_desc& d) { mut(d.blas_nodes, 0).a = 0; }},
        {FIRST, PBRS_E_INVALID, "mesh root out of range", [](pbrs_scene_desc& d) { mut(d.meshes, 0).root = d.n_blas_nodes; }},
        {FIRST, PBRS_E_INVALID, "instance material out of range", [](pbrs_scene_desc& d) { mut(d.instances, d.n_instances - 1).material = d.n_materials; }},
        {FIRST, PBRS_E_INVALID, "unknown shape kind", [](pbrs_scene_desc& d) { mut(d.instances, 2).shape_kind = PBRS_SHAPE_MESH + 1; }},
        {FIRST, PBRS_E_INVALID, "instance shape out of range", [](pbrs_scene_desc& d) { mut(d.instances, 2).shape_index = d.n_shapes; }},
        {FIRST, PBRS_E_INVALID, "instance blas_root out of range", [](pbrs_scene_desc& d) { mut(d.instances, mesh_instance(d)).blas_root = d.n_blas_nodes; }},
        {FIRST, PBRS_E_INVALID, "material lobes out of range", [](pbrs_scene_desc& d) { mut(d.materials, 0).n_bxdfs = PBRS_MAX_BXDFS + 1; }},
        {FIRST, PBRS_E_INVALID, "material visualiser record out of range", [](pbrs_scene_desc& d) { mut(d.materials, 0).vis_bxdf = d.n_bxdfs + 1; }},
        {FIRST, PBRS_E_INVALID, "lobe texture out of range", [](pbrs_scene_desc& d) { mut(d.bxdfs, 0).tex = d.n_textures + 1; }},
        {FIRST, PBRS_E_INVALID, "unknown lobe kind", [](pbrs_scene_desc& d) { mut(d.bxdfs, 0).kind = PBRS_BXDF_FOURIER + 1; }},
        {FIRST, PBRS_E_INVALID, "Fourier lobe table out of range", [](pbrs_scene_desc& d) { mut(d.bxdfs, 0).kind = PBRS_BXDF_FOURIER; }},
        {TEXTURED, PBRS_E_INVALID, "Fourier table: sizes", [](pbrs_scene_desc& d) { mut(d.fourier_tables, 0).n_mu = 2; }},
        {TEXTURED, PBRS_E_INVALID, "Fourier table: arrays out of range", [](pbrs_scene_desc& d) { mut(d.fourier_tables, 0).mu = d.n_tex_floats - 2; }},
        {TEXTURED, PBRS_E_INVALID, "Fourier table: mu is not finite and strictly ascending",
         [](pbrs_scene_desc& d) { mut(d.tex_floats, d.fourier_tables[0].mu + 2) = d.tex_floats[d.fourier_tables[0].mu + 1]; }},
        {TEXTURED, PBRS_E_INVALID, "Fourier table: series out of range",
         [](pbrs_scene_desc& d) { mut(d.tex_words, d.fourier_tables[0].m_lookup + 8) = d.fourier_tables[0].m_max + 1; }},
        {TEXTURED, PBRS_E_INVALID, "perlin tables out of range", [](pbrs_scene_desc& d) { mut(d.textures, texture_of_kind(d, PBRS_TEX_PERLIN)).perm = d.n_tex_words - 767; }},
        {TEXTURED, PBRS_E_INVALID, "perlin permutation entry above 255",
         [](pbrs_scene_desc& d) { mut(d.tex_words, d.textures[texture_of_kind(d, PBRS_TEX_PERLIN)].perm + 767) = 256; }},
        {TEXTURED, PBRS_E_INVALID, "image texels out of range", [](pbrs_scene_desc& d) { mut(d.textures, texture_of_kind(d, PBRS_TEX_IMAGE)).data = d.n_tex_floats - 11; }},
        {TEXTURED, PBRS_E_INVALID, "unknown texture kind", [](pbrs_scene_desc& d) { mut(d.textures, 0).kind = PBRS_TEX_IMAGE + 1; }},
        {FIRST, PBRS_E_INVALID, "unknown environment kind", [](pbrs_scene_desc& d) { d.env_kind = 99; }},
        {FIRST, PBRS_E_INVALID, "environment map is not an image texture", [](pbrs_scene_desc& d) { d.env_kind = PBRS_ENV_IMAGE; }},
        {FIRST, PBRS_E_INVALID, "area light shape kind", [](pbrs_scene_desc& d) { mut(d.area_lights, 0).shape_kind = PBRS_SHAPE_CUBOID; }},
    };
    return r;
}
// Left out: each needs an input too large for a test (a tree 81 levels deep; 2^31 nodes; 4 GiB of nodes).
const char* const kLeftOut[] = {"traversal stack exceeds the LDS budget", "too many BVH nodes", "too many BVH nodes (the walks address them with 32-bit byte offsets)"};

void check_refusals(const Owned& first, const Owned& textured, const char* source_path) {
    REQUIRE(check_scene(first.d).code == PBRS_OK && check_scene(textured.d).code == PBRS_OK, "an unmutated scene is refused: %s / %s",
            check_scene(first.d).message, check_scene(textured.d).message);
    for (const Row& row : rows()) {
        Owned o(row.scene == FIRST ? first : textured);
        row.mutate(o.d);
        const SceneCheck c = check_scene(o.d);
        REQUIRE(c.code == row.code && c.message && std::strcmp(c.message, row.message) == 0, "row \"%s\": got %d \"%s\", expected %d", row.message, c.code,
                c.message ? c.message : "(accepted)", row.code);
    }
    // every `return refuse(` of check_scene has a row or is listed as left out
    std::ifstream in(source_path);
    REQUIRE(in.good(), "cannot read %s", source_path);
    std::stringstream ss;
    ss << in.rdbuf();
    std::string text = ss.str();
    const size_t a = text.find("\nSceneCheck check_scene("), b = text.find("\nPreparedScene prepare_scene(");
    REQUIRE(a != std::string::npos && b != std::string::npos && a < b, "check_scene not found in %s", source_path);
    text = text.substr(a, b - a);
    const std::regex site("return refuse\\((PBRS_E_[A-Z]+), \"([^\"]*)\"\\)");
    size_t sites = 0, plain_returns = 0;
    for (auto it = std::sregex_iterator(text.begin(), text.end(), site); it != std::sregex_iterator(); ++it, ++sites) {
        const std::string code = (*it)[1], msg = (*it)[2];
        bool found = false;
        for (const Row& row : rows()) found = found || (msg == row.message && code == (row.code == PBRS_E_INVALID ? "PBRS_E_INVALID" : "PBRS_E_LIMIT"));
        for (const char* l : kLeftOut) found = found || (msg == l && code == "PBRS_E_LIMIT");
        REQUIRE(found, "check_scene refuses with \"%s\" (%s) and no row covers it", msg.c_str(), code.c_str());
    }
    for (size_t at = text.find("return "); at != std::string::npos; at = text.find("return ", at + 1)) ++plain_returns;
    REQUIRE(sites == rows().size() + std::size(kLeftOut), "%zu refusal sites, %zu rows + %zu left out", sites, rows().size(), std::size(kLeftOut));
    REQUIRE(plain_returns == sites + 1, "check_scene has %zu returns for %zu refusals and one acceptance", plain_returns, sites);
    std::printf("refusals: %zu rows, %zu left out, %zu sites\n", rows().size(), std::size(kLeftOut), sites);
}

// ---- prepared layout ----
struct Expect {
    const char* name;
    bool scanned, flat_feature, exact_extent, fast_slab, wide;
};
uint32_t height(const pbrs_node* n, uint32_t i) { return (n[i].b & PBRS_LEAF_FLAG) ? 1u : 1u + std::max(height(n, i + 1), height(n, n[i].a)); }
void leaves_left_first(const pbrs_node* n, uint32_t i, std::vector<uint32_t>& out) {
    if (n[i].b & PBRS_LEAF_FLAG) return out.push_back(i);
    leaves_left_first(n, i + 1, out);
    leaves_left_first(n, n[i].a, out);
}
// wide levels below the inner node x of the binary tree: two binary levels per wide node
uint32_t wide_levels_of(const pbrs_node* n, uint32_t x) {
    uint32_t below = 0;
    for (uint32_t ch : {x + 1u, n[x].a})
        if (!(n[ch].b & PBRS_LEAF_FLAG))
            for (uint32_t g : {ch + 1u, n[ch].a})
                if (!(n[g].b & PBRS_LEAF_FLAG)) below = std::max(below, wide_levels_of(n, g));
    return 1u + below;
}
bool same_box(const pbrs_wnode& w, uint32_t k, const pbrs_node& n) {
    bool same = true;
    for (int a = 0; a < 3; ++a) same = same && bits(w.lo[a][k]) == bits(n.min[a]) && bits(w.hi[a][k]) == bits(n.max[a]);
    return same;
}
// The wide node `wi` stands for the inner node x of `nodes` (the prepared array, absolute links): slots, boxes, axis bits; appends the
// leaves it reaches through slots 0 .. 3.
void walk_wide(const PreparedScene& P, uint32_t wi, uint32_t x, std::vector<uint32_t>& leaves) {
    const std::vector<pbrs_node>& n = P.nodes;
    REQUIRE(wi < P.wide.size(), "wide index %u out of %zu", wi, P.wide.size());
    const pbrs_wnode& w = P.wide[wi];
    const uint32_t child[2] = {x + 1u, n[x].a};
    uint32_t slot_node[4];
    bool used[4] = {false, false, false, false};
    uint32_t axis[3] = {n[x].b & 3u, 0u, 0u};
    for (uint32_t s = 0; s < 2; ++s) {
        const pbrs_node& ch = n[child[s]];
        if (ch.b & PBRS_LEAF_FLAG) {
            slot_node[2 * s] = child[s], used[2 * s] = true;
        } else {
            axis[1 + s] = ch.b & 3u;
            slot_node[2 * s] = child[s] + 1u, slot_node[2 * s + 1] = ch.a, used[2 * s] = used[2 * s + 1] = true;
        }
    }
    REQUIRE((w.child[0] >> PBRS_WREF_AXIS_SHIFT & 3u) == axis[0] && (w.child[0] >> (PBRS_WREF_AXIS_SHIFT + 2) & 3u) == axis[1] &&
                (w.child[2] >> PBRS_WREF_AXIS_SHIFT & 3u) == axis[2],
            "wide node %u: axis bits", wi);
    for (uint32_t k = 0; k < 4; ++k) {
        if (!used[k]) {
            REQUIRE(w.child[k] == PBRS_WREF_NONE, "wide node %u slot %u: unused slot names %08x", wi, k, w.child[k]);
            for (int a = 0; a < 3; ++a)
                REQUIRE(w.lo[a][k] == 1152921504606846976.0f && w.hi[a][k] == -1152921504606846976.0f, "wide node %u slot %u: unused planes", wi, k);
            continue;
        }
        REQUIRE(same_box(w, k, n[slot_node[k]]), "wide node %u slot %u: box differs from node %u", wi, k, slot_node[k]);
        const uint32_t axis_bits = k == 0 ? 15u << PBRS_WREF_AXIS_SHIFT : k == 2 ? 3u << PBRS_WREF_AXIS_SHIFT : 0u;
        const uint32_t ref = w.child[k] & ~axis_bits;
        if (n[slot_node[k]].b & PBRS_LEAF_FLAG) {
            REQUIRE(ref == (PBRS_WREF_LEAF | slot_node[k]), "wide node %u slot %u: leaf reference %08x, node %u", wi, k, w.child[k], slot_node[k]);
            leaves.push_back(slot_node[k]);
        } else {
            REQUIRE(!(ref & PBRS_WREF_LEAF) && ref == (ref & PBRS_WREF_INDEX), "wide node %u slot %u: inner reference %08x", wi, k, w.child[k]);
            walk_wide(P, ref, slot_node[k], leaves);
        }
    }
}
// the lobe signature of a material, restated: two materials shade alike where these agree
std::vector<std::tuple<uint32_t, uint32_t, uint32_t, bool, bool>> signature(const pbrs_scene_desc& d, uint32_t m) {
    std::vector<std::tuple<uint32_t, uint32_t, uint32_t, bool, bool>> s;
    for (uint32_t k = 0; k < d.materials[m].n_bxdfs; ++k) {
        const pbrs_bxdf& b = d.bxdfs[d.materials[m].first_bxdf + k];
        s.emplace_back(b.kind, b.kind == PBRS_BXDF_SPECULAR ? b.intrusion : 0u, b.kind == PBRS_BXDF_DIFFUSE ? b.oren_nayar : b.fresnel,
                       b.kind == PBRS_BXDF_MICROFACET && b.alpha_x != b.alpha_y, b.tex != 0u);
    }
    return s;
}

PreparedScene check_layout(const Owned& o, const Expect& e) {
    const pbrs_scene_desc& d = o.d;
    const SceneCheck chk = check_scene(d);
    REQUIRE(chk.code == PBRS_OK, "%s: refused: %s", e.name, chk.message);
    const PreparedScene P = prepare_scene(d, chk.levels, DevOverrides{});
    const DevScene& S = P.S;
    // nodes: the TLAS bit for bit, its leaves in pre-order (2 .. 32 instances), the BLAS nodes with shifted inner links
    std::vector<pbrs_node> flat;
    if (d.n_instances >= 2 && d.n_instances <= 32)
        for (uint32_t i = 0; i < d.n_tlas_nodes; ++i)
            if (d.tlas_nodes[i].b & PBRS_LEAF_FLAG) flat.push_back(d.tlas_nodes[i]);
    REQUIRE(!flat.empty() == e.scanned, "%s: %zu leaf copies expected", e.name, flat.size());
    const uint32_t blas_off = d.n_tlas_nodes + (uint32_t)flat.size();
    REQUIRE(P.nodes.size() == (size_t)blas_off + d.n_blas_nodes, "%s: %zu nodes", e.name, P.nodes.size());
    REQUIRE(std::memcmp(P.nodes.data(), d.tlas_nodes, d.n_tlas_nodes * sizeof(pbrs_node)) == 0, "%s: the TLAS is not copied bit for bit", e.name);
    REQUIRE(flat.empty() || std::memcmp(P.nodes.data() + d.n_tlas_nodes, flat.data(), flat.size() * sizeof(pbrs_node)) == 0, "%s: leaf copies", e.name);
    REQUIRE(S.flat_off == d.n_tlas_nodes && S.n_flat == flat.size(), "%s: flat_off %u n_flat %u", e.name, S.flat_off, S.n_flat);
    for (uint32_t i = 0; i < d.n_blas_nodes; ++i) {
        pbrs_node want = d.blas_nodes[i];
        if (!(want.b & PBRS_LEAF_FLAG)) want.a += blas_off;
        REQUIRE(std::memcmp(&P.nodes[blas_off + i], &want, sizeof want) == 0, "%s: BLAS node %u", e.name, i);
    }
    // instances
    REQUIRE(P.inst.size() == d.n_instances, "%s: %zu instances", e.name, P.inst.size());
    uint32_t flagged = 0;
    for (uint32_t i = 0; i < d.n_instances; ++i) {
        const pbrs_instance &in = d.instances[i], &out = P.inst[i];
        pbrs_instance want = in;
        if (in.shape_kind == PBRS_SHAPE_MESH) want.blas_root += blas_off;
        bool identity = true;
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) identity = identity && bits(in.inv[r][k]) == bits(r == k ? 1.0f : 0.0f);
        want.flags = (in.flags & ~0x100u) | (identity ? 0x100u : 0u);
        flagged += identity ? 1u : 0u;
        want.pad[0] = out.pad[0], want.pad[1] = out.pad[1];
        REQUIRE(std::memcmp(&out, &want, sizeof want) == 0, "%s: instance %u (blas_root %u, flags %x)", e.name, i, out.blas_root, out.flags);
        REQUIRE((out.pad[0] == 0u) == (d.materials[in.material].n_bxdfs == 0u), "%s: instance %u: class %u", e.name, i, out.pad[0]);
        for (uint32_t j = 0; j < i; ++j)
            REQUIRE((out.pad[0] == P.inst[j].pad[0]) == (signature(d, in.material) == signature(d, d.instances[j].material)), "%s: classes of instances %u and %u", e.name, i,
                    j);
    }
    // stack depth, from a recursive height
    const uint32_t h_tlas = height(d.tlas_nodes, 0);
    uint32_t h_blas = 0;
    bool quad = false, mesh = false;
    for (uint32_t i = 0; i < d.n_meshes; ++i) h_blas = std::max(h_blas, height(d.blas_nodes, d.meshes[i].root));
    for (uint32_t i = 0; i < d.n_instances; ++i) {
        if (d.instances[i].shape_kind == PBRS_SHAPE_MESH) h_blas = std::max(h_blas, height(d.blas_nodes, d.instances[i].blas_root)), mesh = true;
        quad = quad || d.instances[i].shape_kind == PBRS_SHAPE_QUAD;
    }
    REQUIRE((quad && mesh) == e.exact_extent && S.exact_extent == (e.exact_extent ? 1u : 0u) && P.facts.exact_extent == e.exact_extent, "%s: exact_extent %u", e.name,
            S.exact_extent);
    const uint32_t depth = std::max(h_tlas, h_tlas - 1u + h_blas) + (e.exact_extent ? h_tlas + 1u : 0u);
    REQUIRE(P.stack_depth == depth, "%s: stack depth %u, expected %u (h_tlas %u, h_blas %u)", e.name, P.stack_depth, depth, h_tlas, h_blas);
    REQUIRE(P.facts.stack_bytes == (size_t)depth * 256u * 4u, "%s: stack bytes", e.name);
    REQUIRE(S.fast_slab == (e.fast_slab ? 1u : 0u) && P.facts.full_steps == !e.fast_slab, "%s: fast_slab %u", e.name, S.fast_slab);
    REQUIRE(P.facts.tlas_scanned == e.scanned && ((S.features & PBRS_FEAT_FLAT_TLAS) != 0u) == e.flat_feature && P.facts.features == S.features, "%s: features %x", e.name,
            S.features);
    // the four-wide tree
    uint32_t levels = 0;
    for (uint32_t i = 0; i < d.n_instances; ++i)
        if (d.instances[i].shape_kind == PBRS_SHAPE_MESH && !(d.blas_nodes[d.instances[i].blas_root].b & PBRS_LEAF_FLAG))
            levels = std::max(levels, wide_levels_of(d.blas_nodes, d.instances[i].blas_root));
    REQUIRE((e.scanned && e.fast_slab && levels >= PBRS_WIDE_MIN_LEVELS) == e.wide, "%s: %u wide levels", e.name, levels);
    REQUIRE(!P.wide.empty() == e.wide && P.facts.wide_ok == e.wide, "%s: %zu wide nodes", e.name, P.wide.size());
    const uint32_t cap = e.wide ? std::max(4u, std::min(3u * levels + 1u, (uint32_t)PBRS_WIDE_STACK_MAX)) : 4u;
    REQUIRE(S.wide_cap == cap && P.facts.wide_stack_bytes == (size_t)cap * 256u * 4u, "%s: wide_cap %u, expected %u", e.name, S.wide_cap, cap);
    for (uint32_t i = 0; i < d.n_instances; ++i) {
        const pbrs_instance& out = P.inst[i];
        if (!e.wide || out.shape_kind != PBRS_SHAPE_MESH || (P.nodes[out.blas_root].b & PBRS_LEAF_FLAG)) {
            REQUIRE(out.pad[1] == PBRS_WREF_NONE, "%s: instance %u has a wide root", e.name, i);
            continue;
        }
        std::vector<uint32_t> got, want;
        walk_wide(P, out.pad[1], out.blas_root, got);
        leaves_left_first(P.nodes.data(), out.blas_root, want);
        REQUIRE(got == want, "%s: instance %u: the wide tree reaches %zu leaves, the binary tree %zu, or in another order", e.name, i, got.size(), want.size());
    }
    std::printf("%s: %zu nodes (%u leaf copies), stack depth %u, %zu wide nodes in %u levels, %u of %u instances translated only\n", e.name, P.nodes.size(), S.n_flat,
                P.stack_depth, P.wide.size(), e.wide ? levels : 0u, flagged, d.n_instances);
    return P;
}

void check_layouts(const Owned& first) {
    const PreparedScene p1 = check_layout(first, {"first scene", true, true, false, true, true});
    // not vacuous: both kinds of instance transform, shared and distinct classes, an emitter
    REQUIRE((p1.inst[0].flags & 0x100u) && !(p1.inst[1].flags & 0x100u), "first scene: translation flags %x %x", p1.inst[0].flags, p1.inst[1].flags);
    REQUIRE(p1.inst[0].pad[0] == p1.inst[1].pad[0] && p1.inst[0].pad[0] != p1.inst[2].pad[0] && p1.inst[4].pad[0] == 0u && p1.S.n_classes == 2u, "first scene: classes");
    {  // a -0.0 off the diagonal is not the identity bit for bit
        Owned o(first);
        mut(o.d.instances, 0).inv[0][1] = -0.0f;
        REQUIRE(!(prepare_scene(o.d, check_scene(o.d).levels, DevOverrides{}).inst[0].flags & 0x100u), "an instance with -0.0 in inv[0][1] is flagged as translated only");
    }
    check_layout(build(WITH_QUAD), {"with a quad", true, true, true, true, true});
    const PreparedScene p3 = check_layout(build(SPHERES), {"40 spheres", false, false, false, true, false});
    REQUIRE(p3.S.n_flat == 0u && p3.nodes.size() == 79u, "40 spheres: %zu nodes", p3.nodes.size());
    const PreparedScene p4 = check_layout(build(BIG_MESH), {"large mesh", true, true, false, true, true});
    REQUIRE(p4.wide_levels >= PBRS_WIDE_MIN_LEVELS && p4.S.wide_cap > 4u, "large mesh: %u wide levels", p4.wide_levels);
    const PreparedScene p5 = check_layout(build(BIG_MESH_TINY), {"large mesh, one height 1e-30", true, true, false, false, false});
    REQUIRE(p5.facts.full_steps && p5.facts.long_walks && p5.wide.empty(), "large mesh, one height 1e-30: full steps %d", (int)p5.facts.full_steps);
}

// ---- kernel choice ----
#define SHADE_KEY(I, T, SP) std::make_tuple((uint32_t)(I), (bool)(T), (uint32_t)(SP)),
const std::set<std::tuple<uint32_t, bool, uint32_t>> kShadeKeys = {PBRS_SHADE_KERNELS(SHADE_KEY)};
#undef SHADE_KEY

void check_choice(const SceneFacts& f, const DevOverrides& dev, const char* what) {
    const KernelChoice ch = choose_kernels(f, dev);
    bool ok = extend_key_ok(ch.extend[0].key) && extend_key_ok(ch.extend[1].key) && (ch.extend[1].key & kStatsKey) && !(ch.extend[0].key & kStatsKey);
    ok = ok && shadow_key_ok(ch.shadow[0].key) && shadow_key_ok(ch.shadow[1].key) && (ch.shadow[1].key & kStatsKey) && !(ch.shadow[0].key & kStatsKey);
    ok = ok && (!ch.wide_shadow || (shadow_key_ok(ch.shadow_slow.key) && !(ch.shadow_slow.key & (kStatsKey | PBRS_FEAT_WIDE)) && (ch.shadow[0].key & PBRS_FEAT_WIDE)));
    for (const TraversalKey* k : {&ch.extend[0], &ch.extend[1], &ch.shadow[0], &ch.shadow[1]}) ok = ok && k->key < kTraversalKeys && k->lds <= kLdsBytesPerCU / 2;
    for (const IntegratorChoice& ic : ch.integ) {
        ok = ok && ic.n_shade >= 1u && ic.n_shade <= 2u;
        for (uint32_t k = 0; k < ic.n_shade && ok; ++k) ok = kShadeKeys.count(std::make_tuple(ic.shade[k].integ, ic.shade[k].tex, ic.shade[k].spec)) != 0;
    }
    REQUIRE(ok,
            "%s: features %x scanned %d extent %d long %d full %d wide %d classes %u lambert_class %u fourier_class %u textured %d fourier %d lambert %d light %u shade_lds %u "
            "stack %zu scene %zu top %zu: extend %x / %x, shadow %x / %x / %x, path shade (%d, %x) (%d, %x)",
            what, f.features, f.tlas_scanned, f.exact_extent, f.long_walks, f.full_steps, f.wide_ok, f.n_classes, f.lambert_class, f.fourier_class, f.textured, f.fourier,
            f.lambert, f.light_spec, f.shade_lds, f.stack_bytes, f.scene_bytes, f.top_bytes, ch.extend[0].key, ch.extend[1].key, ch.shadow[0].key, ch.shadow[1].key,
            ch.shadow_slow.key, (int)ch.integ[0].shade[0].tex, ch.integ[0].shade[0].spec, (int)ch.integ[0].shade[1].tex, ch.integ[0].shade[1].spec);
}

// choose_kernels over every combination of SceneFacts prepare_scene can produce (kernel_choice_sweep.h: the producibility rules), under `dev`.
size_t sweep_choices(const DevOverrides& dev, const char* what) {
    return sweep_scene_facts([&](const SceneFacts& f) { check_choice(f, dev, what); });
}

void check_choices() {
    std::vector<std::pair<const char*, DevOverrides>> devs;
    auto add = [&](const char* name, const std::function<void(DevOverrides&)>& change) {
        devs.emplace_back(name, DevOverrides{});
        change(devs.back().second);
    };
    add("default overrides", [](DevOverrides&) {});
    add("overlap_passes", [](DevOverrides& o) { o.overlap_passes = false; });
    add("sort_classes", [](DevOverrides& o) { o.sort_classes = false; });
    add("split_lambert", [](DevOverrides& o) { o.split_lambert = false; });
    add("split_fourier", [](DevOverrides& o) { o.split_fourier = false; });
    add("split_queue", [](DevOverrides& o) { o.split_queue = false; });
    add("wide_shadow", [](DevOverrides& o) { o.wide_shadow = false; });
    add("lds_scene", [](DevOverrides& o) { o.lds_scene = false; });
    add("lds_top", [](DevOverrides& o) { o.lds_top = false; });
    add("raygen_tiles8", [](DevOverrides& o) { o.raygen_tiles8 = false; });
    add("shade_spec 0", [](DevOverrides& o) { o.shade_spec = 0u; });
    add("shade_spec LAMBERT", [](DevOverrides& o) { o.shade_spec = PBRS_SHADE_LAMBERT; });
    add("shade_lds 0", [](DevOverrides& o) { o.shade_lds = 0u; });
    add("shade_lds RECORDS", [](DevOverrides& o) { o.shade_lds = PBRS_SHADE_LDS_RECORDS; });
    add("shade_lds TRIS", [](DevOverrides& o) { o.shade_lds = PBRS_SHADE_LDS_TRIS; });
    add("long_walks 0", [](DevOverrides& o) { o.long_walks = false; });
    add("long_walks 1", [](DevOverrides& o) { o.long_walks = true; });
    add("full_steps 0", [](DevOverrides& o) { o.full_steps = false; });
    add("full_steps 1", [](DevOverrides& o) { o.full_steps = true; });
    add("overlap_from", [](DevOverrides& o) { o.overlap_from = 3u; });
    add("refill_below", [](DevOverrides& o) { o.refill_below = 32u; });
    add("raygen_chunk", [](DevOverrides& o) { o.raygen_chunk = 256u; });
    add("lds_min", [](DevOverrides& o) { o.lds_min = 32768; });
    size_t each = 0;
    for (const auto& dv : devs) each = sweep_choices(dv.second, dv.first);
    std::printf("kernel choice: %zu combinations of SceneFacts under each of %zu override sets, every key instantiated\n", each, devs.size());
}

}  // namespace

int main(int argc, char** argv) {
    REQUIRE(argc == 2, "usage: scene_prepare_check <path of host/scene_prepare.cpp>");
    const Owned first = build(FIRST), textured = build(TEXTURED);
    check_refusals(first, textured, argv[1]);
    check_layouts(first);
    check_choices();
    std::printf("ok\n");
    return 0;
}
