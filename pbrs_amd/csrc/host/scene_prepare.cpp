// host/scene_prepare.cpp — check_scene and prepare_scene (host/scene_prepare.h): plain C++, linked into libpbrs_gpu.so and into the
// CPU check of tests/scene_prepare_check.cpp.
#include "scene_prepare.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <string>

#include "../../../include/pbrs_numeric.h"
#include "../../../include/pbrs_scene_spec.h"
#include "../device/entry_nodes.h"
#include "../device/split_planes.h"

namespace pbrs {
namespace {

SceneCheck refuse(int code, const char* message) { return SceneCheck{code, message, SceneLevels{}}; }

// h[i] = levels of the subtree of node i (a lone leaf: 1).  Children come after their parent (left = i + 1, right = a > i,
// check_scene): one reverse pass.
void tree_heights(const pbrs_node* nodes, uint32_t n, std::vector<uint32_t>& h) {
    h.assign(n, 1u);
    for (uint32_t i = n; i-- > 0;)
        if (!(nodes[i].b & PBRS_LEAF_FLAG)) h[i] = std::max(h[i + 1], h[nodes[i].a]) + 1u;
}

// Depth of the per-lane stack, from the trees themselves (the heights in the description are not trusted: an entry
// too few would let a lane write into its neighbour's LDS).  h = levels of a tree (a lone leaf: 1).  A walk pops a node
// of level l with l - 1 entries pending and pushes two: at most h_tlas entries in the TLAS, h_tlas - 1 pending below an
// instance, and h_blas more inside it — max(h_tlas, h_tlas - 1 + h_blas) entries.  One level matters: C4's 4 + 23 levels
// need 26 KB per block, six blocks per CU instead of five.
// `d`: its node links, mesh roots and instances are in range and its nodes in pre-order.
SceneLevels scene_levels(const pbrs_scene_desc& d) {
    SceneLevels l;
    std::vector<uint32_t> th, bh;
    tree_heights(d.tlas_nodes, d.n_tlas_nodes, th);
    tree_heights(d.blas_nodes, d.n_blas_nodes, bh);
    l.tlas = th[0];
    for (uint32_t i = 0; i < d.n_meshes; ++i) l.max_blas = std::max(l.max_blas, bh[d.meshes[i].root]);
    // a walk enters a BLAS through the instance's own blas_root (range-checked), which need not be a listed mesh root
    for (uint32_t i = 0; i < d.n_instances; ++i)
        if (d.instances[i].shape_kind == PBRS_SHAPE_MESH) l.max_blas = std::max(l.max_blas, bh[d.instances[i].blas_root]);
    l.stack = std::max(l.tlas, l.tlas - 1u + l.max_blas);
    // A ParallelQuad reports hits in the mirrored quadrants of its plane, outside its own box (D1); a mesh may return a hit beyond the
    // extent it was given, which RAISES ray.t_max when its subtree is a left one (bvh.rs:84-88).  Together they make the rise visible
    // (a box the best hit would have pruned is entered and holds a nearer hit: fuzz seed 211699), so the closest-hit walks of such a
    // scene follow ray.t_max to the letter (PBRS_FEAT_EXTENT): a pending TLAS entry then takes two stack words.
    bool has_quad = false, has_mesh = false;
    for (uint32_t i = 0; i < d.n_instances; ++i) {
        has_quad = has_quad || d.instances[i].shape_kind == PBRS_SHAPE_QUAD;
        has_mesh = has_mesh || d.instances[i].shape_kind == PBRS_SHAPE_MESH;
    }
    l.exact_extent = has_quad && has_mesh;
    if (l.exact_extent) l.stack += l.tlas + 1u;
    return l;
}

// The TLAS leaves are copied behind the TLAS for the wave's shared scan (DevScene::flat_off).
bool tlas_scanned(const pbrs_scene_desc& d) { return d.n_instances >= PBRS_FLAT_TLAS_MIN && d.n_instances <= PBRS_FLAT_TLAS_MAX_ANYHIT; }

// Four-wide nodes over the binary subtree of inner node x (device/wide.h): the boxes of x's grandchildren — or of a child that is
// a leaf — in left-first order, with the three split axes that order them.  Returns the index of x's wide node in `out`.
// `nodes`: DevScene::nodes as uploaded (absolute links; checked: children come after their parent, so the recursion ends).
uint32_t build_wide(const std::vector<pbrs_node>& nodes, uint32_t x, std::vector<pbrs_wnode>& out, uint32_t level, uint32_t& levels) {
    const uint32_t me = (uint32_t)out.size();
    out.push_back(pbrs_wnode{});
    levels = std::max(levels, level + 1u);
    uint32_t slot_node[4] = {0, 0, 0, 0};
    uint32_t used = 0, info = nodes[x].b & 3u;
    const uint32_t child[2] = {x + 1u, nodes[x].a};
    for (uint32_t s = 0; s < 2; ++s) {
        const pbrs_node& ch = nodes[child[s]];
        if (ch.b & PBRS_LEAF_FLAG) {
            slot_node[2 * s] = child[s];
            used |= 1u << (2 * s);
        } else {
            info |= (ch.b & 3u) << (2 + 2 * s);
            slot_node[2 * s] = child[s] + 1u;
            slot_node[2 * s + 1] = ch.a;
            used |= 3u << (2 * s);
        }
    }
    pbrs_wnode w{};
    for (uint32_t k = 0; k < 4; ++k) {
        w.child[k] = PBRS_WREF_NONE;
        if (!((used >> k) & 1u)) {  // never passes the filter (device/wide.h)
            for (int a = 0; a < 3; ++a) w.lo[a][k] = PBRS_WIDE_UNUSED_PLANE, w.hi[a][k] = -PBRS_WIDE_UNUSED_PLANE;
            continue;
        }
        const pbrs_node& n = nodes[slot_node[k]];
        for (int a = 0; a < 3; ++a) {
            w.lo[a][k] = n.min[a];
            w.hi[a][k] = n.max[a];
        }
        w.child[k] = (n.b & PBRS_LEAF_FLAG) ? (PBRS_WREF_LEAF | slot_node[k]) : build_wide(nodes, slot_node[k], out, level + 1u, levels);
    }
    w.child[0] |= (info & 15u) << PBRS_WREF_AXIS_SHIFT;  // slots 0 and 2 are always in use
    w.child[2] |= ((info >> 4) & 3u) << PBRS_WREF_AXIS_SHIFT;
    out[me] = w;
    return me;
}

// A coordinate inside the guarded range of the division-free box test (prepare_scene, DevScene::fast_slab)
bool coord_ok(float b) {
    const uint32_t u = pn_bits(b) & 0x7fffffffu, e = u >> 23;
    return u == 0u || (e >= 127u - 60u && e <= 127u + 40u);
}

// The split planes of inner BLAS node x (device/split_planes.h), packed for its b word; 0 — planes that cull nothing — unless both
// children's boxes lie inside x's (the cull's argument rests on that, device/traverse.h, and no check before this one asks it of a
// description).  Each number is the largest whose plane, evaluated as the device evaluates it, stays on its side of the child; a plane
// the walk's quotient is not exact for (non-zero below 2^-60: cancellation next to a coordinate of the other sign) gives way to q = 0.
uint32_t split_planes(const std::vector<pbrs_node>& nodes, uint32_t x) {
    const pbrs_node &X = nodes[x], &L = nodes[x + 1u], &R = nodes[X.a];
    for (int a = 0; a < 3; ++a) {
        const bool inside = X.min[a] <= L.min[a] && L.min[a] <= L.max[a] && L.max[a] <= X.max[a] && X.min[a] <= R.min[a] && R.min[a] <= R.max[a] && R.max[a] <= X.max[a];
        if (!inside) return 0u;  // (a NaN coordinate fails every comparison)
    }
    const uint32_t k = X.b & 3u;
    const float lo = X.min[k], hi = X.max[k], step = pbrs_plane_step(lo, hi);
    if (!(step > 0.0f) || !pn_isfinite(step)) return 0u;
    // both planes move monotonically with q (one correctly rounded operation of a monotone exact value) and q = 0 holds: bisection
    uint32_t qd = 0u, qu = 0u;
    for (uint32_t bit = 1u << (PBRS_PLANE_BITS - 1u); bit; bit >>= 1) {
        if (pbrs_plane_down(qd | bit, step, lo) <= R.min[k]) qd |= bit;
        if (pbrs_plane_up(qu | bit, step, hi) >= L.max[k]) qu |= bit;
    }
    if (!coord_ok(pbrs_plane_down(qd, step, lo))) qd = 0u;
    if (!coord_ok(pbrs_plane_up(qu, step, hi))) qu = 0u;
    return pbrs_plane_pack(qd, qu);
}

// Does every child box of the BLAS under `root` lie inside its parent's?  (device/entry_nodes.h; `nodes`: absolute links, children after
// their parent.)  A NaN coordinate fails every comparison.
bool blas_nested(const std::vector<pbrs_node>& nodes, uint32_t root) {
    std::vector<uint32_t> todo = {root};
    while (!todo.empty()) {
        const uint32_t x = todo.back();
        todo.pop_back();
        const pbrs_node& X = nodes[x];
        if (X.b & PBRS_LEAF_FLAG) continue;
        for (uint32_t c : {x + 1u, X.a}) {
            const pbrs_node& C = nodes[c];
            for (int a = 0; a < 3; ++a)
                if (!(X.min[a] <= C.min[a] && C.min[a] <= C.max[a] && C.max[a] <= X.max[a])) return false;
            todo.push_back(c);
        }
    }
    return true;
}

// The analytic instance that IS area light `L` (prepare_scene, PreparedScene::light_link): an instance of the light's shape kind whose shape parameters are the light's
// world-space ones bit for bit and whose two matrices are bit-exactly the identity — so that a sample on the light lies on the instance.
// What the kinds compare: a sphere's centre and radius, a disk's centre, normal and radial, a quad's origin and two sides.
bool is_light_instance(const pbrs_scene_desc& d, const pbrs_area_light& L, const pbrs_instance& in) {
    const uint32_t k = L.shape_kind;
    if (!(k == PBRS_SHAPE_SPHERE || k == PBRS_SHAPE_DISK || k == PBRS_SHAPE_QUAD) || in.shape_kind != k || in.shape_index >= d.n_shapes) return false;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            const uint32_t one = pn_bits(r == c ? 1.0f : 0.0f);
            if (pn_bits(in.inv[r][c]) != one || pn_bits(in.fwd[r][c]) != one) return false;
        }
    const float* p = d.shapes[in.shape_index].p;
    for (uint32_t j = 0, n = k == PBRS_SHAPE_SPHERE ? 4u : 9u; j < n; ++j)
        if (pn_bits(p[j]) != pn_bits(L.p[j])) return false;
    return true;
}

}  // namespace

// Host-side shape checks: every index the kernels dereference must be in range before any launch.
SceneCheck check_scene(const pbrs_scene_desc& d) {
    if (d.n_tlas_nodes == 0 || d.n_instances == 0) return refuse(PBRS_E_INVALID, "scene without instances");
    for (uint32_t i = 0; i < d.n_tlas_nodes; ++i) {
        const pbrs_node& n = d.tlas_nodes[i];
        if (n.b & PBRS_LEAF_FLAG) {
            if (n.a >= d.n_instances) return refuse(PBRS_E_INVALID, "tlas leaf references a missing instance");
        } else if (n.a >= d.n_tlas_nodes || i + 1 >= d.n_tlas_nodes) {
            return refuse(PBRS_E_INVALID, "tlas child out of range");
        } else if (n.a <= i) {
            return refuse(PBRS_E_INVALID, "tlas nodes are not in pre-order");
        }
    }
    for (uint32_t i = 0; i < d.n_blas_nodes; ++i) {
        const pbrs_node& n = d.blas_nodes[i];
        if (n.b & PBRS_LEAF_FLAG) {
            uint32_t cnt = n.b & ~PBRS_LEAF_FLAG;
            if ((uint64_t)n.a + cnt > d.n_triangles) return refuse(PBRS_E_INVALID, "blas leaf range out of range");
        } else if (n.a >= d.n_blas_nodes || i + 1 >= d.n_blas_nodes || (n.b & 3u) > 2u) {
            return refuse(PBRS_E_INVALID, "blas child out of range");
        } else if (n.a <= i) {
            return refuse(PBRS_E_INVALID, "blas nodes are not in pre-order");
        }
    }
    for (uint32_t i = 0; i < d.n_meshes; ++i)
        if (d.meshes[i].root >= d.n_blas_nodes) return refuse(PBRS_E_INVALID, "mesh root out of range");
    for (uint32_t i = 0; i < d.n_instances; ++i) {
        const pbrs_instance& in = d.instances[i];
        if (in.material >= d.n_materials) return refuse(PBRS_E_INVALID, "instance material out of range");
        if (in.shape_kind > PBRS_SHAPE_MESH) return refuse(PBRS_E_INVALID, "unknown shape kind");
        if (in.shape_kind == PBRS_SHAPE_MESH ? in.shape_index >= d.n_meshes : in.shape_index >= d.n_shapes)
            return refuse(PBRS_E_INVALID, "instance shape out of range");
        if (in.shape_kind == PBRS_SHAPE_MESH ? in.blas_root >= d.n_blas_nodes : (in.shape_kind == PBRS_SHAPE_TRIANGLE && in.blas_root >= d.n_triangles))
            return refuse(PBRS_E_INVALID, "instance blas_root out of range");
    }
    for (uint32_t i = 0; i < d.n_materials; ++i) {
        const pbrs_material& m = d.materials[i];
        if (m.n_bxdfs > PBRS_MAX_BXDFS || (uint64_t)m.first_bxdf + m.n_bxdfs > d.n_bxdfs) return refuse(PBRS_E_INVALID, "material lobes out of range");
        if (m.vis_bxdf > d.n_bxdfs) return refuse(PBRS_E_INVALID, "material visualiser record out of range");
    }
    for (uint32_t i = 0; i < d.n_bxdfs; ++i) {
        const uint32_t t = d.bxdfs[i].tex & ~PBRS_BXDF_TEX_DROP_IF_BLACK;
        if (t > d.n_textures) return refuse(PBRS_E_INVALID, "lobe texture out of range");
        if (d.bxdfs[i].kind > PBRS_BXDF_FOURIER) return refuse(PBRS_E_INVALID, "unknown lobe kind");
        if (d.bxdfs[i].kind == PBRS_BXDF_FOURIER && d.bxdfs[i].intrusion >= d.n_fourier_tables) return refuse(PBRS_E_INVALID, "Fourier lobe table out of range");
    }
    // Fourier tables (geometry/src/fourier.rs:99-151): every array inside the pools, every series inside the coefficients;
    // with finite, strictly ascending nodes the interpolation weights are finite for every direction the lobe accepts (a NaN
    // direction is refused there), and the lobe skips neighbours outside the table: no lane indexes outside the pools
    for (uint32_t i = 0; i < d.n_fourier_tables; ++i) {
        const pbrs_fourier_table& t = d.fourier_tables[i];
        const uint64_t n = t.n_mu, nn = n * n, nf = d.n_tex_floats, nw = d.n_tex_words;
        if (n < 3 || (t.n_channels != 1 && t.n_channels != 3)) return refuse(PBRS_E_INVALID, "Fourier table: sizes");
        if (t.mu + n > nf || t.cdf + nn > nf || t.a0 + nn > nf || (uint64_t)t.a + t.n_coeffs > nf || (uint64_t)t.recip + t.m_max > nf ||
            t.a_offset + nn > nw || t.m_lookup + nn > nw)
            return refuse(PBRS_E_INVALID, "Fourier table: arrays out of range");
        for (uint64_t k = 0; k < n; ++k) {  // finite, strictly ascending nodes: no interval of zero width, no NaN weight (device/fourier.h)
            const float m0 = d.tex_floats[t.mu + k];
            if (!pn_isfinite(m0) || (k + 1 < n && !(m0 < d.tex_floats[t.mu + k + 1]))) return refuse(PBRS_E_INVALID, "Fourier table: mu is not finite and strictly ascending");
        }
        for (uint64_t k = 0; k < nn; ++k) {
            const uint64_t off = d.tex_words[t.a_offset + k], len = d.tex_words[t.m_lookup + k];
            if (len > t.m_max || off + len * t.n_channels > t.n_coeffs) return refuse(PBRS_E_INVALID, "Fourier table: series out of range");
        }
    }
    for (uint32_t i = 0; i < d.n_textures; ++i) {
        const pbrs_texture& t = d.textures[i];
        if (t.kind == PBRS_TEX_PERLIN) {
            if ((uint64_t)t.data + 768 > d.n_tex_floats || (uint64_t)t.perm + 768 > d.n_tex_words) return refuse(PBRS_E_INVALID, "perlin tables out of range");
            for (uint32_t k = 0; k < 768; ++k)
                if (d.tex_words[t.perm + k] > 255u) return refuse(PBRS_E_INVALID, "perlin permutation entry above 255");
        } else if (t.kind == PBRS_TEX_IMAGE) {
            if (t.width == 0 || t.height == 0 || (uint64_t)t.data + 3ull * t.width * t.height > d.n_tex_floats)
                return refuse(PBRS_E_INVALID, "image texels out of range");
        } else if (t.kind != PBRS_TEX_CHECKER) {
            return refuse(PBRS_E_INVALID, "unknown texture kind");
        }
    }
    if (d.env_kind > PBRS_ENV_DUSK) return refuse(PBRS_E_INVALID, "unknown environment kind");
    if (d.env_kind == PBRS_ENV_IMAGE && (d.env_texture >= d.n_textures || d.textures[d.env_texture].kind != PBRS_TEX_IMAGE))
        return refuse(PBRS_E_INVALID, "environment map is not an image texture");
    for (uint32_t i = 0; i < d.n_area_lights; ++i) {
        uint32_t k = d.area_lights[i].shape_kind;
        if (!(k == PBRS_SHAPE_SPHERE || k == PBRS_SHAPE_DISK || k == PBRS_SHAPE_TRIANGLE || k == PBRS_SHAPE_QUAD))
            return refuse(PBRS_E_INVALID, "area light shape kind");
    }
    // The limits of the device code: a lane's stack rows in LDS, node indices and byte offsets in 32 bits
    const SceneLevels levels = scene_levels(d);
    if ((size_t)levels.stack * kBlock * sizeof(uint32_t) > kLdsBytesPerCU / 2) return refuse(PBRS_E_LIMIT, "traversal stack exceeds the LDS budget");
    uint64_t n_nodes = (uint64_t)d.n_tlas_nodes;  // DevScene::nodes up to the BLASes: the TLAS and its leaf copies
    if (tlas_scanned(d))
        for (uint32_t i = 0; i < d.n_tlas_nodes; ++i) n_nodes += (d.tlas_nodes[i].b & PBRS_LEAF_FLAG) ? 1u : 0u;
    if (n_nodes + d.n_blas_nodes > 0x7fffffffull) return refuse(PBRS_E_LIMIT, "too many BVH nodes");
    if ((n_nodes + d.n_blas_nodes) * sizeof(pbrs_node) >= (1ull << 32)) return refuse(PBRS_E_LIMIT, "too many BVH nodes (the walks address them with 32-bit byte offsets)");
    return SceneCheck{PBRS_OK, nullptr, levels};
}

PreparedScene prepare_scene(const pbrs_scene_desc& d, const SceneLevels& lv, const DevOverrides& dev) {
    PreparedScene P;
    DevScene& S = P.S;
    SceneFacts& f = P.facts;
    P.stack_depth = lv.stack;
    // The division-free box test (device/traverse.h) is exact when every node coordinate b is finite, |b| <= 2^40 and (b == 0 or
    // |b| >= 2^-60) — the range of a ray's origin components (origin_in_range); otherwise every lane uses the literal divisions.
    // With o and b both zero or at least 2^-60 the numerator RN(o - b) is zero or at least 2^-83, its first quotient q0 = nn nr at least
    // 2^-123 (normal: rounded at full precision), the residual e = d q0 + nn a multiple of 2^-131 (exact, if subnormal: the kernels run
    // with f32 denormals on, .amdhsa_float_denorm_mode_32 3) and the result normal: the three instructions return RN(n / d) as they
    // do at any other scale (tools/microbench/div_exhaustive.hip).  Rounds 1-3 asked 2^-20 of the box coordinates — a bound of the
    // f64 route of rounds 1-2 that the f32 quotient inherited: c4xl's 8.4 M vertices hold three heights below it (1.6e-7, 7.4e-7,
    // -9.8e-8), and the WHOLE scene walked on the literal divisions, its lean node steps sitting idle (round 3's "-11 % out of cache").
    {
        bool ok = true;
        for (uint32_t i = 0; i < d.n_tlas_nodes && ok; ++i)
            for (int a = 0; a < 3; ++a) ok = ok && coord_ok(d.tlas_nodes[i].min[a]) && coord_ok(d.tlas_nodes[i].max[a]);
        for (uint32_t i = 0; i < d.n_blas_nodes && ok; ++i)
            for (int a = 0; a < 3; ++a) ok = ok && coord_ok(d.blas_nodes[i].min[a]) && coord_ok(d.blas_nodes[i].max[a]);
        S.fast_slab = ok ? 1u : 0u;
    }
    S.exact_extent = lv.exact_extent ? 1u : 0u;

    // DevScene::nodes: the TLAS, then its leaves alone in pre-order when the TLAS is small (the shared scan), then every
    // BLAS, in one array with absolute links — a walk reads nodes + index whatever tree it is in.
    const bool scan = tlas_scanned(d);
    std::vector<pbrs_node>& nodes = P.nodes;
    nodes.assign(d.tlas_nodes, d.tlas_nodes + d.n_tlas_nodes);
    S.flat_off = (uint32_t)nodes.size();
    if (scan)
        for (uint32_t i = 0; i < d.n_tlas_nodes; ++i)
            if (d.tlas_nodes[i].b & PBRS_LEAF_FLAG) nodes.push_back(d.tlas_nodes[i]);
    S.n_flat = (uint32_t)nodes.size() - S.flat_off;
    const uint64_t blas_off = nodes.size();
    nodes.insert(nodes.end(), d.blas_nodes, d.blas_nodes + d.n_blas_nodes);
    for (size_t i = blas_off; i < nodes.size(); ++i)
        if (!(nodes[i].b & PBRS_LEAF_FLAG)) nodes[i].a += (uint32_t)blas_off;  // right child; the left one is i + 1
    // The split planes of the inner BLAS nodes (device/split_planes.h), one word per node of `nodes`: pbrs_upload_scene ORs them into
    // the b words of the copy it uploads; `nodes` itself stays the description's.  Only rays on the division-free box test read them.
    P.node_planes.assign(nodes.size(), 0u);
    if (S.fast_slab != 0u)
        for (size_t i = blas_off; i < nodes.size(); ++i)
            if (!(nodes[i].b & PBRS_LEAF_FLAG)) P.node_planes[i] = split_planes(nodes, (uint32_t)i);
    P.walk_bytes = nodes.size() * sizeof(pbrs_node) + (uint64_t)d.n_triangles * sizeof(pbrs_tri_verts) + (uint64_t)d.n_instances * sizeof(pbrs_instance);

    std::vector<pbrs_instance>& inst = P.inst;
    inst.assign(d.instances, d.instances + d.n_instances);
    // Shading classes: one per distinct lobe signature among the materials (class 0: no lobes — emitters — and misses)
    std::vector<uint32_t> mat_class(d.n_materials, 0u);
    {
        std::vector<std::string> sigs;
        for (uint32_t m = 0; m < d.n_materials; ++m) {
            const pbrs_material& mt = d.materials[m];
            if (mt.n_bxdfs == 0) continue;
            std::string sig;
            for (uint32_t k = 0; k < mt.n_bxdfs; ++k) {
                const pbrs_bxdf& bx = d.bxdfs[mt.first_bxdf + k];
                sig += (char)('a' + bx.kind);
                sig += (char)('a' + (bx.kind == PBRS_BXDF_SPECULAR ? bx.intrusion : 0u));
                sig += (char)('a' + (bx.kind == PBRS_BXDF_DIFFUSE ? bx.oren_nayar : bx.fresnel));
                sig += (char)('a' + (bx.kind == PBRS_BXDF_MICROFACET && bx.alpha_x != bx.alpha_y ? 1 : 0));
                sig += bx.tex ? 't' : '-';
            }
            size_t at = 0;
            while (at < sigs.size() && sigs[at] != sig) ++at;
            if (at == sigs.size()) sigs.push_back(sig);
            mat_class[m] = (uint32_t)std::min<size_t>(at + 1, PBRS_MAX_CLASSES - 1);
        }
        S.n_classes = (uint32_t)std::min<size_t>(sigs.size(), PBRS_MAX_CLASSES - 1);
        // the class of the materials that are one untextured Lambertian DiffuseReflect (signature: kind 1, not Oren-Nayar)
        const std::string lam_sig = {(char)('a' + PBRS_BXDF_DIFFUSE), 'a', 'a', 'a', '-'};
        for (size_t at = 0; at < sigs.size() && at + 1 < PBRS_MAX_CLASSES - 1; ++at)
            if (sigs[at] == lam_sig) f.lambert_class = (uint32_t)at + 1;
        // ... and of the materials that are one Fourier BSDF (material/src/lib.rs:451-475: whatever their tables, one signature)
        const std::string fou_sig = {(char)('a' + PBRS_BXDF_FOURIER), 'a', 'a', 'a', '-'};
        for (size_t at = 0; at < sigs.size() && at + 1 < PBRS_MAX_CLASSES - 1; ++at)
            if (sigs[at] == fou_sig) f.fourier_class = (uint32_t)at + 1;
    }
    for (pbrs_instance& in : inst) {
        in.pad[0] = mat_class[in.material];
        if (in.shape_kind == PBRS_SHAPE_MESH) in.blas_root += (uint32_t)blas_off;
        bool linear_identity = true;  // bit patterns: -0.0 would not do
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) linear_identity = linear_identity && pn_bits(in.inv[r][k]) == pn_bits(r == k ? 1.0f : 0.0f);
        in.flags &= ~PBRS_INSTANCE_TRANSLATION;
        if (linear_identity) in.flags |= PBRS_INSTANCE_TRANSLATION;
    }
    // Four-wide nodes over every BLAS a mesh instance enters (device/wide.h): pad[1] of the device copy of the instance is
    // the wide node of its root, PBRS_WREF_NONE where the mesh is a single leaf.  Built and uploaded only for scenes whose
    // k_shadow can walk them: a scanned TLAS and coordinates inside the guarded range of the division-free box test (the
    // deciding PBRS_WIDE_MIN_LEVELS is known once they are built).  A wide array of 4 GiB or more (32-bit byte offsets) is not
    // an error: the scene keeps the binary walks.  Nor is a node array of more than 2^26 nodes, in which a leaf's index would reach the
    // bit that marks a reference carrying its triangles (PBRS_WREF_PACKED, pack_wide_leaves).
    for (pbrs_instance& in : inst) in.pad[1] = PBRS_WREF_NONE;
    S.wide_cap = 4u;
    if (scan && S.fast_slab != 0u) {
        std::vector<pbrs_wnode>& wide = P.wide;
        std::map<uint32_t, uint32_t> wide_of_root;
        uint32_t levels = 0;
        for (pbrs_instance& in : inst) {
            if (in.shape_kind != PBRS_SHAPE_MESH || (nodes[in.blas_root].b & PBRS_LEAF_FLAG)) continue;
            auto it = wide_of_root.find(in.blas_root);
            if (it == wide_of_root.end()) it = wide_of_root.emplace(in.blas_root, build_wide(nodes, in.blas_root, wide, 0u, levels)).first;
            in.pad[1] = it->second;
        }
        if (levels >= PBRS_WIDE_MIN_LEVELS && wide.size() * sizeof(pbrs_wnode) < (1ull << 32) && nodes.size() <= PBRS_WREF_PACKED) {
            P.walk_bytes += wide.size() * sizeof(pbrs_wnode);
            // DevScene::tri_leaf: the BLAS leaf that holds each triangle record (0xffffffff: none — an IsolatedTriangle's record)
            P.tri_leaf.assign(d.n_triangles, 0xffffffffu);
            for (size_t i = blas_off; i < nodes.size(); ++i)
                if (nodes[i].b & PBRS_LEAF_FLAG)
                    for (uint32_t t = nodes[i].a, end = t + (nodes[i].b & ~PBRS_LEAF_FLAG); t < end; ++t) P.tri_leaf[t] = (uint32_t)i;  // (in range: check_scene)
            P.walk_bytes += P.tri_leaf.size() * sizeof(uint32_t);
            S.n_wnodes = (uint32_t)wide.size();
            // a node step pushes up to three survivors per level; deeper stacks than PBRS_WIDE_STACK_MAX entries are not given LDS:
            // a ray that would need one (none on the BASELINE scenes) is traced by the binary-walk kernel instead
            S.wide_cap = std::max(4u, std::min(3u * levels + 1u, (uint32_t)PBRS_WIDE_STACK_MAX));
            P.wide_levels = levels;
        } else {
            wide.clear();  // (and no tri_leaf)
            for (pbrs_instance& in : inst) in.pad[1] = PBRS_WREF_NONE;
        }
    }

    S.n_area = d.n_area_lights;
    S.n_delta = d.n_delta_lights;
    S.env_kind = d.env_kind;
    S.env_texture = d.env_texture;
    std::memcpy(S.env_scale, d.env_scale, sizeof S.env_scale);
    std::memcpy(S.env, d.env_constant, sizeof S.env);
    // Scene::has_env_light for EnvLight::Constant (scene/src/lib.rs:96-102): !c.is_black()
    S.has_env = (d.env_kind != PBRS_ENV_CONSTANT || !(S.env[0] <= 0.0f && S.env[1] <= 0.0f && S.env[2] <= 0.0f)) ? 1u : 0u;
    S.refill_below = lv.max_blas >= PBRS_LONG_WALK_HEIGHT ? PBRS_REFILL_BELOW_LONG : PBRS_REFILL_BELOW_SHORT;
    S.refill_below_shadow = lv.max_blas >= PBRS_LONG_WALK_HEIGHT ? PBRS_REFILL_BELOW_LONG_SHADOW : PBRS_REFILL_BELOW_SHORT;
    if (dev.refill_below) S.refill_below = S.refill_below_shadow = *dev.refill_below;
    // long walks: the levels a ray actually walks — the deepest BLAS, plus the TLAS where it is not scanned
    f.long_walks = (S.n_flat ? 0u : lv.tlas) + lv.max_blas >= PBRS_LONG_WALK_HEIGHT;
    // lean further node steps for rays on the division-free box test; a scene whose coordinates leave its guarded range walks every
    // ray on the literal divisions, which the lean steps do not carry: full steps (kernels.h)
    f.full_steps = S.fast_slab == 0u;
    // the leaf copies serve k_shadow up to PBRS_FLAT_TLAS_MAX_ANYHIT instances, k_extend up to PBRS_FLAT_TLAS_MAX
    f.tlas_scanned = S.n_flat != 0u;
    S.features = (S.n_flat != 0u && d.n_instances <= PBRS_FLAT_TLAS_MAX) ? PBRS_FEAT_FLAT_TLAS : 0u;
    // the walks over four-wide nodes: scenes whose TLAS the stage scans and whose coordinates admit the division-free box test
    // ... and that have a BLAS deep enough for it to matter (PBRS_WIDE_MIN_LEVELS wide nodes on the way down: meshes of a few
    // triangles are a leaf or two, where the binary walks at their six waves per SIMD are faster — C2: 105 against 140 ms)
    // k_shadow gains (C4: 250 -> 236 ms per frame at five waves per SIMD); k_extend keeps the binary walk (a four-wide closest-hit
    // walk needed 117 registers, four waves per SIMD, and lost against the binary walk at six: 459 -> 506 ms)
    f.wide_ok = S.fast_slab != 0u && P.wide_levels >= PBRS_WIDE_MIN_LEVELS;
    for (uint32_t i = 0; i < d.n_instances; ++i) {
        const pbrs_instance& in = d.instances[i];
        if (in.shape_kind == PBRS_SHAPE_MESH) {
            if (!(in.mesh_flags & PBRS_MESH_SHADING_OK_MASK)) S.features |= PBRS_FEAT_SHADING_CHECK;
        } else if (in.shape_kind != PBRS_SHAPE_TRIANGLE) {  // isolated triangles go through the triangle-record path
            S.features |= PBRS_FEAT_ANALYTIC;
        }
    }
    // Entry nodes of the camera rays (device/entry_nodes.h): at most one instance per scene gets a table — the mesh instance with the
    // deepest BLAS (the first of equals), if that BLAS has PBRS_LONG_WALK_HEIGHT levels or more, the instance is the identity or a pure
    // translation, the scene lies inside the guarded range of the division-free box test, and EVERY child box of that BLAS lies inside
    // its parent's (the argument rests on the nesting of whole subtrees; split_planes asks it node by node and only gives up its planes).
    S.entry_inst = PBRS_ENTRY_NONE;
    if (S.fast_slab != 0u && !lv.exact_extent) {
        std::vector<uint32_t> h;
        tree_heights(nodes.data(), (uint32_t)nodes.size(), h);
        uint32_t best = PBRS_ENTRY_NONE;
        for (uint32_t i = 0; i < d.n_instances; ++i)
            if (inst[i].shape_kind == PBRS_SHAPE_MESH && (best == PBRS_ENTRY_NONE || h[inst[i].blas_root] > h[inst[best].blas_root])) best = i;
        // (PBRS_INSTANCE_TRANSLATION: set above from the matrix's own bits, the identity included)
        if (best != PBRS_ENTRY_NONE && h[inst[best].blas_root] >= PBRS_LONG_WALK_HEIGHT && (inst[best].flags & PBRS_INSTANCE_TRANSLATION) &&
            blas_nested(nodes, inst[best].blas_root)) {
            S.entry_inst = best;
            P.entry_height = h[inst[best].blas_root];
            P.entry_rows = lv.stack - (lv.tlas - 1u);
        }
    }
    f.entry_nodes = S.entry_inst != PBRS_ENTRY_NONE;
    f.features = S.features;
    f.exact_extent = lv.exact_extent;
    f.n_classes = S.n_classes;
    P.has_vis_records = d.n_materials > 0;
    for (uint32_t i = 0; i < d.n_materials; ++i) P.has_vis_records = P.has_vis_records && d.materials[i].vis_bxdf != 0;
    for (uint32_t i = 0; i < d.n_bxdfs; ++i) {
        f.textured = f.textured || (d.bxdfs[i].tex & ~PBRS_BXDF_TEX_DROP_IF_BLACK) != 0;
        f.fourier = f.fourier || d.bxdfs[i].kind == PBRS_BXDF_FOURIER;
    }
    // k_shade specialisation: every lobe an untextured Lambertian DiffuseReflect (at most one per material); every area light
    // of one shape
    f.lambert = !f.textured;
    for (uint32_t i = 0; i < d.n_materials && f.lambert; ++i) {
        const pbrs_material& m = d.materials[i];  // its lobes only: the array also holds the visualisers' records
        f.lambert = m.n_bxdfs <= 1;
        for (uint32_t k = 0; k < m.n_bxdfs && f.lambert; ++k) {
            const pbrs_bxdf& bx = d.bxdfs[m.first_bxdf + k];
            f.lambert = bx.kind == PBRS_BXDF_DIFFUSE && bx.oren_nayar == 0 && bx.tex == 0;
        }
    }
    if (d.n_area_lights) {
        const uint32_t k0 = d.area_lights[0].shape_kind;
        bool same = true;
        for (uint32_t i = 1; i < d.n_area_lights; ++i) same = same && d.area_lights[i].shape_kind == k0;
        if (same && k0 == PBRS_SHAPE_SPHERE) f.light_spec = PBRS_SHADE_LIGHT_SPHERE;
        if (same && k0 == PBRS_SHAPE_TRIANGLE) f.light_spec = PBRS_SHADE_LIGHT_TRIANGLE;
    }
    // The light a shadow ray is aimed at (device/scene.h, PBRS_SKIP_*): per area light, the first instance that is the light itself, and
    // that instance's leaf among the leaf copies where k_shadow scans them.  Which instance a light is linked to only decides where
    // the saving lies: k_shade tags a ray only where the linked instance's own test is false for it (device/shade.h, light_skip_tag).
    P.light_link.assign(d.n_area_lights, 0u);
    for (uint32_t l = 0; l < d.n_area_lights; ++l)
        for (uint32_t i = 0; i < d.n_instances && i + 1u <= PBRS_SKIP_INST_MASK; ++i) {
            if (!is_light_instance(d, d.area_lights[l], d.instances[i])) continue;
            uint32_t leaf = 0u;
            for (uint32_t k = S.n_flat; k-- > 0u;)
                if (nodes[S.flat_off + k].a == i) leaf = k + 1u;
            P.light_link[l] = (i + 1u) | leaf << PBRS_SKIP_FLAT_SHIFT;
            break;
        }
    // what the traversal kernels may stage in LDS next to the stack rows (choose_kernels)
    f.stack_bytes = (size_t)lv.stack * kBlock * sizeof(uint32_t);
    f.wide_stack_bytes = (size_t)S.wide_cap * kBlock * sizeof(uint32_t);
    f.scene_bytes = nodes.size() * sizeof(pbrs_node) + (size_t)d.n_triangles * sizeof(pbrs_tri_verts) + (size_t)d.n_instances * sizeof(pbrs_instance) +
                    (size_t)d.n_shapes * sizeof(pbrs_shape);
    f.top_bytes = (size_t)d.n_tlas_nodes * sizeof(pbrs_node);
    // k_shade: the shading records (instances, shapes, materials, lobes, lights) in LDS where they are a few KB, the triangle records
    // too where everything is (kernels.h, stage_shade_scene); five blocks of the Lambert variants share a CU's 160 KB with the rest
    S.n_inst = d.n_instances; S.n_shapes = d.n_shapes; S.n_tris = d.n_triangles; S.n_mats = d.n_materials; S.n_bxdfs = d.n_bxdfs;
    f.shade_rec_bytes = (size_t)d.n_instances * sizeof(pbrs_instance) + (size_t)d.n_shapes * sizeof(pbrs_shape) + (size_t)d.n_materials * sizeof(pbrs_material) +
                        (size_t)d.n_bxdfs * sizeof(pbrs_bxdf) + (size_t)d.n_area_lights * sizeof(pbrs_area_light) + (size_t)d.n_delta_lights * sizeof(pbrs_delta_light);
    f.shade_tri_bytes = (size_t)d.n_triangles * (sizeof(pbrs_tri_verts) + sizeof(pbrs_tri_shade));
    const size_t budget = 16u << 10;
    f.shade_lds = f.shade_rec_bytes + f.shade_tri_bytes <= budget ? PBRS_SHADE_LDS_ALL : f.shade_rec_bytes <= budget ? PBRS_SHADE_LDS_RECORDS : 0u;
    return P;
}

// Leaf references that carry their triangles (device/scene.h, PBRS_WREF_PACKED), on the wide nodes as they are uploaded — like the split
// planes, which ride on the uploaded copy of the nodes.  A leaf keeps the node form unless it has one to four triangles, the first of them
// below 2^24, and tri_leaf leads from each of them back to it (a description whose leaves share a triangle record: the table names one leaf
// only).  No reference of the node form has the flag bit set: prepare_scene builds wide nodes only over node arrays of at most 2^26 nodes.
uint32_t pack_wide_leaves(PreparedScene& P) {
    uint32_t packed = 0;
    for (pbrs_wnode& w : P.wide)
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t ref = w.child[k];
            if (ref == PBRS_WREF_NONE || !(ref & PBRS_WREF_LEAF)) continue;
            const uint32_t ni = ref & PBRS_WREF_INDEX;
            const pbrs_node& n = P.nodes[ni];
            const uint32_t cnt = n.b & ~PBRS_LEAF_FLAG;
            if (cnt == 0u || cnt > PBRS_WREF_COUNT_MAX || n.a > PBRS_WREF_TRI) continue;
            bool own = true;
            for (uint32_t j = 0; j < cnt; ++j) own = own && P.tri_leaf[n.a + j] == ni;
            if (!own) continue;
            w.child[k] = (ref & ~PBRS_WREF_INDEX) | PBRS_WREF_PACKED | (cnt - 1u) << PBRS_WREF_COUNT_SHIFT | n.a;
            ++packed;
        }
    return packed;
}

// What pbrs_upload_scene does to its copy of the area lights: the links ride in the records' two padding words, as bit patterns
// (pad[0]: instance + 1, pad[1]: flat leaf + 1; 0: none).  The description's own records are not written.
void write_light_links(const PreparedScene& P, std::vector<pbrs_area_light>& lights) {
    for (size_t l = 0; l < lights.size() && l < P.light_link.size(); ++l) {
        const uint32_t inst = P.light_link[l] & PBRS_SKIP_INST_MASK, leaf = P.light_link[l] >> PBRS_SKIP_FLAT_SHIFT;
        std::memcpy(&lights[l].pad[0], &inst, sizeof inst);
        std::memcpy(&lights[l].pad[1], &leaf, sizeof leaf);
    }
}

}  // namespace pbrs
