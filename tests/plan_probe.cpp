// tests/plan_probe.cpp — what pbrs_upload_scene would plan for a scene, asked on a CPU: check_scene, prepare_scene and choose_kernels
// (pbrs_amd/csrc/host/), the library's own sources, behind three extern "C" functions that tests/plan_probe.py compiles with g++ and
// loads with ctypes.  Default DevOverrides throughout: what the shipped library runs with.
//
//   plan_probe_scene      the SceneFacts and the KernelChoice of a descriptor, as two arrays of 64-bit words (orders: plan_probe.py)
//   plan_probe_shade_keys the k_shade instantiations, expanded from PBRS_SHADE_KERNELS
//   plan_probe_reachable  the traversal keys choose_kernels yields over the fact combinations of kernel_choice_sweep.h
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../pbrs_amd/csrc/host/scene_prepare.h"
#include "kernel_choice_sweep.h"

using namespace pbrs;

namespace {

// The lobe signature of a material, restated (prepare_scene keeps its own): two materials shade alike where these agree.
std::string signature(const pbrs_scene_desc& d, uint32_t m) {
    std::string s;
    for (uint32_t k = 0; k < d.materials[m].n_bxdfs; ++k) {
        const pbrs_bxdf& b = d.bxdfs[d.materials[m].first_bxdf + k];
        const uint32_t w[5] = {b.kind, b.kind == PBRS_BXDF_SPECULAR ? b.intrusion : 0u, b.kind == PBRS_BXDF_DIFFUSE ? b.oren_nayar : b.fresnel,
                               (b.kind == PBRS_BXDF_MICROFACET && b.alpha_x != b.alpha_y) ? 1u : 0u, b.tex != 0u ? 1u : 0u};
        for (uint32_t x : w) s += std::to_string(x) + ",";
        s += ";";
    }
    return s;
}
bool single_lobe(const pbrs_scene_desc& d, uint32_t m, uint32_t kind) {
    if (d.materials[m].n_bxdfs != 1u) return false;
    const pbrs_bxdf& b = d.bxdfs[d.materials[m].first_bxdf];
    return b.kind == kind && b.tex == 0u && (kind != PBRS_BXDF_DIFFUSE || b.oren_nayar == 0u);
}

}  // namespace

extern "C" {

// facts[32], choice[80]: see FACTS and the layout of `choice` in plan_probe.py.  Returns check_scene's code (0: accepted; the arrays are
// filled only then).
int plan_probe_scene(const pbrs_scene_desc* d, uint64_t* facts, uint64_t* choice) {
    const SceneCheck chk = check_scene(*d);
    if (chk.code != PBRS_OK) return chk.code;
    const PreparedScene P = prepare_scene(*d, chk.levels, DevOverrides{});
    const SceneFacts& f = P.facts;
    // signatures in material order, as the classes are numbered: count, the positions (1-based) of the Lambert and the Fourier signature,
    // and how many different signatures the instances' materials bring to the overflow class
    std::vector<std::string> sigs;
    uint64_t lambert_at = 0, fourier_at = 0;
    std::set<std::string> overflow;
    std::vector<size_t> at_of(d->n_materials, 0);
    for (uint32_t m = 0; m < d->n_materials; ++m) {
        if (d->materials[m].n_bxdfs == 0u) continue;
        const std::string s = signature(*d, m);
        size_t at = std::find(sigs.begin(), sigs.end(), s) - sigs.begin();
        if (at == sigs.size()) sigs.push_back(s);
        at_of[m] = at + 1;
        if (single_lobe(*d, m, PBRS_BXDF_DIFFUSE)) lambert_at = at + 1;
        if (single_lobe(*d, m, PBRS_BXDF_FOURIER)) fourier_at = at + 1;
    }
    for (uint32_t i = 0; i < d->n_instances; ++i) {
        const uint32_t m = d->instances[i].material;
        if (at_of[m] >= PBRS_MAX_CLASSES - 1u) overflow.insert(signature(*d, m));
    }
    uint32_t max_class = 0;
    for (const pbrs_instance& in : P.inst) max_class = std::max(max_class, in.pad[0]);
    const uint64_t fv[] = {f.features, f.tlas_scanned, f.exact_extent, f.long_walks, f.full_steps, f.wide_ok, f.stack_bytes, f.wide_stack_bytes, f.scene_bytes,
                           f.top_bytes, f.n_classes, f.lambert_class, f.fourier_class, f.textured, f.fourier, f.lambert, f.light_spec, f.shade_lds,
                           f.shade_rec_bytes, f.shade_tri_bytes,
                           // beyond SceneFacts: the levels, and the signatures restated above
                           chk.levels.tlas, chk.levels.max_blas, chk.levels.stack, P.wide_levels, sigs.size(), lambert_at, fourier_at, overflow.size(), max_class,
                           d->n_instances, d->n_triangles, d->n_materials};
    static_assert(sizeof fv / sizeof fv[0] == 32, "facts[32]");
    std::memcpy(facts, fv, sizeof fv);

    const KernelChoice c = choose_kernels(f, DevOverrides{});
    uint64_t* o = choice;
    for (const TraversalKey* k : {&c.extend[0], &c.extend[1], &c.shadow[0], &c.shadow[1], &c.shadow_slow}) *o++ = k->key, *o++ = k->lds;
    *o++ = c.wide_shadow, *o++ = c.split_queue, *o++ = c.lds_staging;
    for (const IntegratorChoice& ic : c.integ) {
        *o++ = ic.order, *o++ = ic.last_class, *o++ = ic.n_shade;
        for (const ShadeKey& s : ic.shade) *o++ = s.integ, *o++ = s.tex, *o++ = s.spec, *o++ = s.lds, *o++ = s.range;
    }
    return (o - choice) == 13 + 4 * 13 ? PBRS_OK : -1;
}

// out[3 * i ..]: integrator, textured, spec.  Returns the number of instantiations (writes at most `cap` of them).
uint32_t plan_probe_shade_keys(uint32_t* out, uint32_t cap) {
#define SHADE_KEY(I, T, SP) {(uint32_t)(I), (uint32_t)(T), (uint32_t)(SP)},
    const uint32_t keys[][3] = {PBRS_SHADE_KERNELS(SHADE_KEY)};
#undef SHADE_KEY
    const uint32_t n = sizeof keys / sizeof keys[0];
    for (uint32_t i = 0; i < n && i < cap; ++i) std::memcpy(out + 3 * i, keys[i], sizeof keys[i]);
    return n;
}

// out[2 * i ..]: table (0 k_extend, 1 k_shadow, 2 k_shadow's slow list), key — of the shipped (not instrumented) kernels, sorted.
// Returns their number (writes at most `cap` of them).
uint32_t plan_probe_reachable(uint32_t* out, uint32_t cap) {
    std::set<std::pair<uint32_t, uint32_t>> keys;
    sweep_scene_facts([&](const SceneFacts& f) {
        const KernelChoice c = choose_kernels(f, DevOverrides{});
        keys.insert({0u, c.extend[0].key});
        keys.insert({1u, c.shadow[0].key});
        if (c.wide_shadow) keys.insert({2u, c.shadow_slow.key});
    });
    uint32_t i = 0;
    for (const auto& k : keys) {
        if (i < cap) out[2 * i] = k.first, out[2 * i + 1] = k.second;
        ++i;
    }
    return i;
}

}  // extern "C"
