// host/kernel_choice.cpp — choose_kernels (host/kernel_choice.h): plain C++, linked into libpbrs_gpu.so and into the CPU check of
// tests/scene_prepare_check.cpp.
#include "kernel_choice.h"

#include <algorithm>

namespace pbrs {

KernelChoice choose_kernels(const SceneFacts& f, const DevOverrides& dev) {
    KernelChoice p;
    const bool long_walks = dev.long_walks.value_or(f.long_walks);
    const bool full_steps = dev.full_steps.value_or(f.full_steps);
    const uint32_t steps = long_walks ? PBRS_FEAT_LONG_WALKS | (full_steps ? PBRS_FEAT_FULL_STEPS : 0u) : 0u;
    p.wide_shadow = f.tlas_scanned && f.wide_ok && dev.wide_shadow;
    // The arrays the walks read, staged in every block's LDS (kernels.h, stage_scene) where they fit next to the stack rows with
    // eight blocks to a CU: scenes of a few KB whose walks are short (no wide nodes, lean-step choice irrelevant) ...
    const bool lds_scene = dev.lds_scene && !p.wide_shadow && !full_steps && f.stack_bytes + f.scene_bytes <= kLdsBytesPerCU / 8;
    // ... or the TLAS alone, where it is too large for the wave's shared scan (no leaf copies) and fits with seven blocks to a CU
    const bool lds_top = dev.lds_top && !lds_scene && !f.tlas_scanned && !full_steps && f.stack_bytes + f.top_bytes + 512 <= kLdsBytesPerCU / 7;
    p.lds_staging = lds_scene ? PBRS_FEAT_LDS_SCENE : lds_top ? PBRS_FEAT_LDS_TOP : 0u;
    const size_t stack = std::max(f.stack_bytes, dev.lds_min);
    const size_t staged = stack + (lds_scene ? f.scene_bytes : lds_top ? f.top_bytes : 0u);
    if (f.exact_extent) {  // (scenes with a ParallelQuad next to a mesh: no benchmark holds one)
        p.extend[0] = {kExtentFeatures, stack};
        p.extend[1] = {kStatsKey | kExtentFeatures, stack};
    } else {
        p.extend[0] = {(f.features & PBRS_FEAT_ALL) | steps | p.lds_staging, staged};
        p.extend[1] = {kStatsKey | PBRS_FEAT_ALL, stack};
    }
    p.entry_extend = f.entry_nodes && extend_entry_ok(p.extend[0].key);
    const uint32_t shadow_feat = (f.features & PBRS_FEAT_ANALYTIC) | (f.tlas_scanned ? PBRS_FEAT_FLAT_TLAS : 0u) | steps;
    if (p.wide_shadow) {
        p.shadow[0] = {shadow_feat | PBRS_FEAT_WIDE, f.wide_stack_bytes};
        p.shadow_slow = {shadow_feat, stack};
    } else {
        p.shadow[0] = {shadow_feat | p.lds_staging, staged};
    }
    p.shadow[1] = {kStatsKey | kShadowStatsFeatures, stack};
    p.split_queue = f.n_classes <= 1u && dev.split_queue;

    // k_shade.  The path integrator's untextured variants stage the scene's shading records (and triangle records) in LDS where they fit,
    // and leave out what the scene's materials and lights do not need (the light shape alone does not pay: without the Lambert cut the
    // kernel grows to 135-141 VGPRs, three waves per SIMD; C2 shade 110.5 -> 117.0 ms, C4 150.6 -> 169.3)
    const uint32_t shade_lds = f.shade_lds & dev.shade_lds;
    const uint32_t path_lds = (shade_lds == PBRS_SHADE_LDS_ALL || shade_lds == PBRS_SHADE_LDS_RECORDS) ? shade_lds : 0u;
    const size_t path_lds_bytes = path_lds == PBRS_SHADE_LDS_ALL ? f.shade_rec_bytes + f.shade_tri_bytes : path_lds ? f.shade_rec_bytes : 0u;
    uint32_t spec = f.lambert ? (PBRS_SHADE_LAMBERT | f.light_spec) & dev.shade_spec : 0u;
    if (!(spec & PBRS_SHADE_LAMBERT)) spec = 0u;
    auto shade = [](IntegratorChoice& ip, uint32_t integ, bool tex, uint32_t sp, size_t lds, uint32_t range) {
        ip.shade[ip.n_shade++] = ShadeKey{integ, tex, sp, lds, range};
    };
    auto path_untextured = [&](IntegratorChoice& ip, uint32_t sp, uint32_t range) { shade(ip, PBRS_INTEGRATOR_PATH, false, sp | path_lds, path_lds_bytes, range); };
    // several shading classes (and an integrator that shades): the queue is ordered by class first; counted as shade time
    const bool sorted = f.n_classes > 1u && dev.sort_classes;
    for (uint32_t i = PBRS_INTEGRATOR_PATH; i <= PBRS_INTEGRATOR_DIRECT; ++i) {
        IntegratorChoice& ip = p.integ[i];
        const bool path = i == PBRS_INTEGRATOR_PATH;
        // ... and where one of the classes is Lambertian (and the integrator has a Lambert variant), class-major over the whole
        // queue, so that the class gets a launch of that variant and the other classes one of the general kernel
        const bool split = sorted && path && f.lambert_class && dev.split_lambert && !f.textured && !f.fourier;
        // ... or a Fourier BSDF: its lobe's code (168 registers and scratch in k_shade's variants that carry it) then runs over
        // the vertices on such a material only, the other classes take the kernels without it
        const bool fsplit = sorted && f.fourier && f.fourier_class && dev.split_fourier;
        ip.order = (split || fsplit) ? IntegratorChoice::CLASS_MAJOR : sorted ? IntegratorChoice::CLASS_SORT : IntegratorChoice::NO_ORDER;
        ip.last_class = split ? f.lambert_class : fsplit ? f.fourier_class : 0u;
        if (fsplit) {  // (one untextured Fourier lobe per material: the variant cut down to it)
            shade(ip, i, false, PBRS_SHADE_FOURIER_ALONE, 0, f.fourier_class);
            shade(ip, i, f.textured, 0u, 0, PBRS_MAX_CLASSES);
        } else if (f.fourier && f.fourier_class && f.n_classes == 1u) {  // every material with lobes is a Fourier BSDF
            shade(ip, i, false, PBRS_SHADE_FOURIER_ALONE, 0, 0u);
        } else if (f.fourier) {  // some material is a Fourier BSDF: the kernels that carry the lobe (and textures)
            shade(ip, i, true, PBRS_SHADE_FOURIER, 0, 0u);
        } else if (f.textured) {  // some material evaluates a non-Solid texture per hit
            shade(ip, i, true, 0u, 0, 0u);
        } else if (!path) {
            shade(ip, i, false, 0u, 0, 0u);
        } else if (split) {
            path_untextured(ip, PBRS_SHADE_LAMBERT | f.light_spec, f.lambert_class);
            path_untextured(ip, 0u, PBRS_MAX_CLASSES);
        } else {
            path_untextured(ip, spec, 0u);
        }
    }
    shade(p.integ[PBRS_INTEGRATOR_MATERIALS], PBRS_INTEGRATOR_MATERIALS, false, 0u, 0, 0u);
    shade(p.integ[PBRS_INTEGRATOR_NORMALS], PBRS_INTEGRATOR_NORMALS, false, 0u, 0, 0u);
    return p;
}

}  // namespace pbrs
