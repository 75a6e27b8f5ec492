// tests/kernel_choice_sweep.h — every combination of SceneFacts prepare_scene can produce, for the CPU checks that walk them:
// tests/scene_prepare_check.cpp (every choice names an instantiated kernel) and tests/plan_probe.cpp (the traversal keys a scene can be
// given).  What makes a combination producible:
//   PBRS_FEAT_FLAT_TLAS => the TLAS is scanned           (k_extend scans up to 20 instances, k_shadow up to 32)
//   wide_ok => scanned and not full_steps                (wide nodes are built for a scanned TLAS inside the guarded range)
//   lambert => neither textured nor Fourier              (every lobe an untextured Lambertian)
//   fourier_class => fourier; a class index => that many classes; the two classes differ
// Byte sizes: a stack of 4 KB with scene and TLAS sizes on both sides of the two staging budgets (kLdsBytesPerCU / 8 and / 7 - 512), and a
// stack of the largest size check_scene accepts.  The rules say nothing of how the sizes, the levels and the feature bits hang together
// in a scene, so they bound what a scene can be given from above (tests/test_variant_census.py: a traversal key of this set that no scene
// reaches must be listed there with the relation that rules it out; none is).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../pbrs_amd/csrc/host/kernel_choice.h"

namespace pbrs {

// visit(const SceneFacts&) for each combination; returns how many there were.
template <class Visit>
size_t sweep_scene_facts(Visit&& visit) {
    size_t count = 0;
    SceneFacts f;
    f.shade_rec_bytes = 2048, f.shade_tri_bytes = 6144;
    f.wide_stack_bytes = 13u * kBlock * 4u;
    const size_t stack = 4096, big_stack = kLdsBytesPerCU / 2;
    const size_t sizes[][3] = {{stack, kLdsBytesPerCU / 8 - stack, kLdsBytesPerCU / 7 - 512 - stack},
                               {stack, kLdsBytesPerCU / 8 - stack + 1, kLdsBytesPerCU / 7 - 512 - stack},
                               {stack, kLdsBytesPerCU / 8 - stack + 1, kLdsBytesPerCU / 7 - 512 - stack + 1},
                               {big_stack, 8192, 1024}};
    for (uint32_t feat = 0; feat < 8; ++feat)
        for (int scanned = 0; scanned < 2; ++scanned)
            for (int extent = 0; extent < 2; ++extent)
                for (int lw = 0; lw < 2; ++lw)
                    for (int full = 0; full < 2; ++full)
                        for (int wide = 0; wide < 2; ++wide) {
                            if ((feat & PBRS_FEAT_FLAT_TLAS) && !scanned) continue;
                            if (wide && (!scanned || full)) continue;
                            f.features = feat, f.tlas_scanned = scanned, f.exact_extent = extent, f.long_walks = lw, f.full_steps = full, f.wide_ok = wide;
                            for (const auto& sz : sizes)
                                for (uint32_t nc = 0; nc < 4; ++nc)
                                    for (uint32_t lc = 0; lc <= nc; ++lc)
                                        for (uint32_t fc = 0; fc <= nc; ++fc)
                                            for (int tex = 0; tex < 2; ++tex)
                                                for (int fou = 0; fou < 2; ++fou)
                                                    for (int lam = 0; lam < 2; ++lam) {
                                                        if ((lc && lc == fc) || (fc && !fou) || (lam && (tex || fou))) continue;
                                                        f.stack_bytes = sz[0], f.scene_bytes = sz[1], f.top_bytes = sz[2];
                                                        f.n_classes = nc, f.lambert_class = lc, f.fourier_class = fc, f.textured = tex, f.fourier = fou, f.lambert = lam;
                                                        for (uint32_t light : {0u, PBRS_SHADE_LIGHT_SPHERE, PBRS_SHADE_LIGHT_TRIANGLE})
                                                            for (uint32_t lds : {0u, PBRS_SHADE_LDS_RECORDS, PBRS_SHADE_LDS_ALL}) {
                                                                f.light_spec = light, f.shade_lds = lds;
                                                                visit(static_cast<const SceneFacts&>(f));
                                                                ++count;
                                                            }
                                                    }
                        }
    return count;
}

}  // namespace pbrs
