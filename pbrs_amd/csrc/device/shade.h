// device/shade.h — the shade stage (device/kernels.h): k_shade.
#pragma once
#include "lights.h"
#include "path_state.h"
#include "textures.h"

#ifndef PBRS_SHADE_WAVES  // min waves per SIMD asked of the register allocator for k_shade (2nd arg of __launch_bounds__)
#define PBRS_SHADE_WAVES 3
#endif
#ifndef PBRS_FOURIER_SHADE_WAVES  // ... and for its variants that carry the Fourier lobe (device/fourier.h).  At three waves they keep 168
#define PBRS_FOURIER_SHADE_WAVES 3  // registers and 428 bytes of scratch per lane, at two 255 registers and none — and are SLOWER: a 960 x 640,
#endif                              // 64-spp frame of tests/fourier_scenes.py shades in 124 / 228 ms at three and 147 / 285 ms at two
                                    // (tools/fourier_bench.py).  The spill code sits outside the series loops (one reload in 7 300
                                    // instructions at loop depth 2); what the lobe costs is the recomputed series itself.


PD float power_heuristic2(float f_pdf, float g_pdf) {  // src/directlighting.rs:224-232, BETA = 2, nf = ng = 1
    float f = 1.0f * f_pdf;
    float g = 1.0f * g_pdf;
    return pn_powi(f, 2) / (pn_powi(f, 2) + pn_powi(g, 2));
}

// Developer probe (tools/shade_probe.py; -DPBRS_PROBE_SHADE builds only): wall cycles of k_shade's regions, summed per wave.
// g_shade_probe[16] is defined by the unit that owns k_shade and the probe's reader (shade.hip), before it includes this file.
#ifdef PBRS_PROBE_SHADE
#ifndef PBRS_SHADE_PROBE_DEFINED
#error "device/shade.h in a -DPBRS_PROBE_SHADE build: only the unit that defines g_shade_probe may include it, after defining it (shade.hip)"
#endif
#define PBRS_SHADE_MARK(k)                                          \
    do {                                                            \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
        probe_acc[k] += now_ - probe_t;                             \
        probe_t = now_;                                             \
    } while (0)
#else
#define PBRS_SHADE_MARK(k) \
    do {                   \
    } while (0)
#endif

// ---- shade -----------------------------------------------------------------------------------------------------
// SPEC: what the scene's materials and lights allow the stage to leave out, and what it stages in LDS: the PBRS_SHADE_* bits of device/scene.h
#ifndef PBRS_FOURIER_AK_ROWS
#define PBRS_FOURIER_AK_ROWS 48u  // terms of a luminance series kept in LDS per lane; longer series are recomputed where they are consumed
#endif
template <uint32_t SPEC>
PD DevScene stage_shade_scene(const DevScene& G, uint32_t* lds_base) {
    DevScene S = G;
    uint4* dst = reinterpret_cast<uint4*>(__builtin_assume_aligned(lds_base, 16));
    if (SPEC & PBRS_SHADE_LDS_RECORDS) {
        S.inst = reinterpret_cast<const pbrs_instance*>(dst);
        dst = stage_array(dst, G.inst, G.n_inst * (uint32_t)(sizeof(pbrs_instance) / 16));
        S.shapes = reinterpret_cast<const pbrs_shape*>(dst);
        dst = stage_array(dst, G.shapes, G.n_shapes * (uint32_t)(sizeof(pbrs_shape) / 16));
        S.mats = reinterpret_cast<const pbrs_material*>(dst);
        dst = stage_array(dst, G.mats, G.n_mats * (uint32_t)(sizeof(pbrs_material) / 16));
        S.bxdfs = reinterpret_cast<const pbrs_bxdf*>(dst);
        dst = stage_array(dst, G.bxdfs, G.n_bxdfs * (uint32_t)(sizeof(pbrs_bxdf) / 16));
        S.alights = reinterpret_cast<const pbrs_area_light*>(dst);
        dst = stage_array(dst, G.alights, G.n_area * (uint32_t)(sizeof(pbrs_area_light) / 16));
        S.dlights = reinterpret_cast<const pbrs_delta_light*>(dst);
        dst = stage_array(dst, G.dlights, G.n_delta * (uint32_t)(sizeof(pbrs_delta_light) / 16));
    }
    if (SPEC & PBRS_SHADE_LDS_TRIS) {
        S.tv = reinterpret_cast<const pbrs_tri_verts*>(dst);
        dst = stage_array(dst, G.tv, G.n_tris * (uint32_t)(sizeof(pbrs_tri_verts) / 16));
        S.ts = reinterpret_cast<const pbrs_tri_shade*>(dst);
        dst = stage_array(dst, G.ts, G.n_tris * (uint32_t)(sizeof(pbrs_tri_shade) / 16));
    }
    __syncthreads();
    return S;
}
static_assert(sizeof(pbrs_material) % 16 == 0 && sizeof(pbrs_bxdf) % 16 == 0 && sizeof(pbrs_area_light) % 16 == 0 && sizeof(pbrs_delta_light) % 16 == 0 &&
                  sizeof(pbrs_tri_shade) % 16 == 0,
              "stage_shade_scene copies 16-byte pieces");
// The light a shadow ray was aimed at, for k_shadow to pass over (traverse.h, AnyWalk::skip).  A sample on an area light ends at t_max =
// 0.999, just short of the light's own surface, so the box of the instance that IS the light passes k_shadow's TLAS test for nearly
// every such ray, and the walk, having exhausted the terrain, still crossed two instance boundaries to learn that the light does not
// occlude the sample taken on it.  `Lt` is the chosen light; pad[0] / pad[1] of the uploaded record name the instance that is the light
// and its flat leaf (PBRS_SKIP_*; pbrs_upload_scene, from PreparedScene::light_link); `r` the ray exactly as it is stored in sr[0] / sr[1]: the
// instance's own test — the function the walk would call, on the same floats — is evaluated here, where the wave is full and the records
// are at hand, and the ray is tagged only if the value is FALSE.  Where it is true (a ray that grazes past its sample, a sample seen
// from inside the light) the ray goes untagged and walks as before.  Lone rays only: a path's two MIS rays have no sr[2] record.
template <uint32_t SPEC>
PD uint32_t light_skip_tag(const DevScene& S, const pbrs_area_light& Lt, const ShadowRay& r) {
    const uint32_t link = __float_as_uint(Lt.pad[0]) | __float_as_uint(Lt.pad[1]) << PBRS_SKIP_FLAT_SHIFT;
    if (link == 0u) return 0u;
    Cnt<false> cnt;
    const pbrs_instance& in = S.inst[(link & PBRS_SKIP_INST_MASK) - 1u];
    // a linked instance has its light's shape (host/scene_prepare.cpp): known at compile time where every light is a sphere
    const uint32_t kind = (SPEC & PBRS_SHADE_LIGHT_SPHERE) ? (uint32_t)PBRS_SHAPE_SPHERE : in.shape_kind;
    const bool own = analytic_occludes(S, in, kind, r.o, r.d, r.t_max, cnt);
    return own ? 0u : link;
}

template <uint32_t INTEG, bool TEX, uint32_t SPEC>
__global__ void __launch_bounds__(256, (SPEC & 8u) ? PBRS_FOURIER_SHADE_WAVES : PBRS_SHADE_WAVES) k_shade(DevScene G, PathState st, RenderConst rc, uint32_t bounce, const uint32_t* count, uint32_t n_direct,
                                              uint32_t* count_out, uint32_t* nee_queue, unsigned long long* nee_shadow_count, uint32_t sorted, const uint2* range,
                                              const uint32_t* rng_hi0) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_shade_scene[];
    // per-hit lobe lists of textured materials (Bsdf::hit_lobe / hit_albedo); absent from the untextured instantiation
    __shared__ uint32_t s_hit_lobe[TEX ? PBRS_MAX_BXDFS * 256 : 1];
    __shared__ float s_hit_albedo[TEX ? 3 * PBRS_MAX_BXDFS * 256 : 1];
    // the luminance series of a sampled Fourier direction pair, one column per lane (device/fourier.h, sample_fourier): 48 KB — three
    // blocks of the Fourier-only variants, which carry no texture lists, still fit a CU's LDS
    __shared__ float s_fourier_ak[(SPEC & 16u) ? PBRS_FOURIER_AK_ROWS * 256 : 1];
#ifdef PBRS_PROBE_SHADE
    unsigned long long probe_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long probe_t = __builtin_amdgcn_s_memtime();
#endif
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t n = count ? *count : n_direct;
    if (range) {  // one launch per group of shading classes: this one's lanes of the class-major permutation (k_class_scatter)
        const uint2 r = *range;
        i += r.x;
        n = r.y;
        if (blockIdx.x * blockDim.x + r.x >= n) return;  // the grid is sized for the whole queue
    } else if (blockIdx.x * blockDim.x >= n) {
        return;  // ... of the pass: a block beyond the bounce's queue has nothing to shade, nothing to compact
    }
    const DevScene S = (SPEC & (PBRS_SHADE_LDS_RECORDS | PBRS_SHADE_LDS_TRIS)) ? stage_shade_scene<SPEC>(G, lds_shade_scene) : G;
    bool valid = i < n;
    bool alive = false, cast0 = false, cast1 = false;
    uint32_t slot = 0;
    ShadowRay sr0, sr1;  // the rays to cast, kept until their queue positions are known
    sr0.o = sr0.d = sr1.o = sr1.d = gray(0.0f);
    sr0.t_max = sr1.t_max = -1.0f;
    f3 L_vis = gray(0.0f);  // a lone shadow ray: the path's radiance if it turns out unoccluded
    // ... and the light it was aimed at (light_skip_tag).  The chosen area light waits in LDS until the rays are stored: a register
    // carried through the shading code in between would cost the Lambert variants their sixth wave.  Not in the variants of scenes
    // whose lights are all triangles (links name analytic instances: there are none) nor in those that carry the Fourier lobe, which
    // live on spilled registers and would pay for the tag in scratch: their rays go untagged and walk as before.
    constexpr bool TAGS = !(SPEC & (PBRS_SHADE_LIGHT_TRIANGLE | PBRS_SHADE_FOURIER));
    __shared__ uint32_t s_light[TAGS ? 256 : 1];  // the chosen area light + 1; 0: none
    if (TAGS) s_light[threadIdx.x] = 0u;
    // the path's next record, kept until the compaction below has given it a queue position
    f3 next_o = gray(0.0f), next_d = gray(0.0f), next_beta = gray(0.0f);
    uint64_t next_rng = 0;
    uint32_t next_spec = 0;
    if (valid) {
        const uint32_t set = bounce & 1u;
        // several shading classes: lanes take the paths in class order (k_class_sort), so that a wave runs one material's code; a
        // queue k_extend split into kept and dropped paths: lanes take the kept positions (class 1 of a class-major order)
        const uint32_t src = sorted ? st.perm[i] : i;
        const float4 r1 = ld_stream(&st.q[set][1][src]), rh = ld_stream(&st.hit[src]);
        f3 o, beta, L;
        float post_w;  // the direct integrator's 1 / mass rides next to the radiance
        uint32_t rng_hi;
        bool specular_bounce;
        if (bounce == 0) {
            // a camera path (wave-uniform: `bounce` is a kernel argument): what k_raygen would have stored for it is the same for every
            // path but the RNG's high word — no q[0][0] / q[0][2] fetch, and no L round trip behind the slot
            slot = src;
            o = ld3(rc.cam.center);
            specular_bounce = false;
            beta = gray(1.0f);
            L = gray(0.0f);
            post_w = 0.0f;
            rng_hi = __builtin_nontemporal_load(&rng_hi0[src]);
        } else {
            const float4 r0 = ld_stream(&st.q[set][0][src]), r2 = ld_stream(&st.q[set][2][src]);
            slot = __float_as_uint(r0.w) & PBRS_SLOT_MASK;
            const float4 rl = st.L[slot];
            o = xyz(r0);
            specular_bounce = (__float_as_uint(r0.w) >> 31) != 0;
            beta = xyz(r2);
            L = xyz(rl);
            post_w = rl.w;
            rng_hi = __float_as_uint(r2.w);
        }
        f3 d = xyz(r1);
        const uint64_t rng_in = ((uint64_t)rng_hi << 32) | (uint64_t)__float_as_uint(r1.w);
        Hit h;
        h.t = rh.x;
        h.inst = __float_as_uint(rh.y);
        h.prim = __float_as_uint(rh.z);
        bool has_hit = h.inst != 0xffffffffu;
        const pbrs_material* mat = nullptr;
        if (has_hit) mat = S.mats + S.inst[h.inst].material;
        // The direct-lighting integrator (INTEG 1, src/directlighting.rs:14-56) runs on the same stage: bounce 0 is
        // direct_lighting_integrator, bounce 1 the debug integrator behind one specular lobe.  Its result is
        // direct + (S * f) * (1 / mass): f travels in the beta columns, 1 / mass in the flags column (as float bits).
        bool emitter_hit = false;
        float post = 1.0f;
        if (INTEG == PBRS_INTEGRATOR_MATERIALS) {  // material_visualizer, src/directlighting.rs:234-271
            if (has_hit) {
                float r = 0.0f, g = 0.0f, b = 0.0f;  // pal[index], :235-246; Color::rgb = u8 / 255.0 (color.rs:51-53)
                switch (mat->vis_class) {
                    case 0: r = 232.0f, g = 207.0f, b = 59.0f; break;
                    case 1: r = 124.0f, g = 188.0f, b = 126.0f; break;
                    case 2: r = 30.0f, g = 68.0f, b = 176.0f; break;
                    case 3: r = 15.0f, g = 142.0f, b = 205.0f; break;
                    case 4: r = 44.0f, g = 180.0f, b = 172.0f; break;
                    case 5: r = 216.0f, g = 39.0f, b = 252.0f; break;
                    case 6: r = 143.0f, g = 112.0f, b = 252.0f; break;
                    default: break;
                }
                L = mk3(r / 255.0f, g / 255.0f, b / 255.0f);
                if (mat->vis_class == 7u) L = gray(0.3f);
                if (mat->vis_class == 8u) L = gray(0.9f);
            } else {
                const int parity = (int)((uint32_t)pn_f32_to_i32(pn_floor(d.x * 50.0f)) + (uint32_t)pn_f32_to_i32(pn_floor(d.y * 50.0f)));
                L = gray(parity % 2 == 0 ? 0.9f : 0.7f);
            }
            emitter_hit = true;  // nothing below runs for this lane
        } else if (INTEG == PBRS_INTEGRATOR_NORMALS) {  // normal_visualizer, src/directlighting.rs:273-289
            if (!has_hit) {
                L = env_eval(S, d);
            } else {
                const Isect is = reconstruct_isect(S, h, o, d);
                const pbrs_bxdf& lobe0 = S.bxdfs[mat->first_bxdf];
                const pbrs_bxdf& vis = S.bxdfs[mat->vis_bxdf - 1u];
                f3 albedo = gray(0.0f);  // `let (_, albedo) = mtl.scatter(-ray.dir, &hit)`; black where scatter is todo!()
                switch (mat->vis_class) {
                    case 8:  // Lambertian, material/src/lib.rs:163-177
                        albedo = vis.tex ? tex_value(S, (vis.tex & ~PBRS_BXDF_TEX_DROP_IF_BLACK) - 1u, is.u, is.v, is.pos) : ld3(vis.albedo);
                        break;
                    case 7:  // Metal :192-199: Fresnel::conductor(eta, k).eval(|n . wi|), wi = -ray.dir as it is
                        albedo = fresnel_eval(lobe0, pn_abs(dot(is.normal, -d)));
                        break;
                    case 5:  // Mirror :224-228
                    case 0:  // Plastic :427-432
                        albedo = ld3(vis.albedo);
                        break;
                    case 4: {  // Dielectric :246-264
                        const float ior = lobe0.eta[1];
                        const f3 wi = hat(-d);
                        const float ndw = dot(is.normal, wi);
                        const bool inside = ndw < 0.0f;
                        const f3 outward = inside ? -is.normal : is.normal;
                        const float ratio = inside ? ior : 1.0f / ior;
                        const float cosine = inside ? -ndw : ndw;
                        f3 wt;
                        const bool transmits = refract3(outward, wi, ratio, wt);
                        float reflect_pr = 1.0f;
                        albedo = ld3(lobe0.albedo);  // self.reflect
                        if (transmits) {
                            float r0 = (1.0f - ior) / (1.0f + ior);  // schlick, :477-481
                            r0 = r0 * r0;
                            reflect_pr = r0 + (1.0f - r0) * pn_powi(1.0f - cosine, 5);
                            albedo = ld3(vis.albedo);  // self.transmit
                        }
                        uint64_t rng = rng_in;
                        if (pn_rng_f32(&rng) < reflect_pr) albedo = ld3(lobe0.albedo);
                        break;
                    }
                    default: break;  // DiffuseLight: black (:282-286); Glossy / Uber / Substrate / Fourier: todo!()
                }
                L = (albedo + is.normal) * 0.5f;
            }
            emitter_hit = true;
        } else if (INTEG == PBRS_INTEGRATOR_PATH) {
            if (bounce == 0 || specular_bounce) {  // pathintegrator.rs:19-22
                f3 e = has_hit ? ld3(mat->emission) : env_eval(S, d);
                L = L + cmul(beta, e);
            }
        } else if (bounce == 0) {
            if (!has_hit) {
                L = env_eval(S, d);  // scene.eval_env_light(ray), directlighting.rs:45
            } else if (!is_black(ld3(mat->emission))) {
                L = ld3(mat->emission);  // :27-28
                emitter_hit = true;
            }
        } else {
            post = post_w;
            if (!has_hit) L = L + cmul(env_eval(S, d), beta) * post;  // :54, then spec_refl * f * pr.mass().weak_recip() (:37)
        }
        PBRS_SHADE_MARK(0);  // queue + state loads, emission
        if (has_hit && !emitter_hit) {
            uint64_t rng = rng_in;
#ifdef PBRS_ABL_NO_RECON  // timing-only ablation build: skips the Interaction rebuild, results are wrong
            Isect is;
            is.pos = o + h.t * d;
            is.normal = mk3(0.0f, 1.0f, 0.0f);
            is.wo = -d;
            is.tangent = mk3(1.0f, 0.0f, 0.0f);
#else
            Isect is = reconstruct_isect(S, h, o, d);
#endif
            Bsdf bs = bsdf_new_frame(is, S.bxdfs + mat->first_bxdf, mat->n_bxdfs);
            bs.lam = (SPEC & PBRS_SHADE_LAMBERT) != 0u;
            if ((SPEC & PBRS_SHADE_LAMBERT) && mat->n_bxdfs) bs.a0 = ld3(S.bxdfs[mat->first_bxdf].albedo);
            const FourierView fourier_view{S.fourier, S.tex_floats, S.tex_words, (SPEC & PBRS_SHADE_FOURIER_ONLY) ? s_fourier_ak + threadIdx.x : nullptr,
                                           (SPEC & PBRS_SHADE_FOURIER_ONLY) ? PBRS_FOURIER_AK_ROWS : 0u, (SPEC & PBRS_SHADE_FOURIER_ONLY) != 0u};
            bs.fourier = (SPEC & PBRS_SHADE_FOURIER) ? &fourier_view : nullptr;
            if (TEX && (mat->flags & PBRS_MATERIAL_TEXTURED)) {
                // `mtl.bxdfs_at(&hit)` with non-Solid textures (material/src/lib.rs:180-184, :317-365): evaluate each
                // lobe's colour at (uv, pos) once, keep the lobes the material pushes for this hit
                uint32_t* hl = s_hit_lobe + threadIdx.x;
                float* ha = s_hit_albedo + threadIdx.x;
                uint32_t kept = 0;
                for (uint32_t k = 0; k < mat->n_bxdfs; ++k) {
                    const pbrs_bxdf& lb = bs.lobes[k];
                    f3 colour = ld3(lb.albedo);
                    if (lb.tex) {
                        colour = tex_value(S, (lb.tex & ~PBRS_BXDF_TEX_DROP_IF_BLACK) - 1u, is.u, is.v, is.pos);
                        if ((lb.tex & PBRS_BXDF_TEX_DROP_IF_BLACK) && is_black(colour)) continue;
                    }
                    hl[kept * 256u] = k;
                    ha[(3u * kept) * 256u] = colour.x;
                    ha[(3u * kept + 1u) * 256u] = colour.y;
                    ha[(3u * kept + 2u) * 256u] = colour.z;
                    ++kept;
                }
                bs.n = kept;
                bs.hit_lobe = hl;
                bs.hit_albedo = ha;
            }
            PBRS_SHADE_MARK(1);  // interaction rebuild + frame

            // uniform_sample_one_light, directlighting.rs:58-99
            uint32_t num_lights = S.n_delta + S.n_area + S.has_env;
#ifdef PBRS_ABL_NO_NEE  // timing-only ablation build (tools/ablate.sh): skips next-event estimation, results are wrong
            if (num_lights > 0) {
                for (int k = 0; k < 5; ++k) pn_rng_f32(&rng);
                num_lights = 0;
            }
#endif
            if (num_lights > 0) {
                float light_pdf = 1.0f / (float)num_lights;
                float uidx = pn_rng_f32(&rng);
                uint32_t chosen = (uint32_t)(uidx * (float)num_lights);
                if (chosen > num_lights - 1) chosen = num_lights - 1;
                float lu = pn_rng_f32(&rng), lv = pn_rng_f32(&rng);
                float su = pn_rng_f32(&rng), sv = pn_rng_f32(&rng);
                float scale = 1.0f / light_pdf;
                const f3 wo_l = world_to_local(bs, is.wo);  // once for eval, pdf and the MIS sample below
                f3 c1 = gray(0.0f), c2 = gray(0.0f);
                ShadowRay v1, v2;
                v1.t_max = -1.0f;
                v2.t_max = -1.0f;
                v1.o = v1.d = v2.o = v2.d = gray(0.0f);
                uint32_t mode;
                if (chosen < S.n_delta) {  // estimate_direct_delta_light :101-153
                    mode = 1;
                    f3 li, wi;
                    ShadowRay vis;
                    delta_sample_incident(S.dlights[chosen], is, li, wi, vis);
                    f3 bv = bsdf_eval_l(bs, wo_l, wi) * pn_abs(dot(is.normal, wi));
                    if (!(is_black(li) || is_black(bv))) {
                        c1 = cmul(bv, li) * 1.0f * pn_weak_recip(1.0f);
                        v1 = vis;
                    }
                } else if (chosen >= S.n_delta && chosen < S.n_area) {  // Q6 guard; estimate_direct_area_light :155-222
                    mode = 0;
                    const pbrs_area_light& Lt = S.alights[chosen - S.n_delta];
                    const uint32_t lkind = (SPEC & PBRS_SHADE_LIGHT_SPHERE) ? (uint32_t)PBRS_SHAPE_SPHERE
                                           : (SPEC & PBRS_SHADE_LIGHT_TRIANGLE) ? (uint32_t)PBRS_SHAPE_TRIANGLE : Lt.shape_kind;
                    if (TAGS) s_light[threadIdx.x] = chosen - S.n_delta + 1u;
                    f3 li, wi;
                    float lpdf;
                    ShadowRay vis;
                    area_sample_incident(Lt, lkind, is, lu, lv, li, wi, lpdf, vis);
                    PBRS_SHADE_MARK(2);  // NEE: draws + light sample + its pdf
                    if (lpdf > 0.0f && !is_black(li)) {
                        f3 bv = bsdf_eval_l(bs, wo_l, wi) * pn_abs(dot(is.normal, wi));
                        float spdf = bsdf_pdf_l(bs, wo_l, wi);
                        if (!is_black(bv) && spdf > 0.0f) {
                            float weight = power_heuristic2(lpdf, spdf);
                            c1 = cmul(bv, li) * weight * pn_weak_recip(lpdf);
                            v1 = vis;
                        }
                    }
                    PBRS_SHADE_MARK(3);  // NEE term 1: BSDF eval + pdf + MIS weight
                    f3 f2, wi2;
                    ProbD pr2;
                    bsdf_sample_l(bs, wo_l, su, sv, f2, wi2, pr2);
                    f2 = f2 * pn_abs(dot(is.normal, wi2));
                    if (!(is_black(f2) || !(pr2.v > 0.0f))) {
                        f3 le;
                        float lpdf2;
                        ShadowRay vis2;
                        if (area_radiance_to(Lt, lkind, is, wi2, le, lpdf2, vis2)) {
                            if (!(is_black(le) || lpdf2 <= 0.0f)) {
                                float weight = pr2.is_mass ? 1.0f : power_heuristic2(pr2.v, lpdf2);
                                c2 = (weight * cmul(f2, le)) * pn_weak_recip(pr2.v);
                                v2 = vis2;
                            }
                        }
                    }
                } else {  // :80-96 environment
                    mode = 2;
                    f3 f2, wi2;
                    ProbD pr2;
                    bsdf_sample_l(bs, wo_l, su, sv, f2, wi2, pr2);
                    spawn_ray(is, wi2, v1.o, v1.d);
                    v1.t_max = pn_inf();
                    float ac = pn_abs(dot(wi2, is.normal));
                    float wr = pn_weak_recip(pr2.v);
                    c1 = cmul(env_eval(S, v1.d), f2) * ac * wr;  // scene.eval_env_light(incident_ray), :90-95
                    c2 = cmul(gray(0.0f), f2) * ac * wr;  // Color::black() * f * ..., the occluded arm
                }
                PBRS_SHADE_MARK(4);  // NEE term 2: BSDF sample + light intersection + pdf
                cast0 = v1.t_max >= 0.0f;
                cast1 = v2.t_max >= 0.0f;
                if (cast0 && cast1) {
                    // two rays (area light, both MIS terms alive): directlighting.rs:193 and :219 add up in k_nee_resolve
                    st.nee[0][slot] = pack4(c1, scale);
                    st.nee[1][slot] = pack4(c2, post);
                    st.nee[2][slot] = pack4(beta, 0.0f);
                } else if (cast0 || cast1) {
                    // one ray: the lane that traces it finishes the estimate (directlighting.rs:193 / :219 / :90-96, then
                    // :98 and pathintegrator.rs:35), so both outcomes are evaluated here with the reference's operations
                    f3 cr = cast0 ? c1 : c2;
                    f3 one_v, one_o;
                    if (mode == 0) {
                        one_o = gray(0.0f);
                        one_v = gray(0.0f) + cr;
                    } else if (mode == 1) {
                        one_o = gray(0.0f);
                        one_v = cr;
                    } else {
                        one_o = c2;
                        one_v = cr;
                    }
                    f3 add_v = cmul(beta, one_v * scale);
                    f3 add_o = cmul(beta, one_o * scale);
                    if (INTEG != PBRS_INTEGRATOR_PATH) {
                        add_v = add_v * post;
                        add_o = add_o * post;
                    }
                    // pathintegrator.rs:35 is one f32 add per channel either way: the occluded outcome goes into L here,
                    // the unoccluded one travels with the ray and replaces it (k_shadow) — nothing below touches L
                    L_vis = L + add_v;
                    L = L + add_o;
                } else {
                    // nothing to test: the estimate is black; pathintegrator.rs:35 still adds beta * (black * n)
                    f3 z = cmul(beta, gray(0.0f) * scale);
                    if (INTEG != PBRS_INTEGRATOR_PATH) z = z * post;
                    L = L + z;
                }
                sr0 = v1;
                sr1 = v2;
            }

            if (INTEG != PBRS_INTEGRATOR_PATH) {
                // directlighting.rs:31-41: one level of perfect specular reflection / refraction
                f3 f, wi;
                ProbD pr;
                if (bounce == 0 && bsdf_sample_specular(bs, is.wo, f, wi, pr)) {
                    f3 no, nd;
                    spawn_ray(is, wi, no, nd);
                    alive = true;
                    next_o = no;
                    next_d = nd;
                    next_beta = f;
                    next_rng = rng;
                    post_w = pn_weak_recip(pr.v);
                }
            } else {
            PBRS_SHADE_MARK(5);  // NEE bookkeeping (cast flags, both outcomes)
            // pathintegrator.rs:46-71
            float r0 = pn_rng_f32(&rng), r1 = pn_rng_f32(&rng);
            f3 f, wi;
            ProbD pr;
            bsdf_sample(bs, -d, r0, r1, f, wi, pr);
            if (!(is_black(f) || pr.v == 0.0f)) {
                specular_bounce = pr.is_mass;
                beta = cmul(beta, f) * dot(wi, is.normal) * pn_recip(pr.v);  // Q9: no abs
                f3 no, nd;
                spawn_ray(is, wi, no, nd);
                bool cont = true;
                if (bounce > 3) {
                    float q = pn_max(1.0f - luminance(beta), 0.05f);
                    if (pn_rng_f32(&rng) < q)
                        cont = false;
                    else
                        beta = beta * pn_recip(1.0f - q);
                }
                if (cont && bounce + 1 < rc.max_depth) {
                    alive = true;
                    next_o = no;
                    next_d = nd;
                    next_beta = beta;
                    next_rng = rng;
                    next_spec = specular_bounce ? 0x80000000u : 0u;
                }
            }
            }
        }
        st.L[slot] = pack4(L, post_w);
        PBRS_SHADE_MARK(6);  // bounce: BSDF sample, beta, spawn, roulette, state stores
    }
    // Stream compaction of the three outputs.  A hot queue tail serialises at ~10 ns per atomic on gfx950, so the
    // counts are first summed per block through LDS and the tails are bumped by TWO atomics per block: the
    // next-bounce tail, and one 64-bit add carrying the nee-path count (low half) and the shadow-ray count (high).
    __shared__ uint32_t s_cnt[4][4];   // [wave][alive, nee, cast0, cast1]
    __shared__ uint32_t s_base[4];     // block bases: alive, nee, shadow
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const bool both = cast0 && cast1;
    const uint32_t lone = (!both && (cast0 || cast1)) ? 0x40000000u : 0u;
    const uint64_t m_alive = __ballot(alive), m_nee = __ballot(both), m_c0 = __ballot(cast0), m_c1 = __ballot(cast1);
    if (lane == 0) {
        s_cnt[wave][0] = (uint32_t)__popcll(m_alive);
        s_cnt[wave][1] = (uint32_t)__popcll(m_nee);
        s_cnt[wave][2] = (uint32_t)__popcll(m_c0);
        s_cnt[wave][3] = (uint32_t)__popcll(m_c1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t_alive = 0, t_nee = 0, t_sh = 0;
        for (int w = 0; w < 4; ++w) {
            t_alive += s_cnt[w][0];
            t_nee += s_cnt[w][1];
            t_sh += s_cnt[w][2] + s_cnt[w][3];
        }
        uint32_t a = 0u;
        unsigned long long packed = 0ull;
        if (t_alive | t_nee | t_sh) {  // both in flight before either is waited for: the whole block sits out their latency
            a = atomicAdd(count_out, t_alive);
            packed = atomicAdd(nee_shadow_count, ((unsigned long long)t_sh << 32) | (unsigned long long)t_nee);
        }
        s_base[0] = a;
        s_base[1] = (uint32_t)packed;
        s_base[2] = (uint32_t)(packed >> 32);
    }
    __syncthreads();
    uint32_t b_alive = s_base[0], b_nee = s_base[1], b_sh = s_base[2];
    for (uint32_t w = 0; w < wave; ++w) {
        b_alive += s_cnt[w][0];
        b_nee += s_cnt[w][1];
        b_sh += s_cnt[w][2] + s_cnt[w][3];
    }
    if (alive) {
        const uint32_t j = b_alive + lane_prefix(m_alive), out = (bounce + 1u) & 1u;
        st_stream(&st.q[out][0][j], pack4(next_o, slot | next_spec));
        st_stream(&st.q[out][1][j], pack4(next_d, (uint32_t)next_rng));
        st_stream(&st.q[out][2][j], pack4(next_beta, (uint32_t)(next_rng >> 32)));
    }
    if (both) nee_queue[b_nee + lane_prefix(m_nee)] = slot;
    uint32_t skip_tag = 0u;  // travels in sr[2][j].w: lone rays (both MIS rays aim at the chosen light; a pair has no sr[2] record)
    if (TAGS && lone) {
        uint32_t t = threadIdx.x;
        asm volatile("" : "+v"(t));  // the word's address is formed again: kept from the write above, it held a register through the bounce code
        const uint32_t light = s_light[t];
        if (light != 0u) skip_tag = light_skip_tag<SPEC>(S, S.alights[light - 1u], cast0 ? sr0 : sr1);
    }
    if (cast0) {
        const size_t j = (size_t)b_sh + lane_prefix(m_c0);
        st_stream(&st.sr[0][j], pack4(sr0.o, sr0.t_max));
        st_stream(&st.sr[1][j], pack4(sr0.d, slot | lone));
        if (lone) st_stream(&st.sr[2][j], pack4(L_vis, skip_tag));
    }
    if (cast1) {
        const size_t j = (size_t)b_sh + s_cnt[wave][2] + lane_prefix(m_c1);
        st_stream(&st.sr[0][j], pack4(sr1.o, sr1.t_max));
        st_stream(&st.sr[1][j], pack4(sr1.d, slot | 0x80000000u | lone));
        if (lone) st_stream(&st.sr[2][j], pack4(L_vis, skip_tag));
    }
#ifdef PBRS_PROBE_SHADE
    PBRS_SHADE_MARK(7);  // compaction + queue / record writes
    if ((threadIdx.x & 63u) == 0 && __ballot(valid) != 0 && (blockIdx.x % 61u) == 0)  // a sample of the blocks
        for (int k = 0; k < 8; ++k) atomicAdd(&g_shade_probe[((SPEC & PBRS_SHADE_LAMBERT) ? 0 : 8) + k], probe_acc[k]);  // [0..7] the Lambert variants, [8..15] the others
#endif
}
