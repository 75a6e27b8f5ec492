// device/bsdf_probe.h — the developer entry point pbrs_bsdf_eval's kernel: src/bsdf.rs through the code k_shade runs (device/bsdf.h), for
// caller-supplied frames, directions and random numbers (include/pbrs_gpu.h: the query and result words, the ops).
//
// The kernel builds the Bsdf as k_shade does (device/shade.h, "Bsdf bs = bsdf_new_frame") and makes k_shade's calls; it holds no
// shading arithmetic of its own.  LAM: bs.lam as the PBRS_SHADE_LAMBERT variants have it, a compile-time constant; FOURIER: the scene's
// tables behind bs.fourier as the PBRS_SHADE_FOURIER variants have them in the generic form (no LDS series column, `only` false),
// nullptr — a compile-time constant — otherwise.  The host has checked every query's material index and, for the sample op, that
// 0 <= u < 1: bsdf_sample_l reads lobe (uint32_t)(u * n) (pbrs_bsdf_eval).
#pragma once
#include "bsdf.h"

template <bool LAM, bool FOURIER>
__global__ void __launch_bounds__(256) k_bsdf_eval(DevScene S, uint32_t op, uint32_t n, const uint32_t* queries, uint32_t* results) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* q = queries + (size_t)i * PBRS_BSDF_QUERY_WORDS;
    auto vec = [q](uint32_t k) { return mk3(pn_from_bits(q[k]), pn_from_bits(q[k + 1u]), pn_from_bits(q[k + 2u])); };
    const pbrs_material* mat = S.mats + q[0];
    Isect is;
    is.pos = mk3(0.0f, 0.0f, 0.0f);
    is.normal = vec(1u);
    is.tangent = vec(4u);
    is.wo = vec(7u);
    is.u = is.v = 0.0f;
    const f3 wi_w = vec(10u);
    const float u = pn_from_bits(q[13]), v = pn_from_bits(q[14]);  // (word 15 is spare)
    Bsdf bs = bsdf_new_frame(is, S.bxdfs + mat->first_bxdf, mat->n_bxdfs);
    bs.lam = LAM;
    if (LAM && mat->n_bxdfs) bs.a0 = ld3(S.bxdfs[mat->first_bxdf].albedo);
    const FourierView fourier_view{S.fourier, S.tex_floats, S.tex_words, nullptr, 0u, false};
    bs.fourier = FOURIER ? &fourier_view : nullptr;

    f3 f = mk3(0.0f, 0.0f, 0.0f), wi_out = mk3(0.0f, 0.0f, 0.0f);
    ProbD pr = density(0.0f);
    uint32_t flags = 0u;
    if (op == PBRS_BSDF_SAMPLE_SPECULAR) {
        if (bsdf_sample_specular(bs, is.wo, f, wi_out, pr)) flags |= PBRS_BSDF_FOUND;
    } else {
        const f3 wo_l = world_to_local(bs, is.wo);
        if (op == PBRS_BSDF_EVAL) f = bsdf_eval_l(bs, wo_l, wi_w);
        else if (op == PBRS_BSDF_PDF) pr = density(bsdf_pdf_l(bs, wo_l, wi_w));
        else bsdf_sample_l(bs, wo_l, u, v, f, wi_out, pr);
    }
    if (pr.is_mass) flags |= PBRS_BSDF_IS_MASS;
    uint32_t* r = results + (size_t)i * PBRS_BSDF_RESULT_WORDS;
    r[0] = pn_bits(f.x); r[1] = pn_bits(f.y); r[2] = pn_bits(f.z);
    r[3] = pn_bits(wi_out.x); r[4] = pn_bits(wi_out.y); r[5] = pn_bits(wi_out.z);
    r[6] = pn_bits(pr.v);
    r[7] = flags;
}
