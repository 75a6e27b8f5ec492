/* pbrs_filter.h — the 1-D factors of the pixel reconstruction filters (include/pbrs_gpu.h, pbrs_pixel_filter), shared by
 * the device (pbrs_amd/csrc/device/film.h) and the host library.  Every operation is an IEEE f32 operation in the order
 * written, and the transcendentals are pbrs_numeric.h's: compiled with -ffp-contract=off, both sides agree bit for bit.
 *
 * The forms are math/src/filter.rs:33-90 per axis (the weight of a sample is fx(ox) * fy(oy), each factor with its own
 * axis's radius), with one deliberate deviation: filter.rs:40-41 misses the `.exp()` of the Gaussian's first term, which
 * makes every Gaussian weight 0; pbrt-v3's exp(-alpha o^2) - exp(-alpha r^2) is used instead (the reference never calls
 * `eval`, so nothing observable depends on it).
 */
#ifndef PBRS_FILTER_H
#define PBRS_FILTER_H

#include "pbrs_gpu.h"
#include "pbrs_numeric.h"

/* Filter::sinc (filter.rs:63-70) */
PN_FN float pf_sinc(float x) { return pn_abs(x) < 1e-5f ? 1.0f : pn_sin(PN_PI * x) / (PN_PI * x); }

/* The factor of one axis at offset `o` from the pixel centre, `r` the axis's radius; a, b as pbrs_pixel_filter. */
PN_FN float pf_factor(uint32_t kind, float o, float r, float a, float b) {
    if (kind == PBRS_FILTER_BOX) return 1.0f;
    if (kind == PBRS_FILTER_TRIANGLE) return pn_max(r - pn_abs(o), 0.0f);
    if (kind == PBRS_FILTER_GAUSSIAN) return pn_max(pn_exp((-a * o) * o) - pn_exp((-a * r) * r), 0.0f);  /* pbrt-v3, see above */
    if (kind == PBRS_FILTER_MITCHELL) {
        /* mitchell_netravali_1d(o / r, B, C) (filter.rs:72-90); the polynomial is float.rs:106-110's Horner fold */
        const float x = pn_abs(2.0f * (o / r));
        float c0, c1, c2, c3;
        if (x > 1.0f) {
            c0 = 8.0f * a + 24.0f * b;
            c1 = -12.0f * a - 48.0f * b;
            c2 = 6.0f * a + 30.0f * b;
            c3 = -a - 6.0f * b;
        } else {
            c0 = 6.0f - 2.0f * a;
            c1 = 0.0f;
            c2 = -18.0f + 12.0f * a + 6.0f * b;
            c3 = 12.0f - 9.0f * a - 6.0f * b;
        }
        float d = 0.0f;
        d = d * x + c3;
        d = d * x + c2;
        d = d * x + c1;
        d = d * x + c0;
        return (1.0f / 6.0f) * d;
    }
    /* PBRS_FILTER_LANCZOS: the windowed sinc of filter.rs:50-59, tau = a (the window is the support test) */
    return pf_sinc(pn_abs(o) / a) * pf_sinc(pn_abs(o));
}

/* The halo of one axis: every sample that can lie inside the support of a pixel is at most floor(r + 0.5) pixels away. */
PN_FN uint32_t pf_halo(float r) { return (uint32_t)pn_floor(r + 0.5f); }

#endif /* PBRS_FILTER_H */
