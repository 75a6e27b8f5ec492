// device/raygen.h — the raygen stage (device/kernels.h): one camera ray per slot of the pass.
#pragma once
#include "path_state.h"

// ---- raygen --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_raygen(PathState st, RenderConst rc, uint32_t* rng_hi0) {
    uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= rc.n_slots) return;
    uint32_t k, pix;
    sample_of_slot(slot, rc.n_pixels, rc.n_slots / rc.n_pixels, rc.chunk_pixels, k, pix);
    pix = pixel_of_order(pix, rc.w, rc.tiles8_per_row);
    uint32_t col = rc.x0 + pix % rc.w, vrow = pix / rc.w;
    uint32_t row = rc.y0 + (rc.band_count > 1 ? ((vrow / rc.band_rows) * rc.band_count + rc.band_index) * rc.band_rows + vrow % rc.band_rows : vrow);
    uint32_t i = rc.pass_first_sample + k;
    uint64_t rng = pn_rng_init(rc.seed, row * rc.cam.width + col, i);
    float r0 = pn_rng_f32(&rng), r1 = pn_rng_f32(&rng);
    // src/main.rs:198-201 with msaa -> (strata_x, strata_y): i / msaa, i % msaa
    float jx = ((float)(i / rc.strata_y) + r0) / (float)rc.strata_x;
    float jy = ((float)(i % rc.strata_y) + r1) / (float)rc.strata_y;
    if (rc.integrator >= PBRS_INTEGRATOR_MATERIALS) jx = jy = 0.0f;  // the visualisers: `shoot_ray(row, col, (0.0, 0.0))`, src/main.rs:170
    // Camera::shoot_ray, camera.rs:65-77
    float x = (float)col + pn_fract(jx);
    float y = (float)row + pn_fract(jy);
    f3 dir = ld3(rc.cam.c) + ld3(rc.cam.a) * x + ld3(rc.cam.b) * y;
    // bounce 0: the queue position of a path is its slot.  beta = 1, L = 0 and the origin are the same for every camera path:
    // bounce 0's k_shade takes them without a record (PathState), so only the RNG's high word travels beside the ray.
    st_stream(&st.q[0][0][slot], pack4(ld3(rc.cam.center), slot));
    st_stream(&st.q[0][1][slot], pack4(dir, (uint32_t)rng));
    __builtin_nontemporal_store((uint32_t)(rng >> 32), &rng_hi0[slot]);
}
