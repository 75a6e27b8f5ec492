// device/raygen.h — the raygen stage (device/kernels.h): one camera ray per slot of the pass.
#pragma once
#include "path_state.h"

// ---- raygen --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_raygen(PathState st, RenderConst rc, uint32_t* rng_hi0) {
    uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= rc.n_slots) return;
    uint32_t k, pix;
    sample_of_slot(slot, rc.n_pixels, rc.n_slots / rc.n_pixels, rc.chunk_pixels, k, pix);
    uint32_t col, row;
    film_pixel_of_order(rc, pix, col, row);
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
    float dv[3];
    pbrs_camera_dir(rc.cam, x, y, dv);  // (device/entry_nodes.h: the pre-pass of the entry nodes bounds a pixel's directions with the same function)
    const f3 dir = ld3(dv);
    // bounce 0: the queue position of a path is its slot.  beta = 1, L = 0 and the origin are the same for every camera path:
    // bounce 0's k_shade takes them without a record (PathState), so only the RNG's high word travels beside the ray.
    st_stream(&st.q[0][0][slot], pack4(ld3(rc.cam.center), slot));
    st_stream(&st.q[0][1][slot], pack4(dir, (uint32_t)rng));
    __builtin_nontemporal_store((uint32_t)(rng >> 32), &rng_hi0[slot]);
}

// ---- entry nodes of the camera rays (device/entry_nodes.h) -----------------------------------------------------------
// Once per render, before its first pass: one lane per pixel of the traced region, in the passes' pixel order (the index sample_of_slot
// yields), so that neighbouring lanes write neighbouring records and the lanes of k_extend<.., EntryArgs> read them coalesced.  The origin
// goes into the table instance's space as enter_instance (traverse.h) takes a ray on the division-free box test there.
// info[0 .. 3]: pixels with entries, pixels with an empty list, pixels without a table, entries written.
__global__ void __launch_bounds__(256) k_entry_nodes(DevScene S, RenderConst rc, uint32_t height, uint32_t rows, uint4* table, uint32_t* info) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = q < rc.n_pixels;
    uint32_t n = PBRS_ENTRY_ROOT;
    if (valid) {
        uint32_t col, row;
        film_pixel_of_order(rc, q, col, row);
        const pbrs_instance& in = S.inst[S.entry_inst];
        f3 o = ld3(rc.cam.center);
        if (!((in.flags & PBRS_INSTANCE_IDENTITY) && o.x != 0.0f && o.y != 0.0f && o.z != 0.0f)) o = xf_apply(in.inv, o, 1.0f);
        const float ov[3] = {o.x, o.y, o.z};
        pbrs_dir_box B;
        pbrs_entry_record rec;
        if (pbrs_entry_dir_box(rc.cam, col, row, B) && pbrs_en_origin_in_range(o.x) && pbrs_en_origin_in_range(o.y) && pbrs_en_origin_in_range(o.z)) {
            n = pbrs_entry_record_of(S.nodes, in.blas_root, ov, B, PBRS_ENTRY_FORKS, height, rows, rec);
        } else {
            for (uint32_t i = 0; i < PBRS_ENTRY_MAX; ++i) rec.e[i] = PBRS_ENTRY_UNUSED;
            rec.e[0] = PBRS_ENTRY_ROOT;
        }
        table[2u * q] = make_uint4(rec.e[0], rec.e[1], rec.e[2], rec.e[3]);
        table[2u * q + 1u] = make_uint4(rec.e[4], rec.e[5], rec.e[6], rec.e[7]);
    }
    const uint32_t with = (uint32_t)__popcll(__ballot(valid && n != PBRS_ENTRY_ROOT && n != 0u)), empty = (uint32_t)__popcll(__ballot(valid && n == 0u)),
                   none = (uint32_t)__popcll(__ballot(valid && n == PBRS_ENTRY_ROOT));
    uint32_t sum = (valid && n != PBRS_ENTRY_ROOT) ? n : 0u;
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((threadIdx.x & 63u) == 0u) {
        if (with) atomicAdd(info + 0, with);
        if (empty) atomicAdd(info + 1, empty);
        if (none) atomicAdd(info + 2, none);
        if (sum) atomicAdd(info + 3, sum);
    }
}
