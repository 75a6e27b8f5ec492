// device/path_state.h — what the wavefront stages share: the path state of a pass (PathState), a render's constants (RenderConst), the
// slot order of a pass, the stream loads and stores of the records, the instrumented kernels' counters and the LDS staging copy.
// (The stages: device/kernels.h.)
#pragma once
#include "entry_nodes.h"
#include "shapes.h"  // dmath.h, scene.h, pbrs_f4v

struct PathState {
    // Path records by queue position i, structure-of-float4-arrays, ping-pong by bounce parity (k_shade reads set b & 1
    // and writes set (b + 1) & 1):
    //   q[.][0][i] = origin.xyz, slot | specular_bounce << 31        (t_max is always +inf for path rays: Ray::new)
    //   q[.][1][i] = dir.xyz,    RNG state, low word
    //   q[.][2][i] = beta.xyz,   RNG state, high word
    // Bounce 0 has no q[0][2] record and reads no q[0][0] in k_shade: every camera path starts at cam.center with beta 1, no
    // specular flag, L = 0 and slot = queue position, so k_raygen writes q[0][0] (k_extend's ray), q[0][1] and the one word
    // of the third record that carries information, into a column of the pass set that only k_raygen and k_shade are given:
    //   rng_hi0[i] = RNG state, high word, of the camera sample at slot i
    // (an argument of those two kernels, like the nee queue, and no member: a member moves the arguments of every kernel
    // that takes this struct, the traversal kernels among them)
    float4* q[2][3];
    float4* hit;  // [i] = t, inst (0xffffffff: miss), prim, shading class   written by k_extend at the ray's queue position
    uint8_t* cls;     // [queue position] shading class of the hit, a byte beside hit[].w for the class sort's two passes
    uint32_t* perm;  // scenes with several shading classes: k_shade's lane j shades the path at queue position perm[j] (k_class_sort)
    // class-major order (scenes whose Lambertian class gets the Lambert variant of k_shade): per tile and class, the count
    // and then the offset inside the class; per class (and, at [PBRS_MAX_CLASSES], for all classes but the Lambertian) the
    // range of lanes that shade it
    uint32_t* tile_hist;
    uint2* class_range;
    float4* L;    // [slot] = radiance.xyz, w: the direct integrator's 1 / mass (src/directlighting.rs:37), else unused
                  // First written by bounce 0's k_shade (every path it shades), by k_class_scatter<2u> for the paths a split queue
                  // drops at bounce 0, and by run_pass's memset when the pass has no bounce: nobody reads a slot before that.
    // Next-event estimation hand-off.  Shadow rays by position j in the bounce's shadow queue:
    //   sr[0][j] = origin.xyz, t_max        sr[1][j] = dir.xyz, item
    //   sr[2][j] = lone ray: the path's radiance if the ray is unoccluded (k_shade has stored the occluded outcome in L); .w: the light
    //              the ray was aimed at, where k_shadow need not visit it (scene.h, PBRS_SKIP_*; 0: none)
    // item = slot | 1 << 30 for a path's only shadow ray (the lane that traces it finishes the estimate), else
    // slot | ray index << 31: a path that casts both of its rays (the two MIS terms of an area light) cannot be finished
    // by either tracing lane — its terms wait in nee[] (by slot) and k_nee_resolve combines them with the two occlusion bytes.
    float4* sr[3];
    float4* nee[3];   // [slot]: c1.xyz, 1 / light_pdf | c2.xyz, post factor | beta at the time of the estimate, -
    uint8_t* occ[2];  // [slot], written by k_shadow: 1 = the ray is occluded
};
// (what a path holds of these and of the pass set's other columns: host/pass_plan.h, kPathColumns)

struct RenderConst {
    pbrs_camera cam;
    uint32_t x0, y0, w, h;
    uint32_t strata_x, strata_y;
    uint32_t max_depth;
    uint32_t pass_first_sample;  // sample index of k = 0 in this pass
    uint32_t n_pixels;           // P
    uint32_t n_slots;            // P * K of this pass
    uint32_t chunk_pixels;       // slot order of a pass (slot_of_sample): chunks of this many pixels, each with its K samples
    uint32_t tiles8_per_row;     // w / 8 when the pixels of the tile are taken in 8 x 8 blocks (pixel_of_order), else 0
    uint32_t band_rows, band_count, band_index;  // interleaved row bands (pbrs_render_params)
    uint32_t integrator;                         // PBRS_INTEGRATOR_*
    uint64_t seed;
};

// What k_extend<.., EntryArgs> is given beside the arguments of every k_extend (device/entry_nodes.h): the table k_entry_nodes wrote, by pixel
// of the pass's pixel order, and the pass's slot order (sample_of_slot), which leads from a camera ray's queue position to that pixel.
struct EntryArgs {
    const uint4* table;
    uint32_t n_pixels, k_count, chunk;
};

// Byte / word columns by path slot (the nee hand-off's occlusion bytes).  Slots stay below 2^28 (check_params).
template <class T>
PD T& at(T* base, uint32_t slot) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 1, "column element size");
    return *reinterpret_cast<T*>(reinterpret_cast<char*>(base) + (size_t)(uint32_t)(slot * (uint32_t)sizeof(T)));
}
PD float4 pack4(f3 v, uint32_t w) { return make_float4(v.x, v.y, v.z, __uint_as_float(w)); }
PD float4 pack4(f3 v, float w) { return make_float4(v.x, v.y, v.z, w); }
PD f3 xyz(float4 v) { return mk3(v.x, v.y, v.z); }
#define PBRS_SLOT_MASK 0x3fffffffu
// Queue and state records are streams: written by one kernel, read once by the next, tens of GB apart.  k_shade's and k_raygen's record
// traffic and k_extend's hit store are marked non-temporal, so that they do not push scene data out of the L2 (C4 +0.7 %, C2 +0.6 %, C3
// +1 %, c4xl +0.7 % in same-box A/B: profiles/r04r_ab_nontemporal_streams.log).  The rays a traversal kernel fetches stay ordinary loads:
// a walk reads its ray record again when it leaves an instance (traverse.h, reload_world).
PD float4 ld_stream(const float4* p) {
    const pbrs_f4v v = __builtin_nontemporal_load(reinterpret_cast<const pbrs_f4v*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
PD void st_stream(float4* p, float4 v) {
    pbrs_f4v w;
    w.x = v.x, w.y = v.y, w.z = v.z, w.w = v.w;
    __builtin_nontemporal_store(w, reinterpret_cast<pbrs_f4v*>(p));
}

// ---- slot order of a pass ----------------------------------------------------------------------------------------
// The P * K camera samples of a pass, in queue order: the pixels are cut into chunks of C (RenderConst::chunk_pixels; the
// last one shorter), and a chunk's samples come sample index by sample index — slot = chunk * C * K + k * C_chunk + pixel in
// chunk.  A wave still holds 64 neighbouring pixels of one sample index, but the K samples of a chunk now follow each
// other, and since a traversal kernel's blocks take the queue in eight contiguous segments, one per XCD (wave_fetch), an
// XCD works through its own band of the image chunk by chunk: the BVH subtrees and triangles under a chunk are fetched
// into that XCD's L2 once and serve all K samples, instead of once per sample index in all eight L2s (the order K, then
// pixels, that a plain `slot = k * P + pixel` gives).  The radiance of a sample does not depend on its slot.
PD void sample_of_slot(uint32_t slot, uint32_t n_pixels, uint32_t k_count, uint32_t chunk, uint32_t& k, uint32_t& pix) {
    const uint32_t per_chunk = chunk * k_count;
    const uint32_t c = slot / per_chunk, rem = slot - c * per_chunk, first = c * chunk;
    const uint32_t size = n_pixels - first < chunk ? n_pixels - first : chunk;
    k = rem / size;
    pix = first + (rem - k * size);
}
PD uint32_t slot_of_sample(uint32_t k, uint32_t pix, uint32_t n_pixels, uint32_t k_count, uint32_t chunk) {
    const uint32_t c = pix / chunk, first = c * chunk;
    const uint32_t size = n_pixels - first < chunk ? n_pixels - first : chunk;
    return c * chunk * k_count + k * size + (pix - first);
}

// The order the pixels of the tile are taken in: 8 x 8 blocks, row-major over the blocks and inside a block, when the
// tile's width and height are multiples of 8 (tiles8_per_row != 0) — a wave's 64 camera rays then leave through a square of
// the film instead of a 64-pixel line, and walk the same nodes for longer — else row-major.  order <-> pixel (row-major):
PD uint32_t pixel_of_order(uint32_t q, uint32_t w, uint32_t tiles8_per_row) {
    if (tiles8_per_row == 0u) return q;
    const uint32_t t = q >> 6, r = q & 63u;
    const uint32_t ty = t / tiles8_per_row, tx = t - ty * tiles8_per_row;
    return (ty * 8u + (r >> 3)) * w + tx * 8u + (r & 7u);
}
PD uint32_t order_of_pixel(uint32_t pix, uint32_t w, uint32_t tiles8_per_row) {
    if (tiles8_per_row == 0u) return pix;
    const uint32_t y = pix / w, x = pix - y * w;
    return (((y >> 3) * tiles8_per_row + (x >> 3)) << 6) + ((y & 7u) << 3) + (x & 7u);
}

// Film coordinates of the q-th pixel of a pass's pixel order (what sample_of_slot yields): the tile's 8 x 8 blocks, its offset, and the
// interleaved row bands of a render that traces one band in band_count.  k_raygen's mapping; k_entry_nodes makes the same one.
PD void film_pixel_of_order(const RenderConst& rc, uint32_t q, uint32_t& col, uint32_t& row) {
    const uint32_t pix = pixel_of_order(q, rc.w, rc.tiles8_per_row);
    const uint32_t vrow = pix / rc.w;
    col = rc.x0 + pix % rc.w;
    row = rc.y0 + (rc.band_count > 1 ? ((vrow / rc.band_rows) * rc.band_count + rc.band_index) * rc.band_rows + vrow % rc.band_rows : vrow);
}

struct GlobalCounters {  // instrumented variant only
    unsigned long long tlas_nodes, blas_nodes, instances, instance_hits, triangles, tri_shading, spheres, quads, cuboids, disks, rays, hits;
};

PD uint4* stage_array(uint4* dst, const void* src_, uint32_t n16) {  // one array into the block's LDS, 16 bytes per thread and turn; returns its end
    const uint4* src = reinterpret_cast<const uint4*>(src_);
    for (uint32_t i = threadIdx.x; i < n16; i += PBRS_TRAVERSAL_BLOCK) dst[i] = src[i];
    return dst + n16;
}
