// device/class_sort.h — the class sort between extend and shade (device/kernels.h).
#pragma once
#include "path_state.h"

// ---- class sort ------------------------------------------------------------------------------------------------
// A wave of k_shade that holds paths on different kinds of material runs every kind's code one after the other with most
// lanes masked (C3: 30 of 64 lanes active on average).  Scenes with several shading classes (materials with the same
// lobe signature, pbrs_upload_scene) therefore get their bounce queues ordered by class before shading: a stable
// counting sort of the hit records' class word within tiles of PBRS_SORT_TILE queue positions (one block per tile), which
// writes the permutation k_shade reads its paths through.  The records themselves stay where they are (k_shade gathers
// 4 x 16 bytes per path; inside a class the order is the queue's, so the gathers stay near-sequential) and tiles keep
// the spatial order of the queue at large.  The result of a path does not depend on which lane shades it.  (PBRS_SORT_TILE: device/scene.h)
// Class sizes of the queue positions [base, end) into s_tot[] (zeroed, block-wide).  Sixteen ballots per 64 paths, lane c of a
// wave keeping class c's count, and one LDS add per lane at the end: one LDS atomic per PATH on sixteen words at most was
// what the counting pass spent its time on (0.39 ms per 200 M paths reading bytes, as much as when it read 16-byte records).
template <uint32_t NC>  // classes that occur (16, or 2 for a queue split into kept and dropped paths)
PD void tile_class_histogram(const uint8_t* cls, uint32_t base, uint32_t end, uint32_t* s_tot) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t mine = 0;
    for (uint32_t it = base; it < end; it += 256u) {  // block-uniform trip count
        const uint32_t i = it + threadIdx.x;
        const uint32_t c = i < end ? ((uint32_t)cls[i] & (PBRS_MAX_CLASSES - 1u)) : 0xffffffffu;
#pragma unroll
        for (uint32_t k = 0; k < NC; ++k) {
            const uint32_t nk = (uint32_t)__popcll(__ballot(c == k));
            if (lane == k) mine += nk;
        }
    }
    if (lane < NC && mine) atomicAdd(&s_tot[lane], mine);
}
__global__ void __launch_bounds__(256) k_class_sort(PathState st, const uint32_t* count, uint32_t n_direct) {
    const uint32_t n = count ? *count : n_direct;
    const uint32_t base = blockIdx.x * PBRS_SORT_TILE;
    if (base >= n) return;
    const uint32_t end = base + PBRS_SORT_TILE < n ? base + PBRS_SORT_TILE : n;
    __shared__ uint32_t s_tot[PBRS_MAX_CLASSES];     // class sizes in the tile, then their running write offsets
    __shared__ uint32_t s_wave[4][PBRS_MAX_CLASSES];  // per iteration: class counts of each wave
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (threadIdx.x < PBRS_MAX_CLASSES) s_tot[threadIdx.x] = 0u;
    __syncthreads();
    tile_class_histogram<PBRS_MAX_CLASSES>(st.cls, base, end, s_tot);
    __syncthreads();
    if (threadIdx.x == 0) {  // exclusive prefix over the classes
        uint32_t run = base;
        for (uint32_t c = 0; c < PBRS_MAX_CLASSES; ++c) {
            const uint32_t k = s_tot[c];
            s_tot[c] = run;
            run += k;
        }
    }
    __syncthreads();
    for (uint32_t it = base; it < end; it += 256u) {  // every thread of the block takes part in the barriers
        const uint32_t i = it + threadIdx.x;
        const bool valid = i < end;
        const uint32_t cls = valid ? ((uint32_t)st.cls[i] & (PBRS_MAX_CLASSES - 1u)) : 0xffffffffu;
        uint32_t rank = 0;
        for (uint32_t c = 0; c < PBRS_MAX_CLASSES; ++c) {
            const uint64_t m = __ballot(cls == c);
            if (cls == c) rank = lane_prefix(m);
            if (lane == 0) s_wave[wave][c] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        if (valid) {
            uint32_t pos = s_tot[cls] + rank;
            for (uint32_t w = 0; w < wave; ++w) pos += s_wave[w][cls];
            st.perm[pos] = i;
        }
        __syncthreads();
        if (threadIdx.x < PBRS_MAX_CLASSES) s_tot[threadIdx.x] += s_wave[0][threadIdx.x] + s_wave[1][threadIdx.x] + s_wave[2][threadIdx.x] + s_wave[3][threadIdx.x];
        __syncthreads();
    }
}

// Class-major variant, for scenes whose Lambertian class is shaded by the Lambert variant of k_shade (pbrs_gpu.hip, run_pass):
// the same stable counting sort, over the whole queue — per-tile histograms (k_class_count), their prefix over the tiles per
// class (k_class_scan, one block), then the scatter (k_class_scatter).  Classes come in the order 0, 1, ... with class `last`
// moved to the end, so that "all classes but `last`" is one range of lanes too: class_range[PBRS_MAX_CLASSES].
template <uint32_t NC>
__global__ void __launch_bounds__(256) k_class_count(PathState st, const uint32_t* count, uint32_t n_direct) {
    const uint32_t n = count ? *count : n_direct;
    const uint32_t base = blockIdx.x * PBRS_SORT_TILE;
    if (base >= n) return;
    const uint32_t end = base + PBRS_SORT_TILE < n ? base + PBRS_SORT_TILE : n;
    __shared__ uint32_t s_tot[PBRS_MAX_CLASSES];
    if (threadIdx.x < PBRS_MAX_CLASSES) s_tot[threadIdx.x] = 0u;
    __syncthreads();
    tile_class_histogram<NC>(st.cls, base, end, s_tot);
    __syncthreads();
    if (threadIdx.x < PBRS_MAX_CLASSES) st.tile_hist[blockIdx.x * PBRS_MAX_CLASSES + threadIdx.x] = s_tot[threadIdx.x];
}
// One block of PBRS_MAX_CLASSES waves: wave c turns class c's per-tile counts into offsets inside the class.
// `acc` (optional): adds (paths of class `last`, paths in all) to two counters — what a queue split kept (pbrs_gpu.hip, split_decision).
__global__ void __launch_bounds__(64 * PBRS_MAX_CLASSES) k_class_scan(PathState st, const uint32_t* count, uint32_t n_direct, uint32_t last, unsigned long long* acc) {
    const uint32_t n = count ? *count : n_direct;
    const uint32_t n_tiles = (n + PBRS_SORT_TILE - 1u) / PBRS_SORT_TILE;
    const uint32_t c = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    __shared__ uint32_t s_total[PBRS_MAX_CLASSES];
    uint32_t carry = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += 64u) {  // wave-uniform trip count
        const uint32_t t = t0 + lane;
        const uint32_t v = t < n_tiles ? st.tile_hist[t * PBRS_MAX_CLASSES + c] : 0u;
        uint32_t x = v;  // inclusive scan over the wave
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const uint32_t y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        if (t < n_tiles) st.tile_hist[t * PBRS_MAX_CLASSES + c] = carry + x - v;
        carry += __shfl(x, 63, 64);
    }
    if (lane == 0) s_total[c] = carry;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < PBRS_MAX_CLASSES; ++k) {
            if (k == last) continue;
            st.class_range[k] = make_uint2(run, run + s_total[k]);
            run += s_total[k];
        }
        st.class_range[PBRS_MAX_CLASSES] = make_uint2(0u, run);  // every class but `last`
        if (last < PBRS_MAX_CLASSES) st.class_range[last] = make_uint2(run, run + s_total[last]);
        if (acc && last < PBRS_MAX_CLASSES) {
            atomicAdd(acc, (unsigned long long)s_total[last]);
            atomicAdd(acc + 1, (unsigned long long)n);
        }
    }
}
// `zero_dropped` (two classes, bounce 0 of a split queue only: queue position = slot): the paths the split drops are shaded by nobody, and
// bounce 0's k_shade is what first writes a slot's L — their radiance, 0, is stored here, before any reader of L runs.
template <uint32_t NC>
__global__ void __launch_bounds__(256) k_class_scatter(PathState st, const uint32_t* count, uint32_t n_direct, uint32_t zero_dropped) {
    const uint32_t n = count ? *count : n_direct;
    const uint32_t base = blockIdx.x * PBRS_SORT_TILE;
    if (base >= n) return;
    const uint32_t end = base + PBRS_SORT_TILE < n ? base + PBRS_SORT_TILE : n;
    __shared__ uint32_t s_tot[PBRS_MAX_CLASSES];      // running write offset of each class for this tile
    __shared__ uint32_t s_wave[4][PBRS_MAX_CLASSES];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (threadIdx.x < PBRS_MAX_CLASSES) s_tot[threadIdx.x] = st.class_range[threadIdx.x].x + st.tile_hist[blockIdx.x * PBRS_MAX_CLASSES + threadIdx.x];
    __syncthreads();
    for (uint32_t it = base; it < end; it += 256u) {  // every thread of the block takes part in the barriers
        const uint32_t i = it + threadIdx.x;
        const bool valid = i < end;
        const uint32_t cls = valid ? ((uint32_t)st.cls[i] & (PBRS_MAX_CLASSES - 1u)) : 0xffffffffu;
        uint32_t rank = 0;
#pragma unroll
        for (uint32_t c = 0; c < NC; ++c) {
            const uint64_t m = __ballot(cls == c);
            if (cls == c) rank = lane_prefix(m);
            if (lane == 0) s_wave[wave][c] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        if (valid && !(NC == 2u && cls == 0u)) {  // two classes: a queue split into dropped (0) and kept (1) paths, only the kept are listed
            uint32_t pos = s_tot[cls] + rank;
            for (uint32_t w = 0; w < wave; ++w) pos += s_wave[w][cls];
            st.perm[pos] = i;
        }
        if (NC == 2u && zero_dropped && valid && cls == 0u) st_stream(&st.L[i], make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        __syncthreads();
        if (threadIdx.x < NC) s_tot[threadIdx.x] += s_wave[0][threadIdx.x] + s_wave[1][threadIdx.x] + s_wave[2][threadIdx.x] + s_wave[3][threadIdx.x];
        __syncthreads();
    }
}
