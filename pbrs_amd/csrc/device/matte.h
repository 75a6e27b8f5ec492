// device/matte.h — id mattes (include/pbrs_gpu.h, pbrs_render_tile_matte*, pbrs_matte_mask*): per pixel the few ids that cover it and
// how many of the pixel's camera samples each covers, ranked, and the mask of a set of ids pulled from those layers.
//
// The samples are the ones k_aov folds: right after bounce 0's k_extend a pass holds every sample's hit record (hit[slot]).  k_matte,
// launched where k_aov is (pbrs_gpu.hip, run_pass), folds them into a per-pixel table in sample-index order, pass after pass;
// k_matte_finalize ranks the table once the last pass has run.  k_aov itself is not touched.
//
// State: planar words by pixel ORDER (order_of_pixel), 2 * slots + 1 per pixel — (id, count) of entry 0, of entry 1, ..., overflow.  It
// starts as zeros (pbrs_gpu.hip, render_common): count == 0 marks an empty entry, and the used entries are always a prefix of the table
// (entries fill in order, nothing is evicted), so one scan that stops at the first entry that is empty or holds the id does the whole
// update.
//
// The table lives in registers: every loop over it has a compile-time trip count (the kernels are instantiated on `slots`) and is
// unrolled, and an entry is updated by compare-select, never by a runtime index (which would put the arrays into scratch).
#pragma once
#include "path_state.h"

#define PBRS_MATTE_STATE_WORDS(slots) (2u * (slots) + 1u)

// One thread per pixel, by pixel order q: a sample index's loads are contiguous per wave (slot_of_sample), as in k_aov.  `qsplit`:
// k_extend's split flags (PBRS_QSPLIT_*, device/scene.h; not 0: PBRS_QSPLIT_ON): it split the queue and wrote no hit record for the paths it dropped
// (cls[slot] == 0): misses, as in k_aov.
template <uint32_t SLOTS>
__global__ void __launch_bounds__(256) k_matte(const pbrs_instance* inst, PathState st, uint32_t* state, uint32_t n_pixels, uint32_t k_count, uint32_t chunk,
                                               uint32_t qsplit, uint32_t key) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pixels) return;
    uint32_t id[SLOTS], cnt[SLOTS];
#pragma unroll
    for (uint32_t r = 0; r < SLOTS; ++r) {
        id[r] = state[(size_t)(2u * r) * n_pixels + q];
        cnt[r] = state[(size_t)(2u * r + 1u) * n_pixels + q];
    }
    uint32_t overflow = state[(size_t)(2u * SLOTS) * n_pixels + q];
    for (uint32_t k = 0; k < k_count; ++k) {
        const uint32_t slot = slot_of_sample(k, q, n_pixels, k_count, chunk);
        if (qsplit && st.cls[slot] == 0) continue;  // dropped by the split: a miss
        const uint32_t hit_inst = __float_as_uint(st.hit[slot].y);
        if (hit_inst == 0xffffffffu) continue;
        const uint32_t v = key == PBRS_MATTE_MATERIAL ? inst[hit_inst].material : hit_inst;
        bool placed = false;
#pragma unroll
        for (uint32_t r = 0; r < SLOTS; ++r) {
            const bool take = !placed && (cnt[r] == 0u || id[r] == v);
            id[r] = take ? v : id[r];
            cnt[r] += take ? 1u : 0u;
            placed = placed || take;
        }
        overflow += placed ? 0u : 1u;
    }
#pragma unroll
    for (uint32_t r = 0; r < SLOTS; ++r) {
        state[(size_t)(2u * r) * n_pixels + q] = id[r];
        state[(size_t)(2u * r + 1u) * n_pixels + q] = cnt[r];
    }
    state[(size_t)(2u * SLOTS) * n_pixels + q] = overflow;
}

// Ranks by count, descending; equal counts: the lower id first.  An entry is the 64-bit key count << 32 | ~id, so the order is one
// unsigned comparison and an empty entry (count 0, id 0xffffffff) is the key 0, behind everything.  The network is Batcher's odd-even
// merge sort for eight inputs (19 compare-exchanges); a comparator that touches an index >= SLOTS is left out at compile time, which is
// sound because those inputs stand for key 0 and a comparator only ever moves the smaller key to the higher index.
template <uint32_t SLOTS, uint32_t I, uint32_t J>
PD void matte_cx(unsigned long long (&e)[SLOTS]) {
    if constexpr (I < SLOTS && J < SLOTS) {
        const unsigned long long a = e[I], b = e[J];
        const bool swap = b > a;
        e[I] = swap ? b : a;
        e[J] = swap ? a : b;
    }
}

template <uint32_t SLOTS>
PD void matte_sort(unsigned long long (&e)[SLOTS]) {
    matte_cx<SLOTS, 0, 1>(e), matte_cx<SLOTS, 2, 3>(e), matte_cx<SLOTS, 4, 5>(e), matte_cx<SLOTS, 6, 7>(e);
    matte_cx<SLOTS, 0, 2>(e), matte_cx<SLOTS, 1, 3>(e), matte_cx<SLOTS, 4, 6>(e), matte_cx<SLOTS, 5, 7>(e);
    matte_cx<SLOTS, 1, 2>(e), matte_cx<SLOTS, 5, 6>(e);
    matte_cx<SLOTS, 0, 4>(e), matte_cx<SLOTS, 1, 5>(e), matte_cx<SLOTS, 2, 6>(e), matte_cx<SLOTS, 3, 7>(e);
    matte_cx<SLOTS, 2, 4>(e), matte_cx<SLOTS, 3, 5>(e);
    matte_cx<SLOTS, 1, 2>(e), matte_cx<SLOTS, 3, 4>(e), matte_cx<SLOTS, 5, 6>(e);
}

// The ranked layers, pixel-major ([pixel][rank]), counts scaled as k_aov_finalize scales n_hit; one thread per row-major pixel p.  A
// thread's stores are SLOTS * 4 B apart, so a wave's store of one rank touches SLOTS times the lines a planar layout would; accepted:
// the kernel runs once per frame at 4.6 TB/s as it stands ("Id mattes").
template <uint32_t SLOTS>
__global__ void __launch_bounds__(256) k_matte_finalize(const uint32_t* state, uint32_t n_pixels, uint32_t w, uint32_t tiles8_per_row, float inv_spp,
                                                        uint32_t* ids, float* coverage, float* residual) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    const uint32_t q = order_of_pixel(p, w, tiles8_per_row);
    unsigned long long e[SLOTS];
#pragma unroll
    for (uint32_t r = 0; r < SLOTS; ++r) {
        const uint32_t cnt = state[(size_t)(2u * r + 1u) * n_pixels + q];
        const uint32_t id = cnt ? state[(size_t)(2u * r) * n_pixels + q] : 0xffffffffu;
        e[r] = (unsigned long long)cnt << 32 | (unsigned long long)~id;
    }
    matte_sort<SLOTS>(e);
#pragma unroll
    for (uint32_t r = 0; r < SLOTS; ++r) {
        ids[(size_t)p * SLOTS + r] = ~(uint32_t)e[r];
        coverage[(size_t)p * SLOTS + r] = (float)(uint32_t)(e[r] >> 32) * inv_spp;
    }
    if (residual) residual[p] = (float)state[(size_t)(2u * SLOTS) * n_pixels + q] * inv_spp;
}

// The mask of a set of ids: one thread per pixel; the block stages the selected ids (strictly ascending, n_select * 4 B of dynamic
// LDS) once, a thread looks each of its ranks up by binary search and sums the coverages of the selected ones in rank order from +0.
__global__ void __launch_bounds__(256) k_matte_mask(const uint32_t* ids, const float* coverage, const uint32_t* select, uint32_t n_select, uint32_t n_pixels,
                                                    uint32_t slots, float* mask) {
    extern __shared__ uint32_t matte_sel[];
    for (uint32_t i = threadIdx.x; i < n_select; i += blockDim.x) matte_sel[i] = select[i];
    __syncthreads();
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    float m = 0.0f;
    for (uint32_t r = 0; r < slots; ++r) {
        const uint32_t v = ids[(size_t)p * slots + r];
        uint32_t lo = 0u, hi = n_select;  // the first selected id >= v is in [lo, hi]
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (matte_sel[mid] < v) lo = mid + 1u;
            else hi = mid;
        }
        if (lo < n_select && matte_sel[lo] == v) m = m + coverage[(size_t)p * slots + r];
    }
    mask[p] = m;
}
