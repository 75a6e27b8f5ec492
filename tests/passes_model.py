"""Numpy f32 model of the light passes, written from the text of include/pbrs_gpu.h ("light passes") alone: per-sample radiances after
the first path vertex (D_i) and at full depth (L_i) in, the four buffers and the combined image out.  Sequential over the samples in
sample-index order, vectorised over the pixels; the variance recipe is the variance AOV's (tests/denoise_var_model.py)."""
import numpy as np

import denoise_var_model as vm

f32 = np.float32


def indirect_samples(D, L):
    """I_i = L_i - D_i per component, for (spp, h, w, 3) f32 arrays."""
    with np.errstate(all="ignore"):
        return (np.asarray(L, dtype=f32) - np.asarray(D, dtype=f32)).astype(f32)


def mean(samples):
    """(sum_i x_i, i ascending, from +0) * (1.0f / spp) of a (spp, h, w, 3) f32 array."""
    samples = np.asarray(samples, dtype=f32)
    s = np.zeros(samples.shape[1:], dtype=f32)
    with np.errstate(all="ignore"):
        for x in samples:
            s = (s + x).astype(f32)
        return (s * (f32(1.0) / f32(len(samples)))).astype(f32)


def passes(D, L):
    """The four buffers of pbrs_pass_buffers from the per-sample D_i and L_i, each (spp, h, w, 3) f32."""
    D = np.asarray(D, dtype=f32)
    ind = indirect_samples(D, L)
    return {"direct": mean(D), "indirect": mean(ind), "direct_variance": vm.variance(D), "indirect_variance": vm.variance(ind)}


def combine(direct, indirect):
    with np.errstate(all="ignore"):
        return (np.asarray(direct, dtype=f32) + np.asarray(indirect, dtype=f32)).astype(f32)


def combine_bound(D, L):
    """The header's "only to rounding": per component 4 * spp * 2^-24 * mean_i(|L_i| + |D_i|) bounds |direct + indirect - image| — three
    sums of spp terms and one subtraction per sample, each within one ulp of its operands."""
    D, L = np.asarray(D, dtype=np.float64), np.asarray(L, dtype=np.float64)
    spp = len(D)
    return 4.0 * spp * 2.0 ** -24 * (np.abs(L) + np.abs(D)).mean(axis=0)
