"""The numpy model of pbrsx_compare (include/pbrs_gpu.h, "image comparison"), written from the header's text: f32 fields, f64 terms, and
every sum in the contract's order, the adjacent-pair tree inside each 16 x 16 tile and then over the tile sums.  numpy's f32 and f64
arithmetic is IEEE without fused multiply-add, so the 64 bytes of `record()` and the maps are the device's bit for bit."""
import struct

import numpy as np

TILE = 16
LINEAR, REINHARD = 0, 1
F32, F64 = np.float32, np.float64
G = np.array([np.exp(-k * k / 4.5) for k in range(6)]).astype(F32)  # the header's PBRS_COMPARE_G0 .. G5 (test_compare_model.py)
NAN = np.uint32(0x7FC00000).view(F32)
LUM = (F32(0.21267127), F32(0.71515972), F32(0.07216883))


def transform(x, kind):
    x = np.asarray(x, dtype=F32)
    if kind == LINEAR:
        return x
    with np.errstate(all="ignore"):
        xp = np.where(x < 0, F32(0), x)
        return xp / (F32(1) + xp)


def luminance(c):
    return (LUM[0] * c[..., 0] + LUM[1] * c[..., 1]) + LUM[2] * c[..., 2]


def pair_tree(v):
    """The adjacent-pair tree along the last axis, whose length is a power of two."""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def tile_sums(field):
    """(h, w) f64 -> the sum of every TILE x TILE tile, row-major over tiles, positions outside the image as +0.0."""
    h, w = field.shape
    th, tw = -(-h // TILE), -(-w // TILE)
    padded = np.zeros((th * TILE, tw * TILE), dtype=F64)
    padded[:h, :w] = field
    return pair_tree(padded.reshape(th, TILE, tw, TILE).transpose(0, 2, 1, 3).reshape(th * tw, TILE * TILE))


def ordered_sum(field):
    """T(v) of the header."""
    sums = tile_sums(np.asarray(field, dtype=F64))
    padded = np.zeros(1 << (len(sums) - 1).bit_length(), dtype=F64)
    padded[:len(sums)] = sums
    return pair_tree(padded)


def window_pass(v, axis):
    """One pass of the 11-tap filter along `axis` of an (h, w) f32 field; taps outside the image are zeros, which a sum that starts at
    +0 does not feel."""
    n = v.shape[axis]
    pad = [(0, 0), (0, 0)]
    pad[axis] = (5, 5)
    padded = np.pad(v, pad)
    acc = np.zeros_like(v)
    for j in range(11):
        acc = acc + G[abs(j - 5)] * np.take(padded, range(j, j + n), axis=axis)
    return acc


def window(v):
    return window_pass(window_pass(np.asarray(v, dtype=F32), 1), 0)


def ssim_map(ta, tb, valid, peak):
    """ssim(p) as f32 wherever it can be computed (garbage at invalid pixels: the caller masks them)."""
    x, y = np.where(valid, luminance(ta), F32(0)), np.where(valid, luminance(tb), F32(0))
    m = valid.astype(F32)
    with np.errstate(all="ignore"):
        W, Sx, Sy, Sxx, Syy, Sxy = (window(f) for f in (m, x, y, x * x, y * y, x * y))
        iw = F32(1) / W
        mx, my = Sx * iw, Sy * iw
        sxx, syy, sxy = Sxx * iw - mx * mx, Syy * iw - my * my, Sxy * iw - mx * my
        peak = F32(peak)
        C1, C2 = (F32(0.01) * peak) * (F32(0.01) * peak), (F32(0.03) * peak) * (F32(0.03) * peak)
        s = ((F32(2) * (mx * my) + C1) * (F32(2) * sxy + C2)) / (((mx * mx + my * my) + C1) * ((sxx + syy) + C2))
    assert s.dtype == F32
    return s


def compare(a, b, transform_kind=REINHARD, ssim=True, rel_epsilon=1e-2, peak=1.0):
    """-> dict of the result's fields, plus "error_map" and "ssim_map" ((h, w) f32; the latter None without ssim) and "se", the per-pixel
    f64 terms."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    assert a.shape == b.shape and a.ndim == 3 and a.shape[2] == 3
    valid = np.isfinite(a).all(axis=2) & np.isfinite(b).all(axis=2)
    ta, tb = transform(a, transform_kind), transform(b, transform_kind)
    with np.errstate(all="ignore"):
        A, B = ta.astype(F64), tb.astype(F64)
        D = A - B
        eps = F64(F32(rel_epsilon))
        R = D * D / (B * B + eps)
        se = np.where(valid, (D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2], 0.0)
        ae = np.where(valid, (np.abs(D[..., 0]) + np.abs(D[..., 1])) + np.abs(D[..., 2]), 0.0)
        re = np.where(valid, (R[..., 0] + R[..., 1]) + R[..., 2], 0.0)
        n_valid = int(valid.sum())
        n3 = F64(3 * n_valid)
        out = {"mse": ordered_sum(se) / n3, "rel_mse": ordered_sum(re) / n3, "mae": ordered_sum(ae) / n3, "ssim": F64(0.0),
               "max_abs": F64(np.abs(D)[valid].max()) if n_valid else F64(0.0), "n_valid": n_valid, "n_invalid": int((~valid).sum()), "n_ssim": 0,
               "se": se, "error_map": np.where(valid, se.astype(F32), NAN), "ssim_map": None}
        if ssim:
            s = ssim_map(ta, tb, valid, peak)
            kept = valid & np.isfinite(s)
            out["n_ssim"] = int(kept.sum())
            out["ssim"] = ordered_sum(np.where(kept, s.astype(F64), 0.0)) / F64(out["n_ssim"])
            out["ssim_map"] = np.where(valid, s, NAN)
    return out


FIELDS = ("mse", "rel_mse", "mae", "ssim", "max_abs", "n_valid", "n_invalid", "n_ssim")


def record(r):
    """The 64 bytes of pbrs_compare_result."""
    return struct.pack("<5d6I", *(r[n] for n in FIELDS), 0, 0, 0)
