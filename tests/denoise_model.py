"""CPU model of the denoiser (include/pbrs_gpu.h, pbrs_denoise), written from the header's text in numpy f32, vectorised over the
pixels and sequential over iterations and taps in the prescribed order (dy outer, dx inner).  pn_exp goes through the oracle's
include/pbrs_numeric.h (oracle.binding.numeric_eval); every constant is an f32 so that numpy never widens to f64."""
import numpy as np

from oracle.binding import numeric_eval

f32 = np.float32
ZERO, ONE = f32(0.0), f32(1.0)
K = (f32(0.375), f32(0.25), f32(0.0625))  # the B3 spline
DEMODULATE, ID_STOP = 1, 2
MAX_ITERATIONS = 6


def _exp(x):
    return numeric_eval("exp", np.ascontiguousarray(x, dtype=f32)).reshape(np.shape(x))


def _finite(c):
    """pn_isfinite of every channel -> (h, w) bool."""
    return np.isfinite(c).all(axis=2)


def _d2(e):
    return ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).astype(f32)


def divisor(albedo, albedo_floor, flags, shape):
    """d of the header's demodulation: (h, w, 3)."""
    if not flags & DEMODULATE:
        return np.ones(shape, dtype=f32)
    a = np.asarray(albedo, dtype=f32)
    return np.where(a > f32(albedo_floor), a, ONE).astype(f32)


def iteration(c, k, sigma_color, sigma_normal, sigma_depth, normal=None, depth=None, instance=None):
    """c_{k+1} from c_k (h, w, 3).  `instance` given = the id stop is on."""
    h, w, _ = c.shape
    s = 1 << k
    sc = f32(sigma_color) * f32(2.0 ** -k)  # pn_exp2i(-k)
    ic = ONE / (sc * sc)
    inn = ONE / (f32(sigma_normal) * f32(sigma_normal))
    idd = ONE / (f32(sigma_depth) * f32(sigma_depth))
    S = np.zeros((h, w, 3), dtype=f32)
    W = np.zeros((h, w), dtype=f32)
    px = np.arange(w)[None, :].repeat(h, 0)
    py = np.arange(h)[:, None].repeat(w, 1)
    fin = _finite(c)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qx, qy = px + s * dx, py + s * dy
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                ix, iy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                cq = c[iy, ix]
                use = inside & fin[iy, ix]
                hw = K[abs(dx)] * K[abs(dy)]
                wgt = (hw * _exp(-_d2(cq - c) * ic)).astype(f32)
                if normal is not None:
                    wgt = (wgt * _exp(-_d2(normal[iy, ix] - normal) * inn)).astype(f32)
                else:
                    wgt = wgt * ONE
                if depth is not None:
                    zp, zq = depth, depth[iy, ix]
                    r = (((zq - zp) / zp) / f32(s)).astype(f32)
                    wd = _exp(-(r * r) * idd)
                    pinf, qinf = np.isinf(zp), np.isinf(zq)
                    wd = np.where(pinf & qinf, ONE, np.where(pinf | qinf, ZERO, wd)).astype(f32)
                    wgt = (wgt * wd).astype(f32)
                else:
                    wgt = wgt * ONE
                if instance is not None:
                    wgt = np.where(instance[iy, ix] != instance, ZERO, wgt).astype(f32)
                use = use & ~np.isnan(wgt)
                add = (S + wgt[..., None] * cq).astype(f32)
                S = np.where(use[..., None], add, S).astype(f32)
                W = np.where(use, W + wgt, W).astype(f32)
        out = (S * (ONE / W)[..., None]).astype(f32)
    through = ~fin | (W == ZERO)
    return np.where(through[..., None], c, out).astype(f32)


def denoise(rgb, iterations, sigma_color, sigma_normal, sigma_depth, albedo_floor=0.0, flags=0, albedo=None, normal=None, depth=None,
            instance=None):
    """pbrs_denoise on (h, w, 3) f32 `rgb` with the given guides (None = NULL) -> (h, w, 3) f32."""
    rgb = np.asarray(rgb, dtype=f32)
    assert 1 <= iterations <= MAX_ITERATIONS
    normal = None if normal is None else np.asarray(normal, dtype=f32)
    depth = None if depth is None else np.asarray(depth, dtype=f32)
    ids = np.asarray(instance, dtype=np.uint32) if (flags & ID_STOP) else None
    d = divisor(albedo, albedo_floor, flags, rgb.shape)
    with np.errstate(all="ignore"):
        c = (rgb / d).astype(f32) if flags & DEMODULATE else rgb.copy()
        for k in range(iterations):
            c = iteration(c, k, sigma_color, sigma_normal, sigma_depth, normal, depth, ids)
        return (c * d).astype(f32) if flags & DEMODULATE else c
