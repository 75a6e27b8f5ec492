"""CPU model of the spatial variance estimate for pixels with a short history (include/pbrs_gpu.h, pbrs_spatial_variance), written
from the header's text in numpy f32 like tests/temporal_model.py: vectorised over the pixels, sequential over the taps in the
prescribed order (dy outer, dx inner).  pn_exp goes through the oracle's include/pbrs_numeric.h; every constant is an f32."""
import numpy as np

from denoise_model import ONE, ZERO, _d2, _exp, _finite, f32
from denoise_var_model import INF

ID_STOP, ONLY_UNKNOWN = 1, 2
MAX_RADIUS = 3
DEFAULTS = dict(radius=3, sigma_normal=0.3, sigma_depth=0.2, min_temporal=4.0, id_stop=False, only_unknown=False)


def short_pixels(length, min_temporal):
    """n > 0 && n < min_temporal; a NaN length is not short."""
    length = np.asarray(length, dtype=f32)
    with np.errstate(invalid="ignore"):
        return (length > ZERO) & (length < f32(min_temporal))


def known(variance):
    """Neither NaN, nor < 0, nor +inf."""
    v = np.asarray(variance, dtype=f32)
    with np.errstate(invalid="ignore"):
        return ~(np.isnan(v) | (v < ZERO) | (v == INF))


def spatial_variance(moments, length, variance, depth=None, normal=None, instance=None, details=None, **params):
    """pbrs_spatial_variance -> variance_out (h, w) f32.  Guides given as None are NULL.  `details`: a dict that receives "estimated"
    (the pixels whose variance was replaced) and "W"."""
    pr = dict(DEFAULTS, **params)
    moments = np.asarray(moments, dtype=f32)
    length = np.asarray(length, dtype=f32)
    variance = np.asarray(variance, dtype=f32)
    h, w = length.shape
    assert moments.shape == (h, w, 2) and variance.shape == (h, w)
    radius = int(pr["radius"])
    assert 1 <= radius <= MAX_RADIUS
    if pr["id_stop"]:
        assert instance is not None
    normal = None if normal is None else np.asarray(normal, dtype=f32)
    depth = None if depth is None else np.asarray(depth, dtype=f32)
    ids = np.asarray(instance, dtype=np.uint32) if pr["id_stop"] else None
    inn = ONE / (f32(pr["sigma_normal"]) * f32(pr["sigma_normal"]))
    idd = ONE / (f32(pr["sigma_depth"]) * f32(pr["sigma_depth"]))
    wanted = short_pixels(length, pr["min_temporal"])
    if pr["only_unknown"]:
        wanted &= ~known(variance)
    with np.errstate(all="ignore"):
        valid = (length > ZERO) & _finite(moments)
        M1, M2, W = (np.zeros((h, w), dtype=f32) for _ in range(3))
        px = np.arange(w)[None, :].repeat(h, 0)
        py = np.arange(h)[:, None].repeat(w, 1)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                qx, qy = px + dx, py + dy
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                ix, iy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                use = inside & valid[iy, ix]
                wn = _exp(-_d2(normal[iy, ix] - normal) * inn) if normal is not None else np.ones((h, w), dtype=f32)
                if depth is not None:
                    zp, zq = depth, depth[iy, ix]
                    r = (((zq - zp) / zp) / ONE).astype(f32)  # s = 1
                    wd = _exp(-(r * r) * idd)
                    pinf, qinf = np.isinf(zp), np.isinf(zq)
                    wd = np.where(pinf & qinf, ONE, np.where(pinf | qinf, ZERO, wd)).astype(f32)
                else:
                    wd = np.ones((h, w), dtype=f32)
                wgt = ((ONE * wn) * wd).astype(f32)
                if ids is not None:
                    wgt = np.where(ids[iy, ix] != ids, ZERO, wgt).astype(f32)
                use = use & ~np.isnan(wgt)
                mq = moments[iy, ix]
                M1 = np.where(use, M1 + wgt * mq[..., 0], M1).astype(f32)
                M2 = np.where(use, M2 + wgt * mq[..., 1], M2).astype(f32)
                W = np.where(use, W + wgt, W).astype(f32)
        iw = (ONE / W).astype(f32)
        a, b = (M1 * iw).astype(f32), (M2 * iw).astype(f32)
        v = (b - a * a).astype(f32)
        v = np.where(v < ZERO, ZERO, v).astype(f32)
        v = np.where(np.isnan(v), INF, v).astype(f32)
        est = (v * (ONE / length)).astype(f32)
    estimated = wanted & (W != ZERO)
    if details is not None:
        details["estimated"], details["W"] = estimated, W
    out = variance.copy()  # the pass-through keeps the bits, a NaN's payload included
    out[estimated] = est[estimated]
    return out


def sequence_inputs(w, h, seed, move, frames=3):
    """The inputs of the call as a temporal sequence leaves them: the history tm.run_sequence's model holds after `frames` frames of
    `move`, with what the sequence plants into it (a zero and a NaN length, non-finite moments), the variance rule D wrote beside it and
    the last frame's guides -> dict(moments, length, variance, depth, normal, instance)."""
    import temporal_model as tm
    hist, vout = tm.run_sequence(tm.accumulate, w, h, seed, move, frames=frames)[-1]
    _, frame, plant = list(tm.synthetic_sequence(w, h, seed, move, frames))[-1]
    hist = tm.plant_history(hist, plant)
    return dict(moments=hist["moments"], length=hist["length"], variance=vout, depth=frame["depth"], normal=frame["normal"],
                instance=frame["instance"])
