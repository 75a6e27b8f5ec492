"""CPU model of the guided upsampling (include/pbrs_gpu.h, pbrs_upsample), written from the header's text in numpy f32 like
tests/denoise_model.py: vectorised over the full-size pixels, sequential over the taps in the prescribed order (Y outer, X inner).
pn_exp goes through the oracle's include/pbrs_numeric.h; every constant is an f32 so that numpy never widens to f64."""
import numpy as np

from denoise_model import ONE, ZERO, _d2, _exp, _finite, f32

DEMODULATE, ID_STOP = 1, 2
FACTORS, RADII = (2, 3, 4), (1, 2)
DEFAULTS = dict(radius=1, sigma_normal=0.3, sigma_depth=0.2, albedo_floor=1e-3, min_weight=1e-3, demodulate=False, id_stop=False)


def low_size(w, h, factor):
    return (w + factor - 1) // factor, (h + factor - 1) // factor


def _divisor(albedo, albedo_floor):
    a = np.asarray(albedo, dtype=f32)
    with np.errstate(invalid="ignore"):
        return np.where(a > f32(albedo_floor), a, ONE).astype(f32)


def upsample(rgb_lo, w, h, factor, lo=None, hi=None, details=None, **params):
    """pbrs_upsample -> out (h, w, 3) f32.  `lo`, `hi`: dicts of the guides at the low and at the full size (albedo, normal, depth,
    instance; a missing name or None is NULL).  A guide counts when both give it.  `details`: a dict that receives "W" and "V"."""
    pr = dict(DEFAULTS, **params)
    lo, hi = dict(lo or {}), dict(hi or {})
    f, R = int(factor), int(pr["radius"])
    assert f in FACTORS and R in RADII
    wl, hl = low_size(w, h, f)
    rgb_lo = np.asarray(rgb_lo, dtype=f32)
    assert rgb_lo.shape == (hl, wl, 3), (rgb_lo.shape, (hl, wl, 3))
    for n in ("albedo", "normal", "depth", "instance"):
        assert (lo.get(n) is None) == (hi.get(n) is None), f"{n} given at only one resolution"

    def pair(n, dt):
        if lo.get(n) is None:
            return None, None
        return np.asarray(lo[n], dtype=dt), np.asarray(hi[n], dtype=dt)

    n_lo, n_hi = pair("normal", f32)
    z_lo, z_hi = pair("depth", f32)
    i_lo, i_hi = pair("instance", np.uint32) if pr["id_stop"] else (None, None)
    if pr["id_stop"]:
        assert i_lo is not None
    inn = ONE / (f32(pr["sigma_normal"]) * f32(pr["sigma_normal"]))
    idd = ONE / (f32(pr["sigma_depth"]) * f32(pr["sigma_depth"]))
    with np.errstate(all="ignore"):
        if pr["demodulate"]:
            assert lo.get("albedo") is not None
            d_lo, d_hi = _divisor(lo["albedo"], pr["albedo_floor"]), _divisor(hi["albedo"], pr["albedo_floor"])
            c = (rgb_lo / d_lo).astype(f32)
        else:
            d_hi = np.ones((h, w, 3), dtype=f32)
            c = rgb_lo.copy()
        fin = _finite(c)
        px = np.arange(w, dtype=np.int64)[None, :].repeat(h, 0)
        py = np.arange(h, dtype=np.int64)[:, None].repeat(w, 1)
        X0 = (2 * px + 1 - f) // (2 * f)  # numpy's // floors toward -inf
        Y0 = (2 * py + 1 - f) // (2 * f)
        D = 2 * f * R
        T = np.zeros((h, w, 3), dtype=f32)
        S = np.zeros((h, w, 3), dtype=f32)
        V = np.zeros((h, w), dtype=f32)
        W = np.zeros((h, w), dtype=f32)
        for ty in range(-R + 1, R + 1):
            for tx in range(-R + 1, R + 1):
                X, Y = X0 + tx, Y0 + ty
                nx, ny = np.abs(2 * f * X + f - (2 * px + 1)), np.abs(2 * f * Y + f - (2 * py + 1))
                inside = (X >= 0) & (X < wl) & (Y >= 0) & (Y < hl)
                ix, iy = np.clip(X, 0, wl - 1), np.clip(Y, 0, hl - 1)
                use = inside & (nx < D) & (ny < D) & fin[iy, ix]
                hw = (((D - nx).astype(f32) / f32(D)).astype(f32) * ((D - ny).astype(f32) / f32(D)).astype(f32)).astype(f32)
                cq = c[iy, ix]
                T = np.where(use[..., None], (T + hw[..., None] * cq).astype(f32), T).astype(f32)
                V = np.where(use, V + hw, V).astype(f32)
                wn = _exp(-_d2(n_lo[iy, ix] - n_hi) * inn) if n_lo is not None else np.ones((h, w), dtype=f32)
                if z_lo is not None:
                    zp, zq = z_hi, z_lo[iy, ix]
                    r = (((zq - zp) / zp) / f32(f)).astype(f32)
                    wd = _exp(-(r * r) * idd)
                    pinf, qinf = np.isinf(zp), np.isinf(zq)
                    wd = np.where(pinf & qinf, ONE, np.where(pinf | qinf, ZERO, wd)).astype(f32)
                else:
                    wd = np.ones((h, w), dtype=f32)
                g = ((hw * wn).astype(f32) * wd).astype(f32)
                if i_lo is not None:
                    g = np.where(i_lo[iy, ix] != i_hi, ZERO, g).astype(f32)
                guided = use & ~np.isnan(g)
                S = np.where(guided[..., None], (S + g[..., None] * cq).astype(f32), S).astype(f32)
                W = np.where(guided, W + g, W).astype(f32)
        r_guided = (S * (ONE / W)[..., None]).astype(f32)
        r_tent = (T * (ONE / V)[..., None]).astype(f32)
        r_near = c[py // f, px // f]
        r = np.where((W > f32(pr["min_weight"]))[..., None], r_guided, np.where((V > ZERO)[..., None], r_tent, r_near)).astype(f32)
        out = (r * d_hi).astype(f32)
    if details is not None:
        details["W"], details["V"] = W, V
    return out


def tent(rgb_lo, w, h, factor, radius=1):
    """The call without guides: the plain tent."""
    return upsample(rgb_lo, w, h, factor, radius=radius)


def display_error(out, ref):
    """The display-referred error of the issue: the mean over finite reference pixels of (t(out) - t(ref))^2, t(v) = max(v, 0) / (1 +
    max(v, 0)), in float64."""
    out, ref = np.asarray(out, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ok = np.isfinite(ref).all(axis=2)

    def t(v):
        v = np.maximum(v, 0.0)
        return v / (1.0 + v)
    return float(((t(out[ok]) - t(ref[ok])) ** 2).mean())


def synthetic(w, h, factor, seed, plant=True):
    """Seeded inputs of every kind the header names, at both sizes: a low image with denormal, NaN and +-inf colours, guides with a few
    surfaces (normals, depths with zeros and +inf, ids), albedos with entries below the floor -> (rgb_lo, lo, hi).  Without `plant`
    everything is finite and ordinary."""
    rng = np.random.default_rng(seed)
    wl, hl = low_size(w, h, factor)

    def guides(ww, hh, step):
        yy, xx = np.mgrid[0:hh, 0:ww]
        u, v = (xx + 0.5) * step / max(w, 1), (yy + 0.5) * step / max(h, 1)
        ids = ((u > 0.45).astype(np.uint32) + 2 * (v > 0.6).astype(np.uint32)).astype(np.uint32)
        normal = np.zeros((hh, ww, 3), dtype=f32)
        normal[..., 0] = np.where(ids & 1, 0.6, 0.0)
        normal[..., 1] = np.where(ids & 2, 0.8, 0.0)
        normal[..., 2] = np.sqrt(np.maximum(0.0, 1.0 - normal[..., 0] ** 2 - normal[..., 1] ** 2))
        normal = (normal + rng.normal(0, 0.02, normal.shape)).astype(f32)
        depth = (2.0 + u + 0.5 * v + 1.5 * ids).astype(f32)
        albedo = (0.2 + 0.6 * rng.random((hh, ww, 3))).astype(f32)
        return dict(albedo=albedo, normal=normal, depth=depth, instance=ids)

    lo, hi = guides(wl, hl, factor), guides(w, h, 1)
    rgb_lo = (rng.random((hl, wl, 3)) * 4.0).astype(f32)
    if plant:
        def at(hh, ww, n):
            return rng.integers(0, hh, n), rng.integers(0, ww, n)
        for g, (hh, ww) in ((lo, (hl, wl)), (hi, (h, w))):
            n = max(1, hh * ww // 40)
            for name, value in (("depth", 0.0), ("depth", np.inf), ("depth", np.nan)):
                ys, xs = at(hh, ww, n)
                g[name][ys, xs] = value
            ys, xs = at(hh, ww, n)
            g["normal"][ys, xs, 0] = np.nan
            ys, xs = at(hh, ww, n)
            g["albedo"][ys, xs, rng.integers(0, 3, n)] = 5e-4  # below the default floor
            ys, xs = at(hh, ww, n)
            g["albedo"][ys, xs, 1] = np.nan
        n = max(1, hl * wl // 30)
        for value in (np.nan, np.inf, -np.inf, 1e-41, -3e-39):  # non-finite and denormal colours
            ys, xs = at(hl, wl, n)
            rgb_lo[ys, xs, rng.integers(0, 3, n)] = value
    return rgb_lo, lo, hi
