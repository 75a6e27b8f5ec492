"""CPU model of the variance AOV and of the variance-guided denoiser (include/pbrs_gpu.h, pbrs_render_tile_aovs_var and
pbrs_denoise_var), written from the header's text in numpy f32 like tests/denoise_model.py, whose taps, spline and guide stops it
shares: vectorised over the pixels, sequential over samples, iterations and taps in the prescribed order.  Division and square root
are numpy's (IEEE, correctly rounded, what the device computes); pn_exp goes through the oracle's include/pbrs_numeric.h."""
import numpy as np

import denoise_model as dm
from denoise_model import DEMODULATE, ID_STOP, K, MAX_ITERATIONS, ONE, ZERO, _d2, _exp, _finite, f32  # noqa: F401

INF = f32(np.inf)
TINY = np.finfo(f32).tiny  # the smallest normal f32
G = (f32(0.25), f32(0.125), f32(0.0625))  # the 3 x 3 prefilter: centre, edge, corner


def lum(c):
    return ((f32(0.21267127) * c[..., 0] + f32(0.71515972) * c[..., 1]) + f32(0.07216883) * c[..., 2]).astype(f32)


def variance(samples):
    """The variance AOV of a (spp, h, w, 3) f32 array of per-sample radiances -> (h, w) f32."""
    samples = np.asarray(samples, dtype=f32)
    m1 = np.zeros(samples.shape[1:3], dtype=f32)
    m2 = np.zeros_like(m1)
    n = np.zeros(m1.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        for L in samples:
            y = lum(L)
            fin = np.isfinite(y)
            m1 = np.where(fin, m1 + y, m1).astype(f32)
            m2 = np.where(fin, m2 + y * y, m2).astype(f32)
            n = n + fin
        nn = np.maximum(n, 2)
        inv_n = (ONE / nn.astype(f32)).astype(f32)
        mean = (m1 * inv_n).astype(f32)
        v = (m2 * inv_n - mean * mean).astype(f32)
        v = np.where(v < ZERO, ZERO, v).astype(f32)
        out = (v * (ONE / (nn - 1).astype(f32)).astype(f32)).astype(f32)
    return np.where(n < 2, INF, out).astype(f32)


def _no_denormal(x, where, what):
    """The header's condition for exact scale invariance: no scale-dependent product among the denormals."""
    a = np.abs(x)
    bad = (a > 0) & (a < TINY) & where
    assert not bad.any(), f"{what}: {int(bad.sum())} nonzero value(s) below the smallest normal f32"


def pack(rgb, var, albedo, albedo_floor, flags):
    """-> d (h, w, 3), ld2 (h, w) or None, c_0, v_0."""
    d = dm.divisor(albedo, albedo_floor, flags, rgb.shape)
    with np.errstate(all="ignore"):
        vin = np.where(np.isnan(var) | (var < ZERO), INF, var).astype(f32)
        if flags & DEMODULATE:
            c = (rgb / d).astype(f32)
            ld = lum(d)
            ld2 = (ld * ld).astype(f32)
            v = (vin / ld2).astype(f32)
            v = np.where(np.isnan(v), INF, v).astype(f32)
        else:
            c, ld2, v = rgb.copy(), None, vin
    return d, ld2, c, np.where(_finite(c), v, INF).astype(f32)


def iteration(c, v, k, sigma_luminance, sigma_normal, sigma_depth, normal=None, depth=None, instance=None, strict=False):
    """(c_{k+1}, v_{k+1}) from (c_k, v_k).  `instance` given = the id stop is on.  `strict`: assert the header's no-denormal condition."""
    h, w, _ = c.shape
    s = 1 << k
    inn = ONE / (f32(sigma_normal) * f32(sigma_normal))
    idd = ONE / (f32(sigma_depth) * f32(sigma_depth))
    px = np.arange(w)[None, :].repeat(h, 0)
    py = np.arange(h)[:, None].repeat(w, 1)
    fin = _finite(c)
    everywhere = np.ones((h, w), dtype=bool)
    with np.errstate(all="ignore"):
        A = np.zeros((h, w), dtype=f32)
        B = np.zeros((h, w), dtype=f32)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                qx, qy = px + dx, py + dy
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                vn = v[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]
                ok = inside & np.isfinite(vn)
                g = G[abs(dx) + abs(dy)]
                if strict:
                    _no_denormal(g * vn, ok, "G * v")
                A = np.where(ok, A + g * vn, A).astype(f32)
                B = np.where(ok, B + g, B).astype(f32)
        vbar = np.where(B == ZERO, INF, A * (ONE / B)).astype(f32)
        sd = (f32(sigma_luminance) * np.sqrt(vbar)).astype(f32)
        if strict:
            _no_denormal(vbar, everywhere, "vbar")
            _no_denormal(sd, everywhere, "sd")
        lp = lum(c)
        S = np.zeros((h, w, 3), dtype=f32)
        W = np.zeros((h, w), dtype=f32)
        V = np.zeros((h, w), dtype=f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qx, qy = px + s * dx, py + s * dy
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                ix, iy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                cq, vq = c[iy, ix], v[iy, ix]
                use = inside & fin[iy, ix]
                hw = K[abs(dx)] * K[abs(dy)]
                dl = np.abs(lum(cq) - lp).astype(f32)
                wl = np.where(np.isinf(sd), ONE, np.where(sd == ZERO, np.where(dl == ZERO, ONE, ZERO), _exp(-(dl / sd)))).astype(f32)
                wgt = (hw * wl).astype(f32)
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
                use = use & ~np.isnan(wgt) & fin  # (a pixel whose own colour is not finite passes through: its sums are not used)
                ww = (wgt * wgt).astype(f32)
                open_ = use & (ww != ZERO)
                if strict:
                    _no_denormal(dl, use, "dl")
                    _no_denormal(wgt[..., None] * cq, use[..., None], "wgt * c")
                    _no_denormal(ww * vq, open_, "ww * v")
                S = np.where(use[..., None], S + wgt[..., None] * cq, S).astype(f32)
                W = np.where(use, W + wgt, W).astype(f32)
                V = np.where(open_, V + ww * vq, V).astype(f32)
        iw = (ONE / W).astype(f32)
        out = (S * iw[..., None]).astype(f32)
        vout = (V * (iw * iw)).astype(f32)
        through = ~fin | (W == ZERO)
        if strict:
            _no_denormal(out, ~through[..., None], "S * iw")
            _no_denormal(vout, ~through, "V * (iw * iw)")
        vout = np.where(np.isnan(vout), INF, vout).astype(f32)
        vout = np.where(_finite(out), vout, INF).astype(f32)
    return np.where(through[..., None], c, out).astype(f32), np.where(through, v, vout).astype(f32)


def denoise_var(rgb, var, iterations, sigma_luminance, sigma_normal, sigma_depth, albedo_floor=0.0, flags=0, albedo=None, normal=None,
                depth=None, instance=None, strict=False):
    """pbrs_denoise_var on (h, w, 3) f32 `rgb`, (h, w) f32 `var` and the given guides (None = NULL) -> (out (h, w, 3), variance_out (h, w))."""
    rgb = np.asarray(rgb, dtype=f32)
    var = np.asarray(var, dtype=f32)
    assert 1 <= iterations <= MAX_ITERATIONS
    normal = None if normal is None else np.asarray(normal, dtype=f32)
    depth = None if depth is None else np.asarray(depth, dtype=f32)
    ids = np.asarray(instance, dtype=np.uint32) if (flags & ID_STOP) else None
    d, ld2, c, v = pack(rgb, var, albedo, albedo_floor, flags)
    if strict:
        _no_denormal(c, np.ones(c.shape, dtype=bool), "rgb / d")
        _no_denormal(v, np.ones(v.shape, dtype=bool), "v_0")
    for k in range(iterations):
        c, v = iteration(c, v, k, sigma_luminance, sigma_normal, sigma_depth, normal, depth, ids, strict)
    with np.errstate(all="ignore"):
        if flags & DEMODULATE:
            return (c * d).astype(f32), (v * ld2).astype(f32)
    return c, v


def variance_plane(rgb, seed):
    """A variance for a synthetic image: (a share of the luminance)^2, with everything the header has a rule for planted: a block of
    zeros (a closed stop), +inf (unknown), a NaN and a negative value (both count as +inf)."""
    rng = np.random.default_rng(seed)
    h, w, _ = rgb.shape
    with np.errstate(all="ignore"):
        y = np.nan_to_num(lum(np.asarray(rgb, dtype=f32)), nan=1.0, posinf=1.0, neginf=1.0)
        var = ((y * rng.uniform(0.05, 0.5, size=(h, w)).astype(f32)) ** 2).astype(f32)
    if w * h >= 64:
        ys, xs = rng.integers(0, h - 3, size=6), rng.integers(0, w - 3, size=6)
        var[ys[0]:ys[0] + 4, xs[0]:xs[0] + 4] = 0.0
        var[ys[1]:ys[1] + 2, xs[1]:xs[1] + 3] = np.inf
        var[ys[2], xs[2]] = np.nan
        var[ys[3], xs[3]] = -1.0
        var[ys[4], xs[4]] = 0.0
        var[ys[5], xs[5]] = -np.inf
    return var


def scale_inputs(w, h, seed, level):
    """Inputs for the exact scale-invariance test: a flat colour of the given level with 10 % noise, a variance that matches the noise,
    smooth albedo, normals and depth, ids in blocks, and the exact cases of the variance planted (zeros, +inf, NaN, negative).  The
    luminance contrast between any two pixels stays within a few sd and the guide stops stay near 1, so no weight comes near the
    denormals; the model run with strict=True asserts that."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.array([0.7, 1.0, 1.6], dtype=f32) * f32(level)
    noise = rng.normal(scale=0.1, size=(h, w, 3))
    rgb = (base * (1.0 + np.clip(noise, -0.3, 0.3))).astype(f32)
    albedo = (0.5 + 0.3 * np.sin(xx / 9.0)[..., None] * np.array([1.0, 0.8, 0.6])).astype(f32)
    normal = np.stack([0.1 * np.sin(xx / 11.0), 0.1 * np.cos(yy / 13.0), np.ones((h, w))], axis=2).astype(f32)
    depth = (5.0 + 0.01 * xx + 0.005 * yy).astype(f32)
    instance = ((yy // 16) * 8 + xx // 16).astype(np.uint32)
    var = ((lum(rgb) * f32(0.1)) ** 2).astype(f32)  # the noise above is 10 % of the pixel
    var[3:7, 4:8] = 0.0
    var[h - 4, 2:4] = np.inf
    var[h // 2, w // 2] = np.nan
    var[1, w - 2] = -2.0
    return rgb, var, {"albedo": albedo, "normal": normal, "depth": depth, "instance": instance}
