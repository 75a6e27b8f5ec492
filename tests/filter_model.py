"""CPU model of the filtered film (include/pbrs_gpu.h, pbrs_render_tile_filtered), written from the header's text in numpy f32:
the factors of include/pbrs_filter.h, vectorised over pixels, and the fold over sample index, dy, dx in the prescribed order.
The transcendentals and pn_fract go through the oracle's include/pbrs_numeric.h (oracle.binding.numeric_eval), the jitter
through its RNG (oracle.binding.rng_stream); every constant is an f32 so that numpy never widens to f64."""
import numpy as np

from oracle.binding import numeric_eval, rng_stream

f32 = np.float32
BOX, TRIANGLE, GAUSSIAN, MITCHELL, LANCZOS = range(5)
PI = f32(3.14159265358979323846)
ZERO = f32(0.0)


def _max0(x):
    """pn_max(x, 0.0f) for non-NaN x: x > 0 ? x : +0."""
    return np.where(x > ZERO, x, ZERO).astype(f32)


def _exp(x):
    return numeric_eval("exp", np.asarray(x, dtype=f32))


def _sinc(x):
    x = np.asarray(x, dtype=f32)
    px = (PI * x).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (numeric_eval("sin", px) / px).astype(f32)
    return np.where(np.abs(x) < f32(1e-5), f32(1.0), v).astype(f32)


def factor(kind, o, r, a=0.0, b=0.0):
    """One axis's factor at offsets o (array), radius r."""
    o = np.asarray(o, dtype=f32)
    r, a, b = f32(r), f32(a), f32(b)
    if kind == BOX:
        return np.ones_like(o)
    if kind == TRIANGLE:
        return _max0(r - np.abs(o))
    if kind == GAUSSIAN:
        return _max0(_exp((-a * o) * o) - _exp(np.full_like(o, (-a * r) * r)))
    if kind == MITCHELL:
        x = np.abs(f32(2.0) * (o / r))
        big = x > f32(1.0)
        c0 = np.where(big, f32(8.0) * a + f32(24.0) * b, f32(6.0) - f32(2.0) * a)
        c1 = np.where(big, f32(-12.0) * a - f32(48.0) * b, f32(0.0))
        c2 = np.where(big, f32(6.0) * a + f32(30.0) * b, f32(-18.0) + f32(12.0) * a + f32(6.0) * b)
        c3 = np.where(big, -a - f32(6.0) * b, f32(12.0) - f32(9.0) * a - f32(6.0) * b)
        d = np.zeros_like(x)
        for c in (c3, c2, c1, c0):
            d = (d * x + c).astype(f32)
        return (f32(1.0) / f32(6.0)) * d
    if kind == LANCZOS:
        ao = np.abs(o)
        return (_sinc(ao / a) * _sinc(ao)).astype(f32)
    raise ValueError(kind)


def halo(r):
    return int(np.floor(f32(r) + f32(0.5)))


def sample_positions(seed, width, region, i, strata_x, strata_y):
    """(xs, ys) of sample index i for every pixel of region (x0, y0, w, h): k_raygen's jitter."""
    x0, y0, w, h = region
    xs = np.empty((h, w), dtype=f32)
    ys = np.empty((h, w), dtype=f32)
    jx = np.empty((h, w), dtype=f32)
    jy = np.empty((h, w), dtype=f32)
    for y in range(h):
        for x in range(w):
            r0, r1 = rng_stream(seed, (y0 + y) * width + (x0 + x), i, 2)
            jx[y, x] = (f32(i // strata_y) + r0) / f32(strata_x)
            jy[y, x] = (f32(i % strata_y) + r1) / f32(strata_y)
    cols = np.arange(x0, x0 + w, dtype=np.int64)[None, :].astype(f32)
    rows = np.arange(y0, y0 + h, dtype=np.int64)[:, None].astype(f32)
    xs[:] = cols + numeric_eval("fract", jx)
    ys[:] = rows + numeric_eval("fract", jy)
    return xs, ys


def region_of(tile, film, pf):
    """The tile plus its halo, clipped to the film (width, height)."""
    x0, y0, w, h = tile
    hx, hy = halo(pf[1]), halo(pf[2])
    rx0, ry0 = max(x0 - hx, 0), max(y0 - hy, 0)
    return rx0, ry0, min(x0 + w + hx, film[0]) - rx0, min(y0 + h + hy, film[1]) - ry0


def filtered(pf, tile, film, seed, strata_x, strata_y, radiance):
    """The filtered tile.  pf = (kind, rx, ry, a, b); film = (width, height); radiance(i, region) -> (h, w, 3) f32 radiance of
    sample index i over the region.  Returns (h, w, 3) f32."""
    kind, rx, ry, a, b = pf
    rx, ry = f32(rx), f32(ry)
    x0, y0, w, h = tile
    hx, hy = halo(rx), halo(ry)
    region = region_of(tile, film, pf)
    gx0, gy0, gw, gh = region
    S = np.zeros((h, w, 3), dtype=f32)
    W = np.zeros((h, w), dtype=f32)
    px = np.arange(x0, x0 + w)[None, :].repeat(h, 0)
    py = np.arange(y0, y0 + h)[:, None].repeat(w, 1)
    for i in range(strata_x * strata_y):
        L = radiance(i, region)
        xs, ys = sample_positions(seed, film[0], region, i, strata_x, strata_y)
        for dy in range(-hy, hy + 1):
            for dx in range(-hx, hx + 1):
                qx, qy = px + dx, py + dy
                inside = (qx >= gx0) & (qx < gx0 + gw) & (qy >= gy0) & (qy < gy0 + gh)
                ix, iy = np.clip(qx - gx0, 0, gw - 1), np.clip(qy - gy0, 0, gh - 1)
                ox = xs[iy, ix] - (px.astype(f32) + f32(0.5))
                oy = ys[iy, ix] - (py.astype(f32) + f32(0.5))
                use = inside & (np.abs(ox) <= rx) & (np.abs(oy) <= ry)
                wgt = (factor(kind, ox, rx, a, b) * factor(kind, oy, ry, a, b)).astype(f32)
                with np.errstate(invalid="ignore", over="ignore"):
                    add = S + wgt[..., None] * L[iy, ix]
                S = np.where(use[..., None], add, S).astype(f32)
                W = np.where(use, W + wgt, W).astype(f32)
    out = np.zeros((h, w, 3), dtype=f32)
    nz = W != f32(0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = S * (f32(1.0) / W)[..., None]
    v = np.where(v < f32(0.0), f32(0.0), v)
    out[nz] = v[nz]
    return out
