"""The motion-blur call (include/pbrs_gpu.h, "motion blur") as numpy f32: the header's text tap by tap.  The gather is an explicit loop
over the taps i = 0 .. S - 1 in the stated order, one f32 operation at a time (a multiply, then an add: numpy fuses nothing); the
arrays only hold all pixels at once, which changes no pixel's operations: a pixel that leaves a tap out keeps its sums through
np.where, it does not add a zero.  The dominant velocity of a tile is the first largest ll of its window in row-major order, which is
the lowest y * w + x.  There is no np.sum, no dot product and no f64 anywhere."""
from types import SimpleNamespace

import numpy as np

f32 = np.float32
MAX_RADIUS = 16
TILE = 16
JITTER = 1
BAYER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], dtype=np.float32)  # the display transform's M[y & 3][x & 3]
DEFAULTS = dict(max_radius=16, taps=16, jitter=False, shutter=0.5, z_rel=0.05)


def finite_pixels(rgb):
    """(h, w) bool: every channel passes pn_isfinite."""
    return np.isfinite(rgb).all(axis=2)


def velocity(motion, max_radius, shutter):
    """Step 1 on every pixel of the (h, w, 2) motion AOV -> v (h, w, 2), ll (h, w), len (h, w), all f32."""
    m, R, k = np.asarray(motion, f32), f32(max_radius), (f32(shutter) * f32(0.5)).astype(f32)
    with np.errstate(all="ignore"):
        ok = np.isfinite(m).all(axis=2)
        v = np.where(ok[..., None], (m * k).astype(f32), f32(0)).astype(f32)
        ll = ((v[..., 0] * v[..., 0]).astype(f32) + (v[..., 1] * v[..., 1]).astype(f32)).astype(f32)
        ln = np.sqrt(ll, dtype=f32)
        fast = ln > R
        s = (R / np.where(fast, ln, f32(1))).astype(f32)
        vc = (v * s[..., None]).astype(f32)
        llc = ((vc[..., 0] * vc[..., 0]).astype(f32) + (vc[..., 1] * vc[..., 1]).astype(f32)).astype(f32)
        lnc = np.sqrt(llc, dtype=f32)
        lnc = np.where(lnc < R, lnc, R).astype(f32)
    v = np.where(fast[..., None], vc, v).astype(f32)
    return v, np.where(fast, llc, ll).astype(f32), np.where(fast, lnc, ln).astype(f32)


def dominant(v, ll, ln, max_radius):
    """Step 2 -> per tile (rows, cols): vn (rows, cols, 2), its len (rows, cols) and the winner's row-major index (rows, cols)."""
    h, w = ll.shape
    R = int(max_radius)
    rows, cols = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
    vn, vl, idx = np.zeros((rows, cols, 2), f32), np.zeros((rows, cols), f32), np.zeros((rows, cols), np.int64)
    for ty in range(rows):
        for tx in range(cols):
            y0, y1 = max(ty * TILE - R, 0), min(ty * TILE + TILE + R, h)
            x0, x1 = max(tx * TILE - R, 0), min(tx * TILE + TILE + R, w)
            win = ll[y0:y1, x0:x1]
            k = int(np.argmax(win))  # the first of the largest in row-major order: the lowest y * w + x
            y, x = y0 + k // (x1 - x0), x0 + k % (x1 - x0)
            vn[ty, tx], vl[ty, tx], idx[ty, tx] = v[y, x], ln[y, x], y * w + x
    return vn, vl, idx


def _cyl(dist, length):
    c = ((length - dist).astype(f32) + f32(0.5)).astype(f32)
    c = np.where(c > 0, c, f32(0)).astype(f32)
    return np.where(c < 1, c, f32(1)).astype(f32)


def motion_blur(rgb, depth, motion, max_radius=16, taps=16, jitter=False, shutter=0.5, z_rel=0.05, details=False):
    """pbrsm_motion_blur on the (h, w, 3) f32 image, the (h, w) f32 depth and the (h, w, 2) f32 motion AOV -> the (h, w, 3) f32 image,
    or with `details` a namespace of out, velocity (step 4), len, vn and vn_len per pixel (its tile's), winner (per tile, the row-major
    index of the pixel that gave vn), n (a pixel's counted taps), front (taps with f == 1), behind (taps with f == 0), between (taps
    with 0 < f < 1) and partial (taps with wgt < 1)."""
    rgb, depth, motion = np.ascontiguousarray(rgb, f32), np.ascontiguousarray(depth, f32), np.ascontiguousarray(motion, f32)
    h, w, _ = rgb.shape
    assert depth.shape == (h, w) and motion.shape == (h, w, 2) and 1 <= max_radius <= MAX_RADIUS and 2 <= taps <= 64
    R, S = int(max_radius), int(taps)
    zero = np.zeros((h, w), np.int32)
    if f32(shutter) == 0:  # step 0
        res = SimpleNamespace(out=rgb.copy(), velocity=np.zeros((h, w, 2), f32), len=np.zeros((h, w), f32), vn=np.zeros((h, w, 2), f32),
                              vn_len=np.zeros((h, w), f32), winner=None, n=zero, front=zero.copy(), behind=zero.copy(), between=zero.copy(),
                              partial=zero.copy())
        return res if details else res.out
    v, ll, ln = velocity(motion, R, shutter)
    tvn, tvl, winner = dominant(v, ll, ln, R)
    Y, X = np.mgrid[0:h, 0:w]
    vn, vn_len = tvn[Y // TILE, X // TILE], tvl[Y // TILE, X // TILE]
    good = finite_pixels(rgb)
    active = (vn_len > f32(0.5)) & good
    with np.errstate(all="ignore"):
        zeff = np.where(depth > 0, depth, f32(np.inf)).astype(f32)
    j = (((BAYER[Y & 3, X & 3] + f32(0.5)).astype(f32) / f32(16.0)).astype(f32) - f32(0.5)).astype(f32) if jitter else np.zeros((h, w), f32)
    acc = np.zeros((h, w, 3), f32)
    W = np.zeros((h, w), f32)
    n, front, behind, between, partial = (zero.copy() for _ in range(5))
    Sf, zr, one = f32(S), f32(z_rel), f32(1)
    clean = np.where(good[..., None], rgb, f32(0))
    with np.errstate(all="ignore"):
        den = (zr * zeff).astype(f32)
        for i in range(S):
            t = (((((f32(i) + f32(0.5)).astype(f32) + j).astype(f32) / Sf).astype(f32) * f32(2.0)).astype(f32) - one).astype(f32)
            dx = np.floor(((vn[..., 0] * t).astype(f32) + f32(0.5)).astype(f32)).astype(np.int32)
            dy = np.floor(((vn[..., 1] * t).astype(f32) + f32(0.5)).astype(f32)).astype(np.int32)
            assert (np.abs(dx[active]) <= R).all() and (np.abs(dy[active]) <= R).all()
            qx, qy = X + dx, Y + dy
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            valid = active & inside & ((dx != 0) | (dy != 0)) & good[qy, qx]
            if not valid.any():
                continue
            dist = np.sqrt((dx * dx + dy * dy).astype(f32), dtype=f32)
            zq, lq, cq = zeff[qy, qx], ln[qy, qx], clean[qy, qx]
            level = zq <= zeff
            a = (one - ((zq - zeff).astype(f32) / den).astype(f32)).astype(f32)
            f = np.where(level, one, np.where(a > 0, a, f32(0))).astype(f32)
            wgt = ((f * _cyl(dist, lq)).astype(f32) + ((one - f).astype(f32) * _cyl(dist, ln)).astype(f32)).astype(f32)
            take = valid & (wgt > 0)
            if not take.any():
                continue
            for c in range(3):
                acc[..., c] = np.where(take, (acc[..., c] + (wgt * cq[..., c]).astype(f32)).astype(f32), acc[..., c])
            W = np.where(take, (W + wgt).astype(f32), W)
            n += take
            front += take & (f == one)
            behind += take & (f == 0)
            between += take & (f > 0) & (f < one)
            partial += take & (wgt < one)
        rest = (Sf - W).astype(f32)
        blurred = ((acc + (rest[..., None] * clean).astype(f32)).astype(f32) / Sf).astype(f32)
    out = np.where((n > 0)[..., None], blurred, rgb).astype(f32)
    res = SimpleNamespace(out=out, velocity=v, len=ln, vn=vn, vn_len=vn_len, winner=winner, n=n, front=front, behind=behind, between=between,
                          partial=partial)
    return res if details else res.out
