"""The depth-of-field call (include/pbrs_gpu.h, "depth of field") as numpy f32: the header's text tap by tap.  The gather is an explicit
loop over the taps in the stated order (dy outer, dx inner), one f32 operation at a time (a multiply, then an add: numpy fuses nothing);
the arrays only hold all pixels at once, which changes no pixel's operations: a pixel that leaves a tap out keeps its sums through
np.where, it does not add a zero.  There is no np.sum, no dot product and no f64 anywhere."""
from types import SimpleNamespace

import numpy as np

f32 = np.float32
MAX_RADIUS = 16
DEFAULTS = dict(max_radius=8, focus=1.0, scale=0.0)


def finite_pixels(rgb):
    """(h, w) bool: every channel passes pn_isfinite."""
    return np.isfinite(rgb).all(axis=2)


def circles(depth, max_radius, focus, scale):
    """Step 1 on every pixel of the (h, w) depth -> r, (h, w) f32."""
    z, F, K, R = np.asarray(depth, f32), f32(focus), f32(scale), f32(max_radius)
    with np.errstate(all="ignore"):
        known = z > f32(0)  # false for NaN
        zs = np.where(known & np.isfinite(z), z, f32(1))  # a stand-in where the quotient is not used
        q = np.where(np.isinf(z), f32(1), np.abs(zs - F) / zs).astype(f32)
        r = (K * q).astype(f32)
        r = np.where(r < R, r, R).astype(f32)
    return np.where(known, r, f32(0)).astype(f32)


def signed_circles(depth, r, focus):
    """Step 3: r with the sign bit set where depth < focus (an unordered comparison is false)."""
    with np.errstate(invalid="ignore"):
        near = np.asarray(depth, f32) < f32(focus)
    return (r.view(np.uint32) | np.where(near, np.uint32(0x80000000), np.uint32(0))).view(f32)


def dof(rgb, depth, max_radius=8, focus=1.0, scale=0.0, details=False):
    """pbrsf_dof on the (h, w, 3) f32 image and the (h, w) f32 depth -> the (h, w, 3) f32 image, or with `details` a namespace of
    out, coc (step 3), r (step 1), n (a pixel's tap count; 0 where it passes through or scale is 0), front (taps taken through the
    "in front" branch) and partial (taps with cov < 1)."""
    rgb, depth = np.ascontiguousarray(rgb, f32), np.ascontiguousarray(depth, f32)
    h, w, _ = rgb.shape
    assert depth.shape == (h, w) and 1 <= max_radius <= MAX_RADIUS
    R = int(max_radius)
    zero = np.zeros((h, w), np.int32)
    if f32(scale) == 0:  # step 0
        res = SimpleNamespace(out=rgb.copy(), coc=np.zeros((h, w), f32), r=np.zeros((h, w), f32), n=zero, front=zero.copy(), partial=zero.copy())
        return res if details else res.out
    r = circles(depth, R, focus, scale)
    good = finite_pixels(rgb)
    acc = np.zeros((h, w, 3), f32)
    W = np.zeros((h, w), f32)
    n, front, partial = zero.copy(), zero.copy(), zero.copy()
    half, one = f32(0.5), f32(1)
    # the image with a border of R pixels that are "outside": never good
    pad = lambda a, fill: np.pad(a, [(R, R), (R, R)] + [(0, 0)] * (a.ndim - 2), constant_values=fill)  # noqa: E731
    rgb_p, depth_p, r_p, good_p = pad(np.where(good[..., None], rgb, f32(0)), 0), pad(depth, 0), pad(r, 0), pad(good, False)
    with np.errstate(all="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                win = (slice(R + dy, R + dy + h), slice(R + dx, R + dx + w))
                gq, rq, zq, cq = good_p[win], r_p[win], depth_p[win], rgb_p[win]
                if not gq.any():
                    continue
                dist = np.sqrt(f32(dx * dx + dy * dy), dtype=f32)
                in_front = zq < depth
                e = np.where(in_front, rq, np.where(rq < r, rq, r)).astype(f32)
                cov = ((e - dist).astype(f32) + half).astype(f32)
                take = gq & good & (cov > 0)
                if not take.any():
                    continue
                partial += take & (cov < one)
                cov = np.where(cov < one, cov, one).astype(f32)
                rr = np.where(e > half, e, half).astype(f32)
                wgt = (cov / (rr * rr).astype(f32)).astype(f32)
                for c in range(3):
                    acc[..., c] = np.where(take, (acc[..., c] + (wgt * cq[..., c]).astype(f32)).astype(f32), acc[..., c])
                W = np.where(take, (W + wgt).astype(f32), W)
                n += take
                front += take & in_front
        Ws = np.where(n > 1, W, one)
        blurred = (acc / Ws[..., None]).astype(f32)
    out = np.where((n > 1)[..., None], blurred, rgb).astype(f32)  # n == 1, and the pixels that pass through (n == 0): rgb's bits
    res = SimpleNamespace(out=out, coc=signed_circles(depth, r, focus), r=r, n=n, front=front, partial=partial)
    return res if details else res.out
