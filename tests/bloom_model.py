"""The bloom call (include/pbrs_gpu.h, "bloom") as numpy f32: the header's text step by step.  Every sum is an explicit loop over the taps
in the stated order, one f32 operation at a time (a multiply, then an add: numpy fuses nothing); the arrays only hold all pixels of a
level at once, which changes no pixel's operations.  There is no np.sum, no dot product and no f64 anywhere."""
import numpy as np

f32 = np.float32
MIX = 1
MAX_LEVELS = 8
K = (f32(0.125), f32(0.375), f32(0.375), f32(0.125))
DEFAULTS = dict(levels=6, threshold=1.0, knee=0.5, strength=0.05, spread=0.6, mix=False)


def level_sizes(w, h, levels):
    """[(w_l, h_l)] of the effective levels: `levels` of them, cut at the first that is 1 x 1."""
    sizes = []
    while len(sizes) < levels:
        w, h = (w + 1) // 2, (h + 1) // 2
        sizes.append((w, h))
        if (w, h) == (1, 1):
            break
    return sizes


def lum(c):
    return (f32(0.21267127) * c[..., 0] + f32(0.71515972) * c[..., 1]) + f32(0.07216883) * c[..., 2]


def bright_pass(rgb, threshold, knee):
    """Step 2 on every pixel of the (h, w, 3) image."""
    with np.errstate(all="ignore"):
        good = np.isfinite(rgb).all(axis=2)
        c = np.where(rgb > 0, rgb, f32(0)).astype(f32)
        c[~good] = f32(0)
        Y = lum(c)
        t = f32(threshold)
        k = f32(t * f32(knee))
        lo, hi = f32(t - k), f32(t + k)
        hard = (Y - t) / Y
        s = (Y - t) + k
        soft = ((s * s) * (f32(1.0) / (f32(4.0) * k))) / Y
        f = np.where(Y <= lo, f32(0), np.where(Y >= hi, hard, soft)).astype(f32)
        out = (c * f[..., None]).astype(f32)
    out[~good] = f32(0)
    return out


def downsample(src):
    """Step 3: (sh, sw, 3) -> ((sh + 1) / 2, (sw + 1) / 2, 3)."""
    sh, sw, _ = src.shape
    dh, dw = (sh + 1) // 2, (sw + 1) // 2
    X, Y = np.arange(dw), np.arange(dh)
    acc = np.zeros((dh, dw, 3), f32)
    for dy in range(-1, 3):
        sy = np.clip(2 * Y + dy, 0, sh - 1)
        for dx in range(-1, 3):
            sx = np.clip(2 * X + dx, 0, sw - 1)
            wgt = f32(K[dx + 1] * K[dy + 1])
            acc = acc + wgt * src[sy[:, None], sx[None, :]]
    assert acc.dtype == f32
    return acc


def up(v, fw, fh):
    """Step 4's up(): the (ch, cw, 3) level `v` at the (fh, fw) pixels of the finer one."""
    ch, cw, _ = v.shape
    x, y = np.arange(fw), np.arange(fh)
    x0, y0 = x >> 1, y >> 1
    x1 = np.clip(x0 + np.where(x & 1, 1, -1), 0, cw - 1)
    y1 = np.clip(y0 + np.where(y & 1, 1, -1), 0, ch - 1)
    acc = np.zeros((fh, fw, 3), f32)
    for (ys, wy), (xs, wx) in (((y0, 0.75), (x0, 0.75)), ((y0, 0.75), (x1, 0.25)), ((y1, 0.25), (x0, 0.75)), ((y1, 0.25), (x1, 0.25))):
        acc = acc + f32(f32(wx) * f32(wy)) * v[ys[:, None], xs[None, :]]
    assert acc.dtype == f32
    return acc


def pyramid(rgb, levels, threshold, knee, spread):
    """u_0 of steps 1 to 4."""
    h, w, _ = rgb.shape
    n = len(level_sizes(w, h, levels))
    with np.errstate(all="ignore"):
        d = [downsample(bright_pass(rgb, threshold, knee))]
        for _ in range(1, n):
            d.append(downsample(d[-1]))
        u = d[-1]
        for lv in range(n - 2, -1, -1):
            fh, fw, _ = d[lv].shape
            u = d[lv] + f32(spread) * (up(u, fw, fh) - d[lv])
    assert u.dtype == f32
    return u


def bloom(rgb, levels=6, threshold=1.0, knee=0.5, strength=0.05, spread=0.6, mix=False):
    """pbrsb_bloom of the (h, w, 3) f32 image."""
    rgb = np.ascontiguousarray(rgb, dtype=f32)
    h, w, _ = rgb.shape
    if f32(strength) == 0:
        return rgb.copy()
    with np.errstate(all="ignore"):
        B = up(pyramid(rgb, levels, threshold, knee, spread), w, h)
        out = rgb + f32(strength) * ((B - rgb) if mix else B)
    assert out.dtype == f32
    good = np.isfinite(rgb).all(axis=2)
    out[~good] = rgb[~good]  # the input's bits
    return out
