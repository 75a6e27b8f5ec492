"""A numpy model of the despeckle call, written from the text of include/pbrs_gpu.h ("despeckle"), rule by rule: f32 scalars in the
stated order, no fused multiply-add (numpy rounds every operation), a row-major repair sum.  The tests hold the device to its bytes."""
import numpy as np

f32 = np.float32
CLAMPED, REPAIRED = 1, 2
ZERO, INF = f32(0.0), f32(np.inf)
KR, KG, KB = f32(0.21267127), f32(0.71515972), f32(0.07216883)
FIELDS = ("n_clamped", "n_repaired")


def finite(x):
    """pn_isfinite: the exponent bits are not all ones."""
    return (np.asarray(x, f32).view(np.uint32) & np.uint32(0x7F800000)) != np.uint32(0x7F800000)


def lum(r, g, b):
    """Rule 1."""
    return (KR * r + KG * g) + KB * b


def despeckle(rgb, variance=None, radius=1, rank=2, gain=2.0, floor=0.0):
    """-> {"rgb", "variance" (None without one), "mask", "removed", "n_clamped", "n_repaired"}."""
    rgb = np.ascontiguousarray(rgb, f32)
    h, w, _ = rgb.shape
    gain, floor = f32(gain), f32(floor)
    out, removed, mask = rgb.copy(), np.zeros_like(rgb), np.zeros((h, w), np.uint32)
    vout = None if variance is None else np.ascontiguousarray(variance, f32).copy()
    with np.errstate(all="ignore"):
        L = lum(rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2])
        good = finite(rgb).all(axis=2) & finite(L)  # rule 2
        for y in range(h):
            for x in range(w):
                # rule 3, in row-major order
                G = [(qy, qx) for qy in range(max(y - radius, 0), min(y + radius, h - 1) + 1) for qx in range(max(x - radius, 0), min(x + radius, w - 1) + 1)
                     if (qy, qx) != (y, x) and good[qy, qx]]
                n = len(G)
                # rule 4
                if good[y, x]:
                    c, lp = rgb[y, x].copy(), L[y, x]
                else:
                    c = np.zeros(3, f32)
                    if n:
                        for ch in range(3):
                            a = ZERO
                            for q in G:
                                a = a + rgb[q][ch]
                            c[ch] = a / f32(n)
                        if not (finite(c).all() and finite(lum(c[0], c[1], c[2]))):
                            c = np.zeros(3, f32)
                    lp = lum(c[0], c[1], c[2])
                    mask[y, x] |= REPAIRED
                o, s, clamped = c, None, False
                if n:
                    # rule 5
                    S = sorted((L[q] for q in G), reverse=True)[min(rank, n) - 1]
                    limit = gain * S + floor
                    if not limit > ZERO:
                        limit = ZERO
                    # rule 6
                    if lp > limit:
                        clamped, s = True, limit / lp
                        o = np.array([c[0] * s, c[1] * s, c[2] * s], f32)
                        mask[y, x] |= CLAMPED
                        removed[y, x] = c - o  # rule 9
                out[y, x] = o
                # rule 7
                if vout is not None:
                    if not good[y, x]:
                        vout[y, x] = INF
                    elif clamped and finite(vout[y, x]):
                        vout[y, x] = (vout[y, x] * s) * s
    return {"rgb": out, "variance": vout, "mask": mask, "removed": removed, "n_clamped": int(((mask & CLAMPED) != 0).sum()),
            "n_repaired": int(((mask & REPAIRED) != 0).sum())}


def despeckle_planes(rgb, variance=None, radius=1, rank=2, gain=2.0, floor=0.0):
    """despeckle() for images too large for a loop over pixels: the same rules on whole planes, one f32 operation per rule and element
    in the same order, so the same bytes (tests/test_despeckle_model.py holds the two to each other).  The window is a list of shifted
    planes in row-major order of the taps; a tap that is not in G(p) enters the k-th largest as -inf, which no good luminance equals, and
    the repair sum as +0, which leaves a sum that started at +0 as it is."""
    rgb = np.ascontiguousarray(rgb, f32)
    h, w, _ = rgb.shape
    gain, floor, r = f32(gain), f32(floor), radius
    with np.errstate(all="ignore"):
        L = lum(rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2])
        good = finite(rgb).all(axis=2) & finite(L)  # rule 2

        def shifted(plane, dy, dx, fill):
            """plane(p + (dy, dx)), `fill` outside the image."""
            padded = np.full((h + 2 * r, w + 2 * r) + plane.shape[2:], fill, plane.dtype)
            padded[r:r + h, r:r + w] = plane
            return padded[r + dy:r + dy + h, r + dx:r + dx + w]

        taps = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if (dy, dx) != (0, 0)]  # rule 3
        in_g = [shifted(good, dy, dx, False) for dy, dx in taps]
        n = np.sum(in_g, axis=0, dtype=np.int64)
        # rule 4
        acc = np.zeros((h, w, 3), f32)
        for (dy, dx), g in zip(taps, in_g):
            acc = acc + np.where(g[:, :, None], shifted(rgb, dy, dx, ZERO), ZERO)
        mean = acc / np.maximum(n, 1).astype(f32)[:, :, None]
        mean_good = finite(mean).all(axis=2) & finite(lum(mean[:, :, 0], mean[:, :, 1], mean[:, :, 2]))
        c = np.where(good[:, :, None], rgb, np.where(((n > 0) & mean_good)[:, :, None], mean, ZERO))
        lp = np.where(good, L, lum(c[:, :, 0], c[:, :, 1], c[:, :, 2]))
        # rule 5
        values = np.sort(np.stack([np.where(g, shifted(L, dy, dx, ZERO), -INF) for (dy, dx), g in zip(taps, in_g)]), axis=0)[::-1]
        k = np.clip(np.minimum(rank, n) - 1, 0, len(taps) - 1)
        S = np.take_along_axis(values, k[None], axis=0)[0]
        limit = gain * S + floor
        limit = np.where(limit > ZERO, limit, ZERO)
        # rule 6
        clamped = (n > 0) & (lp > limit)
        s = np.where(clamped, limit / np.where(clamped, lp, f32(1.0)), f32(1.0))
        out = np.where(clamped[:, :, None], c * s[:, :, None], c)
        removed = np.where(clamped[:, :, None], c - out, ZERO)  # rule 9
        mask = (clamped * np.uint32(CLAMPED) + (~good) * np.uint32(REPAIRED)).astype(np.uint32)  # rule 8
        vout = None
        if variance is not None:  # rule 7
            v = np.ascontiguousarray(variance, f32)
            vout = np.where(~good, INF, np.where(clamped & finite(v), (v * s) * s, v)).astype(f32)
            keep = good & ~(clamped & finite(v))  # the input word, a NaN's payload included
            vout.view(np.uint32)[keep] = v.view(np.uint32)[keep]
    return {"rgb": out.astype(f32), "variance": vout, "mask": mask, "removed": removed.astype(f32), "n_clamped": int(clamped.sum()),
            "n_repaired": int((~good).sum())}


def record(r):
    """The 16 bytes of pbrs_despeckle_result."""
    return np.array([r["n_clamped"], r["n_repaired"], 0, 0], np.uint32).tobytes()
