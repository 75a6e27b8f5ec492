"""CPU model of the display transform (include/pbrs_gpu.h, pbrs_display), written from the header's text: the f32 operations are numpy's
(IEEE, correctly rounded, what the device computes without fused multiply-add), pn_exp, pn_ln and pn_ldexp go through the oracle's
include/pbrs_numeric.h (oracle.binding.numeric_eval, as tests/denoise_var_model.py does), and the histogram and its resolve are Python
integers."""
import numpy as np

from oracle.binding import numeric_eval

f32 = np.float32
BINS = 512
FIRST_BITS, INF_BITS = 0x2F800000, 0x7F800000
CURVES = {"none": 0, "reinhard": 1, "aces": 2}
ENCODES = {"sqrt": 0, "srgb": 1}
QUANTIZERS = {"trunc": 0, "round": 1, "dither": 2}
BAYER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], dtype=np.float32)
DEFAULTS = dict(curve="aces", encode="srgb", quantize="round", auto=False, exposure=1.0, key=0.18, white=None, min_exposure=2.0 ** -20,
                max_exposure=2.0 ** 20, adapt=1.0, low_q16=6554, high_q16=62259)


def _exp(x):
    return numeric_eval("exp", np.asarray(x, dtype=f32))


def _ln(x):
    return numeric_eval("ln", np.asarray(x, dtype=f32))


def _ldexp(x, n):
    return numeric_eval("ldexp", np.asarray(x, dtype=f32), np.asarray(n, dtype=f32))


def lum(c):
    c = np.asarray(c, dtype=f32)
    with np.errstate(all="ignore"):
        return ((f32(0.21267127) * c[..., 0] + f32(0.71515972) * c[..., 1]) + f32(0.07216883) * c[..., 2]).astype(f32)


def bins_of(y):
    """(counted, bin) of an array of f32 luminances."""
    u = np.ascontiguousarray(y, dtype=f32).view(np.uint32).astype(np.int64)
    counted = (u >= FIRST_BITS) & (u < INF_BITS)
    return counted, np.minimum((u - FIRST_BITS) >> 20, BINS - 1)


def histogram(rgb):
    """The 512 counts of an (..., 3) f32 image, uint32."""
    counted, b = bins_of(lum(rgb).reshape(-1))
    return np.bincount(b[counted], minlength=BINS).astype(np.uint32)


def _valid(prev):
    return prev is not None and bool(np.isfinite(f32(prev))) and f32(prev) > 0


def resolve(hist, key=0.18, min_exposure=2.0 ** -20, max_exposure=2.0 ** 20, adapt=1.0, low_q16=6554, high_q16=62259, exposure_in=None):
    """The auto exposure e (f32) of a histogram; `details` -> (e, dict of the integers on the way)."""
    n = [int(v) for v in hist]
    N = sum(n)
    prev = f32(exposure_in) if _valid(exposure_in) else None
    if N == 0:
        return prev if prev is not None else f32(1.0)
    lo, hi = (N * low_q16) >> 16, (N * high_q16) >> 16
    if hi == lo:
        lo, hi = 0, N
    K = hi - lo
    S = c = 0
    for b, nb in enumerate(n):
        k = max(0, min(c + nb, hi) - max(c, lo))
        S += k * (2 * b + 1)
        c += nb
    Q = (S << 8) // K
    with np.errstate(all="ignore"):
        x = f32(Q & 4095) * (f32(0.6931472) * f32(0.000244140625))
        lavg = _ldexp(_exp([x]), [(Q >> 12) - 32])[0]
        a = f32(key) / lavg
        a = f32(min_exposure) if a < f32(min_exposure) else a  # pn_clamp
        a = f32(max_exposure) if a > f32(max_exposure) else a
        if prev is not None:
            return f32(prev + f32(f32(a - prev) * f32(adapt)))
    return f32(a)


def curve_encode(v, curve, encode, white=None):
    """g of the header for an array of f32 values v that are already scaled, clamped at +0 and at 65504."""
    one = f32(1.0)
    with np.errstate(all="ignore"):
        if curve == 0:
            t = v
        elif curve == 1:
            w = f32(np.inf) if white is None else f32(white)
            iw2 = one / f32(w * w)
            t = (f32(v * f32(one + f32(v * iw2))) / f32(one + v)).astype(f32)
        else:
            t = ((v * (f32(2.51) * v + f32(0.03)).astype(f32)).astype(f32) / ((v * (f32(2.43) * v + f32(0.59)).astype(f32)).astype(f32) + f32(0.14)).astype(f32)).astype(f32)
        t = np.where(t < one, t, one).astype(f32)
        if encode == 0:
            return np.sqrt(t).astype(f32)
        mid = (f32(1.055) * _exp((_ln(t) * (one / f32(2.4))).astype(f32)) - f32(0.055)).astype(f32)
        return np.where(t <= f32(0.0031308), (f32(12.92) * t).astype(f32), np.where(t >= one, one, mid)).astype(f32)


def quantize(g, d):
    with np.errstate(all="ignore"):
        q = (g * f32(255.0) + d).astype(f32)
        return np.where(q >= f32(255.0), 255, np.where(q >= 0, q, 0).astype(np.int64)).astype(np.uint8)


def apply(rgb, scale, curve=2, encode=1, quantize_mode=1, white=None):
    """The per-pixel part: (h, w, 3) f32 and the f32 scale -> (h, w, 4) uint8."""
    rgb = np.asarray(rgb, dtype=f32)
    h, w, _ = rgb.shape
    with np.errstate(all="ignore"):
        v = (rgb * f32(scale)).astype(f32)
        v = np.where(v > 0, v, f32(0.0)).astype(f32)
        v = np.minimum(v, f32(65504.0)).astype(f32)  # (no NaN is left)
    g = curve_encode(v, curve, encode, white)
    if quantize_mode == 2:
        yy, xx = np.mgrid[0:h, 0:w]
        d = ((BAYER[yy & 3, xx & 3] + f32(0.5)) * f32(0.0625)).astype(f32)[:, :, None]
    else:
        d = f32(0.5) if quantize_mode == 1 else f32(0.0)
    out = np.full((h, w, 4), 255, dtype=np.uint8)
    out[:, :, :3] = quantize(g, d)
    return out


def display(rgb, exposure_in=None, **params):
    """pbrs_display as the header states it -> (rgba8 (h, w, 4) uint8, e f32, histogram (512) uint32).  params: DisplayParams.make's
    keywords."""
    unknown = set(params) - set(DEFAULTS)
    assert not unknown, unknown
    p = dict(DEFAULTS, **params)
    rgb = np.asarray(rgb, dtype=f32)
    hist = histogram(rgb)
    e = f32(1.0)
    if p["auto"]:
        e = resolve(hist, p["key"], p["min_exposure"], p["max_exposure"], p["adapt"], p["low_q16"], p["high_q16"], exposure_in)
    with np.errstate(all="ignore"):
        scale = f32(e * f32(p["exposure"]))
    name = lambda table, v: table[v] if isinstance(v, str) else v  # noqa: E731
    out = apply(rgb, scale, name(CURVES, p["curve"]), name(ENCODES, p["encode"]), name(QUANTIZERS, p["quantize"]), p["white"])
    return out, e, hist
