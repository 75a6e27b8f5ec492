"""CPU model of temporal accumulation (include/pbrs_gpu.h, pbrs_temporal_accumulate), written from the header's text in numpy f32 like
tests/denoise_var_model.py: vectorised over the pixels, the four taps in the prescribed order (j outer, i inner).  Division is numpy's
(IEEE, correctly rounded, what the device computes); pn_floor goes through the oracle's include/pbrs_numeric.h.  `reproject` takes the
number type as a parameter, so that tests can evaluate the same formulas in float64.

Also the synthetic sequences of the tests: a scene of two planes seen through a moving camera (synthetic_sequence)."""
import numpy as np

from denoise_model import ONE, ZERO, _d2, _finite, f32
from denoise_var_model import INF, lum
from oracle.binding import numeric_eval

MISS = 0xFFFFFFFF
HALF = f32(0.5)
DEFAULTS = dict(max_history=32.0, depth_tolerance=0.05, normal_tolerance=0.3, min_temporal=4.0, id_test=False)
MOVES = ("none", "pan", "yaw", "dolly", "away")


class Cam:
    """pbrs_camera: center, c, a, b as f32 triples, and the film size."""

    def __init__(self, center, c, a, b, width, height):
        self.center, self.c, self.a, self.b = (np.asarray(v, dtype=f32) for v in (center, c, a, b))
        self.width, self.height = int(width), int(height)


def _floor(x):
    return numeric_eval("floor", np.ascontiguousarray(x, dtype=f32)).reshape(np.shape(x))


def _dot(p, q):
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def _cross(p, q):
    return np.stack([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]])


def pixel_dirs(cam, dtype=f32):
    """dir of rule B for every pixel -> (h, w, 3)."""
    c, a, b = (np.asarray(v, dtype=dtype) for v in (cam.c, cam.a, cam.b))
    x = (np.arange(cam.width).astype(dtype) + dtype(0.5))[None, :, None]
    yc = (np.arange(cam.height).astype(dtype) + dtype(0.5))[:, None, None]
    return (c + a * x) + b * yc


def reproject(depth, cam, cam_prev, dtype=f32):
    """Rule B up to (wq, xq, yq), each (h, w), in `dtype`; no rejection applied."""
    with np.errstate(all="ignore"):
        z = np.asarray(depth, dtype=dtype)
        P = np.asarray(cam.center, dtype=dtype) + pixel_dirs(cam, dtype) * z[..., None]
        e = P - np.asarray(cam_prev.center, dtype=dtype)
        ap, bp, cp = (np.asarray(v, dtype=dtype) for v in (cam_prev.a, cam_prev.b, cam_prev.c))
        nu, nv, nw = _cross(bp, cp), _cross(cp, ap), _cross(ap, bp)
        D = _dot(ap, nu)
        wq = _dot(e, nw) / D
        xq = (_dot(e, nu) / D) / wq
        yq = (_dot(e, nv) / D) / wq
    return wq, xq, yq


def accumulate(rgb, depth, cam, variance=None, normal=None, instance=None, history=None, prev=None, cam_prev=None, want_variance=True,
               details=None, **params):
    """pbrs_temporal_accumulate -> ({"rgb", "moments", "length"}, variance_out or None).  `history` / `prev` as the GPU binding takes
    them (dicts; None = the first frame).  `details`: a dict that receives "rejected" (hit pixels with a history_in that found no
    history), "disoccluded" (those of them that reproject into the previous frame: every tap was refused there) and "W"."""
    pr = dict(DEFAULTS, **params)
    rgb = np.asarray(rgb, dtype=f32)
    depth = np.asarray(depth, dtype=f32)
    h, w, _ = rgb.shape
    assert (cam.width, cam.height) == (w, h)
    max_history, dtol, ntol, min_temporal = (f32(pr[n]) for n in ("max_history", "depth_tolerance", "normal_tolerance", "min_temporal"))
    if pr["id_test"]:
        assert instance is not None
    fin = _finite(rgb)
    with np.errstate(all="ignore"):
        y = lum(rgb)
        S = np.zeros((h, w, 3), dtype=f32)
        A1, A2, N, W = (np.zeros((h, w), dtype=f32) for _ in range(4))
        valid = np.zeros((h, w), dtype=bool)
        if history is not None:
            assert cam_prev is not None and (cam_prev.width, cam_prev.height) == (w, h)
            hin = {n: np.asarray(history[n], dtype=f32) for n in ("rgb", "moments", "length")}
            zprev = np.asarray(prev["depth"], dtype=f32)
            nprev = prev.get("normal")
            iprev = prev.get("instance")
            assert (normal is None) == (nprev is None) and (instance is None) == (iprev is None)
            valid = np.isfinite(depth) & (depth > ZERO)
            wq, xq, yq = reproject(depth, cam, cam_prev)
            valid &= np.isfinite(wq) & (wq > ZERO)
            fx, fy = (xq - HALF).astype(f32), (yq - HALF).astype(f32)
            valid &= (fx > f32(-1.0)) & (fx < f32(w)) & (fy > f32(-1.0)) & (fy < f32(h))
            fx, fy = np.where(valid, fx, ZERO).astype(f32), np.where(valid, fy, ZERO).astype(f32)  # (keeps the casts in range)
            flx, fly = _floor(fx), _floor(fy)
            ix, iy = flx.astype(np.int64), fly.astype(np.int64)
            tx, ty = (fx - flx).astype(f32), (fy - fly).astype(f32)
            nt2 = ntol * ntol
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = ix + i, iy + j
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    bw = ((tx if i else ONE - tx) * (ty if j else ONE - ty)).astype(f32)
                    cq, mq, lq, zq = hin["rgb"][cy, cx], hin["moments"][cy, cx], hin["length"][cy, cx], zprev[cy, cx]
                    ok = valid & fin & inside & (bw > ZERO) & (lq > ZERO) & _finite(cq) & _finite(mq)
                    ok &= np.isfinite(zq) & (np.abs(zq - wq) <= dtol * wq)
                    if normal is not None:
                        ok &= _d2(np.asarray(nprev, dtype=f32)[cy, cx] - np.asarray(normal, dtype=f32)) <= nt2
                    if pr["id_test"]:
                        ok &= np.asarray(iprev, dtype=np.uint32)[cy, cx] == np.asarray(instance, dtype=np.uint32)
                    S = np.where(ok[..., None], S + bw[..., None] * cq, S).astype(f32)
                    A1 = np.where(ok, A1 + bw * mq[..., 0], A1).astype(f32)
                    A2 = np.where(ok, A2 + bw * mq[..., 1], A2).astype(f32)
                    N = np.where(ok, N + bw * lq, N).astype(f32)
                    W = np.where(ok, W + bw, W).astype(f32)
        has = W != ZERO
        iw = (ONE / W).astype(f32)
        H = (S * iw[..., None]).astype(f32)
        h1, h2, n = (A1 * iw).astype(f32), (A2 * iw).astype(f32), (N * iw).astype(f32)
        n1 = np.fmin(n + ONE, max_history).astype(f32)  # pn_min: a NaN operand is ignored
        al = (ONE / n1).astype(f32)
        out = np.where(has[..., None], H + al[..., None] * (rgb - H), rgb).astype(f32)
        y2 = (y * y).astype(f32)
        m1 = np.where(has, h1 + al * (y - h1), y).astype(f32)
        m2 = np.where(has, h2 + al * (y2 - h2), y2).astype(f32)
        length = np.where(has, n1, ONE).astype(f32)
        # rule A
        out = np.where(fin[..., None], out, rgb).astype(f32)
        m1, m2, length = (np.where(fin, v, ZERO).astype(f32) for v in (m1, m2, length))
        vout = None
        if want_variance:
            v = (m2 - m1 * m1).astype(f32)
            v = np.where(v < ZERO, ZERO, v).astype(f32)
            v = np.where(np.isnan(v), INF, v).astype(f32)
            if variance is None:
                vin = np.full((h, w), INF, dtype=f32)
            else:
                variance = np.asarray(variance, dtype=f32)
                vin = np.where(np.isnan(variance) | (variance < ZERO), INF, variance).astype(f32)
            vout = (np.where(length >= min_temporal, v, vin) * (ONE / length)).astype(f32)
            vout = np.where(fin, vout, INF).astype(f32)
    if details is not None:
        details["W"] = W
        details["rejected"] = fin & np.isfinite(depth) & (depth > ZERO) & ~has if history is not None else np.zeros((h, w), dtype=bool)
        details["disoccluded"] = valid & fin & ~has
    return {"rgb": out, "moments": np.stack([m1, m2], axis=2), "length": length}, vout


# ---- cameras -------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def look_at(w, h, fov_y_deg, origin, target, up=(0.0, 1.0, 0.0)):
    """A camera laid out as the host library lays it out: c, a, b = orientation * the film's corner and its two pixel steps."""
    half_v = np.tan(np.radians(fov_y_deg) * 0.5)
    half_h = half_v * (w / h)
    forward = _unit(np.subtract(target, origin))
    right = _unit(np.cross(up, forward))
    upv = np.cross(forward, right)
    a = right * (half_h / (w / 2.0))
    b = upv * (-half_v / (h / 2.0))
    c = right * -half_h + upv * half_v + forward
    return Cam(origin, c, a, b, w, h)


def rotated(cam, deg, axis=(0.0, 1.0, 0.0), about=None):
    """`cam` turned by `deg` degrees about the world axis `axis` through its own centre (a yaw for the y axis), or through `about`."""
    k = _unit(axis)
    t = np.radians(deg)

    def rot(v):
        v = np.asarray(v, dtype=np.float64)
        return v * np.cos(t) + np.cross(k, v) * np.sin(t) + k * np.dot(k, v) * (1.0 - np.cos(t))
    center = np.asarray(cam.center, dtype=np.float64)
    if about is not None:
        center = np.asarray(about, dtype=np.float64) + rot(center - np.asarray(about, dtype=np.float64))
    return Cam(center, rot(cam.c), rot(cam.a), rot(cam.b), cam.width, cam.height)


def moved_camera(w, h, move, k):
    """Frame k's camera of a move of MOVES."""
    assert move in MOVES
    base = look_at(w, h, 50.0, (0.1, 0.2, -4.0), (0.0, 0.0, 0.0))
    if move == "pan":  # sideways by 0.37 of a pixel per frame, as seen on the far wall of synthetic_sequence
        step = 0.37 * 8.0 * float(np.linalg.norm(base.a))
        return Cam(base.center + f32(k * step) * _unit(base.a).astype(f32), base.c, base.a, base.b, w, h)
    if move == "yaw":
        return rotated(base, 5.0 * k)
    if move == "dolly":
        return Cam(base.center + f32(0.4 * k) * _unit(np.cross(base.b, base.a)).astype(f32), base.c, base.a, base.b, w, h)
    if move == "away":  # odd frames look the other way: from an even frame every pixel lies behind the previous camera
        return rotated(base, 180.0 * (k & 1))
    return base


# ---- a synthetic scene -----------------------------------------------------------------------------------------------------------------
FAR_Z, NEAR_Z, STEP_X = 4.0, 2.5, 0.6  # the wall z = FAR_Z, and in front of it, for world x > STEP_X, the wall z = NEAR_Z


def _frame(cam, seed, k):
    """Frame k seen through `cam`: the noisy colour, its variance and the guides of the two walls, with a hole (a miss) in the far one."""
    w, h = cam.width, cam.height
    rng = np.random.default_rng(1000 * seed + k)
    o = np.asarray(cam.center, dtype=np.float64)
    d = pixel_dirs(cam, np.float64)
    with np.errstate(all="ignore"):
        t_near, t_far = (NEAR_Z - o[2]) / d[..., 2], (FAR_Z - o[2]) / d[..., 2]
        near = (t_near > 0) & ((o[0] + t_near * d[..., 0]) > STEP_X)
        t = np.where(near, t_near, t_far)
        X, Y = o[0] + t * d[..., 0], o[1] + t * d[..., 1]
        hit = (t > 0) & np.isfinite(t) & ~(~near & (np.abs(X + 1.2) < 0.35) & (np.abs(Y - 0.4) < 0.3))
    X, Y = np.where(hit, X, 0.0), np.where(hit, Y, 0.0)
    depth = np.where(hit, t, np.inf).astype(f32)
    normal = np.where(hit[..., None], np.stack([0.1 * np.sin(X * 1.7), 0.1 * np.cos(Y * 1.3), -np.ones_like(X)], axis=2), 0.0).astype(f32)
    instance = np.where(hit, (np.floor(Y / 0.7).astype(np.int64) % 5) * 8 + np.floor(X / 0.7).astype(np.int64) % 7 + 40 * near, MISS).astype(np.uint32)
    base = np.stack([0.6 + 0.3 * np.sin(X * 2.1), 0.5 + 0.3 * np.cos(Y * 1.9), 0.4 + 0.2 * np.sin(X + Y)], axis=2) * np.where(near, 1.6, 1.0)[..., None]
    base = np.where(hit[..., None], base, [0.2, 0.3, 0.5])
    noise = np.clip(rng.normal(scale=0.2, size=(h, w, 3)), -0.6, 0.6)
    rgb = (base * (1.0 + noise)).astype(f32)
    variance = ((lum(base.astype(f32)) * f32(0.2)) ** 2).astype(f32)
    if w * h >= 64:  # everything the header has a rule for
        ys, xs = rng.integers(0, h, size=6), rng.integers(0, w, size=6)
        rgb[ys[0], xs[0], 1] = np.nan
        rgb[ys[1], xs[1]] = np.inf
        depth[ys[2], xs[2]] = 0.0
        depth[ys[3], xs[3]] = np.nan
        variance[ys[4], xs[4]] = np.nan
        variance[ys[5], xs[5]] = -1.0
        variance[0, :3] = np.inf
    return {"rgb": rgb, "variance": variance, "depth": depth, "normal": normal, "instance": instance}


def synthetic_sequence(w, h, seed, move, frames=3):
    """Yields per frame (cam, frame, plant): the camera of `move`, the frame's inputs ({"rgb", "variance", "depth", "normal",
    "instance"}) and what plant_history writes into the history that frame leaves, before it is the next frame's history_in: a length
    of 0, a NaN length, a non-finite colour and a non-finite moment beside lengths that count (none of which a call produces)."""
    for k in range(frames):
        cam = moved_camera(w, h, move, k)
        rng = np.random.default_rng(77 * seed + k)
        plant = []
        if w * h >= 64:
            ys, xs = rng.integers(0, h, size=5), rng.integers(0, w, size=5)
            plant = [("length", (ys[0], xs[0]), 0.0), ("length", (ys[1], xs[1]), np.nan), ("rgb", (ys[2], xs[2], 2), np.inf),
                     ("rgb", (ys[3], xs[3], 0), np.nan), ("moments", (ys[4], xs[4], 1), np.inf)]
        yield cam, _frame(cam, seed, k), plant


def plant_history(history, plant):
    history = {n: np.array(a, dtype=f32) for n, a in history.items()}
    for name, at, value in plant:
        history[name][tuple(at)] = value
    return history


GUIDE_NAMES = ("depth", "normal", "instance")


def run_sequence(step, w, h, seed, move, frames=3, use=("variance", "normal", "instance"), want_variance=True, **params):
    """A synthetic sequence through `step(rgb, depth, cam, variance=, normal=, instance=, history=, prev=, cam_prev=, **params)` (the
    model's accumulate, or the GPU's binding adapted to it) -> [(history, variance_out)] per frame."""
    results, history, prev, cam_prev = [], None, None, None
    for cam, frame, plant in synthetic_sequence(w, h, seed, move, frames):
        given = {n: frame[n] for n in use}
        hist, vout = step(frame["rgb"], frame["depth"], cam, history=history, prev=prev, cam_prev=cam_prev, want_variance=want_variance,
                          **given, **params)
        results.append((hist, vout))
        history = plant_history(hist, plant)
        prev = {n: frame[n] for n in GUIDE_NAMES if n == "depth" or n in use}
        cam_prev = cam
    return results
