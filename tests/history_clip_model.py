"""CPU model of history clipping (include/pbrs_gpu.h, "history clipping"; pbrs_temporal_accumulate_clip), written from the header's text
in numpy f32 beside tests/temporal_model.py and tests/motion_model.py: the box and the clip are this file's, and so is the pass through
rules A to D around them (temporal_model.accumulate runs rules B and C in one piece, and the clip stands between them); reprojection,
the motion step, the helpers and the synthetic sequences are the two neighbours'.  test_history_clip_model.py holds `accumulate` with a
box that clips nothing against motion_model.accumulate, bit for bit.

A clip is None (the call without one: motion_model.accumulate), True (the defaults) or a dict of radius / gamma / clip_history, as
Context.temporal_accumulate takes it."""
import numpy as np

import motion_model as mm
import temporal_model as tm
from denoise_model import ONE, ZERO, _d2, _finite, f32
from denoise_var_model import INF, lum

CLIP_DEFAULTS = dict(radius=1, gamma=1.0, clip_history=None)
MAX_RADIUS = 3


def clip_params(clip):
    """None / True / dict -> None or (radius, gamma f32, clip_history f32), clip_history None being +inf."""
    if clip is None or clip is False:
        return None
    c = dict(CLIP_DEFAULTS, **({} if clip is True else clip))
    assert set(c) == set(CLIP_DEFAULTS) and 1 <= c["radius"] <= MAX_RADIUS
    return int(c["radius"]), f32(c["gamma"]), INF if c["clip_history"] is None else f32(c["clip_history"])


def pn_max(a, b):
    """include/pbrs_numeric.h: a > b ? a : b, a NaN operand ignored."""
    m = np.where(a > b, a, b)
    m = np.where(np.isnan(a), b, m)
    return np.where(np.isnan(b), a, m).astype(f32)


def pn_min(a, b):
    m = np.where(a < b, a, b)
    m = np.where(np.isnan(a), b, m)
    return np.where(np.isnan(b), a, m).astype(f32)


def box(rgb, radius=1, gamma=1.0, details=None):
    """The header's box of every pixel of an (h, w, 3) image -> (lo, hi), (h, w, 3) f32 each.  `details` receives "cnt" (the taps that
    counted), "skipped" (the taps inside the image that were skipped as non-finite), "mu" and "sd"."""
    rgb = np.asarray(rgb, dtype=f32)
    h, w, _ = rgb.shape
    gamma = f32(gamma)
    fin = _finite(rgb)
    s1, s2 = np.zeros((h, w, 3), dtype=f32), np.zeros((h, w, 3), dtype=f32)
    cnt, skipped = np.zeros((h, w), dtype=f32), np.zeros((h, w), dtype=np.int64)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                qy, qx = ys + dy, xs + dx
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cy, cx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                ok = inside & fin[cy, cx]
                c = rgb[cy, cx]
                s1 = np.where(ok[..., None], s1 + c, s1).astype(f32)
                s2 = np.where(ok[..., None], s2 + (c * c).astype(f32), s2).astype(f32)
                cnt = np.where(ok, cnt + ONE, cnt).astype(f32)
                skipped += inside & ~ok
        ic = (ONE / cnt).astype(f32)[..., None]
        mu = (s1 * ic).astype(f32)
        v = ((s2 * ic).astype(f32) - (mu * mu).astype(f32)).astype(f32)
        v = np.where(v < ZERO, ZERO, v).astype(f32)
        sd = np.sqrt(v).astype(f32)
        lo = (mu - (gamma * sd).astype(f32)).astype(f32)
        hi = (mu + (gamma * sd).astype(f32)).astype(f32)
    if details is not None:
        details.update(cnt=cnt, skipped=skipped, mu=mu, sd=sd)
    return lo, hi


def clip_history(H, h1, h2, n, lo, hi, clip_len):
    """The header's clip and what it does to the moments and the length, for every pixel -> (Hc, h1, h2, n, changed)."""
    with np.errstate(all="ignore"):
        Hc = np.where(lo <= hi, pn_min(pn_max(H, lo), hi), H).astype(f32)
        changed = ~(Hc == H).all(axis=2)
        vh = (h2 - (h1 * h1).astype(f32)).astype(f32)
        vh = np.where(vh < ZERO, ZERO, vh).astype(f32)
        vh = np.where(np.isnan(vh), ZERO, vh).astype(f32)
        g1 = lum(Hc).astype(f32)
        g2 = (vh + (g1 * g1).astype(f32)).astype(f32)
        return (Hc, np.where(changed, g1, h1).astype(f32), np.where(changed, g2, h2).astype(f32),
                np.where(changed, pn_min(n, np.full_like(n, clip_len)), n).astype(f32), changed)


def accumulate(rgb, depth, cam, variance=None, normal=None, instance=None, history=None, prev=None, cam_prev=None, want_variance=True,
               motion=None, clip=None, details=None, **params):
    """pbrs_temporal_accumulate_clip: motion_model.accumulate's arguments and results, plus the clip.  `details` (with a clip and a
    history) receives "has" (the finite pixels with a history), "clipped" (those of them the clip changed) and "skipped" (the taps their
    windows skipped as non-finite)."""
    cp = clip_params(clip)
    if cp is None or history is None:  # the first frame has nothing to clip
        if details is not None:
            details.update(has=None, clipped=None, skipped=None)
        return mm.accumulate(rgb, depth, cam, variance=variance, normal=normal, instance=instance, history=history, prev=prev, cam_prev=cam_prev,
                             want_variance=want_variance, motion=motion, **params)
    radius, gamma, clip_len = cp
    pr = dict(tm.DEFAULTS, **params)
    rgb = np.asarray(rgb, dtype=f32)
    depth = np.asarray(depth, dtype=f32)
    h, w, _ = rgb.shape
    assert (cam.width, cam.height) == (w, h) and cam_prev is not None and (cam_prev.width, cam_prev.height) == (w, h)
    max_history, dtol, ntol, min_temporal = (f32(pr[n]) for n in ("max_history", "depth_tolerance", "normal_tolerance", "min_temporal"))
    if pr["id_test"] or motion is not None:
        assert instance is not None
    fin = _finite(rgb)
    with np.errstate(all="ignore"):
        y = lum(rgb)
        # rule B, with the motion step
        S = np.zeros((h, w, 3), dtype=f32)
        A1, A2, N, W = (np.zeros((h, w), dtype=f32) for _ in range(4))
        hin = {n: np.asarray(history[n], dtype=f32) for n in ("rgb", "moments", "length")}
        zprev, nprev, iprev = np.asarray(prev["depth"], dtype=f32), prev.get("normal"), prev.get("instance")
        assert (normal is None) == (nprev is None) and (instance is None) == (iprev is None)
        nm = None if normal is None else mm.moved_normal(normal, instance, motion)
        valid = np.isfinite(depth) & (depth > ZERO)
        wq, xq, yq = mm.reproject(depth, cam, cam_prev, instance, motion)
        valid &= np.isfinite(wq) & (wq > ZERO)
        fx, fy = (xq - tm.HALF).astype(f32), (yq - tm.HALF).astype(f32)
        valid &= (fx > f32(-1.0)) & (fx < f32(w)) & (fy > f32(-1.0)) & (fy < f32(h))
        fx, fy = np.where(valid, fx, ZERO).astype(f32), np.where(valid, fy, ZERO).astype(f32)
        flx, fly = tm._floor(fx), tm._floor(fy)
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        tx, ty = (fx - flx).astype(f32), (fy - fly).astype(f32)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = ix + i, iy + j
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                bw = ((tx if i else ONE - tx) * (ty if j else ONE - ty)).astype(f32)
                cq, mq, lq, zq = hin["rgb"][cy, cx], hin["moments"][cy, cx], hin["length"][cy, cx], zprev[cy, cx]
                ok = valid & fin & inside & (bw > ZERO) & (lq > ZERO) & _finite(cq) & _finite(mq)
                ok &= np.isfinite(zq) & (np.abs(zq - wq) <= dtol * wq)
                if nm is not None:
                    ok &= _d2(np.asarray(nprev, dtype=f32)[cy, cx] - nm) <= ntol * ntol
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
        # the clip
        det = {}
        lo, hi = box(rgb, radius, gamma, det)
        H, h1, h2, n, changed = clip_history(H, h1, h2, n, lo, hi, clip_len)
        # rule C
        n1 = pn_min((n + ONE).astype(f32), np.full((h, w), max_history, dtype=f32))
        al = (ONE / n1).astype(f32)
        out = np.where(has[..., None], H + al[..., None] * (rgb - H), rgb).astype(f32)
        y2 = (y * y).astype(f32)
        m1 = np.where(has, h1 + al * (y - h1), y).astype(f32)
        m2 = np.where(has, h2 + al * (y2 - h2), y2).astype(f32)
        length = np.where(has, n1, ONE).astype(f32)
        # rule A
        out = np.where(fin[..., None], out, rgb).astype(f32)
        m1, m2, length = (np.where(fin, v, ZERO).astype(f32) for v in (m1, m2, length))
        # rule D
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
        on = has & fin
        details.update(has=on, clipped=on & changed, skipped=np.where(on, det["skipped"], 0), lo=lo, hi=hi)
    return {"rgb": out, "moments": np.stack([m1, m2], axis=2), "length": length}, vout


def run_sequence(step, w, h, seed, move, frames=3, use=("variance", "normal", "instance"), want_variance=True, n_motion=mm.N_MOTION, with_table=True,
                 clip=True, **params):
    """motion_model.run_sequence with a clip on every frame that has a history; with_table=False runs the same frames without a motion
    table.  `step` also takes clip= and, the model's, details=; -> [(history, variance_out, details or None)] per frame."""
    results, history, prev, cam_prev = [], None, None, None
    for cam, frame, plant, table in mm.motion_sequence(w, h, seed, move, frames, n_motion):
        given = {n: frame[n] for n in use}
        det = {} if step is accumulate else None
        extra = {} if det is None else {"details": det}
        hist, vout = step(frame["rgb"], frame["depth"], cam, history=history, prev=prev, cam_prev=cam_prev, want_variance=want_variance,
                          motion=table if history is not None and with_table and "instance" in use else None, clip=clip, **given, **extra, **params)
        results.append((hist, vout, det))
        history = tm.plant_history(hist, plant)
        prev = {n: frame[n] for n in tm.GUIDE_NAMES if n == "depth" or n in use}
        cam_prev = cam
    return results
