"""CPU model of moving instances in the reprojection (include/pbrs_gpu.h, "moving instances and motion vectors"), written from the
header's text in numpy f32 on top of tests/temporal_model.py: the motion step and motion_vectors are this file's, rules A, C and D and
the taps of rule B are temporal_model's (accumulate runs tm.accumulate with this file's reprojection in the place of tm.reproject and
with nm in the place of normal(p), which tm.accumulate reads in the normal test alone).

A motion table is a dict {"m": (n, 3, 4) f32, "n": (n, 3, 3) f32, "flags": (n,) u32}; None is the call without a table.

Also the synthetic sequences of the tests: tm.synthetic_sequence with a table per frame (motion_sequence)."""
import numpy as np

import temporal_model as tm
from denoise_model import ZERO, f32
from denoise_var_model import INF

IDENTITY = 1  # PBRS_MOTION_IDENTITY
N_MOTION = 60  # records per table of motion_sequence: the near wall's ids (40 .. 78) reach past it


def identity_table(n):
    return {"m": np.tile(np.eye(3, 4, dtype=f32), (n, 1, 1)), "n": np.tile(np.eye(3, dtype=f32), (n, 1, 1)), "flags": np.full(n, IDENTITY, dtype=np.uint32)}


def table_of(records):
    """[(m (3, 4), n (3, 3), flags)] -> a table, every entry rounded to f32 once."""
    return {"m": np.array([r[0] for r in records], dtype=np.float64).astype(f32).reshape(-1, 3, 4),
            "n": np.array([r[1] for r in records], dtype=np.float64).astype(f32).reshape(-1, 3, 3),
            "flags": np.array([r[2] for r in records], dtype=np.uint32)}


def rigid(R, t, scale=1.0):
    """(m, n) of x -> scale * R x + t: n is the inverse transpose of the linear part."""
    R = np.asarray(R, dtype=np.float64)
    return np.hstack([scale * R, np.asarray(t, dtype=np.float64).reshape(3, 1)]), R / scale


def rotation(axis, deg):
    k = tm._unit(axis)
    t = np.radians(deg)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def _applies(instance, table):
    """Which pixels a record is applied to, and the record's index (0 where none is)."""
    inst = np.asarray(instance, dtype=np.uint32).astype(np.int64)
    n = len(table["flags"])
    inside = inst < n
    idx = np.where(inside, inst, 0)
    return inside & ((table["flags"][idx] & IDENTITY) == 0), idx


def moved(P, instance, table, dtype=f32):
    """The motion step on the surface points P (h, w, 3): Pm."""
    if table is None:
        return P
    on, idx = _applies(instance, table)
    m = table["m"].astype(dtype)[idx]  # (h, w, 3, 4)
    with np.errstate(all="ignore"):
        Pm = np.stack([((m[..., r, 0] * P[..., 0] + m[..., r, 1] * P[..., 1]) + m[..., r, 2] * P[..., 2]) + m[..., r, 3] for r in range(3)], axis=-1)
    return np.where(on[..., None], Pm.astype(dtype), P)


def moved_normal(normal, instance, table):
    """nm of the motion step for normal(p) (h, w, 3) f32."""
    normal = np.asarray(normal, dtype=f32)
    if table is None:
        return normal
    on, idx = _applies(instance, table)
    n = table["n"][idx]
    with np.errstate(all="ignore"):
        nm = np.stack([(n[..., r, 0] * normal[..., 0] + n[..., r, 1] * normal[..., 1]) + n[..., r, 2] * normal[..., 2] for r in range(3)], axis=-1)
    return np.where(on[..., None], nm.astype(f32), normal)


def reproject(depth, cam, cam_prev, instance=None, motion=None, dtype=f32):
    """Rule B up to (wq, xq, yq) with the motion step, each (h, w), in `dtype`; no rejection applied."""
    with np.errstate(all="ignore"):
        z = np.asarray(depth, dtype=dtype)
        P = np.asarray(cam.center, dtype=dtype) + tm.pixel_dirs(cam, dtype) * z[..., None]
        P = moved(P, instance, motion, dtype)
        e = P - np.asarray(cam_prev.center, dtype=dtype)
        ap, bp, cp = (np.asarray(v, dtype=dtype) for v in (cam_prev.a, cam_prev.b, cam_prev.c))
        nu, nv, nw = tm._cross(bp, cp), tm._cross(cp, ap), tm._cross(ap, bp)
        D = tm._dot(ap, nu)
        wq = tm._dot(e, nw) / D
        xq = (tm._dot(e, nu) / D) / wq
        yq = (tm._dot(e, nv) / D) / wq
    return wq, xq, yq


def accumulate(rgb, depth, cam, normal=None, instance=None, motion=None, **kw):
    """pbrs_temporal_accumulate_motion: tm.accumulate's arguments and results, plus the table."""
    if motion is None:
        return tm.accumulate(rgb, depth, cam, normal=normal, instance=instance, **kw)
    assert instance is not None and len(motion["flags"]) > 0

    def with_motion(depth_, cam_, cam_prev_, dtype=f32):
        return reproject(depth_, cam_, cam_prev_, instance, motion, dtype)
    keep = tm.reproject
    tm.reproject = with_motion
    try:
        return tm.accumulate(rgb, depth, cam, normal=None if normal is None else moved_normal(normal, instance, motion), instance=instance, **kw)
    finally:
        tm.reproject = keep


def motion_vectors(depth, cam, cam_prev, instance=None, motion=None):
    """pbrs_motion_vectors -> (motion_out (h, w, 2), prev_depth_out (h, w)), f32."""
    depth = np.asarray(depth, dtype=f32)
    h, w = depth.shape
    wq, xq, yq = reproject(depth, cam, cam_prev, instance, motion)
    with np.errstate(all="ignore"):
        ok = np.isfinite(depth) & (depth > ZERO) & np.isfinite(wq) & (wq > ZERO)
        x = (np.arange(w).astype(f32) + tm.HALF)[None, :]
        yc = (np.arange(h).astype(f32) + tm.HALF)[:, None]
        mv = np.stack([np.where(ok, xq - x, ZERO), np.where(ok, yq - yc, ZERO)], axis=2).astype(f32)
    return mv, np.where(ok, wq, INF).astype(f32)


# ---- synthetic sequences -----------------------------------------------------------------------------------------------------------------
TIP_PIVOT = np.array([-0.35, 0.35, tm.FAR_Z])  # the middle of the far wall's cell with id 6: x in [-0.7, 0), y in [0, 0.7)
TIPPED = rotation((1.0, 0.0, 0.0), 25.0)


def random_table(rng, n=N_MOTION):
    """Small rigid motions about points near the walls (up to 0.4 degrees and 0.03 units: about a pixel at 130 x 70), and one record of
    every special kind: 3 a uniform scale, 5 flagged IDENTITY with garbage in m and n, 6 a turn of 25 degrees about an axis in the far
    wall through the middle of id 6's cell (the points stay within the depth tolerance, the normal does not stay within the normal
    tolerance: only the normal test refuses them), 9 a NaN entry, every record from 11 on whose index is a multiple of 4 a flagged
    identity."""
    records = []
    for i in range(n):
        R = rotation(rng.normal(size=3), rng.uniform(-0.4, 0.4))
        pivot = np.array([rng.uniform(-2.0, 2.0), rng.uniform(-1.5, 1.5), rng.uniform(2.5, 4.0)])
        t = pivot - R @ pivot + rng.uniform(-0.03, 0.03, size=3)
        m, nn = rigid(R, t)
        flags = 0
        if i == 3:
            m, nn = rigid(R, pivot - 1.02 * (R @ pivot), 1.02)
        elif i == 5:
            m, nn, flags = np.full((3, 4), 1e30), np.full((3, 3), np.nan), IDENTITY
            m[1, 2] = np.nan
        elif i == 6:
            m, nn = rigid(TIPPED, TIP_PIVOT - TIPPED @ TIP_PIVOT)
        elif i == 9:
            m[1, 2] = np.nan
        elif i >= 11 and i % 4 == 0:
            m, nn, flags = np.eye(3, 4), np.eye(3), IDENTITY
        records.append((m, nn, flags))
    return table_of(records)


def motion_sequence(w, h, seed, move, frames=3, n_motion=N_MOTION):
    """tm.synthetic_sequence with a table per frame -> (cam, frame, plant, table).  The frames' ids run up to 78, so a table of
    N_MOTION records leaves ids at and above n_motion (static instances) in every frame that sees the near wall."""
    for k, (cam, frame, plant) in enumerate(tm.synthetic_sequence(w, h, seed, move, frames)):
        yield cam, frame, plant, random_table(np.random.default_rng(31 * seed + 7 * k + 1), n_motion)


def run_sequence(step, w, h, seed, move, frames=3, use=("variance", "normal", "instance"), want_variance=True, n_motion=N_MOTION, **params):
    """tm.run_sequence over motion_sequence: `step` also takes motion= (None on the first frame, which has no history)."""
    results, history, prev, cam_prev = [], None, None, None
    for cam, frame, plant, table in motion_sequence(w, h, seed, move, frames, n_motion):
        given = {n: frame[n] for n in use}
        hist, vout = step(frame["rgb"], frame["depth"], cam, history=history, prev=prev, cam_prev=cam_prev, want_variance=want_variance,
                          motion=table if history is not None else None, **given, **params)
        results.append((hist, vout))
        history = tm.plant_history(hist, plant)
        prev = {n: frame[n] for n in tm.GUIDE_NAMES if n == "depth" or n in use}
        cam_prev = cam
    return results


# ---- rendered scenes ----------------------------------------------------------------------------------------------------------------------
SHORT_BOX = 8  # the short box's instance id in the Cornell box: six walls and the light's two triangles come first


def cornell_short_box(short_xf, size=128, material=None):
    """pbrs_amd.scenes.cornell_scene (diffuse) with the short box under `short_xf`, and with `material(sb)` on it if given."""
    from pbrs_amd import scenes
    from pbrs_amd.spec import SceneBuilder, Transform, deg
    sb = SceneBuilder()
    _, white, _ = scenes._cornell_shell(sb)
    sb.instance(scenes.box_mesh(sb, (0, 0, 0), (165, 165, 165)), material(sb) if material else white, short_xf)
    sb.instance(scenes.box_mesh(sb, (0, 0, 0), (165, 330, 165)), white, Transform().rotate_y(deg(-18.0)).translate((130.0, 0.0, 225.0)))
    sb.set_camera(size, size, deg(65.0), (278, 278, 20), (278, 278, 555))
    return sb


def turned_short_box(k, size=128):
    """Frame k of the rendered sequence: the short box turns 4 degrees per frame about its own axis."""
    from pbrs_amd.spec import Transform, deg
    return cornell_short_box(Transform().rotate_y(deg(15.0 + 4.0 * k)).translate((265.0, 0.0, 105.0)), size)


def from_ctypes(table):
    """A ctypes array of api.InstanceMotion -> a table of this model."""
    return {"m": np.array([[list(row) for row in r.m] for r in table], dtype=f32).reshape(-1, 3, 4),
            "n": np.array([[list(row) for row in r.n] for r in table], dtype=f32).reshape(-1, 3, 3),
            "flags": np.array([r.flags for r in table], dtype=np.uint32)}


def to_ctypes(table):
    """A table of this model -> the ctypes array the binding takes (None stays None)."""
    from pbrs_amd import api
    if table is None:
        return None
    out = (api.InstanceMotion * len(table["flags"]))()
    raw = np.zeros((len(table["flags"]), 24), dtype=np.uint32)  # 96 B per record: m, n, flags, pad
    raw[:, :12] = table["m"].reshape(-1, 12).view(np.uint32)
    raw[:, 12:21] = table["n"].reshape(-1, 9).view(np.uint32)
    raw[:, 21] = table["flags"]
    import ctypes
    ctypes.memmove(out, raw.ctypes.data, raw.nbytes)
    return out
