#!/usr/bin/env python3
"""Developer tool (GPU box): what following moving instances costs (include/pbrs_gpu.h, pbrs_temporal_accumulate_motion_device and
pbrs_motion_vectors_device; device/temporal.h).  tools/temporal_cost.py's set-up (a slanted wall seen through a camera that yaws 0.5
degrees, all guides and the id test, 1920 x 1080 and 3840 x 2160) with instance ids in 64 x 64 blocks that run over a table of 130
records of small rigid motions: k_temporal<1,1,1,1> beside its twin without a table, k_temporal<1,1,1,0>, on the same buffers, and
k_motion_vectors<1> with both outputs.  Timed with HIP events on the context's stream (tools/hip_event_timing.py) around --batch
back-to-back calls, after a warm-up, as the median of --runs such batches, per call.  A call with a table also queues the table's copy
(12 480 B from host memory) ahead of its kernel: the events see both.
Writes profiles/motion_cost.json (or --out) and prints it.
    python tools/motion_cost.py [--runs N] [--batch N] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--batch", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_cost.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import pbrs_amd  # noqa: E402
from pbrs_amd import api  # noqa: E402

from hip_event_timing import Timing, check  # noqa: E402

T = Timing(pbrs_amd, warmup=2)
ctx, hip = T.ctx, T.hip
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
N_RECORDS = 130
f32 = np.float32


def camera(w, h, yaw_deg):
    """A 50 degree camera at the origin looking down +z, turned about the y axis."""
    half_v = np.tan(np.radians(25.0))
    half_h = half_v * w / h
    t = np.radians(yaw_deg)
    right, up, fwd = np.array([np.cos(t), 0.0, -np.sin(t)]), np.array([0.0, 1.0, 0.0]), np.array([np.sin(t), 0.0, np.cos(t)])
    cam = api.Camera()
    cam.width, cam.height = w, h
    for name, v in (("center", np.zeros(3)), ("a", right * (half_h / (w / 2))), ("b", up * (-half_v / (h / 2))),
                    ("c", right * -half_h + up * half_v + fwd)):
        getattr(cam, name)[:] = [float(x) for x in v]
    return cam


def wall_depth(cam, w, h):
    """The ray parameter of the wall z = 5 + 0.2 x through every pixel centre."""
    c, a, b = (np.array(list(getattr(cam, n))) for n in ("c", "a", "b"))
    d = c + a * (np.arange(w) + 0.5)[None, :, None] + b * (np.arange(h) + 0.5)[:, None, None]
    return (5.0 / (d[..., 2] - 0.2 * d[..., 0])).astype(f32)


def upload(a):
    a = np.ascontiguousarray(a)
    ptr = T.dev_alloc(a.nbytes)
    check(hip.hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy")  # hipMemcpyHostToDevice
    return ptr.value


def table(rng):
    """N_RECORDS small rigid motions (up to 0.2 degrees about a point of the wall and 0.01 units), none flagged."""
    t = (api.InstanceMotion * N_RECORDS)()
    for r in t:
        k = rng.normal(size=3)
        k /= np.linalg.norm(k)
        ang = np.radians(rng.uniform(-0.2, 0.2))
        K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        R = np.eye(3) + np.sin(ang) * K + (1.0 - np.cos(ang)) * (K @ K)
        pivot = np.array([rng.uniform(-2.0, 2.0), rng.uniform(-1.0, 1.0), 5.0])
        shift = pivot - R @ pivot + rng.uniform(-0.01, 0.01, size=3)
        for a in range(3):
            r.m[a][:] = [float(v) for v in R[a]] + [float(shift[a])]
            r.n[a][:] = [float(v) for v in R[a]]
    return t


result = {"runs": args.runs, "batch": args.batch, "records": N_RECORDS,
          "params": {k: (round(v, 6) if isinstance(v, float) else v) for k, v in api.TemporalParams.make(0, 0, id_test=True).as_dict().items()},
          "sizes": {}}
for w, h in ((1920, 1080), (3840, 2160)):
    rng = np.random.default_rng(1)
    cams = [camera(w, h, 0.0), camera(w, h, 0.5)]
    yy, xx = np.mgrid[0:h, 0:w]
    normal = np.stack([np.full((h, w), -0.2), np.zeros((h, w)), -np.ones((h, w))], axis=2).astype(f32)
    instance = (((yy // 64) * 64 + xx // 64) % N_RECORDS).astype(np.uint32)
    frame = {"rgb": upload(rng.uniform(0.2, 1.0, size=(h, w, 3)).astype(f32)), "variance": upload(rng.uniform(0.0, 0.1, size=(h, w)).astype(f32)),
             "depth": upload(wall_depth(cams[1], w, h)), "normal": upload(normal), "instance": upload(instance)}
    prev = {"depth": upload(wall_depth(cams[0], w, h)), "normal": frame["normal"], "instance": frame["instance"]}
    hist = [{"rgb": upload(rng.uniform(0.2, 1.0, size=(h, w, 3)).astype(f32)), "moments": upload(rng.uniform(0.2, 1.0, size=(h, w, 2)).astype(f32)),
             "length": upload(np.full((h, w), 3.0, dtype=f32))} for _ in (0, 1)]
    vout, mv, wq = upload(np.zeros((h, w), dtype=f32)), upload(np.zeros((h, w, 2), dtype=f32)), upload(np.zeros((h, w), dtype=f32))
    records = table(rng)

    def accumulate(motion):
        def batch():
            for k in range(args.batch):
                ctx.temporal_accumulate_device(frame, hist[(k & 1) ^ 1], w, h, cams[1], hist[k & 1], prev, cams[0], vout, id_test=True, motion=motion)
        return batch

    def vectors():
        for _ in range(args.batch):
            ctx.motion_vectors_device(frame["depth"], mv, w, h, cams[1], cams[0], frame["instance"], records, wq)
    entry = {}
    for name, fn in (("k_temporal<1,1,1,0>", accumulate(None)), ("k_temporal<1,1,1,1>", accumulate(records)), ("k_motion_vectors<1>", vectors)):
        r = T.median_of(fn, args.runs)
        entry[name] = {"batch_ms": r["ms"], "call_us": round(r["median_ms"] / args.batch * 1e3, 2)}
        if name.startswith("k_temporal"):  # how many pixels found a history, from the history the last launch wrote
            length = np.empty((h, w), dtype=f32)
            check(hip.hipMemcpy(length.ctypes.data, C.c_void_p(hist[((args.batch - 1) & 1) ^ 1]["length"]), length.nbytes, 2), "hipMemcpy")
            entry[name]["pixels_with_history"] = round(float((length > 1.0).mean()), 4)
    entry["motion_over_twin"] = round(entry["k_temporal<1,1,1,1>"]["call_us"] / entry["k_temporal<1,1,1,0>"]["call_us"], 4)
    result["sizes"][f"{w}x{h}"] = entry
    print(f"{w} x {h}: " + ", ".join(f"{n} {e['call_us']:.1f} us" for n, e in entry.items() if isinstance(e, dict)) +
          f"; with the table / without {entry['motion_over_twin']:.3f}", flush=True)
    for ptr in set(list(frame.values()) + [prev["depth"], vout, mv, wq] + [p for hd in hist for p in hd.values()]):
        hip.hipFree(C.c_void_p(ptr))
ctx.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"motion_cost": result}, f, indent=1)
    f.write("\n")
print(json.dumps({"motion_cost": result}))
