#!/usr/bin/env python3
"""Developer tool (GPU box): what history clipping costs (include/pbrs_gpu.h, pbrs_temporal_accumulate_clip_device; device/temporal.h,
k_temporal_clip) next to the unclipped accumulation of the same build on the same frame.  tools/temporal_cost.py's set-up at 1920 x 1080:
a frame with a history, all guides and the id test, on synthetic buffers (a slanted wall seen through a camera that yaws 0.5 degrees, so
that every pixel gathers four fractional taps), colours and history uniform in 0.2 .. 1, so that with gamma 1 most pixels are clipped
in some channel.  Timed with HIP events on the context's stream (tools/hip_event_timing.py) around --batch back-to-back launches that
ping-pong two histories, after a warm-up, as the median of --runs such batches, per launch: without a clip, with radius 1 and with
radius 3.  The clipped kernel reads the frame's colours a second time through the block's halo (12 B per staged pixel from the caches:
(16 + 2 r)^2 / 256 = 1.27 of the tile at radius 1, 1.89 at radius 3) and moves the same compulsory bytes from HBM.
Writes profiles/history_clip_cost.json (or --out) and prints it.
    python tools/history_clip_cost.py [--runs N] [--batch N] [--out PATH]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history_clip_cost.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import pbrs_amd  # noqa: E402
from pbrs_amd import api  # noqa: E402

from hip_event_timing import Timing, check  # noqa: E402

T = Timing(pbrs_amd, warmup=2)
ctx, hip = T.ctx, T.hip
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
READ_BYTES, WRITTEN_BYTES = 60, 28  # tools/temporal_cost.py's compulsory bytes of a pixel
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


w, h = 1920, 1080
rng = np.random.default_rng(1)
P = w * h
cams = [camera(w, h, 0.0), camera(w, h, 0.5)]
yy, xx = np.mgrid[0:h, 0:w]
normal = np.stack([np.full((h, w), -0.2), np.zeros((h, w)), -np.ones((h, w))], axis=2).astype(f32)
instance = ((yy // 64) * 64 + xx // 64).astype(np.uint32)
frame = {"rgb": upload(rng.uniform(0.2, 1.0, size=(h, w, 3)).astype(f32)), "variance": upload(rng.uniform(0.0, 0.1, size=(h, w)).astype(f32)),
         "depth": upload(wall_depth(cams[1], w, h)), "normal": upload(normal), "instance": upload(instance)}
prev = {"depth": upload(wall_depth(cams[0], w, h)), "normal": frame["normal"], "instance": frame["instance"]}
start = {"rgb": rng.uniform(0.2, 1.0, size=(h, w, 3)).astype(f32), "moments": rng.uniform(0.2, 1.0, size=(h, w, 2)).astype(f32),
         "length": np.full((h, w), 3.0, dtype=f32)}
hist = [{n: upload(a) for n, a in start.items()} for _ in (0, 1)]
vout = upload(np.zeros((h, w), dtype=f32))
result = {"runs": args.runs, "batch": args.batch, "size": f"{w}x{h}", "read_bytes_per_pixel": READ_BYTES, "written_bytes_per_pixel": WRITTEN_BYTES, "cases": {}}
for name, clip in (("unclipped", None), ("radius_1", dict(radius=1, gamma=1.0)), ("radius_3", dict(radius=3, gamma=1.0))):
    for hd in hist:  # every case starts from the same history
        for n, a in start.items():
            check(hip.hipMemcpy(C.c_void_p(hd[n]), a.ctypes.data, a.nbytes, 1), "hipMemcpy")

    def batch():
        for k in range(args.batch):
            ctx.temporal_accumulate_device(frame, hist[(k & 1) ^ 1], w, h, cams[1], hist[k & 1], prev, cams[0], vout, id_test=True, clip=clip)
    r = T.median_of(batch, args.runs)
    ms = r["median_ms"] / args.batch
    rate = (READ_BYTES + WRITTEN_BYTES) * P / (ms * 1e-3)
    result["cases"][name] = {"batch_ms": r["ms"], "kernel_ms": round(ms, 5), "compulsory_GB_per_s": round(rate / 1e9, 1)}
    print(f"{name}: {ms * 1e3:.1f} us per launch, {rate / 1e9:.0f} GB/s of compulsory traffic", flush=True)
base = result["cases"]["unclipped"]["kernel_ms"]
for name in ("radius_1", "radius_3"):
    result["cases"][name]["over_unclipped"] = round(result["cases"][name]["kernel_ms"] / base, 3)
for ptr in set(list(frame.values()) + [prev["depth"], vout] + [p for hd in hist for p in hd.values()]):
    hip.hipFree(C.c_void_p(ptr))
ctx.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"history_clip_cost": result}, f, indent=1)
    f.write("\n")
print(json.dumps({"history_clip_cost": result}))
