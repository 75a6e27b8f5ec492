#!/usr/bin/env python3
"""Developer tool (GPU box): what the motion-blur call costs (include/pbrs_gpu.h, pbrsm_motion_blur_device).
Time, with HIP events on the context's stream, after a warm-up, as medians of repeated batches (tools/dof_cost.py's method; a batch of
calls between two events), on HDR noise at 1920 x 1080 with the defaults' 16 taps, shutter 1, over three motion fields:
  - "zero":     no pixel moves: every block stages its tile, finds its dominant velocity and copies;
  - "constant": every pixel moves by 2 * max_radius along (0.6, -0.8), len = max_radius: every block gathers all its taps;
  - "eighth":   one 16 x 16 tile in eight moves like that (tile index % 8 == 0), the others stand still: the tiles within max_radius of
                a moving one gather, the rest copy;
each at max_radius 4, 8 and 16 (the kernel's three halo classes), the constant field also with the jitter and with 64 taps, and beside
them, in the same run, two yardsticks:
  - a device-to-device copy of the same image on the same stream, the floor of any operation that reads and writes it once;
  - pbrsf_dof_device at max_radius 8 over a ramp through its focus, the chain's neighbour.
The device is kept busy for --warm seconds before the first timed batch, and the first form is timed again after the last one
("..._again").  Writes profiles/motion_blur_cost.json (or --out) and prints it; --no-write only prints.
    python tools/motion_blur_cost.py [--runs N] [--batch N] [--warm S] [--no-write] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time as clock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--batch", type=int, default=10)
ap.add_argument("--warm", type=float, default=1.0)
ap.add_argument("--no-write", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_blur_cost.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import pbrs_amd  # noqa: E402
from pbrs_amd.roofline import HBM_PEAK_GBS  # noqa: E402

from hip_event_timing import Timing, check  # noqa: E402

T = Timing(pbrs_amd, warmup=2)
ctx, hip = T.ctx, T.hip
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
f32 = np.float32
RADII = (4, 8, 16)
W, H = 1920, 1080
P = W * H


def upload(a):
    a = np.ascontiguousarray(a)
    ptr = T.dev_alloc(a.nbytes)
    check(hip.hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy")  # hipMemcpyHostToDevice
    return ptr.value


def per_call(fn):
    def batch():
        for _ in range(args.batch):
            fn()
    r = T.median_of(batch, args.runs)
    calls = sorted(ms / args.batch for ms in r["ms"])
    return {"batch_ms": r["ms"], "call_ms": round(r["median_ms"] / args.batch, 5), "call_ms_min": round(calls[0], 5), "call_ms_max": round(calls[-1], 5)}


def show(name, r):
    print(f"{name}: {r['call_ms'] * 1e3:.1f} us per call ({r['call_ms_min'] * 1e3:.1f} .. {r['call_ms_max'] * 1e3:.1f})", flush=True)


rng = np.random.default_rng(1)
img = np.exp2(rng.uniform(-6, 6, (H, W, 3))).astype(f32)
rgb, out = upload(img), T.dev_alloc(12 * P).value
depth = upload(np.tile((2.0 * (0.4 + 1.6 * np.arange(W) / (W - 1))).astype(f32), (H, 1)))
tile = (np.arange(H)[:, None] // 16) * ((W + 15) // 16) + np.arange(W)[None, :] // 16
fields = {}
for R in RADII:
    vec = (2.0 * R * np.array((0.6, -0.8))).astype(f32)
    constant = np.broadcast_to(vec, (H, W, 2))
    fields["zero", R] = upload(np.zeros((H, W, 2), f32))
    fields["constant", R] = upload(constant)
    fields["eighth", R] = upload(np.where((tile % 8 == 0)[..., None], constant, f32(0)).astype(f32))


def form(name, R, **kw):
    return lambda: ctx.motion_blur_device(rgb, depth, fields[name, R], out, W, H, max_radius=R, shutter=1.0, **kw)


until = clock.monotonic() + args.warm
while clock.monotonic() < until:
    for _ in range(20):
        form("eighth", 8)()
    ctx.collect_stats()
result = {"runs": args.runs, "batch": args.batch, "warm_s": args.warm, "hbm_peak_GBps": HBM_PEAK_GBS, "size": f"{W}x{H}", "taps": 16, "shutter": 1.0,
          "motion_blur": {}}
order = [(name, R, {}, "") for R in RADII for name in ("zero", "constant", "eighth")]
order += [("constant", 16, {"jitter": True}, "_jitter"), ("constant", 16, {"taps": 64}, "_taps64"), ("constant", 16, {"taps": 64, "jitter": True}, "_taps64_jitter"),
          ("zero", RADII[0], {}, "_again")]
for name, R, kw, suffix in order:
    r = per_call(form(name, R, **kw))
    if name == "constant":
        taps = kw.get("taps", 16)
        r["Gtaps_per_s"] = round(taps * P / (r["call_ms"] * 1e-3) / 1e9, 1)
    result["motion_blur"][f"{name}_r{R}{suffix}"] = r
    show(f"motion_blur_device {W}x{H} {name} R={R}{suffix}", r)
copy = per_call(lambda: check(hip.hipMemcpyAsync(out, rgb, 12 * P, 3, T.stream), "hipMemcpyAsync"))  # hipMemcpyDeviceToDevice
copy["bytes_moved"] = 24 * P
copy["GBps"] = round(copy["bytes_moved"] / (copy["call_ms"] * 1e-3) / 1e9, 1)
result["copy"] = copy
show(f"device-to-device copy {W}x{H}", copy)
dof = per_call(lambda: ctx.dof_device(rgb, depth, out, W, H, max_radius=8, focus=2.0, scale=8 / 1.5))
result["dof_ramp_r8"] = dof
show(f"dof_device {W}x{H} ramp R=8", dof)
for r in result["motion_blur"].values():
    r["over_copy"] = round(r["call_ms"] / copy["call_ms"], 3)
    r["over_dof"] = round(r["call_ms"] / dof["call_ms"], 3)
ctx.close()

result = {"motion_blur_cost": result}
if not args.no_write:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, allow_nan=False)
        fh.write("\n")
print(json.dumps(result))
