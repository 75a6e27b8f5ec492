#!/usr/bin/env python3
"""Developer tool (GPU box): what the depth-of-field call costs (include/pbrs_gpu.h, pbrsf_dof_device).
Time, with HIP events on the context's stream, after a warm-up, as medians of repeated batches (tools/bloom_cost.py's method; a batch of
calls between two events), on HDR noise at 512 x 512 and at 1920 x 1080, max_radius 4, 8 and 16 (the kernel's three halo classes), over
three depths:
  - "sharp":   the depth constant at the focus: every block copies its tile;
  - "ramp":    the depth grows along x through the focus, the circles from 0 to max_radius: blocks cut their loops at their own largest circle;
  - "blurred": nothing hit (+inf), scale above max_radius: every circle is max_radius, every block runs the whole disk of taps;
and beside each size, in the same run, two yardsticks:
  - a device-to-device copy of the same image on the same stream, the floor of any operation that reads and writes it once;
  - pbrsb_bloom_device at the same size with its defaults, the chain's neighbour.
"taps" is the number of (dx, dy) the blurred form's loop visits per pixel, the disk of device/dof.h's block-wide test.
The device is kept busy for --warm seconds before the first timed batch, and the first form is timed again after the last one
("..._again").  Writes profiles/dof_cost.json (or --out) and prints it; --no-write only prints.
    python tools/dof_cost.py [--runs N] [--batch N] [--warm S] [--no-write] [--out PATH]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dof_cost.json"))
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
FOCUS = 2.0
RADII = (4, 8, 16)


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


def disk_taps(R):
    """The taps of a block whose largest circle is R: (R - dist) + 0.5 > 0 in f32."""
    d = np.sqrt((np.arange(-R, R + 1, dtype=f32)[:, None] ** 2 + np.arange(-R, R + 1, dtype=f32)[None, :] ** 2).astype(f32))
    return int((((f32(R) - d).astype(f32) + f32(0.5)) > 0).sum())


result = {"runs": args.runs, "batch": args.batch, "warm_s": args.warm, "hbm_peak_GBps": HBM_PEAK_GBS, "focus": FOCUS, "sizes": {}}
rng = np.random.default_rng(1)
for W, H in ((512, 512), (1920, 1080)):
    P = W * H
    img = np.exp2(rng.uniform(-6, 6, (H, W, 3))).astype(f32)
    rgb, out = upload(img), T.dev_alloc(12 * P).value
    depths = {"sharp": np.full((H, W), FOCUS, f32),
              "ramp": np.tile((FOCUS * (0.4 + 1.6 * np.arange(W) / (W - 1))).astype(f32), (H, 1)),
              "blurred": np.full((H, W), np.inf, f32)}
    dev_depth = {n: upload(z) for n, z in depths.items()}

    def form(name, R):
        # ramp: |z - F| / z reaches 1.5 at the near end: scale R / 1.5 takes the circles from 0 to R; blurred: q = 1, r = R
        scale = {"sharp": float(R), "ramp": R / 1.5, "blurred": 2.0 * R}[name]
        return lambda: ctx.dof_device(rgb, dev_depth[name], out, W, H, max_radius=R, focus=FOCUS, scale=scale)

    until = clock.monotonic() + args.warm
    while clock.monotonic() < until:
        for _ in range(20):
            form("ramp", 8)()
        ctx.collect_stats()
    here = {"dof": {}}
    order = [(name, R, "") for R in RADII for name in depths] + [("sharp", RADII[0], "_again")]
    for name, R, suffix in order:
        r = per_call(form(name, R))
        if name == "blurred":
            r["taps"] = disk_taps(R)
            r["Gtaps_per_s"] = round(r["taps"] * P / (r["call_ms"] * 1e-3) / 1e9, 1)
        here["dof"][f"{name}_r{R}{suffix}"] = r
        show(f"dof_device {W}x{H} {name} R={R}{suffix}", r)
    copy = per_call(lambda: check(hip.hipMemcpyAsync(out, rgb, 12 * P, 3, T.stream), "hipMemcpyAsync"))  # hipMemcpyDeviceToDevice
    copy["bytes_moved"] = 24 * P
    copy["GBps"] = round(copy["bytes_moved"] / (copy["call_ms"] * 1e-3) / 1e9, 1)
    here["copy"] = copy
    show(f"device-to-device copy {W}x{H}", copy)
    bloom = per_call(lambda: ctx.bloom_device(rgb, out, W, H))
    here["bloom"] = bloom
    show(f"bloom_device {W}x{H}", bloom)
    for r in here["dof"].values():
        r["over_copy"] = round(r["call_ms"] / copy["call_ms"], 3)
        r["over_bloom"] = round(r["call_ms"] / bloom["call_ms"], 3)
    result["sizes"][f"{W}x{H}"] = here
ctx.close()

result = {"dof_cost": result}
if not args.no_write:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, allow_nan=False)
        fh.write("\n")
print(json.dumps(result))
