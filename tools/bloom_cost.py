#!/usr/bin/env python3
"""Developer tool (GPU box): what the bloom call costs (include/pbrs_gpu.h, pbrsb_bloom_device).
Time, with HIP events on the context's stream, after a warm-up, as medians of repeated batches (tools/despeckle_cost.py's method; a batch
of calls between two events, because one call is tens of microseconds), on HDR noise at 1920 x 1080 and at 512 x 512, 6 levels:
  - pbrsb_bloom_device with the defaults (additive) and with PBRS_BLOOM_MIX at threshold 0, out of place and in place;
and beside each, in the same run, two yardsticks:
  - a device-to-device copy of the same image on the same stream, the floor of any operation that reads and writes it once;
  - pbrsi_despeckle_device at the same size (radius 1, image only, no record), an operation of the same shape.
--no-tail-lib PATH: a build of the library with -DPBRS_BLOOM_NO_TAIL (make -C pbrs_amd/csrc gpu NAME=abl_bloom_notail
HIPCC_EXTRA=-DPBRS_BLOOM_NO_TAIL), which takes every level through k_bloom_down and k_bloom_up; it is measured by a fresh process of
this tool with PBRS_GPU_LIB set, after this one has closed its context, and lands under "no_tail".
The device is kept busy for --warm seconds before the first timed batch, and the first form is timed again after the last one
("..._again").  Writes profiles/bloom_cost.json (or --out) and prints it; --no-write only prints (the run to put under rocprofv3
--kernel-trace --stats).
    python tools/bloom_cost.py [--runs N] [--batch N] [--warm S] [--no-tail-lib PATH] [--no-write] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time as clock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--batch", type=int, default=20)
ap.add_argument("--warm", type=float, default=1.0)
ap.add_argument("--no-tail-lib", default=None)
ap.add_argument("--no-write", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bloom_cost.json"))
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
LEVELS = 6
FORMS = {"additive": dict(levels=LEVELS), "mix": dict(levels=LEVELS, threshold=0.0, knee=0.0, strength=0.3, mix=True)}


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


def launches(w, h, levels, tail_pixels=5461):
    """(with the tail, without it) of a call at w x h: the header's level sizes and device/bloom.h's rule for where the tail begins."""
    sizes = []
    while len(sizes) < levels:
        w, h = (w + 1) // 2, (h + 1) // 2
        sizes.append(w * h)
        if (w, h) == (1, 1):
            break
    n = len(sizes)
    t = 0
    while t < n - 1 and sum(sizes[t:]) > tail_pixels:
        t += 1
    return (t + 1) + (1 if t < n - 1 else 0) + t + 1, 2 * n


result = {"runs": args.runs, "batch": args.batch, "warm_s": args.warm, "levels": LEVELS, "hbm_peak_GBps": HBM_PEAK_GBS,
          "library": os.path.basename(os.environ.get("PBRS_GPU_LIB") or "libpbrs_gpu.so"), "sizes": {}}
rng = np.random.default_rng(1)
for W, H in ((1920, 1080), (512, 512)):
    P = W * H
    img = np.exp2(rng.uniform(-6, 6, (H, W, 3))).astype(f32)
    rgb, out = upload(img), T.dev_alloc(12 * P).value
    until = clock.monotonic() + args.warm
    while clock.monotonic() < until:
        for _ in range(100):
            ctx.bloom_device(rgb, out, W, H, **FORMS["additive"])
        ctx.collect_stats()
    with_tail, without = launches(W, H, LEVELS)
    here = {"launches_with_tail": with_tail, "launches_without_tail": without, "bloom": {}}
    order = [(name, False, "") for name in FORMS] + [("additive", True, "_in_place"), ("additive", False, "_again")]
    for name, in_place, suffix in order:
        r = per_call(lambda: ctx.bloom_device(rgb, rgb if in_place else out, W, H, **FORMS[name]))
        here["bloom"][name + suffix] = r
        show(f"bloom_device {W}x{H} {name}{suffix}", r)
    check(hip.hipMemcpy(rgb, img.ctypes.data, img.nbytes, 1), "hipMemcpy")  # the in-place form has bloomed the image over and over
    copy = per_call(lambda: check(hip.hipMemcpyAsync(out, rgb, 12 * P, 3, T.stream), "hipMemcpyAsync"))  # hipMemcpyDeviceToDevice
    copy["bytes_moved"] = 24 * P
    copy["GBps"] = round(copy["bytes_moved"] / (copy["call_ms"] * 1e-3) / 1e9, 1)
    here["copy"] = copy
    show(f"device-to-device copy {W}x{H}", copy)
    desp = per_call(lambda: ctx.despeckle_device(rgb, out, W, H, None, {}))
    here["despeckle"] = desp
    show(f"despeckle_device {W}x{H}", desp)
    for r in here["bloom"].values():
        r["over_copy"] = round(r["call_ms"] / copy["call_ms"], 3)
        r["over_despeckle"] = round(r["call_ms"] / desp["call_ms"], 3)
    result["sizes"][f"{W}x{H}"] = here
ctx.close()

if args.no_tail_lib:
    env = dict(os.environ, PBRS_GPU_LIB=os.path.abspath(args.no_tail_lib))
    cmd = [sys.executable, os.path.abspath(__file__), "--runs", str(args.runs), "--batch", str(args.batch), "--warm", str(args.warm), "--no-write"]
    child = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if child.returncode != 0:
        raise RuntimeError(f"the run without the tail failed ({child.returncode}):\n{child.stdout}\n{child.stderr}")
    result["no_tail"] = json.loads(child.stdout.strip().splitlines()[-1])["bloom_cost"]

result = {"bloom_cost": result}
if not args.no_write:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, allow_nan=False)
        fh.write("\n")
print(json.dumps(result))
