#!/usr/bin/env python3
"""Developer tool (GPU box): what the image comparison costs (include/pbrs_gpu.h, pbrsx_compare_device), next to one iteration of the
variance-guided denoiser in the same process.  Timed with HIP events on the context's stream, after a warm-up, as medians of repeated
batches (tools/denoise_var_cost.py's method; a batch of calls between two events, because one call is tens of microseconds):
  - pbrsx_compare_device on a 1920 x 1080 HDR image pair in three forms: with SSIM, without, and with SSIM and both maps;
  - pbrs_denoise_var_device on the same image with all guides, the difference of the 2- and the 1-iteration medians: one iteration.
Beside each form the bytes it must move (24 B per pixel read, 4 B per pixel and map written; a tile's 52-byte record written and read once)
and what share of the HBM peak that is at the measured time: a floor on the traffic (the SSIM forms read their halo through the caches).
Writes profiles/compare_cost.json (or --out) and prints it.
    python tools/compare_cost.py [--runs N] [--batch N] [--out PATH]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare_cost.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import pbrs_amd  # noqa: E402
from pbrs_amd import api  # noqa: E402
from pbrs_amd.roofline import HBM_PEAK_GBS  # noqa: E402

from hip_event_timing import Timing, check  # noqa: E402

T = Timing(pbrs_amd, warmup=2)
ctx, hip = T.ctx, T.hip
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
f32 = np.float32
W, H = 1920, 1080
P = W * H
GUIDES = ("albedo", "normal", "depth", "instance")


def upload(a):
    a = np.ascontiguousarray(a)
    ptr = T.dev_alloc(a.nbytes)
    check(hip.hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy")  # hipMemcpyHostToDevice
    return ptr.value


rng = np.random.default_rng(1)
ref = (rng.random((H, W, 3)) ** 4 * 20).astype(f32)
img = (ref + rng.normal(0, 0.5, ref.shape)).astype(f32)
a, b = upload(img), upload(ref)
error_map, ssim_map, record = (T.dev_alloc(n).value for n in (4 * P, 4 * P, 64))
yy, xx = np.mgrid[0:H, 0:W]
ids = ((xx > 700).astype(np.uint32) + 2 * (yy > 600).astype(np.uint32)).astype(np.uint32)
normal = np.zeros((H, W, 3), dtype=f32)
normal[..., 2] = 1.0
guides = {"albedo": upload((0.2 + 0.6 * rng.random((H, W, 3))).astype(f32)), "normal": upload(normal),
          "depth": upload((2.0 + 0.001 * xx + 0.0005 * yy + 1.5 * ids).astype(f32)), "instance": upload(ids)}
variance = upload((rng.random((H, W)) * 0.1).astype(f32))
out = T.dev_alloc(3 * P * 4).value


def per_call(fn):
    def batch():
        for _ in range(args.batch):
            fn()
    r = T.median_of(batch, args.runs)
    calls = sorted(ms / args.batch for ms in r["ms"])
    return {"batch_ms": r["ms"], "call_ms": round(r["median_ms"] / args.batch, 5), "call_ms_min": round(calls[0], 5), "call_ms_max": round(calls[-1], 5)}


tiles = -(-W // api.CompareParams.TILE) * -(-H // api.CompareParams.TILE)
FORMS = {"ssim": (dict(ssim=True), None, 0), "no_ssim": (dict(ssim=False), None, 0),
         "ssim_both_maps": (dict(ssim=True), {"error_out": error_map, "ssim_out": ssim_map}, 2)}
result = {"size": f"{W}x{H}", "runs": args.runs, "batch": args.batch, "hbm_peak_GBps": HBM_PEAK_GBS, "tiles": tiles, "forms": {}}
for name, (kw, maps, n_maps) in FORMS.items():
    r = per_call(lambda: ctx.compare_device(a, b, W, H, record, maps, **kw))
    r["bytes_moved"] = 24 * P + 4 * P * n_maps + 2 * 52 * tiles + 64
    r["GBps"] = round(r["bytes_moved"] / (r["call_ms"] * 1e-3) / 1e9, 1)
    r["share_of_hbm_peak"] = round(r["GBps"] / HBM_PEAK_GBS, 4)
    result["forms"][name] = r
    print(f"compare_device, {name}: {r['call_ms'] * 1e3:.1f} us per call ({r['call_ms_min'] * 1e3:.1f} .. {r['call_ms_max'] * 1e3:.1f}), "
          f"{r['bytes_moved'] / 1e6:.1f} MB, {r['GBps']:.0f} GB/s, {100 * r['share_of_hbm_peak']:.1f} % of the HBM peak", flush=True)

one, two = (per_call(lambda: ctx.denoise_var_device(a, out, W, H, variance, guides, iterations=n)) for n in (1, 2))
result["denoise_var"] = {"iterations_1": one, "iterations_2": two, "one_iteration_ms": round(two["call_ms"] - one["call_ms"], 5)}
base = result["denoise_var"]["one_iteration_ms"]
print(f"denoise_var_device: {one['call_ms'] * 1e3:.1f} us at one iteration, {two['call_ms'] * 1e3:.1f} us at two: {base * 1e3:.1f} us per iteration", flush=True)
for name, r in result["forms"].items():
    r["over_denoise_var_iteration"] = round(r["call_ms"] / base, 3)
ctx.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump({"compare_cost": result}, fh, indent=1)
    fh.write("\n")
print(json.dumps({"compare_cost": result}))
