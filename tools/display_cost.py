#!/usr/bin/env python3
"""Developer tool (GPU box): what the display transform costs (include/pbrs_gpu.h, pbrs_display_device; device/display.h) at 1920 x 1080,
and what the path it replaces costs on the same machine.

The transform, on device buffers, ACES + sRGB + rounding: k_display_apply alone (a fixed exposure), and with the auto exposure (the
histogram's memset, k_display_hist, k_display_resolve, then k_display_apply), each on a log-normal noise image and on a constant image.
The constant image is the worst case of k_display_hist: every LDS add of a block lands on one address.  Timed with HIP events on the
context's stream (tools/hip_event_timing.py) around --batch back-to-back calls after a warm-up, as the median of --runs such batches, per
call.  The 25 MB plane stays in the Infinity Cache between calls: these are warm numbers, as they are behind a filter that has just
written the plane.  Compulsory bytes per pixel: 12 read + 4 written by the apply kernel, 12 more read by the histogram.

The path this replaces uses nothing of the transform (the same calls exist without it): the f32 plane copied to pageable host memory
(hipMemcpy, a host clock around the synchronous copy) and converted there with pbrs_host_write_png's arithmetic, sqrt then the saturating
cast: once as numpy does it in one thread, and once as the whole pbrs_host_write_png call into a scratch file, which also deflates and
writes the PNG.  Medians of --host-runs.
Writes profiles/display_cost.json (or --out) and prints it.
    python tools/display_cost.py [--runs N] [--batch N] [--host-runs N] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--host-runs", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "display_cost.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import pbrs_amd  # noqa: E402

from hip_event_timing import Timing, check  # noqa: E402

T = Timing(pbrs_amd, warmup=2)
ctx, hip = T.ctx, T.hip
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
f32 = np.float32
w, h = 1920, 1080
P = w * h
rng = np.random.default_rng(1)
images = {"noise": (np.exp2(rng.normal(0.0, 2.0, size=(h, w, 1))) * rng.uniform(0.5, 1.0, size=(h, w, 3))).astype(f32),
          "constant": np.full((h, w, 3), 0.5, dtype=f32)}
out_dev = T.dev_alloc(4 * P)
word = T.dev_alloc(4)
check(hip.hipMemcpy(word, np.ones(1, f32).ctypes.data, 4, 1), "hipMemcpy")
settings = dict(curve="aces", encode="srgb", quantize="round")
result = {"runs": args.runs, "batch": args.batch, "size": f"{w}x{h}", "settings": settings, "cases": {}, "replaced_path": {}}
for name, img in images.items():
    rgb_dev = T.dev_alloc(img.nbytes)
    check(hip.hipMemcpy(rgb_dev, img.ctypes.data, img.nbytes, 1), "hipMemcpy")  # hipMemcpyHostToDevice
    io = {"exposure_in": word.value, "exposure_out": word.value}
    for case, kw, nbytes in (("apply", dict(exposure=0.7), 16), ("auto", dict(auto=True, adapt=0.5), 28)):
        def batch():
            for _ in range(args.batch):
                ctx.display_device(rgb_dev.value, out_dev.value, w, h, io if case == "auto" else None, **settings, **kw)
        r = T.median_of(batch, args.runs)
        ms = r["median_ms"] / args.batch
        result["cases"][f"{name}_{case}"] = {"batch_ms": r["ms"], "call_ms": round(ms, 5), "compulsory_GB_per_s": round(nbytes * P / (ms * 1e-3) / 1e9, 1)}
        print(f"{name}, {case}: {ms * 1e3:.1f} us per call, {nbytes * P / (ms * 1e-3) / 1e9:.0f} GB/s of compulsory traffic", flush=True)
    c = result["cases"]
    c[f"{name}_auto"]["histogram_and_resolve_ms"] = round(c[f"{name}_auto"]["call_ms"] - c[f"{name}_apply"]["call_ms"], 5)
    if name == "noise":  # the path this replaces, on the plane that is on the device now
        host = np.empty_like(img)
        down, conv, png = [], [], []
        with tempfile.TemporaryDirectory() as d:
            for k in range(args.host_runs + 1):
                t0 = time.perf_counter()
                check(hip.hipMemcpy(host.ctypes.data, rgb_dev, img.nbytes, 2), "hipMemcpy")  # hipMemcpyDeviceToHost, synchronous
                t1 = time.perf_counter()
                with np.errstate(invalid="ignore"):
                    g = np.sqrt(host)
                    u8 = np.where(g > 1.0, 255, np.where(g >= 0.0, np.nan_to_num(g * f32(255.0), nan=0.0), 0)).astype(np.uint8)
                t2 = time.perf_counter()
                pbrs_amd.write_image(os.path.join(d, "a.png"), host)
                t3 = time.perf_counter()
                if k:  # the first round warms up
                    down.append(round((t1 - t0) * 1e3, 3)), conv.append(round((t2 - t1) * 1e3, 3)), png.append(round((t3 - t2) * 1e3, 3))
        assert u8.shape == (h, w, 3)
        result["replaced_path"] = {"download_f32_ms": down, "numpy_sqrt_cast_ms": conv, "pbrs_host_write_png_ms": png,
                                   "median_download_ms": statistics.median(down), "median_numpy_sqrt_cast_ms": statistics.median(conv),
                                   "median_pbrs_host_write_png_ms": statistics.median(png)}
        print(f"replaced path: download {statistics.median(down):.2f} ms, numpy sqrt + cast {statistics.median(conv):.2f} ms, "
              f"pbrs_host_write_png (with deflate and the file) {statistics.median(png):.1f} ms", flush=True)
    hip.hipFree(rgb_dev)
c = result["cases"]
result["constant_over_noise_histogram"] = round(c["constant_auto"]["histogram_and_resolve_ms"] / c["noise_auto"]["histogram_and_resolve_ms"], 3)
hip.hipFree(out_dev)
hip.hipFree(word)
ctx.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"display_cost": result}, f, indent=1)
    f.write("\n")
print(json.dumps({"display_cost": result}))
