#!/usr/bin/env python3
"""Developer tool (GPU box): what the spatial variance estimate costs (include/pbrs_gpu.h, pbrs_spatial_variance_device;
device/spatial_variance.h).  The one kernel, in place on the variance, with all guides and the id stop at radius 3, on synthetic buffers
(a slanted wall, ids in 64-pixel blocks as tools/temporal_cost.py lays them out; the time depends on the guides only through how many
taps they close), at 1920 x 1080 and 3840 x 2160, for three histories:
    all_short    every length 1: the first frame of a sequence; every block stages its tile and every pixel runs its 49 taps
    all_long     every length 8: the steady state; every block votes, writes variance_in through and returns
    blocks_20    about 20 % of the 64-pixel id blocks are short, the rest long: disocclusions; a 16 x 16 block is all one or the other
Timed with HIP events on the context's stream (tools/hip_event_timing.py) around --batch back-to-back launches after a warm-up, as the
median of --runs such batches, per launch.  Next to the time: the compulsory bytes of the history over it (a pixel of a block that
stages reads 36 B: moments, length, variance, depth, normal, instance; a pixel of a block that passes through reads 8 B: length and
variance; both write 4 B), and for all_long the same window around --batch device-to-device copies of one plane (4 B read, 4 B
written per pixel).  Back-to-back launches over the same planes: what fits the Infinity Cache (256 MB; the 1920 x 1080 planes do) is
read from there, not from HBM.
Writes profiles/spatial_variance_cost.json (or --out) and prints it.
    python tools/spatial_variance_cost.py [--runs N] [--batch N] [--out PATH]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_variance_cost.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import pbrs_amd  # noqa: E402
from pbrs_amd import api  # noqa: E402

from hip_event_timing import Timing, check  # noqa: E402

T = Timing(pbrs_amd, warmup=2)
ctx, hip = T.ctx, T.hip
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
STAGED_READ, THROUGH_READ, WRITTEN, HBM_COPY_RATE = 36, 8, 4, 6.3e12
f32 = np.float32


def upload(a):
    a = np.ascontiguousarray(a)
    ptr = T.dev_alloc(a.nbytes)
    check(hip.hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy")  # hipMemcpyHostToDevice
    return ptr.value


params = dict(radius=3, id_stop=True)
result = {"runs": args.runs, "batch": args.batch, "staged_read_bytes_per_pixel": STAGED_READ, "pass_through_read_bytes_per_pixel": THROUGH_READ,
          "written_bytes_per_pixel": WRITTEN,
          "params": {k: (round(v, 6) if isinstance(v, float) else v) for k, v in api.SpatialVarianceParams.make(0, 0, **params).as_dict().items()},
          "sizes": {}}
for w, h in ((1920, 1080), (3840, 2160)):
    rng = np.random.default_rng(1)
    P = w * h
    yy, xx = np.mgrid[0:h, 0:w]
    y = rng.normal(2.0, 0.5, size=(h, w)).astype(f32)
    block = (yy // 64) * 64 + xx // 64
    short_block = rng.uniform(size=int(block.max()) + 1) < 0.2
    lengths = {"all_short": np.ones((h, w), f32), "all_long": np.full((h, w), 8.0, f32),
               "blocks_20": np.where(short_block[block], 1.0, 8.0).astype(f32)}
    dev = {"moments": upload(np.stack([y, y * y], axis=2)), "variance": upload(np.full((h, w), np.inf, f32)),
           "depth": upload((5.0 + 0.002 * xx + 0.001 * yy).astype(f32)),
           "normal": upload(np.stack([np.full((h, w), -0.2), np.zeros((h, w)), -np.ones((h, w))], axis=2).astype(f32)),
           "instance": upload(block.astype(np.uint32)), "copy": upload(np.zeros((h, w), f32))}
    guides = {n: dev[n] for n in ("depth", "normal", "instance")}
    sizes = result["sizes"][f"{w}x{h}"] = {}
    for name, length in lengths.items():
        dev_length = upload(length)
        # 16 x 16 blocks that hold a short pixel stage their tile; with 64-pixel id blocks a block is all short or all long
        short = float((length < 4.0).mean())
        nbytes = P * (short * STAGED_READ + (1.0 - short) * THROUGH_READ + WRITTEN)

        def batch():
            for _ in range(args.batch):
                # in place: the variance stays +inf where nothing is short, and is re-estimated from the same moments where it is
                ctx.spatial_variance_device(dev["moments"], dev_length, dev["variance"], dev["variance"], w, h, guides, **params)
        r = T.median_of(batch, args.runs)
        ms = r["median_ms"] / args.batch
        rate = nbytes / (ms * 1e-3)
        sizes[name] = {"batch_ms": r["ms"], "kernel_ms": round(ms, 5), "short_pixels": round(short, 4), "compulsory_MB": round(nbytes / 1e6, 1),
                       "compulsory_GB_per_s": round(rate / 1e9, 1), "share_of_hbm_copy_rate": round(rate / HBM_COPY_RATE, 3),
                       "ns_per_short_pixel": round(ms * 1e6 / (short * P), 4) if short else None}
        print(f"{w} x {h} {name}: {ms * 1e3:.1f} us per launch, {short:.3f} short, {nbytes / 1e6:.1f} MB compulsory -> {rate / 1e9:.0f} GB/s "
              f"({rate / HBM_COPY_RATE:.2f} of the HBM copy rate)", flush=True)
        hip.hipFree(C.c_void_p(dev_length))

    def copies():
        for _ in range(args.batch):
            check(hip.hipMemcpyAsync(C.c_void_p(dev["copy"]), C.c_void_p(dev["variance"]), 4 * P, 3, T.stream), "hipMemcpyAsync")  # DeviceToDevice
    r = T.median_of(copies, args.runs)
    ms = r["median_ms"] / args.batch
    sizes["one_plane_copy"] = {"batch_ms": r["ms"], "copy_ms": round(ms, 5), "GB_per_s": round(8 * P / (ms * 1e-3) / 1e9, 1),
                               "all_long_over_copy": round(sizes["all_long"]["kernel_ms"] / ms, 3)}
    print(f"{w} x {h} one-plane copy: {ms * 1e3:.1f} us; all_long / copy = {sizes['one_plane_copy']['all_long_over_copy']}", flush=True)
    for ptr in dev.values():
        hip.hipFree(C.c_void_p(ptr))
ctx.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"spatial_variance_cost": result}, f, indent=1)
    f.write("\n")
print(json.dumps({"spatial_variance_cost": result}))
