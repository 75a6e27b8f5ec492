#!/usr/bin/env python3
"""Developer tool (GPU box): what the light passes cost and what denoising them apart buys (include/pbrs_gpu.h,
pbrs_render_tile_passes_device, pbrs_combine_passes_device), modelled on tools/denoise_var_cost.py.  In one process, timed with HIP
events on the context's stream after a warm-up:
  - a full frame of each config (default C2 and C4) without passes and with all four: medians of the frame time, and the per-stage
    milliseconds of pbrs_stats of a timed render of each on one stream (k_pass_fold counts in ms_accumulate; k_pass_direct, outside the
    stage brackets, shows in ms_total alone);
  - the Cornell box at a low sample count: the relative mean squared error, against a render at many samples, of the plain image, of
    render_denoised_var (one filter over the image) and of render_denoised_passes (direct and indirect light filtered apart).
Both are measurements to be read, not thresholds.  Writes profiles/passes_cost.json (or --out) and prints it.
    python tools/passes_cost.py [--configs c2,c4] [--runs N] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="c2,c4")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--size", type=int, default=256, help="side of the Cornell box frame of the error comparison")
ap.add_argument("--low", type=int, default=2, help="strata per axis of the denoised renders")
ap.add_argument("--high", type=int, default=48, help="strata per axis of the reference render")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "passes_cost.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import pbrs_amd  # noqa: E402
from pbrs_amd import api, scenes  # noqa: E402

from hip_event_timing import Timing  # noqa: E402

T = Timing(pbrs_amd, warmup=1)
ctx, median_of, dev_alloc = T.ctx, T.median_of, T.dev_alloc
STAGES = ("ms_raygen", "ms_extend", "ms_shade", "ms_shadow", "ms_accumulate", "ms_total")
result = {"runs": args.runs, "frames": {}}

for name in args.configs.split(","):
    sb, cfg = scenes.build_config(name)
    W, H = cfg["width"], cfg["height"]
    sx, sy, depth = cfg["strata_x"], cfg["strata_y"], cfg["depth"]
    ctx.upload(pbrs_amd.HostScene(sb))
    P = W * H
    rgb = dev_alloc(3 * P * 4).value
    layers = {n: dev_alloc(api.PASS_CHANNELS[n] * P * 4).value for n in api.PASSES}
    frames = {}
    for which, ptrs in (("plain", {}), ("passes", layers)):
        def frame(ptrs=ptrs, **kw):
            ctx.render_passes_device(rgb, ptrs, sx, sy, depth, args.seed, **kw)
        frames[which] = median_of(frame, args.runs)
        # timed renders on one stream: the stages' exclusive milliseconds
        ctx.set_pass_overlap(False)
        timed = []
        for _ in range(3):
            frame(timing=True)
            timed.append(ctx.collect_stats())
        ctx.set_pass_overlap(True)
        frames[which]["stages_ms"] = {s: round(statistics.median(st[s] for st in timed), 3) for s in STAGES}
        frames[which]["passes"] = timed[-1]["passes"]
        print(f"{name} frame, {which}: {frames[which]['median_ms']:.2f} ms; one stream: {frames[which]['stages_ms']} over {timed[-1]['passes']} passes",
              flush=True)
    frames["passes_over_plain"] = round(frames["passes"]["median_ms"] / frames["plain"]["median_ms"], 4)
    frames["samples"] = P * sx * sy
    result["frames"][name] = frames
    for ptr in [rgb] + list(layers.values()):
        T.hip.hipFree(C.c_void_p(ptr))

# denoising the layers apart against denoising the image, on the Cornell box
sb, cfg = scenes.build_config("c2", width=args.size, height=args.size)
ctx.upload(pbrs_amd.HostScene(sb))
depth = cfg["depth"]
ref, _ = ctx.render(args.high, args.high, depth, args.seed + 100)


def rel_mse(img):
    return float(np.mean((img.astype(np.float64) - ref) ** 2 / (ref.astype(np.float64) ** 2 + 1e-2)))


one, noisy, _ = ctx.render_denoised_var(args.low, args.low, depth, args.seed, keep_noisy=True)
split, _ = ctx.render_denoised_passes(args.low, args.low, depth, args.seed)
result["cornell_rel_mse"] = {"size": args.size, "spp": args.low ** 2, "reference_spp": args.high ** 2, "noisy": rel_mse(noisy),
                             "render_denoised_var": rel_mse(one), "render_denoised_passes": rel_mse(split)}
print("Cornell relative MSE:", result["cornell_rel_mse"], flush=True)
ctx.close()

with open(args.out, "w") as f:
    json.dump({"passes_cost": result}, f, indent=1)
    f.write("\n")
print(json.dumps({"passes_cost": result}))
