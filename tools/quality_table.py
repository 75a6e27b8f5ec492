#!/usr/bin/env python3
"""Developer tool (GPU box): what every step of the image chain buys, measured by the library's own comparison (Context.compare,
include/pbrs_gpu.h "image comparison": REINHARD transform, SSIM at peak 1).  The Cornell box at 256 x 256 against a reference of
--ref-strata^2 samples per pixel, at 1, 4 and 16 samples per pixel:
    noisy                 Context.render
    denoise               Context.render_denoised
    denoise_var           Context.render_denoised_var
    accumulated_8         the eighth frame of Context.render_temporal over a still camera, before the filter
    accumulated_8_filter  ... and after it
    upscaled_x2           Context.render_upscaled at factor 2 (the samples are per traced, low-resolution pixel)
For each mse, rel_mse, ssim and psnr, next to the milliseconds of the driver call that made the image (HIP events around the whole call,
copies back included; medians of --runs after a warm-up; the sequence's figure is all eight frames).
Writes profiles/quality_table.json (or --out) and prints it.
    python tools/quality_table.py [--size 256] [--ref-strata 32] [--runs N] [--out PATH]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--ref-strata", type=int, default=32)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality_table.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import pbrs_amd  # noqa: E402
from pbrs_amd import scenes  # noqa: E402

from hip_event_timing import Timing  # noqa: E402

T = Timing(pbrs_amd, warmup=1)
ctx = T.ctx
n, depth = args.size, args.depth
hs = pbrs_amd.HostScene(scenes.cornell_scene(width=n, height=n))
ctx.upload(hs)
reference, _ = ctx.render(args.ref_strata, args.ref_strata, depth, 4242)
FRAMES = 8


def sequence(s):
    last = None
    for last in ctx.render_temporal([hs.camera] * FRAMES, s, s, depth, [100 + k for k in range(FRAMES)]):
        pass
    return last


STEPS = {
    "noisy": lambda s: ctx.render(s, s, depth, 17)[0],
    "denoise": lambda s: ctx.render_denoised(s, s, depth, 17)[0],
    "denoise_var": lambda s: ctx.render_denoised_var(s, s, depth, 17)[0],
    "accumulated_8": lambda s: sequence(s)[1],
    "accumulated_8_filter": lambda s: sequence(s)[0],
    "upscaled_x2": lambda s: ctx.render_upscaled(s, s, depth, 17, factor=2)[0],
}
result = {"scene": "cornell", "size": f"{n}x{n}", "depth": depth, "reference": f"{args.ref_strata}x{args.ref_strata} strata, seed 4242",
          "runs": args.runs, "compare": pbrs_amd.CompareParams.make(n, n).as_dict(), "spp": {}}
for s in (1, 2, 4):
    rows = {}
    for name, step in STEPS.items():
        kept = {}

        def run(step=step):
            kept["image"] = step(s)
        t = T.median_of(run, args.runs)
        r = ctx.compare(kept["image"], reference)
        rows[name] = {"mse": r.mse, "rel_mse": r.rel_mse, "ssim": r.ssim, "psnr_db": round(r.psnr(), 3), "n_valid": r.n_valid,
                      "median_ms": t["median_ms"], "ms": t["ms"]}
        print(f"{s * s:2d} spp {name:22s} mse {r.mse:.3e} rel_mse {r.rel_mse:.3e} ssim {r.ssim:.4f} psnr {r.psnr():6.2f} dB  {t['median_ms']:8.3f} ms", flush=True)
    result["spp"][str(s * s)] = rows
ctx.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump({"quality_table": result}, fh, indent=1)
    fh.write("\n")
print(json.dumps({"quality_table": result}))
