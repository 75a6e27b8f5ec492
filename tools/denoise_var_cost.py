#!/usr/bin/env python3
"""Developer tool (GPU box): what the variance AOV and the variance-guided denoiser cost (include/pbrs_gpu.h,
pbrs_render_tile_aovs_var_device, pbrs_denoise_var_device), next to the plain denoiser in the same process on the same image.  Timed
with HIP events on the context's stream, after a warm-up, as medians of repeated runs (tools/denoise_cost.py's method):
  - pbrs_denoise_var_device and pbrs_denoise_device alone on a 1920 x 1080 image with all guides and both flags, for 1 .. 6
    iterations; the difference of two consecutive medians is the iteration at the larger spacing (the 1-iteration figure also holds
    pack and unpack);
  - a frame of one config (default C4) with the AOVs, and with the AOVs and the variance: the frame times, and pbrs_stats::ms_accumulate
    of a timed render of each (the moments kernel's time counts there), per pass.
Writes profiles/denoise_var_cost.json (or --out) and prints it.
    python tools/denoise_var_cost.py [--config c4] [--runs N] [--out PATH] [--once]
--once: no timing, one variance-guided and one plain denoise at five iterations (the run to put under rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--config", default="c4")
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--once", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_var_cost.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import pbrs_amd  # noqa: E402
from pbrs_amd import api, scenes  # noqa: E402

from hip_event_timing import Timing  # noqa: E402

T = Timing(pbrs_amd, warmup=2)
ctx, median_of, dev_alloc = T.ctx, T.median_of, T.dev_alloc

sb, cfg = scenes.build_config(args.config)
W, H = cfg["width"], cfg["height"]
sx, sy, depth = cfg["strata_x"], cfg["strata_y"], cfg["depth"]
ctx.upload(pbrs_amd.HostScene(sb))
P = W * H
CHANNELS = {"rgb": 3, "out": 3, "albedo": 3, "normal": 3, "depth": 1, "instance": 1, "variance": 1}
dev = {n: dev_alloc(ch * P * 4) for n, ch in CHANNELS.items()}
guides = {n: dev[n].value for n in ("albedo", "normal", "depth", "instance")}
rgb, out, var = dev["rgb"].value, dev["out"].value, dev["variance"].value

# the image, its guides and its variance, rendered once at few samples (the cost depends little on the values' noise)
ctx.render_aovs_var_device(rgb, guides, var, 2, 2, depth, args.seed)
ctx.collect_stats()

if args.once:
    ctx.denoise_var_device(rgb, out, W, H, var, guides, iterations=5)
    ctx.denoise_device(rgb, out, W, H, guides, iterations=5)
    ctx.collect_stats()
    ctx.close()
    sys.exit(0)

result = {"config": args.config, "width": W, "height": H, "runs": args.runs,
          "params": {k: (round(v, 6) if isinstance(v, float) else v) for k, v in api.DenoiseVarParams.for_guides(W, H, True, True).as_dict().items()}}
alone = {"var": {}, "plain": {}}
for n in range(1, api.DenoiseVarParams.MAX_ITERATIONS + 1):
    alone["var"][n] = median_of(lambda: ctx.denoise_var_device(rgb, out, W, H, var, guides, iterations=n), args.runs)
    alone["plain"][n] = median_of(lambda: ctx.denoise_device(rgb, out, W, H, guides, iterations=n), args.runs)
    print(f"{n} iterations: variance-guided {alone['var'][n]['median_ms']:.3f} ms, plain {alone['plain'][n]['median_ms']:.3f} ms", flush=True)
result["denoise_alone_by_iterations"] = alone
result["ms_per_iteration_by_spacing"] = {
    which: {str(1 << (n - 1)): round(t[n]["median_ms"] - (t[n - 1]["median_ms"] if n > 1 else 0.0), 4) for n in t} for which, t in alone.items()}
result["note_spacing_1"] = "the spacing-1 figures also hold the pack and unpack kernels"
result["var_over_plain_at_5_iterations"] = round(alone["var"][5]["median_ms"] / alone["plain"][5]["median_ms"], 4)

# the moments kernel: a frame with the AOVs, with and without the variance
frames = {}
for name, v in (("aovs", None), ("aovs_variance", var)):
    def frame(v=v):
        if v is None:
            ctx.render_aovs_device(rgb, guides, sx, sy, depth, args.seed)
        else:
            ctx.render_aovs_var_device(rgb, guides, v, sx, sy, depth, args.seed)
    frames[name] = median_of(frame, max(3, args.runs // 3), warmup=1)
    # one timed render on one stream: the stage's exclusive milliseconds
    ctx.set_pass_overlap(False)
    acc = []
    for _ in range(3):
        if v is None:
            ctx.render_aovs_device(rgb, guides, sx, sy, depth, args.seed, timing=True)
        else:
            ctx.render_aovs_var_device(rgb, guides, v, sx, sy, depth, args.seed, timing=True)
        st = ctx.collect_stats()
        acc.append(round(st["ms_accumulate"], 4))
    ctx.set_pass_overlap(True)
    frames[name]["ms_accumulate"] = acc
    frames[name]["ms_accumulate_median"] = statistics.median(acc)
    frames[name]["passes"] = st["passes"]
    print(f"{args.config} frame, {name}: {frames[name]['median_ms']:.2f} ms, ms_accumulate {acc} over {st['passes']} passes", flush=True)
result["frame"] = frames
result["moments_ms_per_pass"] = round((frames["aovs_variance"]["ms_accumulate_median"] - frames["aovs"]["ms_accumulate_median"]) / frames["aovs"]["passes"], 5)
ctx.close()

with open(args.out, "w") as f:
    json.dump({"denoise_var_cost": result}, f, indent=1)
    f.write("\n")
print(json.dumps({"denoise_var_cost": result}))
