#!/usr/bin/env python3
"""Developer tool (GPU box): what the denoiser costs (include/pbrs_gpu.h, pbrs_denoise_device).  In one process, timed with HIP events
on the context's stream, after a warm-up, as medians of repeated runs:
  - pbrs_denoise_device alone on a 1920 x 1080 image with all four guides and both flags, for 1 .. 6 iterations; the difference of
    two consecutive medians is the iteration at the larger spacing (the 1-iteration figure also holds pack and unpack);
  - a frame of one config (default C4: 1920x1080, 512 spp, depth 8): plain, with the AOVs, and with the AOVs and the denoise chained.
With --parent-tree DIR (a built checkout of the parent commit) the plain frame is also timed with that tree's package and library and
with this one's, in child processes that alternate, so that the denoise's share can be stated against the parent's frame time and the
plain frame of the two builds compared on one box.  Writes profiles/denoise_cost.json (or --out) and prints it.
    python tools/denoise_cost.py [--config c4] [--runs N] [--parent-tree DIR] [--out PATH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--config", default="c4")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--pairs", type=int, default=2, help="with --parent-tree: child processes per build")
ap.add_argument("--frame-only", action="store_true", help="(child) time the plain frame only and print one JSON line")
ap.add_argument("--tree", default=ROOT, help="(child) the checkout whose package and library are timed")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_cost.json"))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import pbrs_amd  # noqa: E402
from pbrs_amd import api, scenes  # noqa: E402

from hip_event_timing import Timing  # noqa: E402

T = Timing(pbrs_amd, warmup=1)
ctx, median_of, dev_alloc = T.ctx, T.median_of, T.dev_alloc

sb, cfg = scenes.build_config(args.config)
W, H = cfg["width"], cfg["height"]
sx, sy, depth = cfg["strata_x"], cfg["strata_y"], cfg["depth"]
ctx.upload(pbrs_amd.HostScene(sb))
P = W * H
CHANNELS = {"rgb": 3, "out": 3, "albedo": 3, "normal": 3, "depth": 1, "instance": 1}
dev = {n: dev_alloc(ch * P * 4) for n, ch in CHANNELS.items()}
guides = {n: dev[n].value for n in ("albedo", "normal", "depth", "instance")}


def plain():
    ctx.render_device(dev["rgb"].value, sx, sy, depth, args.seed)


def with_aovs():
    ctx.render_aovs_device(dev["rgb"].value, guides, sx, sy, depth, args.seed)


def chained():
    with_aovs()
    ctx.denoise_device(dev["rgb"].value, dev["out"].value, W, H, guides)


if args.frame_only:
    print(json.dumps({"frame_only": median_of(plain, args.runs), "lib": pbrs_amd.lib_paths()[1]}), flush=True)
    ctx.close()
    sys.exit(0)

result = {"config": args.config, "width": W, "height": H, "spp": sx * sy, "depth": depth, "runs": args.runs,
          "params": {k: (round(v, 6) if isinstance(v, float) else v) for k, v in api.DenoiseParams.for_guides(W, H, True, True).as_dict().items()}}
# the denoise alone, on the frame's own image and guides (rendered once, at few samples: its cost does not depend on the values' noise)
ctx.render_aovs_device(dev["rgb"].value, guides, 2, 2, depth, args.seed)
ctx.collect_stats()
alone = {}
for n in range(1, api.DenoiseParams.MAX_ITERATIONS + 1):
    alone[n] = median_of(lambda: ctx.denoise_device(dev["rgb"].value, dev["out"].value, W, H, guides, iterations=n), max(args.runs, 9), warmup=2)
    print(f"denoise alone, {n} iterations: {alone[n]['median_ms']:.3f} ms", flush=True)
result["denoise_alone_by_iterations"] = alone
result["ms_per_iteration_by_spacing"] = {str(1 << (n - 1)): round(alone[n]["median_ms"] - (alone[n - 1]["median_ms"] if n > 1 else 0.0), 4)
                                         for n in alone}
result["note_spacing_1"] = "the spacing-1 figure also holds k_denoise_pack and k_denoise_unpack"
# bytes the algorithm needs per iteration (32 B read + 16 B written per pixel) and what the taps read (25 x 2 x 16 B per pixel)
result["bytes_per_iteration"] = {"unavoidable": 48 * P, "taps": 25 * 2 * 16 * P}
frames = {}
for name, fn in (("plain", plain), ("aovs", with_aovs), ("aovs_denoise", chained)):
    frames[name] = median_of(fn, args.runs)
    print(f"{args.config} frame, {name}: {frames[name]['median_ms']:.2f} ms", flush=True)
result["frame"] = frames
result["denoise_share_of_plain_frame"] = round(alone[5]["median_ms"] / frames["plain"]["median_ms"], 6)
ctx.close()

if args.parent_tree:
    ab = {"parent": [], "this": []}
    for _ in range(args.pairs):
        for name, tree in (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--frame-only", "--tree", tree, "--config", args.config, "--runs",
                                  str(args.runs), "--seed", str(args.seed)], capture_output=True, text=True, timeout=600, check=True).stdout
            line = next(l for l in out.splitlines() if l.startswith('{"frame_only"'))
            ab[name].append(json.loads(line)["frame_only"]["median_ms"])
            print(f"plain frame, {name} library: {ab[name][-1]:.2f} ms", flush=True)
    parent, this = statistics.median(ab["parent"]), statistics.median(ab["this"])
    result["plain_frame_ab"] = {"parent_ms": ab["parent"], "this_ms": ab["this"], "this_over_parent": round(this / parent, 5)}
    result["denoise_share_of_parent_frame"] = round(alone[5]["median_ms"] / parent, 6)

with open(args.out, "w") as f:
    json.dump({"denoise_cost": result}, f, indent=1)
    f.write("\n")
print(json.dumps({"denoise_cost": result}))
