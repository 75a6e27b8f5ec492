#!/usr/bin/env python3
"""Developer tool (GPU box): what the first-hit AOVs cost (include/pbrs_gpu.h, pbrs_aov_buffers).  Full-size C2 and C4 frames in one
process, without (A) and with every AOV (B), alternating A/B/A/B after a warm-up of each; prints ms_total of every run, the median
ratio B / A per config and one JSON line.     python tools/aov_bench.py [--pairs N] [--configs c2,c4]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pbrs_amd  # noqa: E402
from pbrs_amd import scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=4)
ap.add_argument("--configs", default="c2,c4")
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()

ctx = pbrs_amd.Context(0)
result = {}
for name in args.configs.split(","):
    sb, cfg = scenes.build_config(name)
    hs = pbrs_amd.HostScene(sb)
    ctx.upload(hs)
    sx, sy, depth = cfg["strata_x"], cfg["strata_y"], cfg["depth"]

    def run(aovs):
        if aovs:
            return ctx.render_aovs(sx, sy, depth, args.seed, timing=True)[2]["ms_total"]
        return ctx.render(sx, sy, depth, args.seed, timing=True)[1]["ms_total"]

    run(False), run(True)  # warm-up: the working set, the queue-split decision, the AOV state
    a, b = [], []
    for i in range(args.pairs):
        a.append(run(False))
        b.append(run(True))
        print(f"{name} pair {i}: without {a[-1]:.2f} ms, with all AOVs {b[-1]:.2f} ms, ratio {b[-1] / a[-1]:.4f}", flush=True)
    ratio = statistics.median(y / x for x, y in zip(a, b))
    print(f"{name} {cfg['width']}x{cfg['height']} {sx * sy} spp depth {depth}: median ratio {ratio:.4f} ({(ratio - 1) * 100:+.2f} % of ms_total)")
    result[name] = {"width": cfg["width"], "height": cfg["height"], "spp": sx * sy, "depth": depth, "ms_total_without": a, "ms_total_with": b,
                    "median_ratio": round(ratio, 5)}
ctx.close()
print(json.dumps({"aov_cost": result}))
