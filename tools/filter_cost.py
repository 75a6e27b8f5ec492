#!/usr/bin/env python3
"""Developer tool (GPU box): what the filtered film costs (include/pbrs_gpu.h, pbrs_render_tile_filtered).  The full bench workload of
one config (default C4: 1920x1080, 512 spp, depth 8) in one process: the plain render, then mitchell r2, gaussian r2 and lanczos r4
through the filter, each timed (pbrs_stats ms_total / ms_accumulate) after a warm-up; prints every run and one JSON line.
    python tools/filter_cost.py [--config c4] [--runs N]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pbrs_amd  # noqa: E402
from pbrs_amd import PixelFilter, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="c4")
ap.add_argument("--runs", type=int, default=2)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()

ctx = pbrs_amd.Context(0)
sb, cfg = scenes.build_config(args.config)
ctx.upload(pbrs_amd.HostScene(sb))
sx, sy, depth = cfg["strata_x"], cfg["strata_y"], cfg["depth"]
variants = [("plain", None), ("mitchell_r2", PixelFilter.mitchell()), ("gaussian_r2", PixelFilter.gaussian()),
            ("lanczos_r4", PixelFilter.lanczos())]


def run(pf):
    if pf is None:
        return ctx.render(sx, sy, depth, args.seed, timing=True)[1]
    return ctx.render_filtered(pf, sx, sy, depth, args.seed, timing=True)[1]


result = {}
run(None)  # warm-up: the working set and the queue-split decision
for name, pf in variants:
    if pf is not None:
        run(pf)  # warm-up: the filter sums
    totals, accs = [], []
    for i in range(args.runs):
        st = run(pf)
        totals.append(round(st["ms_total"], 2))
        accs.append(round(st["ms_accumulate"], 3))
        print(f"{name} run {i}: ms_total {st['ms_total']:.2f}, ms_accumulate {st['ms_accumulate']:.3f}, samples {st['samples']}", flush=True)
    result[name] = {"ms_total": totals, "ms_accumulate": accs}
plain_total = statistics.median(result["plain"]["ms_total"])
plain_acc = statistics.median(result["plain"]["ms_accumulate"])
for name, r in result.items():
    r["filter_stage_share_of_plain_frame"] = round((statistics.median(r["ms_accumulate"]) - plain_acc) / plain_total, 5)
    r["ms_total_ratio"] = round(statistics.median(r["ms_total"]) / plain_total, 5)
ctx.close()
print(json.dumps({"filter_cost": {"config": args.config, "width": cfg["width"], "height": cfg["height"], "spp": sx * sy, "depth": depth,
                                  **result}}))
