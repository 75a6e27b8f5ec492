#!/usr/bin/env python3
"""Developer tool (GPU box): what the id matte costs (include/pbrs_gpu.h, pbrs_render_tile_matte_device, pbrs_matte_mask_device), next
to the same frame with the first-hit AOVs alone in the same process.  Timed with HIP events on the context's stream, after a warm-up
(tools/hip_event_timing.py), at 1920 x 1080 and the config's own strata and depth, for every config of --configs (default c2, c4):
  - the frame through render_aovs_device (the baseline: albedo, normal, depth, instance, coverage) and through render_matte_device with
    the same AOVs for `slots` 1, 4, 6, 8 — baseline and the four features alternate inside every repeat, so a drift of the box falls on
    all of them alike; medians, and the min .. max of every series: the baseline's own spread is the yardstick for the extra time;
  - matte_mask_device alone on the 6-slot layers of that frame with 16 selected ids.
Also states the bytes k_matte must move per pass (16 B of hit record per sample, the state read and written), to set against its kernel
time from a rocprofv3 --kernel-trace --stats run of `--once`.
Writes profiles/matte_cost.json (or --out) and prints it.
    python tools/matte_cost.py [--configs c2,c4] [--runs N] [--out PATH] [--once]
--once: no timing; one 6-slot matte frame and one mask per config (the run to put under rocprofv3 --kernel-trace --stats); with
--no-overlap the passes stay on one stream, so that no kernel's time in the trace includes another stream's work."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="c2,c4")
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--once", action="store_true")
ap.add_argument("--no-overlap", action="store_true", help="every pass on one stream (pbrs_set_pass_overlap 0): a kernel trace then shows exclusive kernel times")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matte_cost.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import statistics  # noqa: E402

import pbrs_amd  # noqa: E402
from pbrs_amd import scenes  # noqa: E402

from hip_event_timing import Timing  # noqa: E402

T = Timing(pbrs_amd, warmup=2)
ctx, dev_alloc = T.ctx, T.dev_alloc
if args.no_overlap:
    ctx.set_pass_overlap(False)
W, H = 1920, 1080
P = W * H
SLOTS = (1, 4, 6, 8)
MAX_SLOTS = 8
AOVS = {"albedo": 3, "normal": 3, "depth": 1, "instance": 1, "coverage": 1}
dev = {n: dev_alloc(ch * P * 4) for n, ch in {"rgb": 3, "ids": MAX_SLOTS, "cov": MAX_SLOTS, "residual": 1, "mask": 1, **AOVS}.items()}
aov_ptrs = {n: dev[n].value for n in AOVS}
matte_ptrs = {"ids": dev["ids"].value, "coverage": dev["cov"].value, "residual": dev["residual"].value}
select = list(range(0, 32, 2))


def series(ms):
    return {"ms": ms, "median_ms": round(statistics.median(ms), 4), "min_ms": min(ms), "max_ms": max(ms)}


result = {"width": W, "height": H, "runs": args.runs, "aovs": list(AOVS), "configs": {}}
for config in args.configs.split(","):
    sb, cfg = scenes.build_config(config, width=W, height=H)
    sx, sy, depth = cfg["strata_x"], cfg["strata_y"], cfg["depth"]
    ctx.upload(pbrs_amd.HostScene(sb))

    def baseline():
        ctx.render_aovs_device(dev["rgb"].value, aov_ptrs, sx, sy, depth, args.seed)

    def matte(slots):
        ctx.render_matte_device(dev["rgb"].value, matte_ptrs, sx, sy, depth, args.seed, slots=slots, aov_device_ptrs=aov_ptrs)

    def mask():
        ctx.matte_mask_device(dev["ids"].value, dev["cov"].value, dev["mask"].value, W, H, 6, select)

    if args.once:
        matte(6)
        mask()
        ctx.collect_stats()
        continue
    for _ in range(T.warmup):
        T.timed(baseline)
        for s in SLOTS:
            T.timed(lambda: matte(s))
    ms = {"aovs": [], **{f"matte_{s}": [] for s in SLOTS}}
    for _ in range(args.runs):
        ms["aovs"].append(round(T.timed(baseline), 4))
        for s in SLOTS:
            ms[f"matte_{s}"].append(round(T.timed(lambda: matte(s)), 4))
    frames = {k: series(v) for k, v in ms.items()}
    matte(6)
    st = ctx.collect_stats()
    frames_mask = T.median_of(mask, args.runs)
    spp, passes = sx * sy, st["passes"]
    r = {"strata": [sx, sy], "depth": depth, "passes": passes, "frame": frames,
         "baseline_spread_ms": round(frames["aovs"]["max_ms"] - frames["aovs"]["min_ms"], 4),
         "matte_extra_ms_median": {str(s): round(frames[f"matte_{s}"]["median_ms"] - frames["aovs"]["median_ms"], 4) for s in SLOTS},
         "mask_6_slots_16_ids": frames_mask,
         # per frame: every sample's hit record once, the state read and written once per pass
         "k_matte_bytes_per_frame": {str(s): 16 * P * spp + 2 * 4 * (2 * s + 1) * P * passes for s in SLOTS},
         "k_matte_finalize_bytes_per_frame": {str(s): 4 * (2 * s + 1) * P + 4 * (2 * s + 1) * P for s in SLOTS},
         "k_matte_mask_bytes_6_slots": 4 * (2 * 6 + 1) * P}
    result["configs"][config] = r
    print(f"{config}: aovs {frames['aovs']['median_ms']:.2f} ms (min {frames['aovs']['min_ms']:.2f}, max {frames['aovs']['max_ms']:.2f}); matte extra "
          f"{r['matte_extra_ms_median']} ms; mask {frames_mask['median_ms']:.3f} ms; {passes} passes", flush=True)
ctx.close()
if args.once:
    sys.exit(0)

with open(args.out, "w") as f:
    json.dump({"matte_cost": result}, f, indent=1)
    f.write("\n")
print(json.dumps({"matte_cost": result}))
