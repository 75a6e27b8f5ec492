#!/usr/bin/env python3
"""Developer tool (GPU box): what the despeckle call costs and what it buys (include/pbrs_gpu.h, pbrsi_despeckle_device).
Time, with HIP events on the context's stream, after a warm-up, as medians of repeated batches (tools/compare_cost.py's method; a batch of
calls between two events, because one call is tens of microseconds), at 1920 x 1080 on HDR noise with fireflies and NaNs sown in:
  - pbrsi_despeckle_device at radius 1 and 2, with the image alone, with the variance pair, and with the variance pair, the mask and the
    removed energy; beside each the bytes it must move and what share of the HBM peak that is at the measured time;
  - pbrs_denoise_var_device on the same image with all guides, the difference of the 2- and the 1-iteration medians: one iteration.
Quality, through Context.compare (REINHARD, SSIM at peak 1): the Cornell box with the glass and the metal sphere at --size^2 and --strata^2
samples per pixel against --ref-strata^2, for the noisy frame, the variance-guided filter, and the filter behind the despeckle step, over
rank 1 .. 3 and gain 1.5, 2, 4 at radius 1 (and the defaults at radius 2), with the counts and the mean of removed_out (the energy the
step takes out: it is biased); and the last of --frames frames of render_temporal with and without despeckle=.
The image-only form is also timed without a record ("..._no_record": no memset, no counts, no adds), which says what the counts cost.
The device is kept busy for --warm seconds before the first timed batch, and the first form is timed again after the last one
("..._again"): a form of some 20 ms would otherwise be timed while the clocks still rise.  --skip-quality: the timing alone, the run to
put under rocprofv3 --kernel-trace --stats.
Writes profiles/despeckle_cost.json (or --out) and prints it.
    python tools/despeckle_cost.py [--runs N] [--batch N] [--warm S] [--size 256] [--strata 2] [--ref-strata 32] [--frames 3] [--skip-quality] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time as clock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--batch", type=int, default=20)
ap.add_argument("--warm", type=float, default=1.0)
ap.add_argument("--skip-quality", action="store_true")
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--strata", type=int, default=2)
ap.add_argument("--ref-strata", type=int, default=32)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--frames", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "despeckle_cost.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import pbrs_amd  # noqa: E402
from pbrs_amd import scenes  # noqa: E402
from pbrs_amd.roofline import HBM_PEAK_GBS  # noqa: E402

from hip_event_timing import Timing, check  # noqa: E402

T = Timing(pbrs_amd, warmup=2)
ctx, hip = T.ctx, T.hip
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
f32 = np.float32
W, H = 1920, 1080
P = W * H


def upload(a):
    a = np.ascontiguousarray(a)
    ptr = T.dev_alloc(a.nbytes)
    check(hip.hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy")  # hipMemcpyHostToDevice
    return ptr.value


def per_call(fn):
    def batch():
        for _ in range(args.batch):
            fn()
    r = T.median_of(batch, args.runs)
    calls = sorted(ms / args.batch for ms in r["ms"])
    return {"batch_ms": r["ms"], "call_ms": round(r["median_ms"] / args.batch, 5), "call_ms_min": round(calls[0], 5), "call_ms_max": round(calls[-1], 5)}


# ---- time ----
rng = np.random.default_rng(1)
img = (rng.random((H, W, 3)) ** 4 * 20).astype(f32)
sown = rng.random((H, W))
img[sown < 1e-3] *= f32(300)  # one firefly per thousand pixels
img[sown > 1 - 1e-5] = np.nan  # and a NaN per hundred thousand
rgb, out, removed = upload(img), T.dev_alloc(12 * P).value, T.dev_alloc(12 * P).value
variance = upload((rng.random((H, W)) * 0.1).astype(f32))
variance_out, mask, record = T.dev_alloc(4 * P).value, T.dev_alloc(4 * P).value, T.dev_alloc(16).value
yy, xx = np.mgrid[0:H, 0:W]
ids = ((xx > 700).astype(np.uint32) + 2 * (yy > 600).astype(np.uint32)).astype(np.uint32)
normal = np.zeros((H, W, 3), dtype=f32)
normal[..., 2] = 1.0
guides = {"albedo": upload((0.2 + 0.6 * rng.random((H, W, 3))).astype(f32)), "normal": upload(normal),
          "depth": upload((2.0 + 0.001 * xx + 0.0005 * yy + 1.5 * ids).astype(f32)), "instance": upload(ids)}
pair = {"variance_in": variance, "variance_out": variance_out}
FORMS = {"image": ({}, 24), "variance": (pair, 32), "variance_mask_removed": ({**pair, "mask_out": mask, "removed_out": removed}, 48)}
time = {"size": f"{W}x{H}", "runs": args.runs, "batch": args.batch, "warm_s": args.warm, "hbm_peak_GBps": HBM_PEAK_GBS, "forms": {}}
until = clock.monotonic() + args.warm
while clock.monotonic() < until:
    for _ in range(100):
        ctx.despeckle_device(rgb, out, W, H, record, pair)
    ctx.collect_stats()
ORDER = [(radius, name, "") for radius in (1, 2) for name in FORMS] + [(1, "image", "_no_record"), (2, "image", "_no_record"), (1, "image", "_again")]
for radius, name, suffix in ORDER:
    planes, bytes_per_pixel = FORMS[name]
    r = per_call(lambda: ctx.despeckle_device(rgb, out, W, H, None if suffix == "_no_record" else record, planes, radius=radius))
    r["bytes_moved"] = bytes_per_pixel * P + (0 if suffix == "_no_record" else 16)
    r["GBps"] = round(r["bytes_moved"] / (r["call_ms"] * 1e-3) / 1e9, 1)
    r["share_of_hbm_peak"] = round(r["GBps"] / HBM_PEAK_GBS, 4)
    time["forms"][f"radius_{radius}_{name}{suffix}"] = r
    print(f"despeckle_device, radius {radius}, {name}{suffix}: {r['call_ms'] * 1e3:.1f} us per call ({r['call_ms_min'] * 1e3:.1f} .. {r['call_ms_max'] * 1e3:.1f}), "
          f"{r['bytes_moved'] / 1e6:.1f} MB, {r['GBps']:.0f} GB/s, {100 * r['share_of_hbm_peak']:.1f} % of the HBM peak", flush=True)
ctx.collect_stats()
counts = pbrs_amd.DespeckleResult()
check(hip.hipMemcpy(C.addressof(counts), record, 16, 2), "hipMemcpy")  # hipMemcpyDeviceToHost
time["counts_radius_1"] = counts.as_dict()  # of the last form timed
ctx.despeckle_device(rgb, out, W, H, record, {}, radius=2)
ctx.collect_stats()
check(hip.hipMemcpy(C.addressof(counts), record, 16, 2), "hipMemcpy")
time["counts_radius_2"] = counts.as_dict()
one, two = (per_call(lambda: ctx.denoise_var_device(rgb, out, W, H, variance, guides, iterations=n)) for n in (1, 2))
time["denoise_var"] = {"iterations_1": one, "iterations_2": two, "one_iteration_ms": round(two["call_ms"] - one["call_ms"], 5)}
base = time["denoise_var"]["one_iteration_ms"]
print(f"denoise_var_device: {one['call_ms'] * 1e3:.1f} us at one iteration, {two['call_ms'] * 1e3:.1f} us at two: {base * 1e3:.1f} us per iteration", flush=True)
for r in time["forms"].values():
    r["over_denoise_var_iteration"] = round(r["call_ms"] / base, 3)

if args.skip_quality:
    ctx.close()
    print(json.dumps({"despeckle_cost": {"time": time}}))
    sys.exit(0)

# ---- quality ----
n, s, depth = args.size, args.strata, args.depth
hs = pbrs_amd.HostScene(scenes.cornell_scene(width=n, height=n, variant="specular"))
ctx.upload(hs)
reference, _ = ctx.render(args.ref_strata, args.ref_strata, depth, 4242)
GUIDES = ("albedo", "normal", "depth", "instance")
noisy, aov, _ = ctx.render_aovs(s, s, depth, 17, aovs=GUIDES + ("variance",))
guide_planes = {g: aov[g] for g in GUIDES}


def score(image, **extra):
    r = ctx.compare(image, reference)
    return {"mse": r.mse, "rel_mse": r.rel_mse, "ssim": r.ssim, "psnr_db": round(r.psnr(), 3), "n_valid": r.n_valid, **extra}


def show(name, row):
    print(f"{name:34s} mse {row['mse']:.3e} rel_mse {row['rel_mse']:.3e} ssim {row['ssim']:.4f} psnr {row['psnr_db']:6.2f} dB"
          + (f"  clamped {row['n_clamped']} repaired {row['n_repaired']} removed {row['removed_mean']:.3e}" if "n_clamped" in row else ""), flush=True)


quality = {"scene": "cornell, specular", "size": f"{n}x{n}", "spp": s * s, "depth": depth, "reference": f"{args.ref_strata}x{args.ref_strata} strata, seed 4242",
           "compare": pbrs_amd.CompareParams.make(n, n).as_dict(), "reference_mean_over_finite_pixels": float(reference[np.isfinite(reference).all(axis=2)].mean()),
           "reference_pixels_not_finite": int((~np.isfinite(reference).all(axis=2)).sum()), "noisy_pixels_not_finite": int((~np.isfinite(noisy).all(axis=2)).sum()), "rows": {}, "grid": {}, "temporal": {}}
print(f"reference: mean over finite pixels {quality['reference_mean_over_finite_pixels']:.4f}, {quality['reference_pixels_not_finite']} pixels not finite; "
      f"noisy frame: {quality['noisy_pixels_not_finite']} pixels not finite", flush=True)
quality["rows"]["noisy"] = score(noisy)
quality["rows"]["denoise_var"] = score(ctx.denoise_var(noisy, aov["variance"], **guide_planes))
for name, row in quality["rows"].items():
    show(name, row)
GRID = [(1, rank, gain) for rank in (1, 2, 3) for gain in (1.5, 2.0, 4.0)] + [(2, 2, 2.0), (2, 4, 2.0)]
for radius, rank, gain in GRID:
    clean, var, removed_map, res = ctx.despeckle(noisy, aov["variance"], removed=True, radius=radius, rank=rank, gain=gain)
    extra = {"radius": radius, "rank": rank, "gain": gain, "n_clamped": res.n_clamped, "n_repaired": res.n_repaired, "removed_mean": float(removed_map.mean())}
    key = f"radius_{radius}_rank_{rank}_gain_{gain}"
    quality["grid"][key] = {"despeckled": score(clean, **extra), "despeckled_denoise_var": score(ctx.denoise_var(clean, var, **guide_planes), **extra)}
    show(key, quality["grid"][key]["despeckled"])
    show(key + " + denoise_var", quality["grid"][key]["despeckled_denoise_var"])
cams, seeds = [hs.camera] * args.frames, [100 + k for k in range(args.frames)]
for name, kw in (("plain", {}), ("despeckle", {"despeckle": True})):
    last = None
    for last in ctx.render_temporal(cams, s, s, depth, seeds, **kw):
        pass
    extra = last[3]["despeckle"].as_dict() if "despeckle" in last[3] else {}
    quality["temporal"][name] = {"frames": args.frames, "accumulated": score(last[1], **extra), "filtered": score(last[0], **extra)}
    print(f"temporal, {name}: accumulated ssim {quality['temporal'][name]['accumulated']['ssim']:.4f} rel_mse {quality['temporal'][name]['accumulated']['rel_mse']:.3e}; "
          f"filtered ssim {quality['temporal'][name]['filtered']['ssim']:.4f} rel_mse {quality['temporal'][name]['filtered']['rel_mse']:.3e}", flush=True)
ctx.close()

result = {"despeckle_cost": {"time": time, "quality": quality}}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1, allow_nan=False)
    fh.write("\n")
print(json.dumps(result))
