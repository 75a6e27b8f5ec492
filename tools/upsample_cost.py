#!/usr/bin/env python3
"""Developer tool (GPU box): what guided upsampling costs (include/pbrs_gpu.h, pbrs_upsample_device; device/upsample.h) and what it buys.

The call alone, at 1920 x 1080 for every factor and radius with all guides and both flags, on synthetic device planes (a few surfaces: the
cost depends little on the values), and beside it in the same process one iteration of denoise_device at the same size with all guides.
Timed with HIP events on the context's stream (tools/hip_event_timing.py) around --batch back-to-back calls after two warm-up batches, as
the median of --runs such batches, per call.

The frame, on a configuration (C2) at --frame-size squared: render_denoised_var at full size against render_upscaled at factor 2 and 4
with the same strata per traced pixel, each a whole call (device buffers allocated, the chain queued, one wait, the copies back) under HIP
events on the same stream, median of --runs after two warm-up calls; the guide render alone (one sample per full pixel, the path integrator
at depth 1, into device buffers) the same way; and the MSE and the display-referred error (mean of (t(out) - t(ref))^2 over finite
reference pixels, t(v) = max(v, 0) / (1 + max(v, 0))) of each result against a --ref-strata squared render of another seed.
Writes profiles/upsample_cost.json (or --out) and prints it.
    python tools/upsample_cost.py [--runs N] [--batch N] [--config c2] [--frame-size N] [--strata N] [--ref-strata N] [--out PATH]"""
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
ap.add_argument("--config", default="c2")
ap.add_argument("--frame-size", type=int, default=1024)
ap.add_argument("--strata", type=int, default=2)
ap.add_argument("--ref-strata", type=int, default=32)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample_cost.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import pbrs_amd  # noqa: E402
from pbrs_amd import api, scenes  # noqa: E402

from hip_event_timing import Timing, check  # noqa: E402

T = Timing(pbrs_amd, warmup=2)
ctx, hip = T.ctx, T.hip
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
f32 = np.float32
GUIDES = ("albedo", "normal", "depth", "instance")


def planes(w, h, step, rng):
    """An image and its four guides: three surfaces with their own normal, depth ramp and id, a random albedo."""
    yy, xx = np.mgrid[0:h, 0:w]
    u, v = (xx + 0.5) * step, (yy + 0.5) * step
    ids = ((u > 700).astype(np.uint32) + 2 * (v > 600).astype(np.uint32)).astype(np.uint32)
    normal = np.zeros((h, w, 3), dtype=f32)
    normal[..., 0], normal[..., 1] = np.where(ids & 1, 0.6, 0.0), np.where(ids & 2, 0.6, 0.0)
    normal[..., 2] = np.sqrt(1.0 - normal[..., 0] ** 2 - normal[..., 1] ** 2)
    return {"rgb": (rng.random((h, w, 3)) * 2.0).astype(f32), "albedo": (0.2 + 0.6 * rng.random((h, w, 3))).astype(f32), "normal": normal,
            "depth": (2.0 + 0.001 * u + 0.0005 * v + 1.5 * ids).astype(f32), "instance": ids}


def upload(arrays):
    dev = {}
    for n, a in arrays.items():
        a = np.ascontiguousarray(a)
        dev[n] = T.dev_alloc(a.nbytes)
        check(hip.hipMemcpy(dev[n], a.ctypes.data, a.nbytes, 1), "hipMemcpy")  # hipMemcpyHostToDevice
    return dev


def free(dev):
    for ptr in dev.values():
        hip.hipFree(ptr)


result = {"runs": args.runs, "batch": args.batch, "call": {}, "frame": {}}

# ---- the call alone ----
w, h = 1920, 1080
rng = np.random.default_rng(1)
hi = upload(planes(w, h, 1, rng))
out = T.dev_alloc(3 * w * h * 4)
gh = {n: hi[n].value for n in GUIDES}


def per_call(fn):
    def batch():
        for _ in range(args.batch):
            fn()
    r = T.median_of(batch, args.runs)
    return {"batch_ms": r["ms"], "call_ms": round(r["median_ms"] / args.batch, 5)}


result["call"]["size"] = f"{w}x{h}"
result["call"]["denoise_one_iteration"] = per_call(lambda: ctx.denoise_device(hi["rgb"].value, out.value, w, h, gh, iterations=1))
base = result["call"]["denoise_one_iteration"]["call_ms"]
print(f"denoise_device, one iteration, all guides: {base * 1e3:.1f} us per call", flush=True)
for f in api.UpsampleParams.FACTORS:
    wl, hl = api.UpsampleParams.make(w, h, f).low_size
    lo = upload(planes(wl, hl, f, rng))
    gl = {n: lo[n].value for n in GUIDES}
    for R in api.UpsampleParams.RADII:
        r = per_call(lambda: ctx.upsample_device(lo["rgb"].value, out.value, w, h, f, gl, gh, radius=R))
        r["over_denoise_iteration"] = round(r["call_ms"] / base, 3)
        result["call"][f"factor_{f}_radius_{R}"] = r
        print(f"upsample_device, factor {f}, radius {R}, all guides: {r['call_ms'] * 1e3:.1f} us per call, {r['over_denoise_iteration']:.2f} of the "
              f"denoiser's iteration", flush=True)
    free(lo)
free(hi)
hip.hipFree(out)

# ---- the frame ----
n = args.frame_size
sb, _ = scenes.build_config(args.config, width=n, height=n)
ctx.upload(pbrs_amd.HostScene(sb))
s, depth = args.strata, args.depth
ref, _ = ctx.render(args.ref_strata, args.ref_strata, depth, 4242)
ok = np.isfinite(ref).all(axis=2)


def tone(v):
    v = np.maximum(v.astype(np.float64), 0.0)
    return v / (1.0 + v)


def errors(img):
    return {"mse": float(((img[ok].astype(np.float64) - ref[ok]) ** 2).mean()), "display_error": float(((tone(img[ok]) - tone(ref[ok])) ** 2).mean())}


frame = result["frame"]
frame.update({"config": args.config, "size": f"{n}x{n}", "strata_per_traced_pixel": f"{s}x{s}", "depth": depth,
              "reference": f"{args.ref_strata}x{args.ref_strata} strata, seed 4242"})
kept = {}


def full_size():
    kept["full"] = ctx.render_denoised_var(s, s, depth, 17)[0]


r = T.median_of(full_size, args.runs)
frame["render_denoised_var"] = {"ms": r["ms"], "median_ms": r["median_ms"], **errors(kept["full"])}
print(f"render_denoised_var at {n} x {n}: {r['median_ms']:.2f} ms, {errors(kept['full'])}", flush=True)
# the guide render alone, into device buffers
gdev = {g: T.dev_alloc(api.DENOISE_GUIDES[g][0] * n * n * 4) for g in GUIDES}
grgb = T.dev_alloc(3 * n * n * 4)
r = T.median_of(lambda: ctx._render_guides_device(grgb.value, {g: gdev[g].value for g in GUIDES}, 17), args.runs)
frame["guide_render"] = {"ms": r["ms"], "median_ms": r["median_ms"]}
print(f"the guide render at {n} x {n}: {r['median_ms']:.3f} ms", flush=True)
free(gdev)
hip.hipFree(grgb)
for f in (2, 4):
    def upscaled():
        kept["up"] = ctx.render_upscaled(s, s, depth, 17, factor=f)[0]
    r = T.median_of(upscaled, args.runs)
    e = errors(kept["up"])
    frame[f"render_upscaled_factor_{f}"] = {"ms": r["ms"], "median_ms": r["median_ms"], **e,
                                           "over_full_size": round(r["median_ms"] / frame["render_denoised_var"]["median_ms"], 3),
                                           "guide_render_share": round(frame["guide_render"]["median_ms"] / r["median_ms"], 3)}
    print(f"render_upscaled, factor {f}: {r['median_ms']:.2f} ms, {e}", flush=True)
ctx.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump({"upsample_cost": result}, fh, indent=1)
    fh.write("\n")
print(json.dumps({"upsample_cost": result}))
