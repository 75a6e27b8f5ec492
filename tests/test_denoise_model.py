"""The denoiser without a GPU (include/pbrs_gpu.h, pbrs_denoise): the numpy model of tests/denoise_model.py held to the properties
that make it a denoiser, with bounds derived from the arithmetic, and the C ABI against its ctypes mirror."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import denoise_model as dm
import pbrs_amd
from common import SEED
from oracle.binding import OracleScene
from pbrs_amd import api, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
MISS = 0xFFFFFFFF
ENTRY_POINTS = ("pbrs_denoise", "pbrs_denoise_device")
DEFAULTS = api.DenoiseParams.make(1, 1)
SIGMAS = dict(sigma_color=DEFAULTS.sigma_color, sigma_normal=DEFAULTS.sigma_normal, sigma_depth=DEFAULTS.sigma_depth)


def flat_bound(n):
    """A pixel whose counted taps all hold the value v comes out within n * 52 * 2^-24 of v (relative) after n iterations: per
    iteration 25 products wgt * v and 25 additions into a positive partial sum on the S side, 25 additions on the W side (each a
    relative 2^-24 at most on a sum of positive terms), one reciprocal and one product — S / W = v up to (25 + 25 + 2) roundings."""
    return n * 52 * 2.0 ** -24


def rel_err(out, want):
    return float(np.max(np.abs(out.astype(np.float64) - want) / np.abs(want)))


@pytest.mark.parametrize("iterations", (1, 3, 6))
def test_a_constant_image_stays_constant(iterations):
    rng = np.random.default_rng(11)
    h, w = 23, 31
    colour = np.array([0.3, 1.7, 42.0], dtype=f32)
    rgb = np.broadcast_to(colour, (h, w, 3)).copy()
    normal = rng.normal(size=(h, w, 3)).astype(f32)
    depth = rng.uniform(1.0, 10.0, size=(h, w)).astype(f32)
    out = dm.denoise(rgb, iterations, normal=normal, depth=depth, **SIGMAS)
    err = rel_err(out, colour.astype(np.float64))
    print(f"constant image, {iterations} iterations: relative error {err:.3g}, bound {flat_bound(iterations):.3g}")
    assert err <= flat_bound(iterations)


def _halves(h=24, w=40):
    left = np.zeros((h, w), dtype=bool)
    left[:, : w // 2] = True
    a, b = np.array([0.2, 0.9, 3.0], dtype=f32), np.array([5.0, 0.4, 0.01], dtype=f32)
    return left, a, b, np.where(left[..., None], a, b).astype(f32)


@pytest.mark.parametrize("guide", ("normal", "depth", "instance"))
def test_two_flat_halves_do_not_bleed(guide):
    """Orthogonal normals at sigma_normal 0.1 (d2 = 2, pn_exp(-200) = 0), +inf against a finite depth, or two instance ids: with a
    colour sigma that stops nothing, every tap across the edge still weighs 0 and each half stays flat."""
    left, a, b, rgb = _halves()
    kw = dict(sigma_color=1e6, sigma_normal=0.1, sigma_depth=SIGMAS["sigma_depth"])
    if guide == "normal":
        kw["normal"] = np.where(left[..., None], f32([1, 0, 0]), f32([0, 1, 0])).astype(f32)
    elif guide == "depth":
        kw["depth"] = np.where(left, f32(3.5), f32(np.inf)).astype(f32)
    else:
        kw["instance"] = np.where(left, 4, MISS).astype(np.uint32)
        kw["flags"] = dm.ID_STOP
    n = 5
    out = dm.denoise(rgb, n, **kw)
    errs = rel_err(out[left], a.astype(np.float64)), rel_err(out[~left], b.astype(np.float64))
    print(f"two halves, {guide} stop: relative errors {errs[0]:.3g}, {errs[1]:.3g}, bound {flat_bound(n):.3g}")
    assert max(errs) <= flat_bound(n)
    # and without the stop the halves do mix: the test would notice a guide that is ignored
    kw.pop(guide), kw.pop("flags", None)
    mixed = dm.denoise(rgb, n, **kw)
    assert rel_err(mixed[left], a.astype(np.float64)) > 1e-2


def test_a_nan_and_an_inf_pixel_stay_and_spread_nowhere():
    rng = np.random.default_rng(5)
    rgb = rng.uniform(0.0, 2.0, size=(20, 26, 3)).astype(f32)
    rgb[7, 9, 1] = np.nan
    rgb[12, 3] = np.inf
    out = dm.denoise(rgb, 4, **SIGMAS)
    bad = np.zeros(rgb.shape[:2], dtype=bool)
    bad[7, 9] = bad[12, 3] = True
    assert np.isnan(out[7, 9, 1]) and (out[7, 9, [0, 2]] == rgb[7, 9, [0, 2]]).all()
    assert (out[12, 3] == np.inf).all()
    assert np.isfinite(out[~bad]).all()
    assert (out[~bad] != rgb[~bad]).any()


def test_a_nan_guide_skips_the_tap_and_a_nan_guide_at_the_centre_passes_through():
    rng = np.random.default_rng(6)
    rgb = rng.uniform(0.0, 2.0, size=(12, 14, 3)).astype(f32)
    normal = np.zeros((12, 14, 3), dtype=f32)
    depth = np.full((12, 14), 2.0, dtype=f32)
    normal[4, 5, 0] = np.nan
    depth[8, 2] = np.nan
    depth[9, 9] = 0.0  # zp == 0: 0 / 0
    out = dm.denoise(rgb, 3, normal=normal, depth=depth, **SIGMAS)
    assert np.isfinite(out).all()
    for y, x in ((4, 5), (8, 2), (9, 9)):
        assert (out[y, x] == rgb[y, x]).all()


def oracle_guides(sb, sx, sy, seed):
    """Depth and instance of the nearest first hit among a pixel's samples (the depth / instance AOVs), from the oracle's camera rays
    and closest hits, as tests/test_gpu_aov.py::_oracle_first_hits takes them."""
    osc = OracleScene(sb)
    ts, insts = [], []
    for s in range(sx * sy):
        o, d = osc.camera_rays(s, sx, sy, seed)
        hits, _, _ = osc.intersect(o, d, np.full(len(o), np.inf, dtype=f32), anyhit=False)
        ts.append(np.where(hits["inst"] != MISS, hits["t"], f32(np.inf)).astype(f32))
        insts.append(hits["inst"].copy())
    ts, insts = np.array(ts), np.array(insts)
    best = np.argmin(ts, axis=0)
    cols = np.arange(ts.shape[1])
    any_hit = (insts != MISS).any(axis=0)
    depth = np.where(any_hit, ts[best, cols], f32(np.inf)).astype(f32)
    inst = np.where(any_hit, insts[best, cols], MISS).astype(np.uint32)
    return depth.reshape(osc.height, osc.width), inst.reshape(osc.height, osc.width)


def mse_ratio(denoised, noisy, ref):
    ok = np.isfinite(ref).all(axis=2) & np.isfinite(noisy).all(axis=2)
    e_d = float(((denoised[ok].astype(np.float64) - ref[ok]) ** 2).mean())
    e_n = float(((noisy[ok].astype(np.float64) - ref[ok]) ** 2).mean())
    return e_d / e_n, e_d, e_n


def test_real_radiance_gets_closer_to_the_converged_image():
    """A 64 x 64 Cornell box at 2 x 2 strata from the oracle, denoised with the default parameters and the depth and instance
    guides of the oracle's first hits, against the oracle's own 16 x 16-strata render with another seed."""
    sb = scenes.cornell_scene(width=64, height=64)
    osc = OracleScene(sb)
    noisy, _ = osc.render(2, 2, 5, SEED)
    ref, _ = osc.render(16, 16, 5, SEED + 1000)
    depth, inst = oracle_guides(sb, 2, 2, SEED)
    out = dm.denoise(noisy, DEFAULTS.iterations, depth=depth, instance=inst, flags=dm.ID_STOP, **SIGMAS)
    ratio, e_d, e_n = mse_ratio(out, noisy, ref)
    print(f"cornell 64 x 64, 4 spp, depth + instance guides: MSE {e_n:.5g} -> {e_d:.5g}, ratio {ratio:.4f}")
    assert ratio < 1.0


def test_the_ctypes_mirrors_match_the_header():
    src = r'''
#include <stddef.h>
#include <stdio.h>
#include "pbrs_gpu.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(pbrs_denoise_params), offsetof(pbrs_denoise_params, w), offsetof(pbrs_denoise_params, h),
    offsetof(pbrs_denoise_params, iterations), offsetof(pbrs_denoise_params, flags), offsetof(pbrs_denoise_params, sigma_color),
    offsetof(pbrs_denoise_params, sigma_normal), offsetof(pbrs_denoise_params, sigma_depth), offsetof(pbrs_denoise_params, albedo_floor));
  printf("%zu %zu %zu %zu %zu\n", sizeof(pbrs_denoise_guides), offsetof(pbrs_denoise_guides, albedo), offsetof(pbrs_denoise_guides, normal),
    offsetof(pbrs_denoise_guides, depth), offsetof(pbrs_denoise_guides, instance));
  printf("%u %u %u\n", PBRS_DENOISE_MAX_ITERATIONS, PBRS_DENOISE_DEMODULATE, PBRS_DENOISE_ID_STOP);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        lines = [[int(x) for x in l.split()] for l in subprocess.check_output([os.path.join(d, "t")]).decode().splitlines()]
    P, G = api.DenoiseParams, api.DenoiseGuides
    assert lines[0][0] == ctypes.sizeof(P) == 32
    assert lines[0][1:] == [getattr(P, n).offset for n, _ in P._fields_]
    assert lines[1][0] == ctypes.sizeof(G) == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert lines[1][1:] == [getattr(G, n).offset for n, _ in G._fields_]
    assert [n for n, _ in G._fields_] == list(api.DENOISE_GUIDES)
    assert lines[2] == [P.MAX_ITERATIONS, P.DEMODULATE, P.ID_STOP] == [dm.MAX_ITERATIONS, dm.DEMODULATE, dm.ID_STOP]


def test_the_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    for n in ENTRY_POINTS:
        assert f"int {n}(" in header, n
        assert n in api.GPU_SYMBOLS, n
        assert getattr(lib, n) is not None, n
    assert pbrs_amd.DenoiseParams is api.DenoiseParams and hasattr(pbrs_amd.Context, "render_denoised")


def test_defaults_follow_the_guides_at_hand():
    p = api.DenoiseParams.for_guides(8, 4, albedo=True, instance=False)
    assert (p.w, p.h, p.iterations, p.flags) == (8, 4, 5, api.DenoiseParams.DEMODULATE)
    p = api.DenoiseParams.for_guides(8, 4, albedo=True, instance=True, demodulate=False, iterations=2)
    assert (p.iterations, p.flags) == (2, api.DenoiseParams.ID_STOP)
