"""The variance AOV and the variance-guided denoiser without a GPU (include/pbrs_gpu.h, pbrs_render_tile_aovs_var, pbrs_denoise_var):
the numpy model of tests/denoise_var_model.py held to the properties the feature exists for — above all that the result does not
depend on the units of the scene, exactly — and the C ABI against its ctypes mirror."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import denoise_model as dm
import denoise_var_model as vm
import pbrs_amd
from common import bits
from pbrs_amd import api
from test_denoise_model import flat_bound, rel_err
from test_gpu_denoise import FLOOR, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ENTRY_POINTS = ("pbrs_render_tile_aovs_var", "pbrs_render_tile_aovs_var_device", "pbrs_denoise_var", "pbrs_denoise_var_device")
DEFAULTS = api.DenoiseVarParams.make(1, 1)
SIGMAS = dict(sigma_luminance=DEFAULTS.sigma_luminance, sigma_normal=DEFAULTS.sigma_normal, sigma_depth=DEFAULTS.sigma_depth)


def same(a, b):
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("level", (1e-3, 1.0, 1e3))
def test_the_result_scales_with_the_scene_exactly(level):
    """model(rgb * 2^j, variance * 4^j) == (2^j * out, 4^j * variance_out) bit for bit, j = -6 and +6.

    Range.  Colours lie within 1e-3 .. 1e3 (the level times 0.49 .. 2.1), so with 2^-6 .. 2^6 within 7.6e-6 .. 1.4e5; demodulated by an
    albedo in 0.2 .. 0.8 within 9e-6 .. 7e5.  The variance is (0.1 * lum)^2: 2.4e-15 .. 4.4e8 over the scales, over ld^2 >= 0.04 at
    most 1.1e10; sd = 4 * sqrt(vbar) lies between 2e-7 and 4.2e5.  The largest intermediate is a V below 25 * 1.1e10, far from 3.4e38.
    At the small end a product wgt * c needs wgt >= 1.18e-38 / 9e-6 = 1.3e-33 and ww * v needs wgt^2 >= 1.18e-38 / 2.4e-15, wgt >=
    2.2e-12, or wgt exactly 0: the inputs keep the luminance contrast within a few sd and the guide stops near 1 (scale_inputs), and the
    model asserts on every scale-dependent product that none is a nonzero value below the smallest normal f32 (strict=True), at all
    three scales.  Under that condition a power of two commutes with every rounding, which is the header's claim.

    The plain denoiser with one fixed sigma_color does not have the property: the same test shows it."""
    rgb, var, guides = vm.scale_inputs(56, 44, 3, level)
    kw = dict(iterations=5, albedo_floor=FLOOR, flags=vm.DEMODULATE | vm.ID_STOP, strict=True, **SIGMAS, **guides)
    out, vout = vm.denoise_var(rgb, var, **kw)
    assert np.isfinite(out).all() and np.isinf(vout).any() and np.isfinite(vout).any() and (out != rgb).any()
    for j in (-6, 6):
        a, b = f32(2.0 ** j), f32(4.0 ** j)
        out_j, vout_j = vm.denoise_var((rgb * a).astype(f32), (var * b).astype(f32), **kw)
        assert (bits(out_j) == bits((out * a).astype(f32))).all(), j
        assert (bits(vout_j) == bits((vout * b).astype(f32))).all(), j
    # the plain denoiser at its default sigma_color: not invariant
    d = api.DenoiseParams.make(1, 1)
    pk = dict(iterations=5, sigma_color=d.sigma_color, sigma_normal=d.sigma_normal, sigma_depth=d.sigma_depth, albedo_floor=FLOOR,
              flags=dm.DEMODULATE | dm.ID_STOP, **guides)
    plain = dm.denoise(rgb, **pk)
    worst = 0.0
    for j in (-6, 6):
        a = f32(2.0 ** j)
        plain_j = dm.denoise((rgb * a).astype(f32), **pk)
        assert (bits(plain_j) != bits((plain * a).astype(f32))).any(), j
        worst = max(worst, rel_err(plain_j, (plain * a).astype(np.float64)))
    print(f"level {level:g}: variance-guided exact at 2^-6 and 2^6; plain denoiser off by up to {worst:.3g} (relative)")


@pytest.mark.parametrize("iterations", (1, 3, 6))
def test_a_constant_image_comes_back_whatever_its_variance(iterations):
    """Every counted tap holds the value v: S / W = v up to the roundings test_denoise_model.flat_bound counts (S.c * (1.0f / W) is not
    an exact quotient, so "unchanged" means within that bound), for any finite variance, zero included."""
    rng = np.random.default_rng(11)
    h, w = 23, 31
    colour = np.array([0.3, 1.7, 42.0], dtype=f32)
    rgb = np.broadcast_to(colour, (h, w, 3)).copy()
    normal = rng.normal(size=(h, w, 3)).astype(f32)
    depth = rng.uniform(1.0, 10.0, size=(h, w)).astype(f32)
    var = (10.0 ** rng.uniform(-8.0, 8.0, size=(h, w))).astype(f32)
    var[rng.uniform(size=(h, w)) < 0.2] = 0.0
    out, vout = vm.denoise_var(rgb, var, iterations, normal=normal, depth=depth, **SIGMAS)
    err = rel_err(out, colour.astype(np.float64))
    print(f"constant image, {iterations} iterations: relative error {err:.3g}, bound {flat_bound(iterations):.3g}")
    assert err <= flat_bound(iterations)
    assert np.isfinite(vout).all()


def test_zero_variance_everywhere_leaves_distinct_values_alone():
    """sd == 0 at every pixel: a tap with another luminance weighs +0, so S = hw * c and W = hw of the centre tap alone, and the pixel
    comes back within the two roundings of S.c * (1.0f / W) per iteration (1 / 0.140625 is not an f32), far inside flat_bound.  The
    variance stays 0."""
    rng = np.random.default_rng(2)
    h, w = 20, 27
    rgb = rng.permutation(np.arange(1, 3 * h * w + 1)).reshape(h, w, 3).astype(f32)  # distinct luminances
    assert len(np.unique(vm.lum(rgb))) == h * w
    n = 4
    out, vout = vm.denoise_var(rgb, np.zeros((h, w), dtype=f32), n, **SIGMAS)
    assert rel_err(out, rgb.astype(np.float64)) <= n * 2 * 2.0 ** -24
    assert (vout == 0).all()
    # and with a variance the same image is smoothed: the stop is what held it
    moved, _ = vm.denoise_var(rgb, np.full((h, w), 1e6, dtype=f32), n, **SIGMAS)
    assert rel_err(moved, rgb.astype(np.float64)) > 1e-2


@pytest.mark.parametrize("iterations", (1, 3, 5))
def test_the_filtered_variance_never_exceeds_what_it_can_reach(iterations):
    """v_{k+1} = sum(w_i^2 v_i) / (sum w_i)^2 <= max v_i * sum(w_i^2) / (sum w_i)^2 <= max v_i.  In f32: at most 25 products and 25
    sums on V, 25 sums on W, which enters squared, the reciprocal and two products: (25 + 25 + 2 * 26 + 2) * 2^-24 = 104 * 2^-24
    relative per iteration.  A pixel reaches 2 * (2^n - 1) pixels per side after n iterations; where the result is finite it is bounded
    by the largest finite v_0 in that window."""
    h, w = 37, 45
    rgb, guides = synthetic(w, h, 21)
    var = vm.variance_plane(rgb, 4)
    _, vout = vm.denoise_var(rgb, var, iterations, normal=guides["normal"], depth=guides["depth"], **SIGMAS)
    v0 = np.where(np.isnan(var) | (var < 0), np.inf, var)
    r = 2 * (2 ** iterations - 1)
    checked = 0
    for y in range(h):
        for x in range(w):
            if not np.isfinite(vout[y, x]):
                continue
            win = v0[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1]
            top = win[np.isfinite(win)].max()
            assert vout[y, x] <= top * (1.0 + iterations * 104 * 2.0 ** -24), (y, x)
            checked += 1
    assert checked > 0 and (vout >= 0).all()  # (the planted +inf spreads: after 5 iterations most of this image is unknown)


def test_a_nan_and_an_inf_pixel_stay_and_spread_nowhere():
    rng = np.random.default_rng(5)
    rgb = rng.uniform(0.0, 2.0, size=(20, 26, 3)).astype(f32)
    rgb[7, 9, 1] = np.nan
    rgb[12, 3] = np.inf
    var = np.full((20, 26), 0.04, dtype=f32)
    out, vout = vm.denoise_var(rgb, var, 4, **SIGMAS)
    bad = np.zeros(rgb.shape[:2], dtype=bool)
    bad[7, 9] = bad[12, 3] = True
    assert np.isnan(out[7, 9, 1]) and (out[7, 9, [0, 2]] == rgb[7, 9, [0, 2]]).all()
    assert (out[12, 3] == np.inf).all()
    assert np.isfinite(out[~bad]).all() and (out[~bad] != rgb[~bad]).any()
    assert np.isinf(vout[bad]).all() and np.isfinite(vout[~bad]).all()  # "unknown" at the pixel itself, and it reaches no neighbour


def test_a_nan_or_negative_variance_counts_as_unknown_and_unknown_spreads():
    rgb, guides = synthetic(40, 33, 8)
    var = vm.variance_plane(rgb, 9)
    assert np.isnan(var).any() and (var < 0).any() and np.isinf(var).any() and (var == 0).any()
    kw = dict(iterations=3, albedo_floor=FLOOR, flags=vm.DEMODULATE | vm.ID_STOP, **SIGMAS, **guides)
    a = vm.denoise_var(rgb, var, **kw)
    b = vm.denoise_var(rgb, np.where(np.isnan(var) | (var < 0), np.inf, var).astype(f32), **kw)
    assert same(a[0], b[0]).all() and same(a[1], b[1]).all()
    # an unknown pixel between known ones: after one iteration its open neighbours are unknown too, closed ones (another id) are not
    rgb = np.ones((9, 9, 3), dtype=f32)
    var = np.full((9, 9), 0.01, dtype=f32)
    var[4, 4] = np.inf
    ids = np.zeros((9, 9), dtype=np.uint32)
    ids[:, 5:] = 1
    _, vout = vm.denoise_var(rgb, var, 1, flags=vm.ID_STOP, instance=ids, **SIGMAS)
    assert np.isinf(vout[2:7, 2:5]).all() and np.isfinite(vout[:, 5:]).all() and np.isfinite(vout[:, :2]).all()


def test_the_variance_fold_on_hand_made_cases():
    inf, nan = np.inf, np.nan
    L = np.zeros((4, 1, 6, 3), dtype=f32)
    L[:, 0, 0] = [[1, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1]]          # constant
    L[:, 0, 1] = [[0, 0, 0], [2, 2, 2], [0, 0, 0], [2, 2, 2]]          # two values
    L[:, 0, 2] = [[nan, 0, 0], [1, 1, 1], [inf, 0, 0], [3, 3, 3]]      # two finite samples
    L[:, 0, 3] = [[nan, 0, 0], [nan, 1, 1], [0, -inf, 0], [3, 3, 3]]   # one finite sample
    L[:, 0, 4] = nan                                                    # none
    L[:, 0, 5] = [[1, 2, 3], [4, 5, 6], [7, 8, 9], [0.5, 0.25, 0.125]]
    v = vm.variance(L)
    one = vm.lum(np.ones(3, dtype=f32))
    assert v[0, 0] == 0.0 or v[0, 0] <= 4 * 2.0 ** -24  # m2 / n - mean^2 of a constant: 0 up to the cancellation the header accepts
    # two values 0, 2y, 0, 2y with y = lum(1, 1, 1): mean y, population variance y^2, of the mean y^2 / 3
    assert abs(float(v[0, 1]) - float(one) ** 2 / 3) <= 8 * 2.0 ** -24
    assert abs(float(v[0, 2]) - float(one) ** 2 / 1) <= 8 * 2.0 ** -24  # samples y and 3y: population variance y^2, n - 1 = 1
    assert v[0, 3] == inf and v[0, 4] == inf
    y = vm.lum(L[:, 0, 5]).astype(np.float64)
    assert abs(float(v[0, 5]) - y.var() / 3) <= 1e-5 * y.var()
    assert vm.variance(L[:1])[0, 0] == inf and (vm.variance(L[:1]) == inf).all()  # 1 spp: unknown everywhere
    # sequential in sample order: the fold over the first two, continued, is the fold over all (no dependence on the passes)
    assert v.dtype == f32 and v.shape == (1, 6)


def test_the_ctypes_mirrors_match_the_header():
    src = r'''
#include <stddef.h>
#include <stdio.h>
#include "pbrs_gpu.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(pbrs_denoise_var_params), offsetof(pbrs_denoise_var_params, w),
    offsetof(pbrs_denoise_var_params, h), offsetof(pbrs_denoise_var_params, iterations), offsetof(pbrs_denoise_var_params, flags),
    offsetof(pbrs_denoise_var_params, sigma_luminance), offsetof(pbrs_denoise_var_params, sigma_normal),
    offsetof(pbrs_denoise_var_params, sigma_depth), offsetof(pbrs_denoise_var_params, albedo_floor));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(pbrs_denoise_var_guides), offsetof(pbrs_denoise_var_guides, albedo),
    offsetof(pbrs_denoise_var_guides, normal), offsetof(pbrs_denoise_var_guides, depth), offsetof(pbrs_denoise_var_guides, instance),
    offsetof(pbrs_denoise_var_guides, variance));
  printf("%zu %zu %zu\n", sizeof(pbrs_aov_buffers), sizeof(pbrs_denoise_params), sizeof(pbrs_denoise_guides));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        lines = [[int(x) for x in l.split()] for l in subprocess.check_output([os.path.join(d, "t")]).decode().splitlines()]
    P, G = api.DenoiseVarParams, api.DenoiseVarGuides
    assert lines[0][0] == ctypes.sizeof(P) == 32
    assert lines[0][1:] == [getattr(P, n).offset for n, _ in P._fields_]
    assert lines[1][0] == ctypes.sizeof(G) == 5 * ctypes.sizeof(ctypes.c_void_p)
    assert lines[1][1:] == [getattr(G, n).offset for n, _ in G._fields_]
    # the existing structs keep their sizes
    assert lines[2] == [ctypes.sizeof(api.AovBuffers), ctypes.sizeof(api.DenoiseParams), ctypes.sizeof(api.DenoiseGuides)] == [56, 32, 32]


def test_the_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    for n in ENTRY_POINTS:
        assert f"int {n}(" in header, n
        assert n in api.GPU_SYMBOLS, n
        assert getattr(lib, n) is not None, n
    assert pbrs_amd.DenoiseVarParams is api.DenoiseVarParams
    for m in ("denoise_var", "denoise_var_device", "render_denoised_var", "render_aovs_var_device"):
        assert hasattr(pbrs_amd.Context, m), m


def test_the_python_defaults_and_names():
    assert DEFAULTS.sigma_luminance == 4.0 and DEFAULTS.iterations == 5
    p = api.DenoiseVarParams.for_guides(8, 4, albedo=True, instance=True, iterations=2)
    assert (p.w, p.h, p.iterations, p.flags) == (8, 4, 2, 3)
    assert "variance" not in api.AOV_NAMES and api._aov_names(api.AOV_NAMES + ("variance",))[-1] == "variance"
    with pytest.raises(ValueError):
        api._aov_names(("variances",))
