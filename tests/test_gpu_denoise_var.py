"""The variance-guided denoiser on the GPU (include/pbrs_gpu.h, pbrs_denoise_var[_device]; device/denoise_var.h): bit for bit against
the CPU model of tests/denoise_var_model.py on synthetic and on rendered buffers, the exact scale invariance on the device, the device
chain of Context.render_denoised_var, the error it removes, and what the header refuses."""
import ctypes as C

import numpy as np
import pytest

import denoise_model as dm
import denoise_var_model as vm
import pbrs_amd
from common import bits
from pbrs_amd import DeviceBuffers, api, scenes
from test_gpu_denoise import FLOOR, GUIDES, SIZES, _configs, same, synthetic

pytestmark = pytest.mark.gpu

f32 = np.float32
SIGMAS = (4.0, 0.3, 0.05)
WITH_VARIANCE = GUIDES + ("variance",)


def both(ctx, rgb, var, guides, iterations, demodulate, id_stop, sigmas=SIGMAS):
    """((out, variance_out) of the GPU, of the model) of one denoise."""
    kw = dict(zip(("sigma_luminance", "sigma_normal", "sigma_depth"), sigmas))
    got = ctx.denoise_var(rgb, var, iterations=iterations, demodulate=demodulate, id_stop=id_stop, albedo_floor=float(FLOOR), return_variance=True,
                          **kw, **guides)
    flags = (vm.DEMODULATE if demodulate else 0) | (vm.ID_STOP if id_stop else 0)
    want = vm.denoise_var(rgb, var, iterations, albedo_floor=FLOOR, flags=flags, **kw, **guides)
    return got, want


def agree(got, want, what):
    for g, w, n in zip(got, want, ("image", "variance")):
        bad = ~same(g, w)
        assert not bad.any(), (what, n, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("iterations", range(1, 7))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matches_the_cpu_model_bit_for_bit_on_synthetic_buffers(gpu_ctx, size, iterations):
    """Every size at every iteration count (the LDS-staged instantiations at spacing 1, 2, 4 and the global-read ones at 8, 16, 32),
    all guides, with and without the two flags; the image and variance_out."""
    w, h = size
    rgb, guides = synthetic(w, h, 100 * iterations + w)
    var = vm.variance_plane(rgb, 7 * iterations + h)
    for demodulate, id_stop in ((True, True), (False, False)):
        got, want = both(gpu_ctx, rgb, var, guides, iterations, demodulate, id_stop)
        agree(got, want, (size, iterations, demodulate, id_stop))
    if w * h >= 64:
        assert np.isnan(got[0]).any() and np.isinf(got[0]).any()  # the planted pixels stay visible
        ok = np.isfinite(rgb).all(axis=2)
        assert np.isfinite(got[0][ok]).all()                      # and reach no neighbour
        assert np.isinf(got[1][~ok]).all()


@pytest.mark.parametrize("size,iterations", (((37, 29), 4), ((5, 70), 6)), ids=("37x29_4", "5x70_6"))
def test_every_flag_combination_and_every_guide_present_or_absent(gpu_ctx, size, iterations):
    rgb, guides = synthetic(size[0], size[1], 7)
    var = vm.variance_plane(rgb, 5)
    seen = {}
    for demodulate, id_stop, present in _configs():
        got, want = both(gpu_ctx, rgb, var, {n: guides[n] for n in present}, iterations, demodulate, id_stop)
        agree(got, want, (demodulate, id_stop, present))
        seen[(demodulate, id_stop, present)] = bits(got[0]).tobytes()
    assert len(seen) == 36
    assert seen[(False, False, ())] != seen[(False, False, ("normal",))] != seen[(False, False, ("normal", "depth"))]
    assert seen[(False, False, ())] == seen[(False, False, ("instance",))] != seen[(False, True, ("instance",))]
    assert seen[(False, False, ("albedo",))] != seen[(True, False, ("albedo",))]
    # the image alone (variance_out NULL): the same bits
    out = gpu_ctx.denoise_var(rgb, var, iterations=iterations, albedo_floor=float(FLOOR), **guides)
    full = gpu_ctx.denoise_var(rgb, var, iterations=iterations, albedo_floor=float(FLOOR), return_variance=True, **guides)
    assert same(out, full[0]).all()


def rendered(ctx, name, strata, depth, seed):
    from test_gpu_pixel_filter import scene
    _, hs = scene(name)
    ctx.upload(hs)
    img, aov, st = ctx.render_aovs(strata[0], strata[1], depth, seed, aovs=WITH_VARIANCE)
    return img, aov, st


@pytest.mark.parametrize("name,depth,seed", (("cornell", 5, 7), ("zoo", 5, 7), ("fuzz39", 7, 50)))
def test_matches_the_cpu_model_bit_for_bit_on_rendered_inputs(gpu_ctx, name, depth, seed):
    img, aov, st = rendered(gpu_ctx, name, (2, 2), depth, seed)
    if name == "fuzz39":
        assert st["invalid_samples"] > 0 and not np.isfinite(img).all()
    var = aov.pop("variance")
    d = api.DenoiseVarParams.make(1, 1)
    for iterations in (3, 5):
        got = gpu_ctx.denoise_var(img, var, iterations=iterations, return_variance=True, **aov)
        want = vm.denoise_var(img, var, iterations, d.sigma_luminance, d.sigma_normal, d.sigma_depth, d.albedo_floor, vm.DEMODULATE | vm.ID_STOP, **aov)
        agree(got, want, (name, iterations))
        assert (np.isfinite(got[0]).all(axis=2) == np.isfinite(img).all(axis=2)).all()


@pytest.mark.parametrize("level", (1e-3, 1.0, 1e3))
def test_the_result_scales_with_the_scene_exactly_on_the_device(gpu_ctx, level):
    """tests/test_denoise_var_model.py::test_the_result_scales_with_the_scene_exactly on the GPU: the same inputs (the model, strict,
    asserts the header's no-denormal condition for them at the three scales), 2^-6 and 2^6, image and variance bit for bit."""
    rgb, var, guides = vm.scale_inputs(56, 44, 3, level)
    kw = dict(iterations=5, albedo_floor=float(FLOOR), return_variance=True, **guides)
    out, vout = gpu_ctx.denoise_var(rgb, var, **kw)
    want = vm.denoise_var(rgb, var, 5, 4.0, 0.3, 0.2, FLOOR, vm.DEMODULATE | vm.ID_STOP, strict=True, **guides)
    agree((out, vout), want, level)
    for j in (-6, 6):
        a, b = f32(2.0 ** j), f32(4.0 ** j)
        vm.denoise_var((rgb * a).astype(f32), (var * b).astype(f32), 5, 4.0, 0.3, 0.2, FLOOR, vm.DEMODULATE | vm.ID_STOP, strict=True, **guides)
        out_j, vout_j = gpu_ctx.denoise_var((rgb * a).astype(f32), (var * b).astype(f32), **kw)
        assert (bits(out_j) == bits((out * a).astype(f32))).all(), j
        assert (bits(vout_j) == bits((vout * b).astype(f32))).all(), j


def test_render_denoised_var_is_render_aovs_then_denoise_var(gpu_ctx):
    img, aov, _ = rendered(gpu_ctx, "cornell", (2, 2), 5, 9)
    var = aov.pop("variance")
    want, vwant = gpu_ctx.denoise_var(img, var, return_variance=True, **aov)
    for _ in range(2):  # two calls: the same bits
        got, noisy, st = gpu_ctx.render_denoised_var(2, 2, 5, 9, keep_noisy=True)
        assert (bits(noisy) == bits(img)).all()
        assert same(got, want).all()
        assert st["samples"] == img.shape[0] * img.shape[1] * 4
    got, _ = gpu_ctx.render_denoised_var(2, 2, 5, 9, guides=("normal", "depth"), iterations=3)
    assert same(got, gpu_ctx.denoise_var(img, var, normal=aov["normal"], depth=aov["depth"], iterations=3)).all()
    # in place on the device (image and variance), and on a caller's buffers
    h, w, _ = img.shape
    with DeviceBuffers({"rgb": img, "out": np.zeros_like(img), "variance": var, "vout": np.zeros_like(var), **aov}) as dev:
        gp = dev.ptrs(aov)
        gpu_ctx.denoise_var_device(dev.ptr("rgb"), dev.ptr("out"), w, h, dev.ptr("variance"), gp, dev.ptr("vout"))
        gpu_ctx.collect_stats()
        assert same(dev.download_like("out", img), want).all()
        assert same(dev.download_like("vout", var), vwant).all()
        gpu_ctx.denoise_var_device(dev.ptr("rgb"), dev.ptr("rgb"), w, h, dev.ptr("variance"), gp, dev.ptr("variance"))
        gpu_ctx.collect_stats()
        assert same(dev.download_like("rgb", img), want).all()
        assert same(dev.download_like("variance", var), vwant).all()


def _mse(img, ref, ok):
    return float(((img[ok].astype(np.float64) - ref[ok]) ** 2).mean())


@pytest.mark.parametrize("strata", (2, 4))
def test_the_default_parameters_remove_error_on_the_cornell_box(gpu_ctx, strata):
    """128 x 128 through render_denoised_var against the plain 32 x 32-strata render (another seed), as
    test_gpu_denoise.py::test_the_default_parameters_remove_error_on_the_cornell_box measures it; the plain denoiser's ratio at the
    same inputs is printed beside it.  Second part: the image times 64 and the variance times 4096 — the variance-guided ratio does not
    move, exactly; the plain denoiser's at its default sigma_color does.  (The measured ratios: DESIGN.md §4, "Variance-guided
    denoiser".)"""
    sb = scenes.cornell_scene(width=128, height=128)
    gpu_ctx.upload(pbrs_amd.HostScene(sb))
    ref, _ = gpu_ctx.render(32, 32, 5, 4242)
    out, noisy, _ = gpu_ctx.render_denoised_var(strata, strata, 5, 17, keep_noisy=True)
    plain, noisy_p, _ = gpu_ctx.render_denoised(strata, strata, 5, 17, keep_noisy=True)
    assert (bits(noisy) == bits(noisy_p)).all()
    ok = np.isfinite(ref).all(axis=2) & np.isfinite(noisy).all(axis=2)
    e_n, e_v, e_p = _mse(noisy, ref, ok), _mse(out, ref, ok), _mse(plain, ref, ok)
    print(f"cornell 128 x 128, {strata * strata} spp, all guides, defaults: noisy MSE {e_n:.5g}; variance-guided {e_v:.5g}, ratio {e_v / e_n:.4f}; "
          f"plain {e_p:.5g}, ratio {e_p / e_n:.4f}")
    assert e_v / e_n < 1.0
    # the same frame in other units
    img, aov, _ = gpu_ctx.render_aovs(strata, strata, 5, 17, aovs=WITH_VARIANCE)
    var = aov.pop("variance")
    assert (bits(img) == bits(noisy)).all()
    base = gpu_ctx.denoise_var(img, var, **aov)
    assert same(base, out).all()
    big = gpu_ctx.denoise_var((img * f32(64.0)).astype(f32), (var * f32(4096.0)).astype(f32), **aov)
    exact = (bits(big) == bits((base * f32(64.0)).astype(f32))).all()
    e_v64 = _mse(big, ref * f32(64.0), ok) / _mse(img * f32(64.0), ref * f32(64.0), ok)
    plain64 = gpu_ctx.denoise((img * f32(64.0)).astype(f32), **aov)
    e_p64 = _mse(plain64, ref * f32(64.0), ok) / _mse(img * f32(64.0), ref * f32(64.0), ok)
    print(f"  x 64: variance-guided ratio {e_v64:.4f} (bits scale exactly: {bool(exact)}), plain ratio {e_p64:.4f}")
    assert e_v64 == e_v / e_n


def test_refusals_leave_the_context_usable(gpu_ctx):
    from test_gpu_pixel_filter import scene
    _, hs = scene("cornell")
    L = gpu_ctx._L
    rgb, guides = synthetic(24, 20, 3)
    guides = dict(guides, variance=vm.variance_plane(rgb, 1))
    out = np.empty_like(rgb)

    def call(fn=L.pbrs_denoise_var, params=True, rgb_in=True, g=True, rgb_out=True, drop=(), **fields):
        p = api.DenoiseVarParams.make(24, 20, demodulate=True, id_stop=True)
        for n, v in fields.items():
            setattr(p, n, v)
        gs = api.DenoiseVarGuides()
        for n in WITH_VARIANCE:
            if n not in drop:
                setattr(gs, n, guides[n].ctypes.data)
        return fn(gpu_ctx._h, C.addressof(p) if params else None, rgb.ctypes.data if rgb_in else None, C.addressof(gs) if g else None,
                  out.ctypes.data if rgb_out else None, None)
    nan, inf = float("nan"), float("inf")
    for fn in (L.pbrs_denoise_var, L.pbrs_denoise_var_device):  # (the device variant refuses before it touches a pointer)
        assert call(fn, params=False) == -1 and call(fn, rgb_in=False) == -1 and call(fn, g=False) == -1 and call(fn, rgb_out=False) == -1
        assert call(fn, drop=("variance",)) == -1
        assert b"variance" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, w=0) == -1 and call(fn, h=0) == -1
        assert call(fn, iterations=0) == -1 and call(fn, iterations=7) == -1
        for s in ("sigma_luminance", "sigma_normal", "sigma_depth"):
            for v in (0.0, -1.0, nan, inf):
                assert call(fn, **{s: v}) == -1, (s, v)
        for v in (-1e-3, nan, inf):
            assert call(fn, albedo_floor=v) == -1, v
        assert call(fn, flags=4) == -1 and call(fn, flags=0x80000003) == -1
        assert call(fn, drop=("albedo",)) == -1 and call(fn, drop=("instance",)) == -1
        assert call(fn, w=1 << 15, h=(1 << 13) + 1) == -4  # PBRS_E_LIMIT
        assert b"2^28" in L.pbrs_last_error(gpu_ctx._h)
    assert call() == 0 and call(iterations=6, albedo_floor=0.0) == 0
    assert call(drop=("albedo",), flags=2) == 0 and call(drop=("instance", "normal", "depth"), flags=1) == 0
    # a plain render afterwards: the bits of a fresh context
    gpu_ctx.upload(hs)
    img, _ = gpu_ctx.render(2, 2, 3, 1)
    fresh = pbrs_amd.Context(0)
    try:
        fresh.upload(hs)
        assert (bits(img) == bits(fresh.render(2, 2, 3, 1)[0])).all()
        # scratch growth: a larger image after a smaller one on a context that starts with none
        for w, h in ((9, 7), (70, 50), (33, 21)):
            rgb2, g2 = synthetic(w, h, w)
            got, want = both(fresh, rgb2, vm.variance_plane(rgb2, h), g2, 5, True, True)
            agree(got, want, (w, h))
    finally:
        fresh.close()
