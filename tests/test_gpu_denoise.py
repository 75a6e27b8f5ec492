"""The denoiser on the GPU (include/pbrs_gpu.h, pbrs_denoise[_device]; device/denoise.h): bit for bit against the CPU model of
tests/denoise_model.py on synthetic and on rendered buffers, the device chain of Context.render_denoised, the error it removes, and
what the header refuses."""
import ctypes as C
import itertools

import numpy as np
import pytest

import denoise_model as dm
import pbrs_amd
from common import bits
from pbrs_amd import DeviceBuffers, api, scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
MISS = 0xFFFFFFFF
GUIDES = ("albedo", "normal", "depth", "instance")
SIZES = ((1, 1), (5, 70), (37, 29), (64, 40), (130, 97))  # (w, h)
FLOOR = f32(1e-3)


def same(a, b):
    """Equal bits, or a NaN on both sides."""
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def synthetic(w, h, seed):
    """An image and its four guides with everything the header has a rule for: colours from 1e-6 to 1e4 (a scale per 8 x 8 block,
    so that neighbours weigh in), planted NaN / +inf / -inf pixels, albedo with zeros and values at and next to the floor, depth
    with +inf, a zero and a NaN, a NaN normal, ids in blocks."""
    rng = np.random.default_rng(seed)
    by, bx = (h + 7) // 8, (w + 7) // 8

    def blocks(values):
        return np.kron(values, np.ones((8, 8), dtype=values.dtype))[:h, :w]
    scale = blocks((10.0 ** rng.uniform(-6.0, 4.0, size=(by, bx))).astype(f32))
    rgb = (scale[..., None] * rng.uniform(0.5, 1.5, size=(h, w, 3))).astype(f32)
    albedo = rng.uniform(0.0, 1.0, size=(h, w, 3)).astype(f32)
    albedo[rng.uniform(size=(h, w, 3)) < 0.1] = 0.0
    albedo[rng.uniform(size=(h, w, 3)) < 0.05] = FLOOR
    albedo[rng.uniform(size=(h, w, 3)) < 0.05] = np.nextafter(FLOOR, f32(1.0))
    n = blocks(rng.integers(0, 3, size=(by, bx)).astype(np.int64))
    normal = (np.eye(3, dtype=f32)[n] + rng.normal(scale=0.05, size=(h, w, 3))).astype(f32)
    depth = (blocks(rng.uniform(1.0, 10.0, size=(by, bx)).astype(f32)) * rng.uniform(0.98, 1.02, size=(h, w))).astype(f32)
    instance = blocks(rng.integers(0, 4, size=(by, bx)).astype(np.uint32))
    sky = blocks((rng.uniform(size=(by, bx)) < 0.2).astype(np.uint8)).astype(bool)
    depth[sky] = np.inf
    instance[sky] = MISS
    if w * h >= 64:
        ys, xs = rng.integers(0, h, size=8), rng.integers(0, w, size=8)
        rgb[ys[0], xs[0], 1] = np.nan
        rgb[ys[1], xs[1]] = np.inf
        rgb[ys[2], xs[2], 2] = -np.inf
        normal[ys[3], xs[3], 0] = np.nan
        depth[ys[4], xs[4]] = np.nan
        depth[ys[5], xs[5]] = 0.0
        depth[ys[6], xs[6]] = -np.inf
        albedo[ys[7], xs[7]] = np.nan
    return rgb, {"albedo": albedo, "normal": normal, "depth": depth, "instance": instance.astype(np.uint32)}


def both(ctx, rgb, guides, iterations, demodulate, id_stop, sigmas=(2.0, 0.3, 0.05)):
    """(GPU, model) of one denoise."""
    kw = dict(zip(("sigma_color", "sigma_normal", "sigma_depth"), sigmas))
    got = ctx.denoise(rgb, iterations=iterations, demodulate=demodulate, id_stop=id_stop, albedo_floor=float(FLOOR), **kw, **guides)
    flags = (dm.DEMODULATE if demodulate else 0) | (dm.ID_STOP if id_stop else 0)
    want = dm.denoise(rgb, iterations, albedo_floor=FLOOR, flags=flags, **kw, **guides)
    return got, want


@pytest.mark.parametrize("iterations", range(1, 7))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matches_the_cpu_model_bit_for_bit_on_synthetic_buffers(gpu_ctx, size, iterations):
    """Every size at every iteration count (the LDS-staged instantiations at spacing 1, 2, 4 and the global-read ones at 8, 16, 32),
    all guides, with and without the two flags."""
    w, h = size
    rgb, guides = synthetic(w, h, 100 * iterations + w)
    for demodulate, id_stop in ((True, True), (False, False)):
        got, want = both(gpu_ctx, rgb, guides, iterations, demodulate, id_stop)
        bad = ~same(got, want)
        assert not bad.any(), (size, iterations, demodulate, id_stop, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    if w * h >= 64:
        assert np.isnan(got).any() and np.isinf(got).any()  # the planted pixels stay visible
        ok = np.isfinite(rgb).all(axis=2)
        assert np.isfinite(got[ok]).all()                  # and reach no neighbour


def _configs():
    """Every flag combination with every subset of the guides the flags allow."""
    for demodulate, id_stop in itertools.product((False, True), repeat=2):
        for k in range(len(GUIDES) + 1):
            for present in itertools.combinations(GUIDES, k):
                if (demodulate and "albedo" not in present) or (id_stop and "instance" not in present):
                    continue
                yield demodulate, id_stop, present


@pytest.mark.parametrize("size,iterations", (((37, 29), 4), ((5, 70), 6)), ids=("37x29_4", "5x70_6"))
def test_every_flag_combination_and_every_guide_present_or_absent(gpu_ctx, size, iterations):
    rgb, guides = synthetic(size[0], size[1], 7)
    seen = {}
    for demodulate, id_stop, present in _configs():
        got, want = both(gpu_ctx, rgb, {n: guides[n] for n in present}, iterations, demodulate, id_stop)
        bad = ~same(got, want)
        assert not bad.any(), (demodulate, id_stop, present, int(bad.sum()))
        seen[(demodulate, id_stop, present)] = bits(got).tobytes()
    assert len(seen) == 36
    # a guide that is given changes the result (an ignored pointer would not); an instance guide without the flag does not
    assert seen[(False, False, ())] != seen[(False, False, ("normal",))] != seen[(False, False, ("normal", "depth"))]
    assert seen[(False, False, ())] == seen[(False, False, ("instance",))] != seen[(False, True, ("instance",))]
    assert seen[(False, False, ("albedo",))] != seen[(True, False, ("albedo",))]


def rendered(ctx, name, strata, depth, seed):
    from test_gpu_pixel_filter import scene
    _, hs = scene(name)
    ctx.upload(hs)
    img, aov, st = ctx.render_aovs(strata[0], strata[1], depth, seed, aovs=GUIDES)
    return img, aov, st


@pytest.mark.parametrize("name,depth,seed", (("cornell", 5, 7), ("zoo", 5, 7), ("fuzz39", 7, 50)))
def test_matches_the_cpu_model_bit_for_bit_on_rendered_inputs(gpu_ctx, name, depth, seed):
    img, aov, st = rendered(gpu_ctx, name, (2, 2), depth, seed)
    if name == "fuzz39":
        assert st["invalid_samples"] > 0 and not np.isfinite(img).all()
    d = api.DenoiseParams.make(1, 1)
    for iterations in (3, 5):
        got = gpu_ctx.denoise(img, iterations=iterations, **aov)
        want = dm.denoise(img, iterations, d.sigma_color, d.sigma_normal, d.sigma_depth, d.albedo_floor, dm.DEMODULATE | dm.ID_STOP, **aov)
        bad = ~same(got, want)
        assert not bad.any(), (name, iterations, int(bad.sum()))
        assert (np.isfinite(got).all(axis=2) == np.isfinite(img).all(axis=2)).all()


def test_render_denoised_is_render_aovs_then_denoise(gpu_ctx):
    img, aov, _ = rendered(gpu_ctx, "cornell", (2, 2), 5, 9)
    want = gpu_ctx.denoise(img, **aov)
    for _ in range(2):  # two calls: the same bits
        got, noisy, st = gpu_ctx.render_denoised(2, 2, 5, 9, keep_noisy=True)
        assert (bits(noisy) == bits(img)).all()
        assert same(got, want).all()
        assert st["samples"] == img.shape[0] * img.shape[1] * 4
    got, _ = gpu_ctx.render_denoised(2, 2, 5, 9, guides=("normal", "depth"), iterations=3)
    assert same(got, gpu_ctx.denoise(img, normal=aov["normal"], depth=aov["depth"], iterations=3)).all()
    # in place on the device, and on a caller's buffers
    h, w, _ = img.shape
    with DeviceBuffers({"rgb": img, "out": np.zeros_like(img), **aov}) as dev:
        gp = dev.ptrs(aov)
        gpu_ctx.denoise_device(dev.ptr("rgb"), dev.ptr("out"), w, h, gp)
        gpu_ctx.denoise_device(dev.ptr("rgb"), dev.ptr("rgb"), w, h, gp)
        gpu_ctx.collect_stats()
        assert same(dev.download_like("out", img), want).all()
        assert same(dev.download_like("rgb", img), want).all()


def test_the_default_parameters_remove_error_on_the_cornell_box(gpu_ctx):
    """128 x 128 at 2 x 2 strata through render_denoised against the plain 32 x 32-strata render (another seed)."""
    sb = scenes.cornell_scene(width=128, height=128)
    gpu_ctx.upload(pbrs_amd.HostScene(sb))
    ref, _ = gpu_ctx.render(32, 32, 5, 4242)
    out, noisy, _ = gpu_ctx.render_denoised(2, 2, 5, 17, keep_noisy=True)
    ok = np.isfinite(ref).all(axis=2) & np.isfinite(noisy).all(axis=2)
    e_d = float(((out[ok].astype(np.float64) - ref[ok]) ** 2).mean())
    e_n = float(((noisy[ok].astype(np.float64) - ref[ok]) ** 2).mean())
    print(f"cornell 128 x 128, 4 spp, all guides, defaults: MSE {e_n:.5g} -> {e_d:.5g}, ratio {e_d / e_n:.4f}")
    assert e_d / e_n < 1.0


def test_refusals_leave_the_context_usable(gpu_ctx):
    from test_gpu_pixel_filter import scene
    _, hs = scene("cornell")
    L = gpu_ctx._L
    rgb, guides = synthetic(24, 20, 3)
    out = np.empty_like(rgb)

    def call(fn=L.pbrs_denoise, params=True, rgb_in=True, g=True, rgb_out=True, drop=(), **fields):
        p = api.DenoiseParams.make(24, 20, demodulate=True, id_stop=True)
        for n, v in fields.items():
            setattr(p, n, v)
        gs = api.DenoiseGuides()
        for n in GUIDES:
            if n not in drop:
                setattr(gs, n, guides[n].ctypes.data)
        return fn(gpu_ctx._h, C.addressof(p) if params else None, rgb.ctypes.data if rgb_in else None, C.addressof(gs) if g else None,
                  out.ctypes.data if rgb_out else None)
    nan, inf = float("nan"), float("inf")
    for fn in (L.pbrs_denoise, L.pbrs_denoise_device):  # (the device variant refuses before it touches a pointer)
        assert call(fn, params=False) == -1 and call(fn, rgb_in=False) == -1 and call(fn, g=False) == -1 and call(fn, rgb_out=False) == -1
        assert call(fn, w=0) == -1 and call(fn, h=0) == -1
        assert call(fn, iterations=0) == -1 and call(fn, iterations=7) == -1
        for s in ("sigma_color", "sigma_normal", "sigma_depth"):
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
            got, want = both(fresh, rgb2, g2, 5, True, True)
            assert same(got, want).all(), (w, h)
    finally:
        fresh.close()
