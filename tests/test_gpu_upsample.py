"""Guided upsampling on the GPU (include/pbrs_gpu.h, pbrs_upsample[_device]; device/upsample.h): bit for bit against the CPU model of
tests/upsample_model.py at every factor and radius on sizes that cover a low image of one pixel, sizes no factor divides, block seams and
the LDS tile's four edges; every guide subset, the three kinds of min_weight, weight_out given and NULL, planted non-finite and denormal
values; the device variant; what the header refuses; the device chains of Context.render_upscaled and render_temporal(upscale=...)
against the same chains assembled by hand; and the quality case of the Cornell box."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import pbrs_amd
import upsample_model as um
from common import bits
from pbrs_amd import DeviceBuffers, api, scenes
from test_gpu_denoise import same
from test_gpu_temporal import _yawed

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = ((1, 1), (2, 2), (5, 3), (16, 16), (17, 15), (33, 31), (130, 97))  # (w, h), full
CASES = [(f, R) for f in um.FACTORS for R in um.RADII]
GUIDES = ("albedo", "normal", "depth", "instance")
# name -> (the guide pairs given, demodulate, id_stop)
SUBSETS = {"none": ((), False, False), "normal": (("normal",), False, False), "depth": (("depth",), False, False),
           "id stop": (("instance",), False, True), "demodulation": (("albedo",), True, False), "all": (GUIDES, True, True)}
MIN_WEIGHTS = (0.0, um.DEFAULTS["min_weight"], 1e30)


@functools.lru_cache(maxsize=None)
def inputs(w, h, f):
    rgb_lo, lo, hi = um.synthetic(w, h, f, 100 * f + w + h)
    for a in (rgb_lo, *lo.values(), *hi.values()):
        a.setflags(write=False)
    return rgb_lo, lo, hi


def agree(got, want, what):
    bad = ~same(got, want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def both(ctx, w, h, f, subset, weight=True, **params):
    """(GPU image, GPU weights or None, model image, model weights) of one call."""
    rgb_lo, lo, hi = inputs(w, h, f)
    names, demodulate, id_stop = SUBSETS[subset]
    g = dict(lo={n: lo[n] for n in names}, hi={n: hi[n] for n in names}, demodulate=demodulate, id_stop=id_stop, **params)
    det = {}
    want = um.upsample(rgb_lo, w, h, f, details=det, **g)
    got = ctx.upsample(rgb_lo, w, h, f, return_weight=weight, **g)
    return (got if weight else (got, None)) + (want, det["W"])


@pytest.mark.parametrize("f,R", CASES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matches_the_cpu_model_bit_for_bit(gpu_ctx, size, f, R):
    """All guides, both flags, the default min_weight, the weights returned; and the call without any guide."""
    w, h = size
    got, gw, want, ww = both(gpu_ctx, w, h, f, "all", radius=R)
    agree(got, want, (size, f, R))
    agree(gw, ww, (size, f, R, "weight_out"))
    got, _, want, _ = both(gpu_ctx, w, h, f, "none", weight=False, radius=R)
    agree(got, want, (size, f, R, "no guides"))
    if size == (130, 97):  # what the inputs plant is there, and reaches all three branches of the result
        rgb_lo, lo, hi = inputs(w, h, f)
        assert np.isnan(rgb_lo).any() and np.isinf(rgb_lo).any() and ((rgb_lo != 0) & (np.abs(rgb_lo) < 1e-38)).any()
        assert (hi["depth"] == 0).any() and np.isinf(hi["depth"]).any() and np.isinf(lo["depth"]).any() and (lo["albedo"] < 1e-3).any()
        assert (ww > 1e-3).any() and (ww == 0).any()


@pytest.mark.parametrize("f,R", CASES)
@pytest.mark.parametrize("size", ((17, 15), (33, 31)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_guide_subset_min_weight_and_weight_out(gpu_ctx, size, f, R):
    w, h = size
    seen = {}
    for (subset, mw), weight in zip(itertools.product(SUBSETS, MIN_WEIGHTS), itertools.cycle((True, False))):
        got, gw, want, ww = both(gpu_ctx, w, h, f, subset, weight=weight, radius=R, min_weight=mw)
        agree(got, want, (size, f, R, subset, mw))
        if weight:
            agree(gw, ww, (size, f, R, subset, mw, "weight_out"))
        seen[subset, mw] = bits(want).tobytes()
    tent = seen["none", 0.0]
    for subset, (_, demodulate, _) in SUBSETS.items():
        if not demodulate:  # (which divides and multiplies by the albedos whatever branch is taken)
            assert seen[subset, 1e30] == tent, subset  # the tent branch everywhere: the call without guides
    assert len({seen[s, um.DEFAULTS["min_weight"]] for s in SUBSETS}) == len(SUBSETS)  # every stop that is switched on changes the result


def test_the_device_variant_on_caller_buffers_equals_the_host_variant(gpu_ctx):
    """On planes at 16-byte alignment and 4 bytes off it (the kernel loads words: both must give the host variant's bits)."""
    for (w, h, f, R), off in zip(((33, 31, 2, 2), (130, 97, 3, 1), (17, 15, 4, 2)), (0, 1, 1)):
        rgb_lo, lo, hi = inputs(w, h, f)
        host, hw_ = gpu_ctx.upsample(rgb_lo, w, h, f, lo=lo, hi=hi, radius=R, return_weight=True)
        pad = lambda a: np.concatenate([np.zeros(off, a.dtype), a.reshape(-1)])  # noqa: E731
        arrays = {"rgb_lo": rgb_lo, "out": np.zeros((h, w, 3), f32), "weight": np.zeros((h, w), f32),
                  **{f"{n}_lo": lo[n] for n in GUIDES}, **{f"{n}_hi": hi[n] for n in GUIDES}}
        with DeviceBuffers({n: pad(a) for n, a in arrays.items()}) as dev:
            at = lambda n: dev.ptr(n) + 4 * off  # noqa: E731
            gpu_ctx.upsample_device(at("rgb_lo"), at("out"), w, h, f, {n: at(f"{n}_lo") for n in GUIDES}, {n: at(f"{n}_hi") for n in GUIDES},
                                    at("weight"), radius=R)
            gpu_ctx.collect_stats()
            agree(dev.download_like("out", pad(host))[off:].reshape(host.shape), host, (w, h, f, R, off))
            agree(dev.download_like("weight", pad(hw_))[off:].reshape(hw_.shape), hw_, (w, h, f, R, off, "weight_out"))
            gpu_ctx.upsample_device(at("rgb_lo"), at("out"), w, h, f, radius=R)  # no guides, no weights
            gpu_ctx.collect_stats()
            agree(dev.download_like("out", pad(host))[off:].reshape(host.shape), gpu_ctx.upsample(rgb_lo, w, h, f, radius=R), (w, h, f, R, off, "tent"))


def test_refusals_leave_the_context_usable(gpu_ctx):
    L = gpu_ctx._L
    w, h, f = 24, 20, 2
    rgb_lo, lo, hi = inputs(w, h, f)
    out, weight = np.empty((h, w, 3), f32), np.empty((h, w), f32)

    def call(fn=L.pbrs_upsample, params=True, drop=(), out_at=None, weight_at="weight", **fields):
        p = api.UpsampleParams.make(w, h, f, demodulate=True, id_stop=True)
        for n, v in fields.items():
            setattr(p, n, v)
        gl, gh = api.DenoiseGuides(), api.DenoiseGuides()
        for n in GUIDES:
            setattr(gl, n, None if f"{n}_lo" in drop else lo[n].ctypes.data)
            setattr(gh, n, None if f"{n}_hi" in drop else hi[n].ctypes.data)
        planes = {"rgb_lo": rgb_lo, "out": out, "weight": weight, **{f"{n}_lo": lo[n] for n in GUIDES}, **{f"{n}_hi": hi[n] for n in GUIDES}}
        ptr = lambda n: None if n is None or n in drop else planes[n].ctypes.data  # noqa: E731
        return fn(gpu_ctx._h, C.addressof(p) if params else None, ptr("rgb_lo"), None if "lo" in drop else C.addressof(gl),
                  None if "hi" in drop else C.addressof(gh), ptr(out_at or "out"), ptr(weight_at))
    nan, inf = float("nan"), float("inf")
    for fn in (L.pbrs_upsample, L.pbrs_upsample_device):  # (the device variant refuses before it touches a pointer)
        assert call(fn, params=False) == -1
        for n in ("rgb_lo", "lo", "hi", "out"):
            assert call(fn, drop=(n,)) == -1, n
        assert call(fn, w=0) == -1 and call(fn, h=0) == -1
        assert call(fn, factor=0) == -1 and call(fn, factor=1) == -1 and call(fn, factor=5) == -1
        assert call(fn, radius=0) == -1 and call(fn, radius=3) == -1
        for n in ("sigma_normal", "sigma_depth"):
            for v in (0.0, -1.0, nan, inf):
                assert call(fn, **{n: v}) == -1, (n, v)
        for n in ("albedo_floor", "min_weight"):
            for v in (-1.0, nan, inf):
                assert call(fn, **{n: v}) == -1, (n, v)
        assert call(fn, flags=4) == -1 and call(fn, flags=0x80000003) == -1
        for n in GUIDES:  # one of a pair
            assert call(fn, drop=(f"{n}_lo",)) == -1 and call(fn, drop=(f"{n}_hi",)) == -1, n
        assert b"only one" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, drop=("albedo_lo", "albedo_hi")) == -1 and b"DEMODULATE" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, drop=("instance_lo", "instance_hi")) == -1 and b"ID_STOP" in L.pbrs_last_error(gpu_ctx._h)
        for n in ("rgb_lo", *(f"{g}_{s}" for g in GUIDES for s in ("lo", "hi"))):
            assert call(fn, out_at=n) == -1, n
            assert call(fn, weight_at=n) == -1, n
        assert call(fn, weight_at="out") == -1
        assert call(fn, w=1 << 15, h=(1 << 13) + 1) == -4  # PBRS_E_LIMIT
        assert b"2^28" in L.pbrs_last_error(gpu_ctx._h)
    # what is allowed: no weights, no guide pairs at all, pairs whose flags are off
    assert call(weight_at=None) == 0
    agree(out, um.upsample(rgb_lo, w, h, f, lo=lo, hi=hi, demodulate=True, id_stop=True), "all guides")
    assert call(drop=tuple(f"{g}_{s}" for g in GUIDES for s in ("lo", "hi")), flags=0) == 0
    agree(out, um.tent(rgb_lo, w, h, f), "no guides")
    assert call(flags=0, radius=2) == 0
    agree(out, um.upsample(rgb_lo, w, h, f, lo=lo, hi=hi, radius=2), "flags off")
    # a plain render afterwards: the bits of a fresh context, which also grows its staging from nothing
    from test_gpu_pixel_filter import scene
    _, hs = scene("cornell")
    gpu_ctx.upload(hs)
    img, _ = gpu_ctx.render(2, 2, 3, 1)
    fresh = pbrs_amd.Context(0)
    try:
        fresh.upload(hs)
        assert (bits(img) == bits(fresh.render(2, 2, 3, 1)[0])).all()
        for (w2, h2, f2) in ((9, 7, 3), (70, 50, 2), (33, 21, 4)):
            r2, l2, h2_ = inputs(w2, h2, f2)
            agree(fresh.upsample(r2, w2, h2, f2, lo=l2, hi=h2_), um.upsample(r2, w2, h2, f2, lo=l2, hi=h2_, demodulate=True, id_stop=True), (w2, h2, f2))
    finally:
        fresh.close()


def _by_hand(ctx, cam, strata, depth, seed, factor, **up):
    """The pieces of one upscaled frame from the existing host calls -> (low image, its AOVs with the variance, the full-size guides)."""
    cam_lo = api.scaled_camera(cam, factor)
    img, aov, _ = ctx.render_aovs(strata, strata, depth, seed, aovs=GUIDES + ("variance",), tile=(0, 0, cam_lo.width, cam_lo.height), camera=cam_lo)
    _, hi, _ = ctx.render_aovs(1, 1, 1, seed, aovs=GUIDES, camera=cam)
    return cam_lo, img, aov, hi


def test_render_upscaled_is_the_chain_assembled_by_hand(gpu_ctx):
    hs = pbrs_amd.HostScene(scenes.cornell_scene(width=32, height=32))
    gpu_ctx.upload(hs)
    for factor, up in ((2, {}), (4, dict(radius=2)), (3, dict(min_weight=0.0))):
        cam_lo, img, aov, hi = _by_hand(gpu_ctx, hs.camera, 2, 5, 9, factor)
        var = aov.pop("variance")
        den = gpu_ctx.denoise_var(img, var, iterations=3, **aov)
        want = gpu_ctx.upsample(den, 32, 32, factor, lo=aov, hi=hi, **up)
        full, low, st = gpu_ctx.render_upscaled(2, 2, 5, 9, factor=factor, upsample=up, iterations=3)
        assert full.shape == (32, 32, 3) and low.shape == (cam_lo.height, cam_lo.width, 3) and st["low_res"] == (cam_lo.width, cam_lo.height)
        assert same(low, den).all() and same(full, want).all(), factor
        agree(full, um.upsample(den, 32, 32, factor, lo=aov, hi=hi, demodulate=True, id_stop=True, **up), (factor, "the model"))


def test_render_temporal_upscaled_is_the_chain_assembled_by_hand(gpu_ctx):
    """32 x 32 Cornell box, three frames, a yaw of 4 degrees per frame: render_temporal(upscale=2) against the host calls; upscale=None
    and a call that never names the keyword give the same bits."""
    hs = pbrs_amd.HostScene(scenes.cornell_scene(width=32, height=32))
    gpu_ctx.upload(hs)
    cams = [_yawed(hs.camera, 4.0 * k) for k in range(3)]
    tparams = dict(id_test=True)
    run = lambda **kw: list(gpu_ctx.render_temporal(cams, 2, 2, 5, [9, 10, 11], temporal=tparams, iterations=3, **kw))  # noqa: E731
    up, none, unnamed = run(upscale=2), run(upscale=None), run()
    shown = run(upscale=dict(factor=2, radius=2), display=True)
    for a, b in zip(none, unnamed):
        assert all((bits(x) == bits(y)).all() for x, y in zip(a[:3], b[:3])) and "low_res" not in a[3]
    history = prev = cam_prev = None
    for k, cam in enumerate(cams):
        cam_lo, img, aov, hi = _by_hand(gpu_ctx, cam, 2, 5, 9 + k, 2)
        var = aov.pop("variance")
        history, v = gpu_ctx.temporal_accumulate(img, aov["depth"], cam_lo, variance=var, normal=aov["normal"], instance=aov["instance"],
                                                 history=history, prev=prev, camera_prev=cam_prev, **tparams)
        den = gpu_ctx.denoise_var(history["rgb"], v, iterations=3, **aov)
        full, acc, noisy, st = up[k]
        assert full.shape == (32, 32, 3) and acc.shape == noisy.shape == (16, 16, 3) and st["low_res"] == (16, 16)
        assert (bits(noisy) == bits(img)).all() and same(acc, history["rgb"]).all(), k
        assert same(full, gpu_ctx.upsample(den, 32, 32, 2, lo=aov, hi=hi)).all(), k
        wide = gpu_ctx.upsample(den, 32, 32, 2, lo=aov, hi=hi, radius=2)
        assert same(shown[k][0], wide).all() and shown[k][3]["display"].shape == (32, 32, 4), k
        prev, cam_prev = {n: aov[n] for n in ("depth", "normal", "instance")}, cam_lo


def test_the_guides_beat_the_plain_tent_on_the_cornell_box(gpu_ctx):
    """128 x 128 from 64 x 64 at 16 x 16 strata through render_upscaled with all guides, against the same low image through the call
    without guides; both against the plain 32 x 32-strata render (seed 4242) in the display-referred error of upsample_model.  Measured on
    an MI355X: guided 1.297e-4, plain tent 1.639e-4, ratio 0.791 ("Guided upsampling")."""
    from test_gpu_spatial_variance import cornell_128
    _, ref = cornell_128(gpu_ctx)
    full, low, _ = gpu_ctx.render_upscaled(16, 16, 5, 17, factor=2)
    plain = gpu_ctx.upsample(low, 128, 128, 2)
    e_g, e_p = um.display_error(full, ref), um.display_error(plain, ref)
    print(f"cornell 128 x 128 from 64 x 64, 256 spp, all guides: display-referred error guided {e_g:.4g}, plain tent {e_p:.4g}, ratio {e_g / e_p:.3f}")
    assert e_g < e_p
