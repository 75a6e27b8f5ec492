"""pbrsx_compare and pbrsx_compare_device on the device against tests/compare_model.py, the numpy model of the header's text: the 64 bytes
of the result and both maps bit for bit, over sizes with partial tiles on both axes and tile counts that are no power of two, invalid
pixels where the tiles and the windows can get them wrong, the header's identities, one render and one frame sequence."""
import ctypes as C
import itertools

import numpy as np
import pytest

import compare_model as cm
import pbrs_amd
from common import bits
from pbrs_amd import DeviceBuffers, api, scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
# (w, h): below the window, one whole tile, partial tiles on both axes with 3 x 2 and 19 x 2 tiles, and 4 x 3 tiles with the invalid pixels
SIZES = ((1, 1), (7, 5), (16, 16), (33, 17), (300, 20), (64, 48))
TRANSFORMS = {"linear": cm.LINEAR, "reinhard": cm.REINHARD}
PEAK = {"linear": 20.0, "reinhard": 1.0}
PATTERN = 0xA5


def hdr_pair(w, h, seed=11):
    rng = np.random.default_rng(seed + 1000 * w + h)
    b = (rng.random((h, w, 3)) ** 4 * 20).astype(f32)
    a = (b + rng.normal(0, 0.5, b.shape)).astype(f32)  # the noise takes dark pixels below zero: REINHARD's clamp is exercised
    if (w, h) == (64, 48):
        nan, inf = f32(np.nan), f32(np.inf)
        a[0, 0, 0], b[0, 63, 1], a[47, 0, 2], b[47, 63, 0] = nan, inf, -inf, nan  # the four corners
        a[5, 15, 1], b[5, 16, 1] = inf, -inf                                      # both sides of a vertical tile border
        b[15, 20, 2], a[16, 20, 0] = nan, nan                                     # ... and of a horizontal one
        a[16:32, 32:48, 0] = nan                                                  # one whole tile
        b[40, :, 1] = inf                                                         # one whole row
        assert (a[np.isfinite(a)] < 0).any()
    return a, b


_models = {}


def model(w, h, transform, ssim):
    key = (w, h, transform, ssim)
    if key not in _models:
        a, b = hdr_pair(w, h)
        _models[key] = cm.compare(a, b, TRANSFORMS[transform], ssim, peak=PEAK[transform])
    return _models[key]


def agree(what, got, error, ssim_map, want, maps):
    assert bytes(got) == cm.record(want), (what, got.as_dict(), {n: want[n] for n in cm.FIELDS})
    if maps:
        assert (bits(error) == bits(want["error_map"])).all(), what
        if want["ssim_map"] is None:
            assert ssim_map is None, what
        else:
            assert (bits(ssim_map) == bits(want["ssim_map"])).all(), what


def on_device(ctx, a, b, maps, **kw):
    """compare_device on buffers of the test's own -> (CompareResult, error map or None, ssim map or None, the ssim plane's bytes)."""
    h, w, _ = a.shape
    planes = {"error": np.full(4 * w * h, PATTERN, np.uint8), "ssim": np.full(4 * w * h, PATTERN, np.uint8)}
    with DeviceBuffers({"a": a, "b": b, "result": np.full(64, PATTERN, np.uint8), **planes}) as dev:
        with_ssim = kw.get("ssim", True)
        ptrs = {"error_out": dev.ptr("error"), "ssim_out": dev.ptr("ssim") if with_ssim else None} if maps else None
        ctx.compare_device(dev.ptr("a"), dev.ptr("b"), w, h, dev.ptr("result"), ptrs, **kw)
        ctx.collect_stats()  # waits for the stream
        result = api.CompareResult.from_buffer_copy(dev.download("result", 64, np.uint8))
        error = dev.download("error", (h, w), f32) if maps else None
        ssim_plane = dev.download("ssim", 4 * w * h, np.uint8)
        return result, error, ssim_plane.view(f32).reshape(h, w) if maps and with_ssim else None, ssim_plane


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matches_the_cpu_model_bit_for_bit(gpu_ctx, size):
    """Both transforms, with and without SSIM, with and without maps, through the host and the device variant: the result's 64 bytes and
    the maps as words, so that the NaN patterns of invalid pixels count."""
    w, h = size
    a, b = hdr_pair(w, h)
    for transform, ssim, maps in itertools.product(TRANSFORMS, (True, False), (True, False)):
        want = model(w, h, transform, ssim)
        kw = dict(transform=transform, ssim=ssim, peak=PEAK[transform])
        what = (size, transform, ssim, maps)
        got = gpu_ctx.compare(a, b, maps=maps, **kw)
        agree(("host",) + what, *(got if maps else (got, None, None)), want, maps)
        result, error, ssim_map, ssim_plane = on_device(gpu_ctx, a, b, maps, **kw)
        agree(("device",) + what, result, error, ssim_map, want, maps)
        if not (maps and ssim):
            assert (ssim_plane == PATTERN).all(), what  # a call that is not given the plane leaves it alone
    if size == (64, 48):
        want = model(w, h, "reinhard", True)
        assert want["n_invalid"] == 4 + 4 + 256 + 64 and want["n_valid"] + want["n_invalid"] == w * h  # (the row crosses none of the others)
        assert 0 < want["n_ssim"] <= want["n_valid"]


@pytest.mark.parametrize("w", (8209, 32787, 131075), ids=lambda w: f"{w}x1")
def test_more_tiles_than_the_finish_kernel_holds_in_lds(gpu_ctx, w):
    """k_compare_finish reduces the last 512 tile records in LDS and joins four records per trip through memory before that: one-row
    images of 514, 2050 and 8193 tiles (the last one partial) take one, two and three such trips, through counts that are no multiple
    of four (514; 2050, 513; 8193, 2049, 513)."""
    a, b = hdr_pair(w, 1)
    a[0, 100, 0], b[0, w - 1, 2] = np.nan, np.inf
    for transform, ssim in (("reinhard", True), ("linear", False)):
        want = cm.compare(a, b, TRANSFORMS[transform], ssim, peak=PEAK[transform])
        kw = dict(transform=transform, ssim=ssim, peak=PEAK[transform])
        agree(("host", w, transform), *gpu_ctx.compare(a, b, maps=True, **kw), want, True)
        result, error, ssim_map, _ = on_device(gpu_ctx, a, b, True, **kw)
        agree(("device", w, transform), result, error, ssim_map, want, True)
    assert want["n_invalid"] == 2


def test_the_identities_hold_on_the_device(gpu_ctx):
    """compare(a, a); the swap symmetry; the LINEAR scale rule for j = 3 and j = -3."""
    for w, h in ((33, 17), (300, 20)):
        a, b = hdr_pair(w, h)
        for transform in TRANSFORMS:
            same, _, smap = gpu_ctx.compare(a, a, maps=True, transform=transform, peak=PEAK[transform])
            assert same.mse == 0.0 and same.mae == 0.0 and same.rel_mse == 0.0 and same.max_abs == 0.0
            assert same.ssim == 1.0 and same.n_ssim == same.n_valid == w * h and (bits(smap) == bits(f32(1.0))).all()
            ab = gpu_ctx.compare(a, b, transform=transform, peak=PEAK[transform])
            ba = gpu_ctx.compare(b, a, transform=transform, peak=PEAK[transform])
            for n in ("mse", "mae", "max_abs", "ssim"):
                assert np.float64(getattr(ab, n)).tobytes() == np.float64(getattr(ba, n)).tobytes(), (w, h, transform, n)
        base, e0, _ = gpu_ctx.compare(a, b, maps=True, transform="linear", ssim=False)
        for j in (3, -3):
            scaled, e1, _ = gpu_ctx.compare(np.ldexp(a, j), np.ldexp(b, j), maps=True, transform="linear", ssim=False)
            assert scaled.mse == np.ldexp(base.mse, 2 * j) and scaled.mae == np.ldexp(base.mae, j) and scaled.max_abs == np.ldexp(base.max_abs, j)
            assert (bits(e1) == bits(np.ldexp(e0, 2 * j))).all()


def test_without_ssim_the_ssim_plane_is_refused_and_untouched(gpu_ctx):
    """The refusal stands in front of the kernel: a call without PBRS_COMPARE_SSIM that names an ssim_out is turned away and writes
    nothing, and the same call without the plane writes the error map beside it and not one byte of the plane."""
    w, h = 33, 17
    a, b = hdr_pair(w, h)
    with DeviceBuffers({"a": a, "b": b, "result": np.zeros(64, np.uint8), "error": np.full(4 * w * h, PATTERN, np.uint8),
                        "ssim": np.full(4 * w * h, PATTERN, np.uint8)}) as dev:
        with pytest.raises(pbrs_amd.PbrsError, match="needs PBRS_COMPARE_SSIM"):
            gpu_ctx.compare_device(dev.ptr("a"), dev.ptr("b"), w, h, dev.ptr("result"), {"error_out": dev.ptr("error"), "ssim_out": dev.ptr("ssim")},
                                   ssim=False)
        gpu_ctx.collect_stats()
        assert (dev.download("ssim", 4 * w * h, np.uint8) == PATTERN).all() and (dev.download("error", 4 * w * h, np.uint8) == PATTERN).all()
        gpu_ctx.compare_device(dev.ptr("a"), dev.ptr("b"), w, h, dev.ptr("result"), {"error_out": dev.ptr("error")}, ssim=False)
        gpu_ctx.collect_stats()
        assert (dev.download("ssim", 4 * w * h, np.uint8) == PATTERN).all()
        want = model(w, h, "reinhard", False)
        assert (bits(dev.download("error", (h, w), f32)) == bits(want["error_map"])).all()
        assert dev.download("result", 64, np.uint8).tobytes() == cm.record(want)


def test_refusals_leave_the_context_usable(gpu_ctx):
    a, b = hdr_pair(7, 5)
    for kw, message in ((dict(peak=0.0), "peak"), (dict(rel_epsilon=float("nan")), "rel_epsilon"), (dict(transform=2), "transform")):
        with pytest.raises(pbrs_amd.PbrsError, match=message):
            gpu_ctx.compare(a, b, **kw)
    p, r = api.CompareParams.make(1 << 15, (1 << 13) + 1), api.CompareResult()
    assert gpu_ctx._L.pbrsx_compare(gpu_ctx._h, C.addressof(p), a.ctypes.data, b.ctypes.data, None, C.addressof(r)) == -4  # PBRS_E_LIMIT
    assert bytes(gpu_ctx.compare(a, b)) == cm.record(model(7, 5, "reinhard", True))


def _cornell_64():
    hs = pbrs_amd.HostScene(scenes.cornell_scene(width=64, height=64))
    return hs, [hs.camera] * 3


def test_a_render_against_its_reference_in_device_buffers(gpu_ctx):
    """The 64 x 64 Cornell box at 2 x 2 strata against 16 x 16 strata, both rendered into device buffers and compared there."""
    hs, _ = _cornell_64()
    gpu_ctx.upload(hs)
    n_rgb = 3 * 64 * 64 * 4
    with DeviceBuffers({"a": n_rgb, "b": n_rgb, "result": 64, "linear": 64}) as dev:
        gpu_ctx.render_device(dev.ptr("a"), 2, 2, 5, 9)
        gpu_ctx.render_device(dev.ptr("b"), 16, 16, 5, 10)
        gpu_ctx.compare_device(dev.ptr("a"), dev.ptr("b"), 64, 64, dev.ptr("result"))
        gpu_ctx.compare_device(dev.ptr("a"), dev.ptr("b"), 64, 64, dev.ptr("linear"), transform="linear", ssim=False)
        gpu_ctx.collect_stats()
        a, b = dev.download("a", (64, 64, 3), f32), dev.download("b", (64, 64, 3), f32)
        result = api.CompareResult.from_buffer_copy(dev.download("result", 64, np.uint8))
        linear = api.CompareResult.from_buffer_copy(dev.download("linear", 64, np.uint8))
    assert np.isfinite(a).all() and np.isfinite(b).all() and result.n_valid == 64 * 64
    assert bytes(result) == cm.record(cm.compare(a, b)) and bytes(linear) == cm.record(cm.compare(a, b, cm.LINEAR, False))
    # any order of n non-negative f64 terms is within n * 2^-53 relative of the exact sum, and so is numpy's: ten times that between the two
    plain = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    assert abs(linear.mse - plain) <= 10 * a.size * 2.0 ** -53 * plain
    denoised, _ = gpu_ctx.render_denoised_var(2, 2, 5, 9)
    filtered = gpu_ctx.compare(denoised, b)
    for name, r in (("noisy", result), ("denoise_var", filtered)):
        print(f"{name}: mse {r.mse:.6g} rel_mse {r.rel_mse:.6g} ssim {r.ssim:.6g} psnr {r.psnr():.2f} dB")
    assert bytes(filtered) == cm.record(cm.compare(denoised, b))


def test_render_temporal_scores_every_frame_on_the_stream(gpu_ctx):
    """Three frames of the 64 x 64 Cornell box with reference=: every frame's record is Context.compare of the yielded image and the
    reference, and the first four entries are the bits of the same call without it."""
    hs, cams = _cornell_64()
    gpu_ctx.upload(hs)
    reference, _ = gpu_ctx.render(8, 8, 5, 77)
    plain = list(gpu_ctx.render_temporal(cams, 2, 2, 5, [9, 10, 11]))
    scored = list(gpu_ctx.render_temporal(cams, 2, 2, 5, [9, 10, 11], reference=reference))
    per_frame = list(gpu_ctx.render_temporal(cams, 2, 2, 5, [9, 10, 11], reference=(reference * f32(k + 1) for k in range(3))))
    assert len(plain) == len(scored) == len(per_frame) == 3
    for k, (p, s, q) in enumerate(zip(plain, scored, per_frame)):
        assert len(p) == 4 and len(s) == 5 and len(q) == 5
        for i in range(3):
            assert (bits(p[i]) == bits(s[i])).all() and (bits(p[i]) == bits(q[i])).all(), (k, i)
        assert p[3].keys() == s[3].keys()
        assert isinstance(s[4], api.CompareResult)
        assert bytes(s[4]) == bytes(gpu_ctx.compare(s[0], reference)) == cm.record(cm.compare(s[0], reference)), k
        assert bytes(q[4]) == bytes(gpu_ctx.compare(q[0], reference * f32(k + 1))), k
    assert all(s[4].mse > 0.0 and s[4].n_valid == 64 * 64 for s in scored)
    with pytest.raises(ValueError, match=r"frame 0's reference is \(64, 64, 3\)"):
        next(gpu_ctx.render_temporal(cams, 2, 2, 5, [9, 10, 11], reference=np.zeros((32, 32, 3), f32)))
    assert bytes(gpu_ctx.compare(reference, reference))[:8] == bytes(8)  # the context is usable: mse == 0.0
