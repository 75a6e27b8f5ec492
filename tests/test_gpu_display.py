"""The display transform on the GPU (include/pbrs_gpu.h, pbrs_display[_device]; device/display.h): bytes, exposure and histogram bit for
bit against the CPU model of tests/display_model.py for every curve, encode and quantiser with and without the auto exposure, the device
variant on caller buffers (aligned, misaligned, the exposure fed back), an image large enough that the kernels' grid-stride loops go
round twice, the constant image, the chain of Context.render_temporal, and what the header refuses."""
import ctypes as C
import itertools

import numpy as np
import pytest

import display_model as dm
import pbrs_amd
from common import bits
from pbrs_amd import DeviceBuffers, api, scenes
from test_display_model import lognormal, specials

pytestmark = pytest.mark.gpu

f32 = np.float32
# (w, h): w * h mod 4 takes all four values (the 4-pixel groups of k_display_apply and their tail), and from 37 x 29 on several blocks feed
# one histogram
SIZES = ((1, 1), (2, 3), (7, 5), (64, 1), (1, 64), (37, 29), (129, 67), (130, 70))
WHITES = (None, 4.0)  # +inf and finite


def _next(v, toward):
    return np.nextafter(f32(v), f32(toward))


def planted():
    """Pixels that sit on the edges of the header's rules."""
    not_counted, edge = specials()
    px = [[v, v, v] for v in not_counted] + [[edge, edge, edge], [0.0, 2.0 ** -31, 0.0], [3e38, 3e38, 3e38], [np.inf, -np.inf, 0.0], [-1.0, 2.0, -3.0],
                                             [np.nan, 1.0, 0.5], [-np.inf, 0.1, 0.2]]
    knee = f32(0.0031308)
    px += [[_next(knee, 0.0), knee, _next(knee, 1.0)], [1.0, _next(1.0, 0.0), _next(1.0, 2.0)]]
    # t whose encoded value times 255 is an integer, or next to one (sqrt: squares of n / 255 and of n / 510; the linear sRGB segment)
    for n in (1, 51, 85, 128, 254):
        g = f32(n / 255.0)
        px.append([f32(g * g), _next(f32(g * g), 0.0), _next(f32(g * g), 1.0)])
    px += [[0.25, 0.0625, 0.5625], [f32(1.0 / (255.0 * 12.92)), f32(5.0 / (255.0 * 12.92)), f32(10.0 / (255.0 * 12.92))]]
    px += [[70000.0, 65504.0, 65520.0], [1e30, _next(65504.0, 0.0), 1e10]]  # above the clamp of the scaled value
    return np.array(px, dtype=f32)


def image(w, h, seed=3):
    img = lognormal(h, w, seed, sigma=1.5)
    flat = img.reshape(-1, 3)
    px = planted()
    n = min(len(px), len(flat))
    rot = (w * 7 + h) % len(px)  # small images see different rows of the table
    flat[:n] = np.roll(px, -rot, axis=0)[:n]
    return img


def gpu(ctx, img, exposure_in=None, **kw):
    out, e, hist = ctx.display(img, exposure_in=exposure_in, return_exposure=True, return_histogram=True, **kw)
    return out, e, hist


def agree(got, want, what):
    (go, ge, gh), (wo, we, wh) = got, want
    assert go.shape == wo.shape and go.dtype == np.uint8
    bad = np.argwhere((go != wo).any(axis=2))
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), go[tuple(bad[0])].tolist(), wo[tuple(bad[0])].tolist())
    assert f32(ge).tobytes() == f32(we).tobytes(), (what, ge, we)
    assert (gh == wh).all(), what


@pytest.mark.parametrize("auto", (False, True), ids=("fixed", "auto"))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matches_the_cpu_model_bit_for_bit(gpu_ctx, size, auto):
    """Every curve x encode x quantiser, white +inf and finite, on a log-normal image with the planted pixels; a fixed exposure of 1
    (the planted values reach the curve as they are) and of 0.75, or the auto exposure with a compensation and trimming."""
    w, h = size
    img = image(w, h)
    seen = set()
    for curve, encode, quantize in itertools.product(dm.CURVES, dm.ENCODES, dm.QUANTIZERS):
        for white in (WHITES if curve == "reinhard" else (None,)):
            for extra in ((dict(exposure=1.5, key=0.25, low_q16=3000, high_q16=60000),) if auto else (dict(exposure=1.0), dict(exposure=0.75))):
                kw = dict(curve=curve, encode=encode, quantize=quantize, white=white, auto=auto, **extra)
                got = gpu(gpu_ctx, img, **kw)
                agree(got, dm.display(img, **kw), (size, kw))
                seen.add(got[0].tobytes())
                assert (got[0][:, :, 3] == 255).all()
    if w * h >= 1000:  # every setting changes the picture
        assert len(seen) == (3 * 2 * 3 + 2 * 3) * (1 if auto else 2)


def test_the_reference_settings_are_the_host_png(gpu_ctx, tmp_path):
    from test_image_io import read_png
    img = image(37, 29)
    pbrs_amd.write_image(tmp_path / "a.png", img)
    out = gpu_ctx.display(img, curve="none", encode="sqrt", quantize="trunc")
    assert (out[:, :, :3] == read_png(tmp_path / "a.png")).all()
    # exposure_out without the auto exposure and without a histogram: only the apply kernel runs, and it writes e = 1
    again, e = gpu_ctx.display(img, curve="none", encode="sqrt", quantize="trunc", return_exposure=True, exposure_in=7.0)
    assert (again == out).all() and f32(e).tobytes() == f32(1.0).tobytes()
    pbrs_amd.write_image_u8(tmp_path / "b.png", out)
    assert (read_png(tmp_path / "b.png") == out[:, :, :3]).all()


def _device_display(ctx, img, offset_words=0, io=None, **kw):
    """display_device on fresh caller buffers; the rgb plane starts `offset_words` floats into its allocation."""
    h, w, _ = img.shape
    pad = np.zeros(offset_words + img.size, dtype=f32)
    pad[offset_words:] = img.reshape(-1)
    with DeviceBuffers({"rgb": pad, "out": np.zeros((h, w), np.uint32)}) as dev:
        ctx.display_device(dev.ptr("rgb") + 4 * offset_words, dev.ptr("out"), w, h, io, **kw)
        ctx.collect_stats()
        return dev.download("out", (h, w), np.uint32).view(np.uint8).reshape(h, w, 4)


@pytest.mark.parametrize("size", ((37, 29), (129, 67), (130, 70), (7, 5), (64, 1)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_device_variant_on_caller_buffers_gives_the_host_variants_bytes(gpu_ctx, size):
    """Aligned planes (the 16-byte path with its tail of w * h mod 4 pixels) and an rgb plane 4 bytes off (the scalar path), no io."""
    w, h = size
    img = image(w, h, seed=8)
    for kw in (dict(curve="aces", encode="srgb", quantize="dither", exposure=0.5), dict(curve="reinhard", encode="sqrt", quantize="round", auto=True, white=2.0)):
        want = gpu_ctx.display(img, **kw)
        assert (want == dm.display(img, **kw)[0]).all()
        for offset in (0, 1):
            assert (_device_display(gpu_ctx, img, offset, **kw) == want).all(), (size, offset, kw)


def test_the_exposure_word_carries_a_sequence_on_the_device(gpu_ctx):
    """Three calls, exposure_out fed back as exposure_in through one device word (the host only looks at it), against the model's three;
    the histogram comes back too."""
    w, h = 37, 29
    imgs = [(lognormal(h, w, 20 + k, sigma=1.0) * f32(4.0 ** k)).astype(f32) for k in range(3)]
    kw = dict(auto=True, adapt=0.25, curve="aces", encode="srgb", quantize="round")
    with DeviceBuffers({"e": np.zeros(1, f32), "hist": np.zeros(dm.BINS, np.uint32)}) as word:
        # without the auto exposure the word receives 1 (from the apply kernel: nothing else is launched) and exposure_in is not read
        out = _device_display(gpu_ctx, imgs[0], io={"exposure_in": word.ptr("e"), "exposure_out": word.ptr("e")}, curve="none", exposure=2.0)
        assert (out == dm.display(imgs[0], curve="none", exposure=2.0)[0]).all()
        assert word.download("e", 1, f32)[0].tobytes() == f32(1.0).tobytes()
        e = None
        for k, img in enumerate(imgs):
            prev = e
            io = {"exposure_in": word.ptr("e") if k else None, "exposure_out": word.ptr("e"), "histogram_out": word.ptr("hist")}
            out = _device_display(gpu_ctx, img, io=io, **kw)
            want, e, hist = dm.display(img, exposure_in=prev, **kw)
            assert (out == want).all(), k
            assert word.download("e", 1, f32)[0].tobytes() == e.tobytes(), k
            assert (word.download("hist", dm.BINS, np.uint32) == hist).all(), k
            agree(gpu(gpu_ctx, img, exposure_in=prev, **kw), (want, e, hist), k)  # the host variant, the same chain
        assert len({float(dm.display(img, **kw)[1]) for img in imgs}) == 3  # the three targets differ: the easing is visible
        assert float(e) != float(dm.display(imgs[2], **kw)[1])


def test_an_image_that_sends_the_grid_stride_loops_round_again(gpu_ctx):
    """k_display_hist and k_display_apply take four pixels per thread and trip, under a cap of 2048 blocks of 256 threads: 2048 x 1025
    pixels are the smallest image of that width whose last 2048 pixels are reached in a second trip (524 288 threads x 4).  No curve, sqrt,
    truncation, auto exposure: the model stays cheap."""
    w, h = 2048, 1025
    assert w * h > 2048 * 256 * 4 >= w * (h - 1)
    img = lognormal(h, w, 31, sigma=1.0)
    img[-1, -3:] = [[0.25, 1.0, 4.0], [np.nan, 0.0625, 0.0], [9.0, 0.5, 0.01]]
    kw = dict(curve="none", encode="sqrt", quantize="trunc", auto=True)
    agree(gpu(gpu_ctx, img, **kw), dm.display(img, **kw), "2048 x 1025")


def test_a_constant_image_counts_every_pixel_in_one_bin(gpu_ctx):
    """Every LDS add of a block lands on one address."""
    img = np.full((70, 130, 3), 0.5, dtype=f32)
    out, e, hist = gpu(gpu_ctx, img, auto=True)
    _, b = dm.bins_of(dm.lum(img[:1, :1]).reshape(-1))
    assert hist[b[0]] == 9100 and hist.sum() == 9100
    agree((out, e, hist), dm.display(img, auto=True), "constant")
    assert len(np.unique(out.reshape(-1, 4), axis=0)) == 1


def _cornell_64():
    hs = pbrs_amd.HostScene(scenes.cornell_scene(width=64, height=64))
    return hs, [hs.camera] * 3


def test_render_temporal_with_a_display_is_the_hand_made_chain(gpu_ctx):
    hs, cams = _cornell_64()
    gpu_ctx.upload(hs)
    dkw = dict(curve="aces", encode="srgb", quantize="dither", adapt=0.5, exposure=1.25)
    e = None
    k = -1
    for k, (den, acc, noisy, st) in enumerate(gpu_ctx.render_temporal(cams, 2, 2, 5, [9, 10, 11], display=dkw)):
        prev = e
        want, e, _ = gpu(gpu_ctx, den, exposure_in=prev, auto=True, **dkw)
        assert st["display"].shape == (64, 64, 4) and st["display"].dtype == np.uint8
        assert (st["display"] == want).all(), k
        assert f32(st["exposure"]).tobytes() == f32(e).tobytes(), k
        assert (want == dm.display(den, exposure_in=prev, auto=True, **dkw)[0]).all(), k
        assert len(np.unique(want[:, :, :3])) > 50
    assert k == 2


def test_without_a_display_a_sequence_keeps_its_bits(gpu_ctx):
    hs, cams = _cornell_64()
    gpu_ctx.upload(hs)
    plain = list(gpu_ctx.render_temporal(cams, 2, 2, 5, [9, 10, 11]))
    named = list(gpu_ctx.render_temporal(cams, 2, 2, 5, [9, 10, 11], display=None))
    shown = list(gpu_ctx.render_temporal(cams, 2, 2, 5, [9, 10, 11], display=True))
    for a, b, c in zip(plain, named, shown):
        for k in range(3):
            assert (bits(a[k]) == bits(b[k])).all() and (bits(a[k]) == bits(c[k])).all()
        assert "display" not in a[3] and "display" not in b[3] and "exposure" not in b[3] and "display" in c[3]
        assert {n: v for n, v in c[3].items() if n not in ("display", "exposure")}.keys() == a[3].keys()


def test_refusals_leave_the_context_usable(gpu_ctx):
    L = gpu_ctx._L
    w, h = 9, 7
    img = image(w, h)
    out = np.zeros((h, w), np.uint32)
    nan, inf = float("nan"), float("inf")

    def call(fn=L.pbrs_display, params=True, rgb=True, dst=True, alias=False, auto=True, io=False, **fields):
        p = api.DisplayParams.make(w, h, auto=auto)
        for n, v in fields.items():
            setattr(p, n, v)
        ios = api.DisplayIO()
        return fn(gpu_ctx._h, C.addressof(p) if params else None, img.ctypes.data if rgb else None, C.addressof(ios) if io else None,
                  (img.ctypes.data if alias else out.ctypes.data) if dst else None)

    for fn in (L.pbrs_display, L.pbrs_display_device):  # (the device variant refuses before it touches a pointer)
        assert call(fn, params=False) == -1 and call(fn, rgb=False) == -1 and call(fn, dst=False) == -1
        assert b"null display" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, w=0) == -1 and call(fn, h=0) == -1
        assert call(fn, curve=3) == -1 and call(fn, encode=2) == -1 and call(fn, quantize=3) == -1
        assert call(fn, flags=2) == -1 and call(fn, flags=0x80000001) == -1
        for n in ("exposure", "key"):
            for v in (0.0, -1.0, nan, inf):
                assert call(fn, **{n: v}) == -1, (n, v)
        for v in (0.0, -1.0, nan):
            assert call(fn, white=v) == -1, v
        for n in ("min_exposure", "max_exposure"):
            for v in (0.0, -1.0, nan, inf):
                assert call(fn, **{n: v}) == -1, (n, v)
        assert call(fn, min_exposure=2.0, max_exposure=1.0) == -1
        for v in (0.0, -0.5, 1.5, nan):
            assert call(fn, adapt=v) == -1, v
        assert call(fn, low_q16=5, high_q16=5) == -1 and call(fn, low_q16=9, high_q16=3) == -1 and call(fn, high_q16=65537) == -1
        assert b"ranks" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, alias=True) == -1
        assert call(fn, w=1 << 15, h=(1 << 13) + 1) == -4  # PBRS_E_LIMIT
        assert b"2^28" in L.pbrs_last_error(gpu_ctx._h)
        # exposure and white are read without the auto exposure too
        assert call(fn, auto=False, exposure=nan) == -1 and call(fn, auto=False, white=0.0) == -1
    # what is allowed: the auto exposure's fields hold anything without its flag; no io, or an io of NULLs
    assert call(auto=False, key=nan, min_exposure=-1.0, max_exposure=inf, adapt=7.0, low_q16=9, high_q16=3) == 0
    assert (out.view(np.uint8).reshape(h, w, 4) == dm.display(img)[0]).all()
    assert call(io=True) == 0
    assert (out.view(np.uint8).reshape(h, w, 4) == dm.display(img, auto=True)[0]).all()
    assert call(white=inf, curve=1) == 0
    assert (out.view(np.uint8).reshape(h, w, 4) == dm.display(img, auto=True, curve="reinhard")[0]).all()
    # a plain render afterwards: the bits of a fresh context, which also grows its scratch and staging from nothing
    from test_gpu_pixel_filter import scene
    _, hs = scene("cornell")
    gpu_ctx.upload(hs)
    rendered, _ = gpu_ctx.render(2, 2, 3, 1)
    fresh = pbrs_amd.Context(0)
    try:
        fresh.upload(hs)
        assert (bits(rendered) == bits(fresh.render(2, 2, 3, 1)[0])).all()
        for size in ((9, 7), (70, 50), (33, 21)):
            i2 = image(*size)
            agree(gpu(fresh, i2, auto=True), dm.display(i2, auto=True), size)
    finally:
        fresh.close()
