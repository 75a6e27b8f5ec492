"""pbrsb_bloom and pbrsb_bloom_device on the device against tests/bloom_model.py, the numpy model of the header's text: bit for bit over
sizes that send every kernel down each of its paths, the call forms, the header's two rules, the refusals, and the chain of
Context.render_temporal."""
import ctypes as C

import numpy as np
import pytest

import bloom_model as bm
import pbrs_amd
from common import bits
from pbrs_amd import DeviceBuffers, api, scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
# (w, h).  One pixel; a level 0 of one row or column; one row and one column (16-byte groups that straddle every row start); a tile and
# its halo cut at every edge; two and four destination tiles; 64 x 64, whose level 0 is 32 x 32; 130 x 67, two tiles and a pixel on x.
# k_bloom_tail takes a level over once it holds, with the levels below it, at most 5461 pixels: the levels of 128 x 128 (4096 + 1024 + 256
# + 64 + 16 + 4 = 5460) go to it from level 0 on, those of 130 x 128 (4160 + 1056 + 272 + 72 + 20 + 6 = 5586) from level 1 on (one
# k_bloom_down on a level, one k_bloom_up), and 300 x 260 (19500, 4875 + 1254 + ...) from level 2 on (two of each).
SIZES = ((1, 1), (2, 3), (1, 40), (40, 1), (17, 9), (33, 31), (64, 64), (130, 67), (128, 128), (130, 128), (300, 260))
# levels 1, 2 and 6; with and without MIX; threshold 0 and 1; knee 0 and 0.5; spread 0, 0.6 and 1: every value once, not the product
CONFIGS = (dict(levels=6, threshold=1.0, knee=0.5, strength=0.5, spread=0.6),
           dict(levels=2, threshold=0.0, knee=0.0, strength=0.75, spread=1.0, mix=True),
           dict(levels=1, threshold=1.0, knee=0.0, strength=1.0, spread=0.0),
           dict(levels=8, threshold=0.5, knee=1.0, strength=0.25, spread=0.3))


def hdr(w, h, seed=11):
    """Seeded HDR noise, log-uniform over twelve octaves, with a few NaN, inf, negative and zero pixels where the tile logic can lose them:
    the corners, both sides of a source tile's border (31 | 32) and of a destination tile's (15 | 16).  A site outside the image is
    skipped."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    rgb = np.exp2(rng.uniform(-6, 6, (h, w, 3))).astype(f32)

    def put(y, x, value):
        if 0 <= y < h and 0 <= x < w:
            rgb[y, x] = value

    put(0, 0, (np.nan, 1.0, 2.0)), put(h - 1, w - 1, (1.0, np.inf, 2.0)), put(0, w - 1, (0.0, 0.0, 0.0)), put(h - 1, 0, (-4.0, 2.0, -0.0))
    put(h // 2, w // 2, (3e38, 3e38, 3e38)), put(3, 5, (-np.inf, 0.0, 1.0)), put(5, 3, (1e-40, 1e-39, 0.0)), put(2, 2, (-1.0, -2.0, -3.0))
    put(31, 31, (np.nan, np.nan, np.nan)), put(32, 32, (500.0, 400.0, 300.0)), put(31, 32, (0.0, 0.0, 0.0)), put(15, 16, (np.inf, np.inf, np.inf))
    put(16, 15, (900.0, 0.0, 0.0)), put(64, 33, (-0.0, 1.0, np.nan))
    return rgb


_images, _models = {}, {}


def image(w, h):
    if (w, h) not in _images:
        _images[w, h] = hdr(w, h)
        _images[w, h].flags.writeable = False
    return _images[w, h]


def model(w, h, **kw):
    key = (w, h, tuple(sorted(kw.items())))
    if key not in _models:
        _models[key] = bm.bloom(image(w, h), **kw)
        _models[key].flags.writeable = False
    return _models[key]


def on_device(ctx, rgb, in_place=False, offset=0, **kw):
    """bloom_device on buffers of the test's own, the planes `offset` bytes into their allocations; the input is read only."""
    h, w, _ = rgb.shape
    n = rgb.nbytes

    def padded(a):
        raw = np.full(n + 16, 0xA5, np.uint8)
        raw[offset:offset + n] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return raw

    with DeviceBuffers({"rgb": padded(rgb), "out": padded(np.zeros_like(rgb))}) as dev:
        src = dev.ptr("rgb") + offset
        dst = src if in_place else dev.ptr("out") + offset
        ctx.bloom_device(src, dst, w, h, **kw)
        ctx.collect_stats()  # waits for the stream
        raw = {name: dev.download(name, n + 16, np.uint8) for name in ("rgb", "out")}
    for name in raw:  # nothing outside the plane is written
        assert (raw[name][:offset] == 0xA5).all() and (raw[name][offset + n:] == 0xA5).all(), name
    if not in_place:
        assert (raw["rgb"][offset:offset + n] == rgb.view(np.uint8).reshape(-1)).all()
    return raw["rgb" if in_place else "out"][offset:offset + n].copy().view(f32).reshape(h, w, 3)


def same(got, want, what):
    diff = bits(got) != bits(want)
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matches_the_cpu_model_bit_for_bit(gpu_ctx, size):
    w, h = size
    rgb = image(w, h)
    for kw in CONFIGS:
        same(on_device(gpu_ctx, rgb, **kw), model(w, h, **kw), kw)
    same(gpu_ctx.bloom(rgb, **CONFIGS[0]), model(w, h, **CONFIGS[0]), "the host form")


@pytest.mark.parametrize("size", ((33, 31), (130, 67), (130, 128)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_call_forms_agree(gpu_ctx, size):
    """The host form, the device form, in place, and planes 4 bytes off a 16-byte boundary (the scalar paths of the first downsample and
    of the composite) give the same bytes, with and without MIX."""
    w, h = size
    rgb = image(w, h)
    for kw in CONFIGS[:2]:
        want = model(w, h, **kw)
        same(gpu_ctx.bloom(rgb, **kw), want, ("host", kw))
        same(on_device(gpu_ctx, rgb, **kw), want, ("device", kw))
        same(on_device(gpu_ctx, rgb, in_place=True, **kw), want, ("in place", kw))
        same(on_device(gpu_ctx, rgb, offset=4, **kw), want, ("4 bytes off", kw))
        same(on_device(gpu_ctx, rgb, offset=4, in_place=True, **kw), want, ("4 bytes off, in place", kw))


def test_strength_zero_returns_the_inputs_bits(gpu_ctx):
    rgb = image(33, 31)
    for mix in (False, True):
        same(on_device(gpu_ctx, rgb, strength=0.0, mix=mix), rgb, mix)
        same(on_device(gpu_ctx, rgb, strength=0.0, mix=mix, in_place=True), rgb, mix)
        same(gpu_ctx.bloom(rgb, strength=0.0, mix=mix), rgb, mix)


@pytest.mark.parametrize("j", (7, -7))
def test_the_scale_rule_holds_on_the_device(gpu_ctx, j):
    rng = np.random.default_rng(j + 40)
    rgb = np.exp2(rng.uniform(-6, 6, (67, 130, 3))).astype(f32)
    rgb[5, 7] = (0.0, 0.0, 0.0)
    rgb[9, 3] = (-1.0, 2.0, 3.0)
    s = f32(2.0) ** j
    for kw in (dict(threshold=1.0, knee=0.5, strength=0.5), dict(threshold=0.0, knee=0.0, strength=0.5, mix=True)):
        base = on_device(gpu_ctx, rgb, **kw)
        scaled = on_device(gpu_ctx, rgb * s, **{**kw, "threshold": float(f32(kw["threshold"]) * s)})
        same(scaled, base * s, kw)
        same(base, bm.bloom(rgb, **kw), kw)


@pytest.mark.parametrize("size", ((1, 1), (5, 3), (33, 17), (130, 128)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_constant_image_is_its_own_bloom_on_the_device(gpu_ctx, size):
    w, h = size
    rgb = np.full((h, w, 3), 0.75, f32)
    for levels, spread, strength in ((6, 0.6, 0.3), (1, 1.0, 1.0)):
        same(on_device(gpu_ctx, rgb, levels=levels, threshold=0.0, knee=0.0, strength=strength, spread=spread, mix=True), rgb, (levels, spread, strength))


def test_refusals_leave_the_context_usable(gpu_ctx):
    L = gpu_ctx._L
    w, h = 9, 7
    img = np.ascontiguousarray(image(17, 9)[:h, :w])
    out = np.zeros_like(img)
    nan, inf = float("nan"), float("inf")

    def call(fn, params=True, rgb=True, dst=True, **fields):
        p = api.BloomParams.make(w, h)
        for n, v in fields.items():
            setattr(p, n, v)
        return fn(gpu_ctx._h, C.addressof(p) if params else None, img.ctypes.data if rgb else None, out.ctypes.data if dst else None)

    for fn in (L.pbrsb_bloom, L.pbrsb_bloom_device):  # (the device variant refuses before it touches a pointer)
        assert call(fn, params=False) == -1 and call(fn, rgb=False) == -1 and call(fn, dst=False) == -1
        assert b"null bloom" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, w=0) == -1 and call(fn, h=0) == -1
        assert call(fn, levels=0) == -1 and call(fn, levels=9) == -1
        assert call(fn, flags=2) == -1 and call(fn, flags=0x80000001) == -1
        for n in ("threshold", "strength"):
            for v in (-1.0, nan, inf):
                assert call(fn, **{n: v}) == -1, (n, v)
        for n in ("knee", "spread"):
            for v in (-0.5, 1.5, nan, inf):
                assert call(fn, **{n: v}) == -1, (n, v)
        assert call(fn, flags=1, strength=1.5) == -1
        assert b"PBRS_BLOOM_MIX" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, w=1 << 15, h=(1 << 13) + 1) == -4
        assert b"2^28" in L.pbrs_last_error(gpu_ctx._h)
    assert (out == 0).all()
    assert call(L.pbrsb_bloom) == 0
    same(out, bm.bloom(img), "a valid call after the refusals")
    same(on_device(gpu_ctx, image(33, 31), **CONFIGS[0]), model(33, 31, **CONFIGS[0]), "the device form after the refusals")


def test_render_temporal_blooms_and_displays_every_frame_on_the_stream(gpu_ctx):
    """Two frames of the Cornell box at 32 x 32 and 2 x 2 strata: the stats' "bloom" is the model on the frame's first image, the display
    image is Context.display of the bloomed one with the exposure carried from frame to frame, and bloom=None is the call without the
    keyword."""
    hs = pbrs_amd.HostScene(scenes.cornell_scene(width=32, height=32))
    gpu_ctx.upload(hs)
    cams, seeds = [hs.camera] * 2, [9, 10]
    bkw = dict(threshold=0.25, knee=0.5, strength=0.5, levels=4)
    plain = list(gpu_ctx.render_temporal(cams, 2, 2, 5, seeds, display=True))
    none = list(gpu_ctx.render_temporal(cams, 2, 2, 5, seeds, display=True, bloom=None))
    frames = list(gpu_ctx.render_temporal(cams, 2, 2, 5, seeds, display=True, bloom=bkw))
    default = list(gpu_ctx.render_temporal(cams, 2, 2, 5, seeds, bloom=True))
    assert len(plain) == len(none) == len(frames) == len(default) == 2
    e = None
    for k, (p, q, f, d) in enumerate(zip(plain, none, frames, default)):
        assert len(p) == len(q) == len(f) == len(d) == 4 and p[3].keys() == q[3].keys() and "bloom" not in q[3]
        for i in range(3):
            same(q[i], p[i], (k, i))
            same(f[i], p[i], (k, i))  # the first image stays the filter's: the glare goes into a buffer of its own
            same(d[i], p[i], (k, i))
        assert (q[3]["display"] == p[3]["display"]).all() and f32(q[3]["exposure"]).tobytes() == f32(p[3]["exposure"]).tobytes()
        assert set(f[3]) - {"bloom"} == set(p[3]) and set(d[3]) - {"bloom"} == set(p[3]) - {"display", "exposure"}
        want = bm.bloom(f[0], **bkw)
        assert f[3]["bloom"].shape == (32, 32, 3) and f[3]["bloom"].dtype == f32
        same(f[3]["bloom"], want, k)
        same(d[3]["bloom"], bm.bloom(d[0]), k)
        assert (bits(want) != bits(f[0])).any()
        shown, e = gpu_ctx.display(want, exposure_in=e, auto=True, return_exposure=True)
        assert (f[3]["display"] == shown).all(), k
        assert f32(f[3]["exposure"]).tobytes() == f32(e).tobytes(), k
    assert any((f[3]["display"] != p[3]["display"]).any() for f, p in zip(frames, plain))
    with pytest.raises(TypeError):
        next(gpu_ctx.render_temporal(cams, 2, 2, 5, seeds, bloom={"sigma": 1.0}))
