"""pbrsi_despeckle and pbrsi_despeckle_device on the device against tests/despeckle_model.py, the numpy model of the header's text: the
image, the variance, the mask, the removed energy and the 16-byte record bit for bit, over the sizes at which the tile and its halo can go
wrong, with the pixels that need care planted where tiles meet; the header's scale rule, the refusals, one render and one sequence."""
import ctypes as C
import itertools

import numpy as np
import pytest

import despeckle_model as dm
import pbrs_amd
from common import bits
from pbrs_amd import DeviceBuffers, api, scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN, INF = f32(np.nan), f32(np.inf)
# (w, h): one pixel, one row, one column, one exact tile, one pixel into the next tile on both axes, a radius-2 halo across two tile
# borders on x
SIZES = ((1, 1), (1, 9), (9, 1), (16, 16), (17, 19), (35, 18))
PATTERN = 0xA5
PAYLOAD = np.array([0x7FC12345], np.uint32).view(f32)[0]  # a NaN whose payload must survive


def planted(w, h, seed=3):
    """Seeded HDR noise and a variance plane, with the header's special cases where the tile logic can lose them: image corners, the first
    and the last row, both sides of the tile borders at 15 | 16 (and 31 | 32), tile corners.  A site outside the image is skipped."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    rgb = (rng.random((h, w, 3)) ** 4 * 20).astype(f32)
    var = (rng.random((h, w)) * 2 + 1e-3).astype(f32)

    def put(y, x, value, plane=rgb):
        if 0 <= y < h and 0 <= x < w:
            plane[y, x] = value

    if w * h >= 9:  # a 3 x 3 block of NaN (what fits of it): its centre has n = 0 at radius 1
        y0, x0 = min(5, max(h - 3, 0)), min(5, max(w - 3, 0))
        rgb[y0:y0 + 3, x0:x0 + 3] = NAN
    bright, dark_bright = (400.0, 300.0, 500.0), (900.0, 0.0, 0.0)
    put(0, 0, (NAN, 1.0, 2.0)), put(0, w - 1, (1.0, INF, 2.0)), put(h - 1, 0, (1.0, 2.0, -INF)), put(h - 1, w - 1, (3e38, 3e38, 3e38))
    put(0, w // 2, (-0.5, 1.0, 2.0)), put(h - 1, w // 2, (0.0, 0.0, 0.0)), put(h // 2, 0, (1e-40, 1e-40, 1e-40)), put(h // 2, w - 1, bright)
    put(15, 4, (1.0, NAN, 1.0)), put(16, 9, (INF, INF, INF)), put(7, 15, (-INF, 0.0, 0.0)), put(11, 16, (3e38, 3e38, 3e38))
    put(3, 15, bright), put(3, 16, bright)  # a pair across the x border
    put(9, 14, (3e38, 3e38, 3e38)), put(9, 15, (NAN, 0.0, 0.0)), put(9, 16, (3e38, 3e38, 3e38))  # a repair whose sum overflows, across it
    put(15, 2, dark_bright), put(16, 2, dark_bright)  # a pair across the y border
    put(12, 12, (-3.0, -2.0, -1.0)), put(13, 13, (0.0, 0.0, 0.0)), put(1, 1, (1e-40, 0.0, 1e-39))
    bx = 31 if w >= 33 else 15  # a 2 x 2 block across a tile corner
    for y, x in itertools.product((15, 16), (bx, bx + 1)):
        put(y, x, bright)
    if w >= 33:  # the other tile corner
        put(15, 15, (NAN, NAN, NAN)), put(15, 16, (3e38, 3e38, 3e38)), put(16, 15, (2.0, -1.0, 0.5)), put(16, 16, (1e-40, 1e-40, 1e-40))
    put(h // 2, w - 1, INF, var), put(15, bx, PAYLOAD, var), put(3, 15, 0.0, var), put(3, 16, 5.0, var)  # at pixels that are clamped
    put(1, 1, INF, var), put(2, 2, PAYLOAD, var), put(0, 0, 0.0, var), put(h - 1, 0, PAYLOAD, var)
    return rgb, var


def inputs(w, h):
    rgb, var = planted(w, h)
    return {"planted": (rgb, var), "all nan": (np.full((h, w, 3), NAN, f32), var),
            "constant": (np.broadcast_to(np.array((0.3, 2.0, 0.1), f32), (h, w, 3)).copy(), var)}


_models = {}


def model(name, w, h, radius, rank):
    key = (name, w, h, radius, rank)
    if key not in _models:
        rgb, var = inputs(w, h)[name]
        _models[key] = dm.despeckle(rgb, var, radius=radius, rank=rank)
    return _models[key]


def agree(what, got, want, variance=True, mask=True, removed=True, result=True):
    assert (bits(got["rgb"]) == bits(want["rgb"])).all(), what
    if variance:
        assert (bits(got["variance"]) == bits(want["variance"])).all(), what
    if mask:
        assert (got["mask"] == want["mask"]).all(), what
    if removed:
        assert (bits(got["removed"]) == bits(want["removed"])).all(), what
    if result:
        assert bytes(got["result"]) == dm.record(want), (what, got["result"].as_dict(), {n: want[n] for n in dm.FIELDS})


def on_device(ctx, rgb, var, variance=True, mask=True, removed=True, result=True, in_place=False, sync=None, **kw):
    """despeckle_device on buffers of the test's own -> {"rgb", "variance", "mask", "removed", "result"}; a plane the call is not given
    must come back untouched."""
    h, w, _ = rgb.shape
    fill = lambda n: np.full(n, PATTERN, np.uint8)  # noqa: E731
    with DeviceBuffers({"rgb": rgb, "var": var, "out": fill(12 * w * h), "vout": fill(4 * w * h), "mask": fill(4 * w * h), "removed": fill(12 * w * h),
                        "result": fill(16)}) as dev:
        planes = {}
        if variance:
            planes.update(variance_in=dev.ptr("var"), variance_out=dev.ptr("var" if in_place else "vout"))
        if mask:
            planes["mask_out"] = dev.ptr("mask")
        if removed:
            planes["removed_out"] = dev.ptr("removed")
        ctx.despeckle_device(dev.ptr("rgb"), dev.ptr("out"), w, h, dev.ptr("result") if result else None, planes, **kw)
        (sync or ctx.collect_stats)()  # waits for the stream
        raw = {n: dev.download(n, size, np.uint8) for n, size in (("vout", 4 * w * h), ("mask", 4 * w * h), ("removed", 12 * w * h), ("result", 16))}
        got = {"rgb": dev.download("out", (h, w, 3), f32), "variance": dev.download("var" if in_place else "vout", (h, w), f32),
               "mask": raw["mask"].view(np.uint32).reshape(h, w), "removed": raw["removed"].view(f32).reshape(h, w, 3),
               "result": api.DespeckleResult.from_buffer_copy(raw["result"])}
        assert (bits(dev.download("rgb", (h, w, 3), f32)) == bits(rgb)).all()  # the input is read only
        if not in_place:
            assert (bits(dev.download("var", (h, w), f32)) == bits(var)).all()
    for n, given in (("vout", variance and not in_place), ("mask", mask), ("removed", removed), ("result", result)):
        if not given:
            assert (raw[n] == PATTERN).all(), n
    return got


def on_host(ctx, rgb, var, mask=True, removed=True, **kw):
    out = list(ctx.despeckle(rgb, var, mask=mask, removed=removed, **kw))
    got = {"rgb": out.pop(0), "result": out.pop()}
    got["variance"] = out.pop(0) if var is not None else None
    got["mask"] = out.pop(0) if mask else None
    got["removed"] = out.pop(0) if removed else None
    assert not out
    return got


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matches_the_cpu_model_bit_for_bit(gpu_ctx, size):
    """Both radii, ranks 1 to 4; the planted image with and without the variance pair and each optional plane, through the device and the
    host form; a wholly NaN and a constant image."""
    w, h = size
    for radius, rank in itertools.product((1, 2), (1, 2, 3, 4)):
        kw = dict(radius=radius, rank=rank)
        for name, (rgb, var) in inputs(w, h).items():
            want = model(name, w, h, radius, rank)
            subsets = itertools.product((True, False), repeat=3) if name == "planted" else ((True, True, True), (False, False, False))
            for variance, mask, removed in subsets:
                what = (size, radius, rank, name, variance, mask, removed)
                agree(("device",) + what, on_device(gpu_ctx, rgb, var, variance, mask, removed, **kw), want, variance, mask, removed)
                agree(("host",) + what, on_host(gpu_ctx, rgb, var if variance else None, mask, removed, **kw), want, variance, mask, removed)
        nan, const = model("all nan", w, h, radius, rank), model("constant", w, h, radius, rank)
        assert (nan["n_clamped"], nan["n_repaired"]) == (0, w * h) and not bits(nan["rgb"]).any() and (bits(nan["variance"]) == bits(INF)).all()
        assert dm.record(const) == bytes(16) and (bits(const["rgb"]) == bits(inputs(w, h)["constant"][0])).all()
    want = model("planted", w, h, 1, 2)
    if w * h >= 9:
        assert want["n_repaired"] >= 3 and (want["mask"] == 3).sum() + (want["mask"] == 2).sum() == want["n_repaired"]
    if w >= 17 and h >= 16:  # the repair between two pixels of 3e38 overflows at either radius and rank: zeros, on the device too
        for radius, rank in itertools.product((1, 2), (1, 4)):
            m = model("planted", w, h, radius, rank)
            assert m["mask"][9, 15] & dm.REPAIRED and not bits(m["rgb"][9, 15]).any(), (radius, rank)
    if size == (35, 18):
        assert want["n_clamped"] >= 8 and (model("planted", w, h, 1, 1)["mask"] != want["mask"]).any()
        assert want["mask"][6, 6] == 2 and not bits(want["rgb"][6, 6]).any()  # the centre of the NaN block: n == 0


def tall(seed=23):
    """17 x 16403: two tiles across, 1026 down, 2052 in all, four more than the grid's 2048 blocks, so that blocks 0 to 3 take a second
    tile (2048 to 2051) and the walk wraps in x on the way.  Noise dim enough for its own pixels never to clamp, with NaNs and bright
    pixels in tiles 0, 2047, 2048 and the last one, and on the borders between them."""
    w, h = 17, 16 * 1025 + 3
    rng = np.random.default_rng(seed)
    rgb = (0.5 + 0.1 * rng.random((h, w, 3))).astype(f32)
    var = (rng.random((h, w)) * 2 + 1e-3).astype(f32)
    rows = {0: 3, 2047: 16 * 1023 + 5, 2048: 16 * 1024 + 2, 2051: h - 2}  # tile -> a row inside it (tile = 2 * (row // 16) + (x >= 16))
    for tile, y in rows.items():
        x = 16 if tile & 1 else 6
        rgb[y, x] = (400.0, 300.0, 500.0)
        rgb[y + 1, x - (0 if tile & 1 else 3)] = NAN
        var[y, x] = 3.0
    rgb[16 * 1024 - 1:16 * 1024 + 1, 15:17] = (90.0, 80.0, 70.0)  # a 2 x 2 block on the corner of tiles 2046, 2047, 2048 and 2049
    rgb[16 * 1024, 8], rgb[16 * 1024 - 1, 8] = (NAN, 1.0, 1.0), (1.0, INF, 1.0)  # both sides of the border between tiles 2046 and 2048
    return rgb, var


def test_a_block_walks_more_than_one_tile(gpu_ctx):
    """More tiles than the grid has blocks: the tile walk, the barrier before a block stages its next tile over the planes, the tile's
    position from its index, and the counts summed over a block's tiles, at both radii, with the variance pair and the record, against
    the model on whole planes (which tests/test_despeckle_model.py holds to the per-pixel one)."""
    rgb, var = tall()
    h, w, _ = rgb.shape
    assert -(-w // 16) == 2 and 2 * -(-h // 16) == 2052 > 2048
    for radius, rank in ((1, 2), (2, 3)):
        want = dm.despeckle_planes(rgb, var, radius=radius, rank=rank)
        tiles = 2 * (np.nonzero(want["mask"])[0] // 16) + (np.nonzero(want["mask"])[1] >= 16)
        assert {0, 2047, 2048, 2051} <= set(tiles.tolist()) and want["n_repaired"] == 6 and want["n_clamped"] >= 4,(radius, sorted(set(tiles.tolist())))
        agree(("device", radius), on_device(gpu_ctx, rgb, var, radius=radius, rank=rank), want)
        agree(("host", radius), on_host(gpu_ctx, rgb, var, radius=radius, rank=rank), want)


def test_the_call_forms_agree(gpu_ctx):
    """No result wanted; the variance in place equals out of place; the device form on a stream set with pbrs_set_stream."""
    w, h = 35, 18
    rgb, var = planted(w, h)
    hip, stream = api.hip_runtime(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0

    def wait():
        assert hip.hipStreamSynchronize(stream) == 0

    try:
        for radius, rank in ((1, 2), (2, 4)):
            want = model("planted", w, h, radius, rank)
            kw = dict(radius=radius, rank=rank)
            agree("no record", on_device(gpu_ctx, rgb, var, result=False, **kw), want, result=False)
            agree("in place", on_device(gpu_ctx, rgb, var, in_place=True, **kw), want)
            gpu_ctx.set_stream(stream.value)
            try:
                agree("on a caller's stream", on_device(gpu_ctx, rgb, var, sync=wait, **kw), want)
            finally:
                gpu_ctx.set_stream(0)
            agree("back on the context's stream", on_device(gpu_ctx, rgb, var, **kw), want)
    finally:
        assert hip.hipStreamDestroy(stream) == 0
    h_none = gpu_ctx.despeckle(rgb)
    assert len(h_none) == 2 and (bits(h_none[0]) == bits(model("planted", w, h, 1, 2)["rgb"])).all()


def test_the_scale_rule_holds_on_the_device(gpu_ctx):
    """floor == 0: the input times 2^j gives the output and the removed energy times 2^j, the variance times 4^j, the same mask and record."""
    rng = np.random.default_rng(17)
    w, h = 35, 18
    rgb = (rng.random((h, w, 3)) ** 4 * 20 + 1e-3).astype(f32)
    var = (rng.random((h, w)) * 2 + 1e-3).astype(f32)
    rgb[15:17, 15:17] *= f32(200)
    rgb[3, 31:33] *= f32(500)
    rgb[0, 0], rgb[17, 34, 1], rgb[16, 16, 2] = NAN, INF, -INF
    var[3, 31] = INF
    base = on_device(gpu_ctx, rgb, var)
    agree("the base", base, dm.despeckle(rgb, var))
    assert base["result"].n_clamped >= 4 and base["result"].n_repaired == 3
    for j in (3, -3):
        scaled = on_device(gpu_ctx, np.ldexp(rgb, j), np.ldexp(var, 2 * j))
        assert (bits(scaled["rgb"]) == bits(np.ldexp(base["rgb"], j))).all() and (bits(scaled["removed"]) == bits(np.ldexp(base["removed"], j))).all()
        assert (bits(scaled["variance"]) == bits(np.ldexp(base["variance"], 2 * j))).all()
        assert (scaled["mask"] == base["mask"]).all() and bytes(scaled["result"]) == bytes(base["result"])


def test_refusals_leave_the_context_usable(gpu_ctx):
    w, h = 17, 19
    rgb, var = planted(w, h)
    L, ctx = gpu_ctx._L, gpu_ctx._h
    out, vout, mask, removed = np.empty_like(rgb), np.empty_like(var), np.empty((h, w), np.uint32), np.empty_like(rgb)

    def call(params=None, result=True, **planes):
        p = api.DespeckleParams.make(w, h, **(params or {}))
        ptrs = dict(rgb_in=rgb.ctypes.data, rgb_out=out.ctypes.data, variance_in=var.ctypes.data, variance_out=vout.ctypes.data, mask_out=mask.ctypes.data,
                    removed_out=removed.ctypes.data)
        ptrs.update(planes)
        io, r = api.DespeckleIO(*(ptrs[n] for n, _ in api.DespeckleIO._fields_)), api.DespeckleResult()
        return L.pbrsi_despeckle(ctx, C.addressof(p), C.addressof(io), C.addressof(r) if result else None)

    assert call() == 0 and call(result=False) == 0
    invalid = [dict(params=dict(radius=0)), dict(params=dict(radius=3)), dict(params=dict(rank=0)), dict(params=dict(rank=5)), dict(params=dict(gain=0.999)),
               dict(params=dict(gain=float("inf"))), dict(params=dict(gain=float("nan"))), dict(params=dict(floor=-1e-30)), dict(params=dict(floor=float("inf"))),
               dict(params=dict(floor=float("nan"))), dict(rgb_in=None), dict(rgb_out=None), dict(variance_in=None), dict(variance_out=None),
               dict(rgb_out=rgb.ctypes.data), dict(rgb_out=var.ctypes.data), dict(variance_out=rgb.ctypes.data), dict(mask_out=rgb.ctypes.data),
               dict(mask_out=var.ctypes.data), dict(removed_out=rgb.ctypes.data), dict(removed_out=var.ctypes.data), dict(variance_out=out.ctypes.data),
               dict(mask_out=out.ctypes.data), dict(removed_out=out.ctypes.data), dict(mask_out=vout.ctypes.data), dict(removed_out=vout.ctypes.data),
               dict(removed_out=mask.ctypes.data)]
    for kw in invalid:
        assert call(**kw) == -1, kw  # PBRS_E_INVALID
    for w0, h0, flags in ((0, h, 0), (w, 0, 0), (w, h, 1), (w, h, 0x80000000)):
        p = api.DespeckleParams.make(w0, h0)
        p.flags = flags
        io = api.DespeckleIO(rgb.ctypes.data, out.ctypes.data)
        assert L.pbrsi_despeckle(ctx, C.addressof(p), C.addressof(io), None) == -1, (w0, h0, flags)
    io = api.DespeckleIO(rgb.ctypes.data, out.ctypes.data)
    assert L.pbrsi_despeckle(ctx, None, C.addressof(io), None) == -1 and L.pbrsi_despeckle(ctx, C.addressof(api.DespeckleParams.make(w, h)), None, None) == -1
    with pytest.raises(pbrs_amd.PbrsError, match="radius"):
        gpu_ctx.despeckle(rgb, radius=3)
    with pytest.raises(pbrs_amd.PbrsError, match="cannot be rgb_in"):
        gpu_ctx.despeckle_device(4096, 4096, w, h)
    p = api.DespeckleParams.make(1 << 15, (1 << 13) + 1)
    assert L.pbrsi_despeckle(ctx, C.addressof(p), C.addressof(io), None) == -4  # PBRS_E_LIMIT
    assert L.pbrsi_despeckle_device(ctx, C.addressof(p), C.addressof(io), None) == -4
    agree("a valid call afterwards", on_host(gpu_ctx, rgb, var), model("planted", w, h, 1, 2))
    agree("... and on the device", on_device(gpu_ctx, rgb, var), model("planted", w, h, 1, 2))


SEED = 9


def _specular_cornell(size):
    hs = pbrs_amd.HostScene(scenes.cornell_scene(width=size, height=size, variant="specular"))
    return hs


def test_a_real_frame(gpu_ctx):
    """The Cornell box with the glass and the metal sphere at 64 x 64 and 2 x 2 strata, with its variance AOV, despeckled on the device."""
    gpu_ctx.upload(_specular_cornell(64))
    rgb, aov, _ = gpu_ctx.render_aovs(2, 2, 8, SEED, aovs=("variance",))
    var = aov["variance"]
    want = dm.despeckle(rgb, var)
    print(f"a real frame: n_clamped {want['n_clamped']} n_repaired {want['n_repaired']} removed mean {want['removed'].mean():.6g} of {rgb[np.isfinite(rgb)].mean():.6g}")
    agree("device", on_device(gpu_ctx, rgb, var), want)
    agree("host", on_host(gpu_ctx, rgb, var), want)
    assert want["n_clamped"] > 0
    for kw in (dict(radius=2, rank=3, gain=1.5), dict(rank=1, gain=4.0, floor=0.05)):
        agree(kw, on_device(gpu_ctx, rgb, var, **kw), dm.despeckle(rgb, var, **kw))


def test_render_temporal_despeckles_every_frame_on_the_stream(gpu_ctx):
    """Three frames at 48 x 48 with despeckle=True against the same chain queued by hand from the public device calls, the despeckle step
    checked against the model on the way; despeckle=None is the call without the keyword."""
    hs = _specular_cornell(48)
    gpu_ctx.upload(hs)
    cams, seeds, w, h = [hs.camera] * 3, [9, 10, 11], 48, 48
    guides = ("albedo", "normal", "depth", "instance")
    plain = list(gpu_ctx.render_temporal(cams, 2, 2, 8, seeds))
    none = list(gpu_ctx.render_temporal(cams, 2, 2, 8, seeds, despeckle=None))
    frames = list(gpu_ctx.render_temporal(cams, 2, 2, 8, seeds, despeckle=True))
    tuned = list(gpu_ctx.render_temporal(cams, 2, 2, 8, seeds, despeckle={"rank": 1, "gain": 4.0}))
    assert len(plain) == len(none) == len(frames) == len(tuned) == 3
    for k, (p, q) in enumerate(zip(plain, none)):
        assert len(p) == len(q) == 4 and p[3].keys() == q[3].keys() and "despeckle" not in q[3]
        for i in range(3):
            assert (bits(p[i]) == bits(q[i])).all(), (k, i)
    # the chain by hand: render with guides and variance, despeckle, accumulate, filter; two ping-pong halves of the guides and the history
    n = w * h * 4
    sizes = {"rgb": 3 * n, "clean": 3 * n, "variance": n, "acc_variance": n, "out": 3 * n, "record": 16}
    kept = [g for g in api.TEMPORAL_GUIDES if g in guides]
    for k in (0, 1):
        sizes.update({f"{g}{k}": api.DENOISE_GUIDES[g][0] * n for g in guides})
        sizes.update({f"h_rgb{k}": 3 * n, f"h_moments{k}": 2 * n, f"h_length{k}": n})
    clamped_somewhere = False
    with DeviceBuffers(sizes) as dev:
        for i, (cam, seed) in enumerate(zip(cams, seeds)):
            cur, old = i & 1, (i & 1) ^ 1
            gp = {g: dev.ptr(f"{g}{cur}") for g in guides}
            hist = [{m: dev.ptr(f"h_{m}{k}") for m in api.TEMPORAL_HISTORY} for k in (0, 1)]
            gpu_ctx.render_aovs_var_device(dev.ptr("rgb"), gp, dev.ptr("variance"), 2, 2, 8, seed)
            gpu_ctx.collect_stats()
            noisy, var = dev.download("rgb", (h, w, 3), f32), dev.download("variance", (h, w), f32)
            gpu_ctx.despeckle_device(dev.ptr("rgb"), dev.ptr("clean"), w, h, dev.ptr("record"),
                                     {"variance_in": dev.ptr("variance"), "variance_out": dev.ptr("variance")})
            gpu_ctx.temporal_accumulate_device({"rgb": dev.ptr("clean"), "variance": dev.ptr("variance"), **{g: gp[g] for g in kept}}, hist[cur], w, h, cam,
                                               hist[old] if i else None, {g: dev.ptr(f"{g}{old}") for g in kept} if i else None, cam if i else None,
                                               dev.ptr("acc_variance"))
            gpu_ctx.denoise_var_device(hist[cur]["rgb"], dev.ptr("out"), w, h, dev.ptr("acc_variance"), gp)
            gpu_ctx.collect_stats()
            want = dm.despeckle(noisy, var)
            assert (bits(dev.download("clean", (h, w, 3), f32)) == bits(want["rgb"])).all(), i
            assert (bits(dev.download("variance", (h, w), f32)) == bits(want["variance"])).all(), i
            assert dev.download("record", 16, np.uint8).tobytes() == dm.record(want), i
            clamped_somewhere |= want["n_clamped"] > 0
            f = frames[i]
            assert len(f) == 4 and isinstance(f[3]["despeckle"], api.DespeckleResult) and bytes(f[3]["despeckle"]) == dm.record(want), i
            assert set(f[3]) - {"despeckle"} == set(plain[i][3])
            assert (bits(f[0]) == bits(dev.download("out", (h, w, 3), f32))).all(), i
            assert (bits(f[1]) == bits(dev.download(f"h_rgb{cur}", (h, w, 3), f32))).all(), i
            assert (bits(f[2]) == bits(noisy)).all() and (bits(f[2]) == bits(plain[i][2])).all(), i  # the noisy image stays the render's own
            assert bytes(tuned[i][3]["despeckle"]) == dm.record(dm.despeckle(noisy, var, rank=1, gain=4.0)), i
    assert clamped_somewhere and any((bits(f[0]) != bits(p[0])).any() for f, p in zip(frames, plain))
    with pytest.raises(TypeError):
        next(gpu_ctx.render_temporal(cams, 2, 2, 8, seeds, despeckle={"sigma": 1.0}))
    agree("the context is usable", on_host(gpu_ctx, *planted(17, 19)), model("planted", 17, 19, 1, 2))
