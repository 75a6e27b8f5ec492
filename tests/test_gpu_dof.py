"""pbrsf_dof and pbrsf_dof_device on the device against tests/dof_model.py, the numpy model of the header's text: bit for bit, image and
circles, over sizes and radii that send the kernel down each of its paths, the call forms, the refusals, and the chain of
Context.render_temporal."""
import ctypes as C

import numpy as np
import pytest

import bloom_model as bm
import dof_model as dm
import pbrs_amd
from common import bits
from pbrs_amd import DeviceBuffers, api, libs, scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
FOCUS = 2.0
# (w, h, max_radius).  The sizes: one pixel; one row and one column; a halo larger than the image on every side; a second tile, a pixel
# wide (16 x 16 tiles); the halo cut at every edge; a whole number of tiles; tiles with a full halo inside the image.  The radii: 1, the
# two sides of the kernel's halo classes (4 | 5 and 8 | 9) and 16, each paired with one size, not the product.
CASES = ((1, 1, 1), (1, 40, 4), (40, 1, 5), (5, 5, 16), (17, 9, 5), (33, 31, 9), (48, 40, 8), (130, 67, 1), (130, 67, 5), (64, 33, 4))
# from this size on the inputs must send the kernel down every path (below)
FULL = (17, 9)


def hdr(w, h, seed=17):
    """Seeded HDR noise, log-uniform over twelve octaves, with NaN, inf, negative and zero pixels where the tile logic can lose them:
    the corners and both sides of a tile's border (15 | 16).  A site outside the image is skipped."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    rgb = np.exp2(rng.uniform(-6, 6, (h, w, 3))).astype(f32)

    def put(y, x, value):
        if 0 <= y < h and 0 <= x < w:
            rgb[y, x] = value

    put(0, 0, (np.nan, 1.0, 2.0)), put(h - 1, w - 1, (1.0, np.inf, 2.0)), put(0, w - 1, (0.0, 0.0, 0.0)), put(h - 1, 0, (-4.0, 2.0, -0.0))
    put(3, 15, (np.inf, np.inf, np.inf)), put(3, 16, (-1.0, -2.0, -3.0)), put(15, 6, (0.0, 0.0, 0.0)), put(16, 6, (-np.inf, 0.0, 1.0))
    put(15, 16, (np.nan, np.nan, np.nan)), put(16, 15, (900.0, 0.0, 0.0)), put(5, 3, (1e-40, 1e-39, 0.0)), put(h // 2, w // 2, (3e38, 3e38, 3e38))
    return rgb


def ramp(w, h):
    """A depth that grows along x through FOCUS (0.4 to 2.0 times it; a little along y too, so that no two rows are alike), with 8 x 8
    blocks pulled near (a tenth of FOCUS) and exactly to FOCUS whose edges fall on both sides of the tile border 15 | 16, in x and in y,
    +inf misses, and a few pixels of 0, -1 and NaN."""
    x, y = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    z = (FOCUS * (0.4 + 1.6 * x / max(w - 1, 1)) * (1.0 + 0.002 * y)).astype(f32)

    def block(y0, x0, value):
        z[max(y0, 0):max(y0 + 8, 0), max(x0, 0):max(x0 + 8, 0)] = value

    block(2, 8, 0.1 * FOCUS), block(0, 16, FOCUS)        # x edges at 15 | 16 from either side
    block(8, 24, 0.1 * FOCUS), block(16, 28, FOCUS)      # y edges at 15 | 16 from either side
    block(12, 10, 0.1 * FOCUS)                           # a near block across the corner of four tiles
    block(h - 6, w - 20, FOCUS), block(h - 12, 40, np.inf)

    def put(y, x, value):
        if 0 <= y < h and 0 <= x < w:
            z[y, x] = value

    put(1, 1, np.inf), put(h - 2, w - 2, np.inf), put(15, 15, np.inf), put(16, 16, np.inf), put(7, 12, np.inf)
    put(4, 2, 0.0), put(h - 1, 3, -1.0), put(2, 5, np.nan), put(15, 17, 0.0), put(16, 14, np.nan), put(0, w - 1, -1.0)
    return z


def params(R):
    """The circles reach max_radius on the near blocks (|z - F| / z = 9) and stay below R / 4 on the ramp, whose columns around FOCUS are
    sharp."""
    return dict(max_radius=R, focus=FOCUS, scale=R / 4.0)


_inputs, _models = {}, {}


def inputs(w, h):
    if (w, h) not in _inputs:
        _inputs[w, h] = (hdr(w, h), ramp(w, h))
        for a in _inputs[w, h]:
            a.flags.writeable = False
    return _inputs[w, h]


def model(w, h, **kw):
    key = (w, h, tuple(sorted(kw.items())))
    if key not in _models:
        _models[key] = dm.dof(*inputs(w, h), details=True, **kw)
    return _models[key]


def on_device(ctx, rgb, depth, offset=0, coc=True, **kw):
    """dof_device on buffers of the test's own, every plane `offset` bytes into its allocation -> (image, circles or None); the inputs
    are read only and nothing outside a plane is written."""
    h, w, _ = rgb.shape
    planes = {"rgb": rgb, "depth": depth, "out": np.full_like(rgb, 7.0), "coc": np.full_like(depth, 7.0)}

    def padded(a):
        raw = np.full(a.nbytes + 16, 0xA5, np.uint8)
        raw[offset:offset + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return raw

    with DeviceBuffers({n: padded(a) for n, a in planes.items()}) as dev:
        ctx.dof_device(dev.ptr("rgb") + offset, dev.ptr("depth") + offset, dev.ptr("out") + offset, w, h, coc_ptr=dev.ptr("coc") + offset if coc else None, **kw)
        ctx.collect_stats()  # waits for the stream
        raw = {n: dev.download(n, a.nbytes + 16, np.uint8) for n, a in planes.items()}
    got = {}
    for n, a in planes.items():
        assert (raw[n][:offset] == 0xA5).all() and (raw[n][offset + a.nbytes:] == 0xA5).all(), n
        got[n] = raw[n][offset:offset + a.nbytes].copy().view(f32).reshape(a.shape)
    assert (bits(got["rgb"]) == bits(rgb)).all() and (bits(got["depth"]) == bits(depth)).all()
    if not coc:
        assert (got["coc"] == 7.0).all()  # not touched
    return got["out"], got["coc"] if coc else None


def same(got, want, what):
    diff = bits(got) != bits(want)
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}-R{c[2]}")
def test_matches_the_cpu_model_bit_for_bit(gpu_ctx, case):
    w, h, R = case
    rgb, depth = inputs(w, h)
    kw = params(R)
    want = model(w, h, **kw)
    if w >= FULL[0] and h >= FULL[1]:
        # a condition on the inputs, from the model alone: they send the kernel down every path
        finite = dm.finite_pixels(rgb)
        assert (want.n[finite] == 1).any() and (want.n > 1).any(), "pixels that keep their bits and pixels that gather"
        assert (want.front > 0).any() and (want.n - want.front > 1).any(), "taps through both occlusion branches"
        assert (want.partial > 0).any() and (want.r == f32(R)).any(), "taps with cov < 1, a pixel with r == max_radius"
    out, coc = on_device(gpu_ctx, rgb, depth, **kw)
    same(out, want.out, "the device form")
    same(coc, want.coc, "the device form's circles")
    out, coc = on_device(gpu_ctx, rgb, depth, offset=4, **kw)  # no plane is 16-byte aligned: float by float
    same(out, want.out, "4 bytes off")
    same(coc, want.coc, "4 bytes off, the circles")
    out, coc = gpu_ctx.dof(rgb, depth, return_coc=True, **kw)
    same(out, want.out, "the host form")
    same(coc, want.coc, "the host form's circles")


@pytest.mark.parametrize("offset", (0, 4))
def test_whole_blocks_copy_and_whole_blocks_run_the_full_loop(gpu_ctx, offset):
    """The largest halo class at its largest radius.  An all-sharp image (the depth constant at the focus) sends every block down the
    copy path; a fully blurred one (every circle 16) takes every block through the whole loop; and the mixed inputs cut the loop per
    block."""
    w, h = 130, 67
    rgb, _ = inputs(w, h)
    sharp = np.full((h, w), FOCUS, f32)
    out, coc = on_device(gpu_ctx, rgb, sharp, offset=offset, max_radius=16, focus=FOCUS, scale=40.0)
    same(out, rgb, "all sharp")
    assert (bits(coc) == 0).all()
    far = np.full((h, w), np.inf, f32)
    want = dm.dof(rgb, far, max_radius=16, focus=FOCUS, scale=40.0, details=True)
    assert (want.r == 16).all() and want.n.max() > 800
    out, coc = on_device(gpu_ctx, rgb, far, offset=offset, max_radius=16, focus=FOCUS, scale=40.0)
    same(out, want.out, "all blurred")
    same(coc, want.coc, "all blurred, the circles")
    mixed = model(w, h, **params(16))
    out, coc = on_device(gpu_ctx, rgb, inputs(w, h)[1], offset=offset, **params(16))
    same(out, mixed.out, "mixed")
    same(coc, mixed.coc, "mixed, the circles")


def test_the_call_forms(gpu_ctx):
    w, h, R = 33, 31, 9
    rgb, depth = inputs(w, h)
    want = model(w, h, **params(R))
    out, coc = on_device(gpu_ctx, rgb, depth, coc=False, **params(R))  # coc_out NULL
    same(out, want.out, "without the circles")
    same(gpu_ctx.dof(rgb, depth, **params(R)), want.out, "the host form without the circles")
    for offset in (0, 4):  # scale 0: a copy, and +0 circles
        out, coc = on_device(gpu_ctx, rgb, depth, offset=offset, max_radius=R, focus=FOCUS, scale=0.0)
        same(out, rgb, "scale 0")
        assert (bits(coc) == 0).all()
    out, coc = gpu_ctx.dof(rgb, depth, return_coc=True, max_radius=R, focus=FOCUS)
    same(out, rgb, "scale 0, the host form")
    assert (bits(coc) == 0).all()
    # focus_pixel: the focus is the depth there
    x, y = 20, 9
    assert np.isfinite(depth[y, x]) and depth[y, x] > 0
    kw = dict(max_radius=R, scale=R / 4.0)
    same(gpu_ctx.dof(rgb, depth, focus_pixel=(x, y), **kw), dm.dof(rgb, depth, focus=float(depth[y, x]), **kw), "focus_pixel")
    with pytest.raises(ValueError):
        gpu_ctx.dof(rgb, depth, focus_pixel=(1, 1), **kw)  # a miss


def test_refusals_leave_the_context_usable(gpu_ctx):
    L = gpu_ctx._L
    w, h = 9, 7
    img = np.ascontiguousarray(inputs(17, 9)[0][:h, :w])
    depth = np.ascontiguousarray(inputs(17, 9)[1][:h, :w])
    out, coc = np.zeros_like(img), np.zeros_like(depth)
    nan, inf = float("nan"), float("inf")

    def call(fn, params=True, rgb=True, z=True, dst=True, in_place=False, **fields):
        p = api.DofParams.make(w, h, max_radius=3, focus=FOCUS, scale=2.0)
        for n, v in fields.items():
            if n.startswith("reserved"):
                p.reserved[int(n[-1])] = v
            else:
                setattr(p, n, v)
        return fn(gpu_ctx._h, C.addressof(p) if params else None, img.ctypes.data if rgb else None, depth.ctypes.data if z else None,
                  (img.ctypes.data if in_place else out.ctypes.data) if dst else None, coc.ctypes.data)

    for fn in (L.pbrsf_dof, L.pbrsf_dof_device):  # (the device variant refuses before it touches a pointer)
        assert call(fn, params=False) == -1 and call(fn, rgb=False) == -1 and call(fn, z=False) == -1 and call(fn, dst=False) == -1
        assert b"null dof" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, in_place=True) == -1
        assert b"must not be its input" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, w=0) == -1 and call(fn, h=0) == -1
        assert call(fn, max_radius=0) == -1 and call(fn, max_radius=17) == -1
        assert call(fn, flags=1) == -1 and call(fn, reserved0=1) == -1 and call(fn, reserved1=1) == -1
        for v in (0.0, -1.0, nan, inf):
            assert call(fn, focus=v) == -1, v
        for v in (-1.0, nan, inf):
            assert call(fn, scale=v) == -1, v
        assert b"scale" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, w=1 << 15, h=(1 << 13) + 1) == -4
        assert b"2^28" in L.pbrs_last_error(gpu_ctx._h)
    assert (out == 0).all() and (coc == 0).all()
    assert call(L.pbrsf_dof) == 0
    want = dm.dof(img, depth, max_radius=3, focus=FOCUS, scale=2.0, details=True)
    same(out, want.out, "a valid call after the refusals")
    same(coc, want.coc, "its circles")
    got, _ = on_device(gpu_ctx, *inputs(33, 31), **params(9))
    same(got, model(33, 31, **params(9)).out, "the device form after the refusals")


def device_array(ptr, shape):
    """A copy of the f32 array at the device address `ptr` (the stream has been waited for)."""
    out = np.empty(shape, f32)
    assert libs.hip_runtime().hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


@pytest.mark.parametrize("size", ((32, 32), (48, 32)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_render_temporal_defocuses_every_frame_on_the_stream(gpu_ctx, size, monkeypatch):
    """Three frames of the Cornell box at 2 x 2 strata.  dof= leaves the four images of a frame alone; the stats' "dof" is Context.dof
    of the frame's first image with the frame's depth (the depth the step was handed, which is also the depth AOV of a render with the
    frame's parameters); bloom reads the defocused image and display reads bloom's; with upscale the depth is the full-size guide
    render's; and a list of keywords, one per frame, pulls the focus."""
    w, h = size
    hs = pbrs_amd.HostScene(scenes.cornell_scene(width=w, height=h))
    gpu_ctx.upload(hs)
    cams, seeds = [hs.camera] * 3, [21, 22, 23]
    handed = []  # (the depth pointer dof_device was handed, w, h, keywords) per call
    plain_dof_device = gpu_ctx.dof_device

    def spy(rgb_ptr, depth_ptr, out_ptr, w_, h_, coc_ptr=None, **kw):
        handed.append((depth_ptr, w_, h_, kw))
        return plain_dof_device(rgb_ptr, depth_ptr, out_ptr, w_, h_, coc_ptr, **kw)

    monkeypatch.setattr(gpu_ctx, "dof_device", spy)
    probe = gpu_ctx.render_aovs(2, 2, 5, seeds[0], aovs=("depth",))[1]["depth"]
    hit = np.isfinite(probe) & (probe > 0)
    assert hit.any()
    lens = dict(max_radius=6, focus=float(np.median(probe[hit])), scale=8.0)
    pull = [dict(lens, focus=lens["focus"] * s) for s in (0.75, 1.0, 1.5)]
    bkw = dict(threshold=0.25, knee=0.5, strength=0.5, levels=3)

    def run(**options):
        """The frames of a sequence, each with the depth and the keywords its dof step was handed."""
        del handed[:]
        frames = []
        for k, f in enumerate(gpu_ctx.render_temporal(cams, 2, 2, 5, seeds, **options)):
            depth = kw = None
            if options.get("dof") is not None:  # the sequence's buffers live until the generator ends
                assert len(handed) == k + 1 and handed[k][1:3] == (w, h)
                depth, kw = device_array(handed[k][0], (h, w)), handed[k][3]
            frames.append((f, depth, kw))
        return frames

    plain = run(display=True)
    none = run(display=True, dof=None)
    focused = run(display=True, dof=lens)
    lit = run(display=True, bloom=bkw, dof=pull)
    up = run(upscale=2, dof=lens)
    up_plain = run(upscale=2)
    assert len(plain) == len(none) == len(focused) == len(lit) == len(up) == len(up_plain) == 3
    e = e_lit = None
    for k in range(3):
        p, q, f, g = plain[k][0], none[k][0], focused[k][0], lit[k][0]
        assert len(p) == len(q) == len(f) == len(g) == 4 and p[3].keys() == q[3].keys() and "dof" not in q[3]
        assert (q[3]["display"] == p[3]["display"]).all()
        for i in range(3):  # the first image stays the filter's: the blur goes into a buffer of its own
            same(q[i], p[i], (k, i)), same(f[i], p[i], (k, i)), same(g[i], p[i], (k, i))
        assert set(f[3]) - {"dof"} == set(p[3]) and set(g[3]) - {"dof", "bloom"} == set(p[3])
        # the depth the step was handed is the frame's depth guide
        depth = focused[k][1]
        same(depth, gpu_ctx.render_aovs(2, 2, 5, seeds[k], aovs=("depth",))[1]["depth"], ("the frame's depth", k))
        assert f[3]["dof"].shape == (h, w, 3) and f[3]["dof"].dtype == f32
        want = gpu_ctx.dof(f[0], depth, **lens)
        same(f[3]["dof"], want, k)
        same(want, dm.dof(f[0], depth, **lens), ("the model", k))
        assert (bits(want) != bits(f[0])).any()
        shown, e = gpu_ctx.display(want, exposure_in=e, auto=True, return_exposure=True)
        assert (f[3]["display"] == shown).all(), k  # without bloom the display reads the defocused image
        # the focus pull, then bloom of the defocused image, then the display of that
        assert lit[k][2] == pull[k] and focused[k][2] == lens and (bits(lit[k][1]) == bits(depth)).all()
        want = gpu_ctx.dof(g[0], depth, **pull[k])
        same(g[3]["dof"], want, ("pull", k))
        glare = bm.bloom(want, **bkw)
        same(g[3]["bloom"], glare, ("bloom", k))
        shown, e_lit = gpu_ctx.display(glare, exposure_in=e_lit, auto=True, return_exposure=True)
        assert (g[3]["display"] == shown).all(), k
        # upscale: the chain runs at half size, the step at full size on the full-size guide render's depth
        u, depth_hi, _ = up[k]
        for i in range(3):
            same(u[i], up_plain[k][0][i], ("upscale", k, i))
        assert u[0].shape == (h, w, 3) and u[1].shape == (h // 2, w // 2, 3) and depth_hi.shape == (h, w)
        same(depth_hi, gpu_ctx.render_aovs(1, 1, 1, seeds[k], aovs=("depth",))[1]["depth"], ("the full-size depth", k))
        same(u[3]["dof"], gpu_ctx.dof(u[0], depth_hi, **lens), ("upscale", k))
    assert (bits(lit[0][0][3]["dof"]) != bits(focused[0][0][3]["dof"])).any()  # another focus, another image
    with pytest.raises(TypeError):
        next(gpu_ctx.render_temporal(cams, 2, 2, 5, seeds, dof={"sigma": 1.0}))
    with pytest.raises(ValueError, match="none for frame 2"):
        list(gpu_ctx.render_temporal(cams, 2, 2, 5, seeds, dof=pull[:2]))

