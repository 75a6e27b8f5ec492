"""pbrsm_motion_blur and pbrsm_motion_blur_device on the device against tests/motion_blur_model.py, the numpy model of the header's
text: bit for bit, image and velocities, over sizes and radii that send the kernel down each of its paths, over motion fields that
reach every branch of the arithmetic, the call forms, the refusals, and the chain of Context.render_animation."""
import ctypes as C

import numpy as np
import pytest

import bloom_model as bm
import dof_model as dm
import motion_blur_model as mb
import motion_model as mm
import pbrs_amd
from common import bits
from pbrs_amd import DeviceBuffers, api, libs

pytestmark = pytest.mark.gpu

f32 = np.float32
FOCUS = 2.0
# (w, h, max_radius, taps).  The sizes: one pixel; one row and one column; a window larger than the image on every side; a second tile,
# a pixel wide (16 x 16 tiles); the halo cut at every edge; a whole number of tiles; tiles with a full halo inside the image.  The radii:
# 1, the two sides of the kernel's halo classes (4 | 5 and 8 | 9) and 16, each paired with one size, not the product; and so are the taps
# 2, 7 and 64 beside the default's 16.
CASES = ((1, 1, 1, 2), (1, 40, 4, 16), (40, 1, 5, 7), (5, 5, 16, 16), (17, 9, 5, 16), (33, 31, 9, 64), (48, 40, 8, 16), (64, 33, 4, 16),
         (130, 67, 1, 16), (130, 67, 16, 16))
# from this size on the fields together must send the kernel down every path (below)
FULL = (17, 9)
BLOCKS = ((2, 8), (0, 16), (8, 24), (16, 28), (12, 10))  # (y0, x0) of the 8 x 8 blocks of `ramp`, the first five


def hdr(w, h, seed=17):
    """tests/test_gpu_dof.py's recipe.  Seeded HDR noise, log-uniform over twelve octaves, with NaN, inf, negative and zero pixels where
    the tile logic can lose them: the corners and both sides of a tile's border (15 | 16).  A site outside the image is skipped."""
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
    """tests/test_gpu_dof.py's recipe.  A depth that grows along x through FOCUS (0.4 to 2.0 times it; a little along y too, so that no
    two rows are alike), with 8 x 8 blocks pulled near (a tenth of FOCUS) and exactly to FOCUS (behind the ramp's left part) whose edges
    fall on both sides of the tile border 15 | 16, in x and in y, one of them across the corner of four tiles, +inf misses, and a few
    pixels of 0, -1 and NaN."""
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


def fields(w, h, R):
    """{name: (h, w, 2) f32 motion vectors}, for shutter 1 (v = motion / 2).  zero: the copy path.  constant, clamped: every pixel at
    len = R along (0.6, -0.8), and at 3 R, which the clamp brings back.  rotation: about the centre, every octant, lengths from 0 through
    0.5 to beyond R.  blocks: the 8 x 8 blocks of `ramp` (near and far ones, edges on both sides of the tile borders, one across four
    tiles' corners) move over a static surround, each its own way; surround: the same blocks stand still in a moving surround.  ties:
    two vectors of equal length and different direction either side of the tile border 15 | 16, within R of both tiles (a third, equal
    one below them, which must lose to both).  nonfinite: the constant field with NaN and inf vectors in it."""
    out = {"zero": np.zeros((h, w, 2), f32)}
    along = np.array((0.6, -0.8))
    out["constant"] = np.broadcast_to((2.0 * R * along).astype(f32), (h, w, 2)).copy()
    out["clamped"] = np.broadcast_to((6.0 * R * along).astype(f32), (h, w, 2)).copy()
    x, y = np.meshgrid(np.arange(w) - (w - 1) / 2.0, np.arange(h) - (h - 1) / 2.0)
    omega = 2.6 * R / max(np.hypot(w - 1, h - 1) / 2.0, 1.0)  # |v| = 1.3 R at the corners
    out["rotation"] = np.stack([-omega * y, omega * x], axis=2).astype(f32)
    blocks, surround = np.zeros((h, w, 2), f32), np.broadcast_to(np.array((-1.6 * R, 1.1 * R), f32), (h, w, 2)).copy()
    ways = ((2.0, 0.0), (0.0, -2.0), (-1.5, 1.5), (1.2, 1.7), (-2.0, -0.4))
    for (y0, x0), way in zip(BLOCKS, ways):
        blocks[y0:y0 + 8, x0:x0 + 8] = np.array(way, f32) * f32(R)
        surround[y0:y0 + 8, x0:x0 + 8] = 0.0
    out["blocks"], out["surround"] = blocks, surround
    ties = np.zeros((h, w, 2), f32)
    for (yy, xx), vec in (((5, 14), (1.8 * R, 0.0)), ((5, 17), (0.0, 1.8 * R)), ((6, 15), (-1.8 * R, 0.0))):
        if yy < h and xx < w:
            ties[yy, xx] = vec
    out["ties"] = ties
    bad = out["constant"].copy()
    for (yy, xx), vec in (((0, 0), (np.nan, 1.0)), ((3, 15), (np.inf, 0.0)), ((3, 16), (1.0, -np.inf)), ((h // 2, w // 3), (np.nan, np.nan)),
                          ((h - 1, w - 1), (-np.inf, np.inf))):
        if yy < h and xx < w:
            bad[yy, xx] = vec
    out["nonfinite"] = bad
    return out


_inputs, _models = {}, {}


def inputs(w, h, R):
    if (w, h, R) not in _inputs:
        _inputs[w, h, R] = (hdr(w, h), ramp(w, h), fields(w, h, R))
        for a in _inputs[w, h, R][:2] + tuple(_inputs[w, h, R][2].values()):
            a.flags.writeable = False
    return _inputs[w, h, R]


def model(w, h, R, field, **kw):
    key = (w, h, R, field, tuple(sorted(kw.items())))
    if key not in _models:
        rgb, depth, motion = inputs(w, h, R)
        _models[key] = mb.motion_blur(rgb, depth, motion[field], max_radius=R, details=True, **kw)
    return _models[key]


def on_device(ctx, rgb, depth, motion, offset=0, velocity=True, **kw):
    """motion_blur_device on buffers of the test's own, every plane `offset` bytes into its allocation -> (image, velocities or None); the
    inputs are read only and nothing outside a plane is written."""
    h, w, _ = rgb.shape
    planes = {"rgb": rgb, "depth": depth, "motion": motion, "out": np.full_like(rgb, 7.0), "vel": np.full_like(motion, 7.0)}

    def padded(a):
        raw = np.full(a.nbytes + 16, 0xA5, np.uint8)
        raw[offset:offset + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return raw

    with DeviceBuffers({n: padded(a) for n, a in planes.items()}) as dev:
        ctx.motion_blur_device(dev.ptr("rgb") + offset, dev.ptr("depth") + offset, dev.ptr("motion") + offset, dev.ptr("out") + offset, w, h,
                               velocity_ptr=dev.ptr("vel") + offset if velocity else None, **kw)
        ctx.collect_stats()  # waits for the stream
        raw = {n: dev.download(n, a.nbytes + 16, np.uint8) for n, a in planes.items()}
    got = {}
    for n, a in planes.items():
        assert (raw[n][:offset] == 0xA5).all() and (raw[n][offset + a.nbytes:] == 0xA5).all(), n
        got[n] = raw[n][offset:offset + a.nbytes].copy().view(f32).reshape(a.shape)
    for n in ("rgb", "depth", "motion"):
        assert (bits(got[n]) == bits(planes[n])).all(), n
    if not velocity:
        assert (got["vel"] == 7.0).all()  # not touched
    return got["out"], got["vel"] if velocity else None


def same(got, want, what):
    diff = bits(got) != bits(want)
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}-R{c[2]}-S{c[3]}")
def test_matches_the_cpu_model_bit_for_bit(gpu_ctx, case):
    w, h, R, taps = case
    rgb, depth, motion = inputs(w, h, R)
    seen = {n: False for n in ("gathers", "keeps", "front", "behind", "between", "partial", "clamped", "copies", "moves")}
    for name, field in motion.items():
        for jitter in (False, True):
            kw = dict(taps=taps, shutter=1.0, jitter=jitter)
            want = model(w, h, R, name, **kw)
            finite = mb.finite_pixels(rgb)
            seen["gathers"] |= bool((want.n > 0).any())
            seen["keeps"] |= bool(((want.n == 0) & finite & (want.vn_len > f32(0.5))).any())
            for n in ("front", "behind", "between", "partial"):
                seen[n] |= bool((getattr(want, n) > 0).any())
            seen["clamped"] |= bool((want.len > f32(R - 0.001)).any())
            seen["copies"] |= bool((want.vn_len <= f32(0.5)).any())
            seen["moves"] |= bool((want.vn_len > f32(0.5)).any())
            what = (name, "jitter" if jitter else "plain")
            out, vel = on_device(gpu_ctx, rgb, depth, field, max_radius=R, **kw)
            same(out, want.out, what + ("the device form",))
            same(vel, want.velocity, what + ("the device form's velocities",))
            out, vel = on_device(gpu_ctx, rgb, depth, field, offset=4, max_radius=R, **kw)  # no plane is 16-byte aligned: float by float
            same(out, want.out, what + ("4 bytes off",))
            same(vel, want.velocity, what + ("4 bytes off, the velocities",))
            if not jitter:
                out, vel = gpu_ctx.motion_blur(rgb, depth, field, return_velocity=True, max_radius=R, **kw)
                same(out, want.out, what + ("the host form",))
                same(vel, want.velocity, what + ("the host form's velocities",))
    if w >= FULL[0] and h >= FULL[1]:
        # a condition on the inputs, from the model alone: together the fields send the kernel down every path
        assert all(seen.values()), seen


def test_the_dominant_velocity_is_the_lowest_index_among_equals(gpu_ctx):
    """The ties field, from the model alone: both tiles of the first tile row take the vector at (5, 14), the lowest index of the three
    equal ones in both windows; and with the first two swapped the device follows."""
    w, h, R = 48, 40, 8
    rgb, depth, motion = inputs(w, h, R)
    want = model(w, h, R, "ties", taps=16, shutter=1.0)
    half = f32(1.8 * R) * f32(0.5)  # the field's vector through shutter 1
    assert want.winner[0, 0] == want.winner[0, 1] == 5 * w + 14 and (want.vn[0, 0] == (half, 0.0)).all() and (want.vn[0, 31] == want.vn[0, 0]).all()
    swapped = motion["ties"].copy()
    swapped[5, 14], swapped[5, 17] = motion["ties"][5, 17], motion["ties"][5, 14]
    other = mb.motion_blur(rgb, depth, swapped, max_radius=R, taps=16, shutter=1.0, details=True)
    assert other.winner[0, 0] == other.winner[0, 1] == 5 * w + 14 and (other.vn[0, 31] == (0.0, half)).all()
    assert (bits(other.out) != bits(want.out)).any()
    for offset in (0, 4):
        out, vel = on_device(gpu_ctx, rgb, depth, swapped, offset=offset, max_radius=R, taps=16, shutter=1.0)
        same(out, other.out, ("swapped", offset))
        same(vel, other.velocity, ("swapped, the velocities", offset))


def test_the_call_forms(gpu_ctx):
    w, h, R = 33, 31, 9
    rgb, depth, motion = inputs(w, h, R)
    kw = dict(taps=64, shutter=1.0)
    want = model(w, h, R, "blocks", **kw)
    out, vel = on_device(gpu_ctx, rgb, depth, motion["blocks"], velocity=False, max_radius=R, **kw)  # velocity_out NULL
    same(out, want.out, "without the velocities")
    same(gpu_ctx.motion_blur(rgb, depth, motion["blocks"], max_radius=R, **kw), want.out, "the host form without the velocities")
    for offset in (0, 4):  # shutter 0: a copy, and +0 velocities
        out, vel = on_device(gpu_ctx, rgb, depth, motion["constant"], offset=offset, max_radius=R, shutter=0.0)
        same(out, rgb, "shutter 0")
        assert (bits(vel) == 0).all()
    out, vel = gpu_ctx.motion_blur(rgb, depth, motion["constant"], return_velocity=True, max_radius=R, shutter=0.0)
    same(out, rgb, "shutter 0, the host form")
    assert (bits(vel) == 0).all()
    # the other parameters reach the kernel: half the shutter, another z_rel
    for more in (dict(shutter=0.5), dict(shutter=1.0, z_rel=0.5), dict(shutter=0.37, z_rel=1e-3, jitter=True)):
        want = mb.motion_blur(rgb, depth, motion["surround"], max_radius=R, taps=16, details=True, **more)
        out, vel = on_device(gpu_ctx, rgb, depth, motion["surround"], max_radius=R, taps=16, **more)
        same(out, want.out, more)
        same(vel, want.velocity, more)


def test_refusals_leave_the_context_usable(gpu_ctx):
    L = gpu_ctx._L
    w, h = 9, 7
    rgb17, depth17, motion17 = inputs(17, 9, 5)
    img, depth = np.ascontiguousarray(rgb17[:h, :w]), np.ascontiguousarray(depth17[:h, :w])
    motion = np.ascontiguousarray(motion17["rotation"][:h, :w])
    out, vel = np.zeros_like(img), np.zeros_like(motion)
    nan, inf = float("nan"), float("inf")

    def call(fn, params=True, rgb=True, z=True, mv=True, dst=True, in_place=False, **fields):
        p = api.MotionBlurParams.make(w, h, max_radius=3, taps=5, shutter=1.0)
        for n, v in fields.items():
            setattr(p, n, v)
        return fn(gpu_ctx._h, C.addressof(p) if params else None, img.ctypes.data if rgb else None, depth.ctypes.data if z else None,
                  motion.ctypes.data if mv else None, (img.ctypes.data if in_place else out.ctypes.data) if dst else None, vel.ctypes.data)

    for fn in (L.pbrsm_motion_blur, L.pbrsm_motion_blur_device):  # (the device variant refuses before it touches a pointer)
        assert call(fn, params=False) == -1 and call(fn, rgb=False) == -1 and call(fn, z=False) == -1 and call(fn, mv=False) == -1 and call(fn, dst=False) == -1
        assert b"null motion blur" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, in_place=True) == -1
        assert b"must not be its input" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, w=0) == -1 and call(fn, h=0) == -1
        assert call(fn, max_radius=0) == -1 and call(fn, max_radius=17) == -1
        assert call(fn, taps=1) == -1 and call(fn, taps=65) == -1
        assert b"taps" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, flags=2) == -1 and call(fn, flags=3) == -1 and call(fn, reserved=1) == -1
        for v in (-1.0, 1.5, nan, inf):
            assert call(fn, shutter=v) == -1, v
        for v in (0.0, -1.0, nan, inf):
            assert call(fn, z_rel=v) == -1, v
        assert b"z_rel" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, w=1 << 15, h=(1 << 13) + 1) == -4
        assert b"2^28" in L.pbrs_last_error(gpu_ctx._h)
    assert (out == 0).all() and (vel == 0).all()
    assert call(L.pbrsm_motion_blur) == 0
    want = mb.motion_blur(img, depth, motion, max_radius=3, taps=5, shutter=1.0, details=True)
    same(out, want.out, "a valid call after the refusals")
    same(vel, want.velocity, "its velocities")
    got, _ = on_device(gpu_ctx, *inputs(33, 31, 9)[:2], inputs(33, 31, 9)[2]["rotation"], max_radius=9, taps=64, shutter=1.0)
    same(got, model(33, 31, 9, "rotation", taps=64, shutter=1.0).out, "the device form after the refusals")


def device_array(ptr, shape, dtype=f32):
    """A copy of the array at the device address `ptr` (the stream has been waited for)."""
    out = np.empty(shape, dtype)
    assert libs.hip_runtime().hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


def test_render_animation_blurs_every_frame_on_the_stream(gpu_ctx, monkeypatch):
    """Eight frames of the 128 x 128 Cornell box whose short box turns (tests/test_gpu_motion.py's sequence, the smallest on which the
    box moves by more than a pixel per frame, so that its tiles gather), at 2 x 2 strata.  motion_blur= leaves the images of a frame
    and every step in front of it alone; from the second frame on the stats' "motion_blur" is the model applied to what the step was
    handed, downloaded: the image (the first image, or the defocused one), the depth and the vectors, which are motion_vectors() of that
    depth and the frame's instance ids against the previous frame; the first frame's is a copy; bloom reads the blurred image and
    display reads bloom's.  Alone with the chain's own vectors, alone with vectors of its own, and together with dof, bloom, display
    and upscale=2."""
    n, size = 8, 128
    scenes_ = [pbrs_amd.HostScene(mm.turned_short_box(k, size=size)) for k in range(n)]
    handed, vectors = [], []  # per frame: what motion_blur_device and, before it, motion_vectors_device were handed
    plain_blur, plain_vectors = gpu_ctx.motion_blur_device, gpu_ctx.motion_vectors_device

    def spy_blur(rgb_ptr, depth_ptr, motion_ptr, out_ptr, w_, h_, velocity_ptr=None, **kw):
        handed.append((rgb_ptr, depth_ptr, motion_ptr, w_, h_, kw))
        return plain_blur(rgb_ptr, depth_ptr, motion_ptr, out_ptr, w_, h_, velocity_ptr, **kw)

    def spy_vectors(depth_ptr, out_ptr, w_, h_, cam, cam_prev, instance_ptr=None, motion=None, prev_depth_ptr=None):
        vectors.append((depth_ptr, out_ptr, w_, h_, instance_ptr))
        return plain_vectors(depth_ptr, out_ptr, w_, h_, cam, cam_prev, instance_ptr, motion, prev_depth_ptr)

    monkeypatch.setattr(gpu_ctx, "motion_blur_device", spy_blur)
    monkeypatch.setattr(gpu_ctx, "motion_vectors_device", spy_vectors)
    mkw = dict(max_radius=8, taps=12, shutter=1.0)
    probe = next(gpu_ctx.render_animation([(scenes_[0], None, 9)], 2, 2, 5, iterations=3))
    lens = dict(max_radius=4, focus=1.0, scale=3.0)
    bkw = dict(threshold=0.25, knee=0.5, strength=0.5, levels=3)
    assert probe[0].shape == (size, size, 3)

    def run(frames=n, **options):
        """The frames of a sequence, each with what its motion blur step was handed, downloaded while the sequence's buffers live."""
        del handed[:], vectors[:]
        got = []
        for k, f in enumerate(gpu_ctx.render_animation([(hs, None, 9 + k) for k, hs in enumerate(scenes_[:frames])], 2, 2, 5,
                                                       temporal=dict(id_test=True, min_temporal=2.0), iterations=3, **options)):
            step = None
            if options.get("motion_blur") is not None:
                assert len(handed) == k + 1 and handed[k][3:5] == (size, size)
                rgb_ptr, depth_ptr, motion_ptr, w_, h_, kw = handed[k]
                step = dict(rgb=device_array(rgb_ptr, (h_, w_, 3)), depth=device_array(depth_ptr, (h_, w_)), kw=kw,
                            motion=device_array(motion_ptr, (h_, w_, 2)) if k else None)
                mine = [v for v in vectors if v[1] == motion_ptr]
                if k:  # the call that made the vectors: from the depth the step reads, and these instance ids
                    assert mine and mine[-1][0] == depth_ptr and mine[-1][2:4] == (w_, h_) and mine[-1][4]
                    step["instance"] = device_array(mine[-1][4], (h_, w_), np.uint32)
                del vectors[:]
            got.append((f, step))
        return got

    def check_step(k, hs, step, stats, mkw_k):
        """Frame k's step against the model, and its vectors against the host form of motion_vectors."""
        assert stats["motion_blur"].shape == (size, size, 3) and stats["motion_blur"].dtype == f32
        if k == 0:
            assert step["kw"] == dict(mkw_k, shutter=0.0)
            same(stats["motion_blur"], step["rgb"], "the first frame's is a copy")
            return
        assert step["kw"] == mkw_k
        gpu_ctx.upload(hs)
        table = api.instance_motion(hs, scenes_[k - 1])
        same(step["motion"], gpu_ctx.motion_vectors(step["depth"], hs.camera, hs.camera, instance=step["instance"], motion=table), ("the vectors", k))
        want = mb.motion_blur(step["rgb"], step["depth"], step["motion"], details=True, **mkw_k)
        assert (want.vn_len > f32(0.5)).any() and (want.n > 0).any(), k  # the turning box's tiles gather
        same(stats["motion_blur"], want.out, ("the model", k))
        assert (bits(want.out) != bits(step["rgb"])).any(), k

    # alone, on the chain's own vectors (motion_vectors=True, no upscale: the "motion" buffer)
    plain = run(motion_vectors=True)
    alone = run(motion_vectors=True, motion_blur=mkw)
    assert len(plain) == len(alone) == n
    for k in range(n):
        (p, _), (a, step) = plain[k], alone[k]
        assert len(p) == len(a) == 5 and set(a[3]) - {"motion_blur"} == set(p[3]) and "motion_blur" not in p[3]
        for i in (0, 1, 2, 4):
            same(a[i], p[i], (k, i))
        same(step["rgb"], a[0], ("the step reads the first image", k))
        if k:
            same(step["motion"], a[4], ("the step reads the chain's vectors", k))
        check_step(k, scenes_[k], step, a[3], mkw)
    # alone, on vectors of its own (no motion_vectors=), per-frame keywords; three frames are enough for the buffer's life
    ramp_kw = [dict(mkw, shutter=s) for s in (1.0, 0.75, 1.0)]
    own = run(frames=3, motion_blur=ramp_kw)
    for k in range(3):
        f, step = own[k]
        assert len(f) == 4
        for i in range(3):
            same(f[i], plain[k][0][i], ("own vectors", k, i))
        check_step(k, scenes_[k], step, f[3], ramp_kw[k])
    # together: upscale, dof, bloom, display
    every = dict(upscale=2, dof=lens, bloom=bkw, display=True)
    base = run(**every)
    full = run(motion_blur=mkw, **every)
    e = None
    for k in range(n):
        (p, _), (a, step) = base[k], full[k]
        assert len(p) == len(a) == 4 and set(a[3]) - {"motion_blur"} == set(p[3])
        for i in range(3):
            same(a[i], p[i], ("together", k, i))
        same(a[3]["dof"], p[3]["dof"], ("the defocused image", k))
        same(step["rgb"], a[3]["dof"], ("the step reads the defocused image", k))
        assert a[0].shape == (size, size, 3) and a[1].shape == (size // 2, size // 2, 3) and a[3]["low_res"] == (size // 2, size // 2)
        same(a[3]["dof"], dm.dof(a[0], step["depth"], **lens), ("the full-size depth is the one dof read", k))
        check_step(k, scenes_[k], step, a[3], mkw)
        glare = bm.bloom(a[3]["motion_blur"], **bkw)
        same(a[3]["bloom"], glare, ("bloom reads the blurred image", k))
        shown, e = gpu_ctx.display(glare, exposure_in=e, auto=True, return_exposure=True)
        assert (a[3]["display"] == shown).all(), k
    assert (bits(full[n - 1][0][3]["bloom"]) != bits(base[n - 1][0][3]["bloom"])).any()
    with pytest.raises(TypeError):
        next(gpu_ctx.render_animation([(scenes_[0], None, 9)], 2, 2, 5, motion_blur={"sigma": 1.0}))
    with pytest.raises(ValueError, match="none for frame 2"):
        list(gpu_ctx.render_animation([(hs, None, 9 + k) for k, hs in enumerate(scenes_[:3])], 2, 2, 5, motion_blur=ramp_kw[:2]))
