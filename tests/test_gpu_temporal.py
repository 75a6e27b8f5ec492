"""Temporal accumulation on the GPU (include/pbrs_gpu.h, pbrs_temporal_accumulate[_device]; device/temporal.h): bit for bit against the
CPU model of tests/temporal_model.py on synthetic sequences and on rendered ones, every guide present or absent, the device variant and
the device chain of Context.render_temporal, the error the accumulation removes, and what the header refuses."""
import contextlib
import ctypes as C
import itertools

import numpy as np
import pytest

import pbrs_amd
import temporal_model as tm
from common import bits
from pbrs_amd import DeviceBuffers, api, scenes
from test_gpu_denoise import same

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = ((1, 1), (2, 3), (7, 5), (64, 1), (1, 64), (37, 29), (130, 70))  # (w, h)
PLANES = ("rgb", "moments", "length")


def api_camera(cam):
    c = api.Camera()
    for n in ("center", "c", "a", "b"):
        getattr(c, n)[:] = [float(v) for v in getattr(cam, n)]
    c.width, c.height = cam.width, cam.height
    return c


def model_camera(c):
    return tm.Cam(list(c.center), list(c.c), list(c.a), list(c.b), c.width, c.height)


def gpu_step(ctx):
    """Context.temporal_accumulate with the signature of the model's accumulate (tm.run_sequence)."""
    def step(rgb, depth, cam, history=None, prev=None, cam_prev=None, want_variance=True, **kw):
        return ctx.temporal_accumulate(rgb, depth, api_camera(cam), history=history, prev=prev, camera_prev=api_camera(cam_prev) if cam_prev else None,
                                       return_variance=want_variance, **kw)
    return step


def agree(got, want, what):
    """One frame's (history, variance_out) of the GPU and of the model."""
    for n in PLANES:
        bad = ~same(got[0][n], want[0][n])
        assert not bad.any(), (what, n, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert (got[1] is None) == (want[1] is None), what
    if want[1] is not None:
        bad = ~same(got[1], want[1])
        assert not bad.any(), (what, "variance_out", int(bad.sum()), np.argwhere(bad)[:4].tolist())


def sequence_bits(results):
    return b"".join(bits(h[n]).tobytes() for h, _ in results for n in PLANES)


@pytest.mark.parametrize("move", tm.MOVES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matches_the_cpu_model_bit_for_bit_on_synthetic_sequences(gpu_ctx, size, move):
    """Three frames, each side fed its own history (what the sequence plants into it included), equal at every frame; all guides, with
    and without the id test."""
    w, h = size
    for id_test in (False, True):
        got = tm.run_sequence(gpu_step(gpu_ctx), w, h, w + h, move, id_test=id_test)
        want = tm.run_sequence(tm.accumulate, w, h, w + h, move, id_test=id_test)
        for k, (g, m) in enumerate(zip(got, want)):
            agree(g, m, (size, move, id_test, k))
    if w * h >= 64:  # the non-finite pixels of a frame stay visible, and nothing else is non-finite
        for (_, frame, _), (hist, _) in zip(tm.synthetic_sequence(w, h, w + h, move), got):
            assert (np.isfinite(hist["rgb"]).all(axis=2) == np.isfinite(frame["rgb"]).all(axis=2)).all() and not np.isfinite(frame["rgb"]).all()
    if size == (130, 70) and move != "away":
        assert (got[-1][0]["length"] > 2.0).any()


def test_every_guide_present_or_absent(gpu_ctx):
    """variance, normal, instance (with and without the id test) and variance_out, each given or not: bit for bit, and a test that is
    switched on changes the result."""
    seen = {}
    tight = dict(normal_tolerance=0.03)  # the walls' normals differ by about 0.04 per pixel at this size: the farther taps are refused
    for variance, normal, instance, vout in itertools.product((False, True), repeat=4):
        for id_test in ((False, True) if instance else (False,)):
            use = tuple(n for n, on in (("variance", variance), ("normal", normal), ("instance", instance)) if on)
            kw = dict(use=use, want_variance=vout, id_test=id_test, **tight)
            got = tm.run_sequence(gpu_step(gpu_ctx), 37, 29, 11, "yaw", **kw)
            want = tm.run_sequence(tm.accumulate, 37, 29, 11, "yaw", **kw)
            for k, (g, m) in enumerate(zip(got, want)):
                agree(g, m, (use, vout, id_test, k))
            seen[(variance, normal, instance, id_test, vout)] = (sequence_bits(got), None if not vout else bits(got[-1][1]).tobytes())
    assert len(seen) == 24
    base = seen[(False, False, False, False, True)]
    assert seen[(False, False, False, False, False)][0] == base[0]           # variance_out NULL: the same history
    assert seen[(True, False, False, False, True)][0] == base[0] and seen[(True, False, False, False, True)][1] != base[1]
    assert seen[(False, True, False, False, True)][0] != base[0]             # the normal test rejects taps
    assert seen[(False, False, True, False, True)] == base                   # ids without the flag: not read
    assert seen[(False, False, True, True, True)][0] != base[0]              # the id test rejects taps


def _yawed(camera, deg):
    return api_camera(tm.rotated(model_camera(camera), deg))


# Degrees of yaw per frame.  Checked in the model with the oracle's first hits at the pixel centres in the place of the AOVs: the zoo at 2
# degrees refuses 29 reprojected pixels (the normal test at the spheres' rims) and keeps a history in 95 % of its hit pixels; the Cornell
# box at 2 degrees refuses none (a yaw has no parallax and its walls are flat), at 4 degrees 22 (the id test at the film's edge), 94 %.
YAW = {"cornell": 4.0, "zoo": 2.0}


@pytest.mark.parametrize("name", ("cornell", "zoo"))
def test_matches_the_cpu_model_bit_for_bit_on_rendered_sequences(gpu_ctx, name):
    """Three frames of 2 x 2 strata, the camera yawing YAW degrees per frame, render_aovs' buffers in, the model's expectation out.  Not
    vacuous: after the third frame at least half of the hit pixels carry a history, and at least one pixel that reprojects into the
    previous frame is refused by its guides there (a disocclusion)."""
    from test_gpu_pixel_filter import scene
    _, hs = scene(name)
    gpu_ctx.upload(hs)
    history = mhistory = prev = cam_prev = None
    disoccluded = 0
    for k in range(3):
        cam = _yawed(hs.camera, YAW[name] * k)
        img, aov, _ = gpu_ctx.render_aovs(2, 2, 5, 7 + k, aovs=("normal", "depth", "instance", "variance"), camera=cam)
        frame = dict(variance=aov["variance"], normal=aov["normal"], instance=aov["instance"])
        got = gpu_ctx.temporal_accumulate(img, aov["depth"], cam, history=history, prev=prev, camera_prev=cam_prev, id_test=True, **frame)
        det = {}
        want = tm.accumulate(img, aov["depth"], model_camera(cam), history=mhistory, prev=prev, cam_prev=model_camera(cam_prev) if cam_prev else None,
                             id_test=True, details=det, **frame)
        agree(got, want, (name, k))
        disoccluded += int(det["disoccluded"].sum())
        history, mhistory, cam_prev = got[0], want[0], cam
        prev = {n: aov[n] for n in ("depth", "normal", "instance")}
    hit = np.isfinite(aov["depth"])
    share = float((got[0]["length"][hit] > 1.0).mean())
    print(f"{name}: {share:.3f} of the hit pixels carry a history after frame 3; {disoccluded} disoccluded pixel(s)")
    assert share >= 0.5 and disoccluded >= 1


def test_the_device_variant_on_caller_buffers_equals_the_host_sequence(gpu_ctx):
    w, h = 37, 29
    host = tm.run_sequence(gpu_step(gpu_ctx), w, h, 5, "yaw", id_test=True)
    like = {"rgb": np.zeros((h, w, 3), f32), "moments": np.zeros((h, w, 2), f32), "length": np.zeros((h, w), f32)}
    cam_prev = prev_dev = None
    with contextlib.ExitStack() as held:
        hist = [held.enter_context(DeviceBuffers(like)) for _ in (0, 1)]
        vout = held.enter_context(DeviceBuffers({"v": like["length"]}))
        for k, (cam, frame, plant) in enumerate(tm.synthetic_sequence(w, h, 5, "yaw")):
            dev = held.enter_context(DeviceBuffers(frame))
            cur, old = hist[k & 1], hist[(k & 1) ^ 1]
            gpu_ctx.temporal_accumulate_device(dev.ptrs(), cur.ptrs(), w, h, api_camera(cam), old.ptrs() if k else None, prev_dev, cam_prev, vout.ptr("v"),
                                               id_test=True)
            gpu_ctx.collect_stats()
            got = {n: cur.download_like(n, like[n]) for n in PLANES}
            agree((got, vout.download_like("v", like["length"])), host[k], k)
            for n, a in tm.plant_history(got, plant).items():  # what the host sequence fed back
                cur.upload(n, a)
            prev_dev, cam_prev = dev.ptrs(tm.GUIDE_NAMES), api_camera(cam)


def test_render_temporal_is_the_hand_made_chain(gpu_ctx):
    from test_gpu_pixel_filter import scene
    _, hs = scene("cornell")
    gpu_ctx.upload(hs)
    cams = [_yawed(hs.camera, 2.0 * k) for k in range(3)]
    guides = ("albedo", "normal", "depth", "instance")
    history = prev = cam_prev = None
    frames = gpu_ctx.render_temporal(cams, 2, 2, 5, [9, 10, 11], temporal=dict(id_test=True, min_temporal=2.0), iterations=3)
    for k, (cam, (den, acc, noisy, st)) in enumerate(zip(cams, frames)):
        img, aov, _ = gpu_ctx.render_aovs(2, 2, 5, 9 + k, aovs=guides + ("variance",), camera=cam)
        var = aov.pop("variance")
        assert (bits(noisy) == bits(img)).all(), k
        history, v = gpu_ctx.temporal_accumulate(img, aov["depth"], cam, variance=var, normal=aov["normal"], instance=aov["instance"], history=history,
                                                 prev=prev, camera_prev=cam_prev, id_test=True, min_temporal=2.0)
        assert same(acc, history["rgb"]).all(), k
        assert same(den, gpu_ctx.denoise_var(history["rgb"], v, iterations=3, **aov)).all(), k
        assert st["samples"] == img.shape[0] * img.shape[1] * 4
        prev, cam_prev = {n: aov[n] for n in tm.GUIDE_NAMES}, cam
    assert k == 2 and (history["length"] > 1.0).mean() > 0.5


def _mse(img, ref, ok):
    return float(((img[ok].astype(np.float64) - ref[ok]) ** 2).mean())


@pytest.mark.parametrize("yaw", (0.0, 1.0), ids=("static", "yaw1"))
def test_accumulation_removes_error_on_the_cornell_box(gpu_ctx, yaw):
    """128 x 128, 2 x 2 strata, 8 frames with seeds 17 .. 24 through render_temporal, against the plain 32 x 32-strata render of
    test_gpu_denoise_var.py (seed 4242) at the last camera.  Static camera: the accumulated image against the last frame alone, and
    accumulated + filtered against that frame through render_denoised_var; a 1 degree yaw per frame: the accumulated image against
    the last frame alone.  Measured: static camera, accumulated MSE / single-frame MSE 0.1422 and accumulated + filtered MSE /
    single-frame denoise_var MSE 0.5653; yaw, accumulated MSE / single-frame MSE 0.0906 ("Temporal accumulation")."""
    sb = scenes.cornell_scene(width=128, height=128)
    hs = pbrs_amd.HostScene(sb)
    gpu_ctx.upload(hs)
    cams = [_yawed(hs.camera, yaw * k) for k in range(8)]
    for den, acc, noisy, _ in gpu_ctx.render_temporal(cams, 2, 2, 5, range(17, 25)):
        pass
    ref, _, _ = gpu_ctx.render_aovs(32, 32, 5, 4242, aovs=(), camera=cams[-1])
    ok = np.isfinite(ref).all(axis=2) & np.isfinite(noisy).all(axis=2) & np.isfinite(acc).all(axis=2)
    e_n, e_a, e_d = _mse(noisy, ref, ok), _mse(acc, ref, ok), _mse(den, ref, ok)
    print(f"cornell 128 x 128, 4 spp, 8 frames, yaw {yaw} deg per frame: single-frame MSE {e_n:.5g}; accumulated {e_a:.5g}, ratio {e_a / e_n:.4f}; "
          f"accumulated + filtered {e_d:.5g}")
    assert e_a / e_n < 1.0
    if yaw == 0.0:
        single, single_noisy, _ = gpu_ctx.render_denoised_var(2, 2, 5, 24, keep_noisy=True)
        assert (bits(single_noisy) == bits(noisy)).all()
        e_s = _mse(single, ref, ok)
        print(f"  single-frame denoise_var MSE {e_s:.5g}; accumulated + filtered / single-frame denoise_var {e_d / e_s:.4f}")
        assert e_d / e_s < 1.0


def test_refusals_leave_the_context_usable(gpu_ctx):
    from test_gpu_pixel_filter import scene
    _, hs = scene("cornell")
    L = gpu_ctx._L
    w, h = 24, 20
    (cam0, f0, _), (cam1, f1, _) = list(tm.synthetic_sequence(w, h, 3, "pan", 2))
    hist0, _ = tm.accumulate(f0["rgb"], f0["depth"], cam0)
    out = {n: np.empty_like(a) for n, a in hist0.items()}
    vout = np.empty((h, w), f32)

    def call(fn=L.pbrs_temporal_accumulate, params=True, cam=True, cam_prev=True, frame=True, prev=True, hin=True, hout=True, drop=(), alias=(),
             size=(w, h), prev_size=(w, h), **fields):
        p = api.TemporalParams.make(w, h, id_test=True)
        for n, v in fields.items():
            setattr(p, n, v)
        cams = [api_camera(cam1), api_camera(cam0)]
        (cams[0].width, cams[0].height), (cams[1].width, cams[1].height) = size, prev_size
        fs = api._temporal_struct(api.TemporalFrame, api.TEMPORAL_FRAME, {n: a.ctypes.data for n, a in f1.items() if "frame." + n not in drop}, "frame")
        gs = api._temporal_struct(api.TemporalGuides, api.TEMPORAL_GUIDES,
                                  {n: f0[n].ctypes.data for n in tm.GUIDE_NAMES if "prev." + n not in drop}, "previous guide")
        hi = api._temporal_struct(api.TemporalHistory, api.TEMPORAL_HISTORY, {n: a.ctypes.data for n, a in hist0.items() if "hin." + n not in drop}, "history")
        ho = api._temporal_struct(api.TemporalHistory, api.TEMPORAL_HISTORY,
                                  {n: (hist0[n] if n in alias else a).ctypes.data for n, a in out.items() if "hout." + n not in drop}, "history")
        return fn(gpu_ctx._h, C.addressof(p) if params else None, C.addressof(cams[0]) if cam else None, C.addressof(cams[1]) if cam_prev else None,
                  C.addressof(fs) if frame else None, C.addressof(gs) if prev else None, C.addressof(hi) if hin else None,
                  C.addressof(ho) if hout else None, vout.ctypes.data)
    nan, inf = float("nan"), float("inf")
    for fn in (L.pbrs_temporal_accumulate, L.pbrs_temporal_accumulate_device):  # (the device variant refuses before it touches a pointer)
        assert call(fn, params=False) == -1 and call(fn, cam=False) == -1 and call(fn, frame=False) == -1 and call(fn, hout=False) == -1
        assert call(fn, drop=("frame.rgb",)) == -1 and call(fn, drop=("frame.depth",)) == -1
        for n in ("rgb", "moments", "length"):
            assert call(fn, drop=("hout." + n,)) == -1 and call(fn, drop=("hin." + n,)) == -1, n
            assert call(fn, alias=(n,)) == -1, n
            assert b"in place" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, cam_prev=False) == -1 and call(fn, prev=False) == -1 and call(fn, drop=("prev.depth",)) == -1
        assert call(fn, drop=("frame.normal",)) == -1 and call(fn, drop=("prev.normal",)) == -1
        assert call(fn, drop=("prev.instance",)) == -1 and call(fn, drop=("frame.instance",), flags=0) == -1
        assert call(fn, drop=("frame.instance", "prev.instance")) == -1  # the id test without ids
        assert call(fn, flags=2) == -1 and call(fn, flags=0x80000001) == -1
        assert call(fn, w=0) == -1 and call(fn, h=0) == -1
        assert call(fn, size=(w + 1, h)) == -1 and call(fn, size=(w, h - 1)) == -1 and call(fn, prev_size=(w, h + 1)) == -1
        for v in (0.5, 0.0, -1.0, nan, inf):
            assert call(fn, max_history=v) == -1, v
        for n in ("depth_tolerance", "normal_tolerance"):
            for v in (0.0, -1.0, nan, inf):
                assert call(fn, **{n: v}) == -1, (n, v)
        for v in (1.5, 0.0, nan, inf):
            assert call(fn, min_temporal=v) == -1, v
        assert call(fn, w=1 << 15, h=(1 << 13) + 1, size=(1 << 15, (1 << 13) + 1), prev_size=(1 << 15, (1 << 13) + 1)) == -4  # PBRS_E_LIMIT
        assert b"2^28" in L.pbrs_last_error(gpu_ctx._h)
    # what is allowed: the first frame without a previous camera or guides, absent guides on both sides, max_history 1, min_temporal 2
    assert call() == 0
    assert call(hin=False, cam_prev=False, prev=False) == 0
    assert call(drop=("frame.normal", "prev.normal", "frame.variance"), max_history=1.0, min_temporal=2.0) == 0
    assert call(drop=("frame.instance", "prev.instance"), flags=0) == 0
    want, _ = tm.accumulate(f1["rgb"], f1["depth"], cam1, variance=f1["variance"], normal=f1["normal"], history=hist0,
                            prev={n: f0[n] for n in ("depth", "normal")}, cam_prev=cam0)
    assert all(same(out[n], want[n]).all() for n in PLANES)
    # a plain render afterwards: the bits of a fresh context
    gpu_ctx.upload(hs)
    img, _ = gpu_ctx.render(2, 2, 3, 1)
    fresh = pbrs_amd.Context(0)
    try:
        fresh.upload(hs)
        assert (bits(img) == bits(fresh.render(2, 2, 3, 1)[0])).all()
        # staging growth: a larger image after a smaller one on a context that starts with none
        for size in ((9, 7), (70, 50), (33, 21)):
            got = tm.run_sequence(gpu_step(fresh), size[0], size[1], 2, "pan", frames=2)
            want = tm.run_sequence(tm.accumulate, size[0], size[1], 2, "pan", frames=2)
            agree(got[1], want[1], size)
    finally:
        fresh.close()


def test_a_refused_host_call_says_why_and_changes_no_later_result(gpu_ctx):
    """13 x 7 (odd, less than one block, no multiple of the 16-pixel cell): a denoise and a two-frame accumulation through the host
    variants, which stage every plane; then a call of each that the C checks refuse (host/arg_checks.cpp), with their messages; then
    the same two calls again, to the same bits."""
    from test_gpu_denoise import synthetic
    w, h = 13, 7
    rgb, guides = synthetic(w, h, 5)

    def both():
        seq = tm.run_sequence(gpu_step(gpu_ctx), w, h, 3, "pan", frames=2, id_test=True)
        return bits(gpu_ctx.denoise(rgb, iterations=3, **guides)).tobytes(), sequence_bits(seq) + bits(seq[-1][1]).tobytes()
    before = both()
    want = tm.run_sequence(tm.accumulate, w, h, 3, "pan", frames=2, id_test=True)
    assert before[1] == sequence_bits(want) + bits(want[-1][1]).tobytes()
    with pytest.raises(pbrs_amd.PbrsError, match=r"pbrs_denoise failed \(-1\): denoise iterations must be 1 \.\. 6$"):
        gpu_ctx.denoise(rgb, iterations=0, **guides)
    cam, frame, _ = next(iter(tm.synthetic_sequence(w, h, 3, "pan", 2)))
    with pytest.raises(pbrs_amd.PbrsError, match=r"pbrs_temporal_accumulate failed \(-1\): the temporal frame needs rgb and depth$"):
        gpu_ctx.temporal_accumulate(frame["rgb"], None, api_camera(cam))
    assert both() == before
