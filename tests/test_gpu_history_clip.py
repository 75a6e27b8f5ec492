"""History clipping on the GPU (include/pbrs_gpu.h, pbrs_temporal_accumulate_clip[_device]; device/temporal.h, k_temporal_clip): bit for
bit against the CPU model of tests/history_clip_model.py on synthetic sequences, every guide present or absent, the device variant in
the chain of Context.render_animation, the entry point without a clip against the motion call, what the header refuses, and the lag of
a moving shadow that the clip removes on a rendered sequence."""
import ctypes as C
import itertools

import numpy as np
import pytest

import history_clip_model as hc
import motion_model as mm
import pbrs_amd
import temporal_model as tm
from common import bits
from pbrs_amd import api
from test_gpu_denoise import same
from test_gpu_temporal import PLANES, agree, api_camera, sequence_bits

pytestmark = pytest.mark.gpu

f32 = np.float32
# (w, h): the smallest sizes at which a tile edge, a halo wider than the image, a single row or a single column can go wrong
SIZES = ((1, 1), (2, 3), (7, 5), (64, 1), (1, 64), (15, 17), (16, 16), (17, 33), (37, 29), (130, 70))
CLIP = dict(gamma=1.0, clip_history=2.0)


def gpu_step(ctx):
    """Context.temporal_accumulate with the signature of the model's accumulate (hc.run_sequence)."""
    def step(rgb, depth, cam, history=None, prev=None, cam_prev=None, want_variance=True, motion=None, clip=None, **kw):
        return ctx.temporal_accumulate(rgb, depth, api_camera(cam), history=history, prev=prev, camera_prev=api_camera(cam_prev) if cam_prev else None,
                                       return_variance=want_variance, motion=mm.to_ctypes(motion), clip=clip, **kw)
    return step


@pytest.mark.parametrize("move", ("none", "pan", "yaw"))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matches_the_cpu_model_bit_for_bit_on_synthetic_sequences(gpu_ctx, size, move):
    """Three frames, each side fed its own history (what the sequence plants into it included); radius 1, 2 and 3, with and without a
    motion table, all guides and the id test.  From 15 x 17 on the case is not vacuous: some pixel is clipped, some pixel with a history
    is not, and some window skips a non-finite tap (the sequences plant a NaN and an infinite pixel into every frame)."""
    w, h = size
    seen = set()
    for radius, with_table in itertools.product((1, 2, 3), (False, True)):
        kw = dict(clip=dict(CLIP, radius=radius), with_table=with_table, id_test=True)
        got = hc.run_sequence(gpu_step(gpu_ctx), w, h, w + h, move, **kw)
        want = hc.run_sequence(hc.accumulate, w, h, w + h, move, **kw)
        for k, (g, m) in enumerate(zip(got, want)):
            agree(g[:2], m[:2], (size, move, radius, with_table, k))
        seen.add(sequence_bits([g[:2] for g in got]))
        if w * h >= 255:
            det = [m[2] for m in want[1:]]
            assert sum(int(d["clipped"].sum()) for d in det) >= 1, (radius, with_table)
            assert sum(int((d["has"] & ~d["clipped"]).sum()) for d in det) >= 1, (radius, with_table)
            assert sum(int(d["skipped"].sum()) for d in det) >= 1, (radius, with_table)
    if size == (130, 70):  # the radius and the table each change the result, and so does the clip
        assert len(seen) == 6
        plain = hc.run_sequence(gpu_step(gpu_ctx), w, h, w + h, move, clip=None, id_test=True)
        assert sequence_bits([g[:2] for g in plain]) not in seen


@pytest.mark.parametrize("variance", (False, True))
def test_every_guide_present_or_absent(gpu_ctx, variance):
    """variance, normal, instance (with and without the id test, with a motion table where there are ids) and variance_out, each given
    or not: the eight instantiations of the kernel, bit for bit."""
    seen = {}
    tight = dict(normal_tolerance=0.03)
    for normal, instance, vout in itertools.product((False, True), repeat=3):
        for id_test, with_table in (((False, False), (True, False), (False, True), (True, True)) if instance else ((False, False),)):
            use = tuple(n for n, on in (("variance", variance), ("normal", normal), ("instance", instance)) if on)
            kw = dict(use=use, want_variance=vout, id_test=id_test, with_table=with_table, clip=dict(CLIP, radius=2), **tight)
            got = hc.run_sequence(gpu_step(gpu_ctx), 37, 29, 11, "yaw", **kw)
            want = hc.run_sequence(hc.accumulate, 37, 29, 11, "yaw", **kw)
            for k, (g, m) in enumerate(zip(got, want)):
                agree(g[:2], m[:2], (use, vout, id_test, with_table, k))
            seen[(normal, instance, id_test, with_table, vout)] = sequence_bits([g[:2] for g in got])
    assert len(seen) == 20
    base = seen[(False, False, False, False, True)]
    assert seen[(False, False, False, False, False)] == base       # variance_out NULL: the same history
    assert seen[(True, False, False, False, True)] != base         # the normal test rejects taps
    assert seen[(False, True, False, False, True)] == base         # ids without the flag and without a table: not read
    assert seen[(False, True, True, False, True)] != base          # the id test rejects taps
    assert seen[(False, True, False, True, True)] != base          # the table moves the taps


def _raw(ctx, fn, w, h, cams, f1, f0, hist0, out, vout, tab, clip, alias=False):
    """One call of `fn` (an entry point with a clip argument) on host arrays; `clip`: a HistoryClipParams or None (NULL)."""
    p = api.TemporalParams.make(w, h)
    fs = api._temporal_struct(api.TemporalFrame, api.TEMPORAL_FRAME, {n: a.ctypes.data for n, a in f1.items()}, "frame")
    gs = api._temporal_struct(api.TemporalGuides, api.TEMPORAL_GUIDES, {n: f0[n].ctypes.data for n in tm.GUIDE_NAMES}, "previous guide")
    hi = api._temporal_struct(api.TemporalHistory, api.TEMPORAL_HISTORY, {n: a.ctypes.data for n, a in hist0.items()}, "history")
    ho = api._temporal_struct(api.TemporalHistory, api.TEMPORAL_HISTORY, {n: a.ctypes.data for n, a in out.items()}, "history")
    if alias:
        ho.rgb = fs.rgb
    return fn(ctx._h, C.addressof(p), C.addressof(cams[0]), C.addressof(cams[1]), C.addressof(fs), C.addressof(gs), C.addressof(hi), C.addressof(ho),
              vout.ctypes.data, C.addressof(tab), len(tab), C.addressof(clip) if clip is not None else None)


def _two_frames(w, h):
    (cam0, f0, _, _), (cam1, f1, _, table) = list(mm.motion_sequence(w, h, 3, "yaw", 2))
    hist0, _ = tm.accumulate(f0["rgb"], f0["depth"], cam0)
    return cam0, f0, cam1, f1, table, hist0


def test_without_a_clip_the_entry_point_is_the_motion_call(gpu_ctx):
    w, h = 37, 29
    cam0, f0, cam1, f1, table, hist0 = _two_frames(w, h)
    out = {n: np.zeros_like(a) for n, a in hist0.items()}
    vout = np.zeros((h, w), f32)
    cams = [api_camera(cam1), api_camera(cam0)]
    assert _raw(gpu_ctx, gpu_ctx._L.pbrs_temporal_accumulate_clip, w, h, cams, f1, f0, hist0, out, vout, mm.to_ctypes(table), None) == 0
    want = gpu_ctx.temporal_accumulate(f1["rgb"], f1["depth"], cams[0], variance=f1["variance"], normal=f1["normal"], instance=f1["instance"], history=hist0,
                                       prev={n: f0[n] for n in tm.GUIDE_NAMES}, camera_prev=cams[1], motion=mm.to_ctypes(table))
    agree((out, vout), want, "clip NULL")
    clipped = gpu_ctx.temporal_accumulate(f1["rgb"], f1["depth"], cams[0], variance=f1["variance"], normal=f1["normal"], instance=f1["instance"],
                                          history=hist0, prev={n: f0[n] for n in tm.GUIDE_NAMES}, camera_prev=cams[1], motion=mm.to_ctypes(table), clip=True)
    assert sequence_bits([clipped]) != sequence_bits([want])
    # the first frame of a sequence has nothing to clip
    first = gpu_ctx.temporal_accumulate(f0["rgb"], f0["depth"], cams[1], clip=True)
    agree(first, tm.accumulate(f0["rgb"], f0["depth"], cam0), "first frame")


def test_refusals_leave_the_context_usable(gpu_ctx):
    L = gpu_ctx._L
    w, h = 24, 20
    cam0, f0, cam1, f1, table, hist0 = _two_frames(w, h)
    out = {n: np.zeros_like(a) for n, a in hist0.items()}
    vout = np.zeros((h, w), f32)
    cams, tab = [api_camera(cam1), api_camera(cam0)], mm.to_ctypes(table)

    def call(fn, alias=False, flags=0, **kw):
        cp = api.HistoryClipParams.make(**kw)
        cp.flags = flags
        return _raw(gpu_ctx, fn, w, h, cams, f1, f0, hist0, out, vout, tab, cp, alias)
    for fn in (L.pbrs_temporal_accumulate_clip, L.pbrs_temporal_accumulate_clip_device):  # (the device variant refuses before it touches a pointer)
        assert call(fn, radius=0) == -1 and b"radius" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, radius=api.HistoryClipParams.MAX_RADIUS + 1) == -1
        assert call(fn, gamma=0.0) == -1 and b"gamma" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, gamma=float("nan")) == -1 and call(fn, gamma=float("inf")) == -1 and call(fn, gamma=-1.0) == -1
        assert call(fn, clip_history=0.5) == -1 and b"clip_history" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, clip_history=float("nan")) == -1
        assert call(fn, flags=1) == -1 and b"flag" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, alias=True) == -1 and b"halo" in L.pbrs_last_error(gpu_ctx._h)
    # what is allowed, and still right after the refusals
    for kw in (dict(radius=3, gamma=0.5, clip_history=1.0), dict(radius=1, gamma=2.0, clip_history=None)):
        assert call(L.pbrs_temporal_accumulate_clip, **kw) == 0
        want = hc.accumulate(f1["rgb"], f1["depth"], cam1, variance=f1["variance"], normal=f1["normal"], instance=f1["instance"], history=hist0,
                             prev={n: f0[n] for n in tm.GUIDE_NAMES}, cam_prev=cam0, motion=table, clip=kw)
        agree((out, vout), want, kw)


def test_render_animation_with_a_clip_is_the_hand_made_chain(gpu_ctx):
    """The device variant, queued between the device render and denoise_var_device on one stream with one wait per frame, equals the
    host variant on the same frames bit for bit."""
    guides = ("albedo", "normal", "depth", "instance")
    clip = dict(radius=2, gamma=1.0, clip_history=3.0)
    scenes_ = [pbrs_amd.HostScene(mm.turned_short_box(k)) for k in range(3)]
    frames = list(gpu_ctx.render_animation([(hs, None, 9 + k) for k, hs in enumerate(scenes_)], 2, 2, 5, temporal=dict(id_test=True, min_temporal=2.0),
                                           clip=clip, iterations=3))
    plain = list(gpu_ctx.render_animation([(hs, None, 9 + k) for k, hs in enumerate(scenes_)], 2, 2, 5, temporal=dict(id_test=True, min_temporal=2.0),
                                          iterations=3))
    history = prev = None
    for k, (hs, (den, acc, noisy, st)) in enumerate(zip(scenes_, frames)):
        gpu_ctx.upload(hs)
        cam = hs.camera
        table = api.instance_motion(hs, scenes_[k - 1]) if k else None
        img, aov, _ = gpu_ctx.render_aovs(2, 2, 5, 9 + k, aovs=guides + ("variance",))
        var = aov.pop("variance")
        assert (bits(noisy) == bits(img)).all(), k
        history, v = gpu_ctx.temporal_accumulate(img, aov["depth"], cam, variance=var, normal=aov["normal"], instance=aov["instance"], history=history,
                                                 prev=prev, camera_prev=cam if k else None, id_test=True, min_temporal=2.0, motion=table, clip=clip)
        assert same(acc, history["rgb"]).all(), k
        assert same(den, gpu_ctx.denoise_var(history["rgb"], v, iterations=3, **aov)).all(), k
        prev = {n: aov[n] for n in tm.GUIDE_NAMES}
    assert (bits(frames[0][1]) == bits(plain[0][1])).all() and (bits(frames[2][1]) != bits(plain[2][1])).any()
    cams = [scenes_[0].camera] * 2
    gpu_ctx.upload(scenes_[0])
    a = list(gpu_ctx.render_temporal(cams, 2, 2, 5, [9, 10], clip=True, iterations=1))
    b = list(gpu_ctx.render_temporal(cams, 2, 2, 5, [9, 10], iterations=1))
    assert (bits(a[0][1]) == bits(b[0][1])).all() and (bits(a[1][1]) != bits(b[1][1])).any()


GAP_FRAMES = 5
# Of the larger of the two ground-truth luminances.  A pixel of a 16 x 16-strata render of this box keeps a relative noise of about a
# tenth (single samples of its indirect light scatter by about their own mean, over sqrt(256)), so the difference of two such renders
# scatters by about 0.15: a difference above 0.2 is the lighting's, not the ground truths' own noise.
GAP_THRESHOLD = 0.2
# Mean absolute error over the region without and with the clip, on the first run on an MI355X (the renders are seeded: a rerun gives
# the same images).
GAP_MEASURED = (1.3304, 1.0295)


def test_the_clip_shortens_the_lag_of_a_moving_shadow(gpu_ctx):
    """The documented gap of the motion call.  The 128 x 128 Cornell box of motion_model.turned_short_box at 2 x 2 strata, five frames
    through render_animation (seeds 9 .. 13, the id test), the short box turning 4 degrees per frame.  Ground truth: the last frame's
    scene rendered alone at 16 x 16 strata.  The region: pixels whose instance id is the same surface other than the short box in the
    first and the last frame's ground-truth render, and whose ground-truth luminance differs between the two scenes by more than
    GAP_THRESHOLD of the larger one — where the box's shadow and its bounce light arrived or left.  Over the region the accumulated
    image's mean absolute error must fall by at least half of what the first run measured (GAP_MEASURED; never less than "strictly
    lower"); over the other pixels it may rise to 1.05 of the unclipped one.
    Measured on one MI355X: the region is 12 pixels, mean absolute error 1.3304 unclipped and 1.0295 clipped (ratio 0.774), so the
    assertion asks for an improvement of at least 0.150; the other 16 372 pixels 0.74655 unclipped and 0.64677 clipped (ratio 0.866)."""
    scenes_ = [pbrs_amd.HostScene(mm.turned_short_box(k)) for k in range(GAP_FRAMES)]
    acc = {}
    for clip in (None, True):
        frames = list(gpu_ctx.render_animation([(hs, None, 9 + k) for k, hs in enumerate(scenes_)], 2, 2, 5, temporal=dict(id_test=True), clip=clip,
                                               iterations=1))
        acc[clip] = frames[-1][1]
    truth = {}
    for k in (0, GAP_FRAMES - 1):
        gpu_ctx.upload(scenes_[k])
        img, aov, _ = gpu_ctx.render_aovs(16, 16, 5, 4242 + k, aovs=("instance",))
        truth[k] = (img, aov["instance"])
    (ref0, inst0), (ref, inst) = truth[0], truth[GAP_FRAMES - 1]
    finite = np.isfinite(ref0).all(axis=2) & np.isfinite(ref).all(axis=2) & np.isfinite(acc[None]).all(axis=2) & np.isfinite(acc[True]).all(axis=2)
    static = (inst0 == inst) & (inst != mm.SHORT_BOX) & (inst != tm.MISS)
    l0, l1 = hc.lum(ref0).astype(np.float64), hc.lum(ref).astype(np.float64)
    region = finite & static & (np.abs(l1 - l0) > GAP_THRESHOLD * np.maximum(l0, l1))
    rest = finite & ~region

    def err(img, where):
        return float(np.abs(img[where].astype(np.float64) - ref[where]).mean())
    e_plain, e_clip = err(acc[None], region), err(acc[True], region)
    o_plain, o_clip = err(acc[None], rest), err(acc[True], rest)
    print(f"region {int(region.sum())} pixels: mean absolute error {e_plain:.5g} unclipped, {e_clip:.5g} clipped (ratio {e_clip / e_plain:.3f}); "
          f"the other {int(rest.sum())} pixels: {o_plain:.5g} unclipped, {o_clip:.5g} clipped (ratio {o_clip / o_plain:.3f})")
    assert region.sum() >= 1
    assert e_clip < e_plain
    assert e_plain - e_clip >= 0.5 * (GAP_MEASURED[0] - GAP_MEASURED[1])
    assert o_clip <= 1.05 * o_plain
