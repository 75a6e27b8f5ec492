"""Moving instances on the GPU (include/pbrs_gpu.h, pbrs_temporal_accumulate_motion[_device] and pbrs_motion_vectors[_device];
device/temporal.h): bit for bit against the CPU model of tests/motion_model.py on synthetic and rendered sequences, against the kernels
without a table where the table says nothing, the device variants and the ordering of the table's copy, Context.render_animation, the
error a table removes on a sliding box, and what the header refuses."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import motion_model as mm
import pbrs_amd
import temporal_model as tm
from common import bits
from pbrs_amd import DeviceBuffers, api, scenes
from test_gpu_denoise import same
from test_gpu_temporal import PLANES, agree, api_camera, model_camera, sequence_bits
from test_motion_model import SLIDE_FRAMES, sliding_box_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = ((1, 1), (7, 5), (64, 1), (37, 29), (130, 70))  # (w, h)


def gpu_step(ctx, table_of=mm.to_ctypes):
    """Context.temporal_accumulate with the signature of the model's accumulate (mm.run_sequence)."""
    def step(rgb, depth, cam, history=None, prev=None, cam_prev=None, want_variance=True, motion=None, **kw):
        return ctx.temporal_accumulate(rgb, depth, api_camera(cam), history=history, prev=prev, camera_prev=api_camera(cam_prev) if cam_prev else None,
                                       return_variance=want_variance, motion=table_of(motion), **kw)
    return step


@pytest.mark.parametrize("move", ("none", "yaw"))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matches_the_cpu_model_bit_for_bit_on_synthetic_sequences(gpu_ctx, size, move):
    """Three frames, each side fed its own history; the four MOTION instantiations (normal test x id test), and a table of one record
    under ids that reach far past it."""
    w, h = size
    seen = {}
    cases = [(normals, id_test, mm.N_MOTION) for normals in (False, True) for id_test in (False, True)] + [(True, True, 1)]
    for normals, id_test, n_motion in cases:
        kw = dict(use=("variance", "normal", "instance") if normals else ("variance", "instance"), id_test=id_test, n_motion=n_motion)
        got = mm.run_sequence(gpu_step(gpu_ctx), w, h, w + h, move, **kw)
        want = mm.run_sequence(mm.accumulate, w, h, w + h, move, **kw)
        for k, (g, m) in enumerate(zip(got, want)):
            agree(g, m, (size, move, normals, id_test, n_motion, k))
        seen[(normals, id_test, n_motion)] = sequence_bits(got)
    if size == (130, 70):  # every switch changes the result: four different kernels ran, and the short table leaves most pixels static
        assert len(set(seen.values())) == 5
        plain = tm.run_sequence(tm.accumulate, w, h, w + h, move, id_test=True)
        assert sequence_bits(plain) != seen[(True, True, mm.N_MOTION)]
        assert (got[-1][0]["length"] > 2.0).any()


def test_a_table_of_identity_records_gives_the_bits_of_the_call_without_a_table(gpu_ctx):
    """GPU against GPU: the MOTION kernels beside the existing ones, with and without normals and the id test."""
    def flagged(table):
        return mm.to_ctypes(None if table is None else dict(table, flags=np.full_like(table["flags"], mm.IDENTITY)))

    def none(table):
        return None
    for move in ("none", "yaw"):
        for normals in (False, True):
            for id_test in (False, True):
                kw = dict(use=("variance", "normal", "instance") if normals else ("variance", "instance"), id_test=id_test)
                a = mm.run_sequence(gpu_step(gpu_ctx, flagged), 130, 70, 9, move, **kw)
                b = mm.run_sequence(gpu_step(gpu_ctx, none), 130, 70, 9, move, **kw)
                for k, (g, m) in enumerate(zip(a, b)):
                    agree(g, m, (move, normals, id_test, k))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_motion_vectors_match_the_cpu_model_bit_for_bit(gpu_ctx, size):
    w, h = size
    for move in ("none", "yaw"):
        (camp, _, _, _), (cam, frame, _, table) = list(mm.motion_sequence(w, h, w + h, move, 2))
        plants = [(0.0,), (np.nan,), (np.inf,)] if w * h == 1 else [(0.0, np.nan, np.inf)]
        for plant in plants:
            depth = frame["depth"].copy()
            for i, v in enumerate(plant):
                depth.reshape(-1)[(5 * i) % (w * h)] = v
            for t in (None, table):
                inst = frame["instance"] if t is not None else None
                want = mm.motion_vectors(depth, cam, camp, inst, t)
                mv, wq = gpu_ctx.motion_vectors(depth, api_camera(cam), api_camera(camp), instance=inst, motion=mm.to_ctypes(t), return_prev_depth=True)
                assert same(mv, want[0]).all() and same(wq, want[1]).all(), (size, move, plant, t is not None)
                only = gpu_ctx.motion_vectors(depth, api_camera(cam), api_camera(camp), instance=inst, motion=mm.to_ctypes(t))
                assert same(only, want[0]).all()
                bad = ~(np.isfinite(depth) & (depth > 0))
                assert (bits(mv[bad]) == 0).all() and np.isposinf(wq[bad]).all() and bad.sum() >= 1
        if size == (130, 70):
            assert (bits(mm.motion_vectors(depth, cam, camp, frame["instance"], table)[0]) != bits(mm.motion_vectors(depth, cam, camp)[0])).any()


def test_the_device_variants_equal_the_host_ones_and_the_tables_copy_is_ordered(gpu_ctx):
    """Two accumulations and two motion vector calls back to back on caller buffers, with two different tables and one wait at the end:
    each equals the host call with its own table."""
    w, h = 130, 70
    (cam0, f0, _, _), (cam1, f1, _, ta) = list(mm.motion_sequence(w, h, 5, "yaw", 2))
    tb = mm.random_table(np.random.default_rng(99))
    c0, c1 = api_camera(cam0), api_camera(cam1)
    hist0, _ = gpu_ctx.temporal_accumulate(f0["rgb"], f0["depth"], c0, variance=f0["variance"], normal=f0["normal"], instance=f0["instance"])
    prev = {n: f0[n] for n in tm.GUIDE_NAMES}
    host = [gpu_ctx.temporal_accumulate(f1["rgb"], f1["depth"], c1, variance=f1["variance"], normal=f1["normal"], instance=f1["instance"],
                                        history=hist0, prev=prev, camera_prev=c0, id_test=True, motion=mm.to_ctypes(t)) for t in (ta, tb)]
    host_mv = [gpu_ctx.motion_vectors(f1["depth"], c1, c0, instance=f1["instance"], motion=mm.to_ctypes(t), return_prev_depth=True) for t in (ta, tb)]
    assert sequence_bits([host[0]]) != sequence_bits([host[1]]) and (bits(host_mv[0][0]) != bits(host_mv[1][0])).any()
    like = {"rgb": np.zeros((h, w, 3), f32), "moments": np.zeros((h, w, 2), f32), "length": np.zeros((h, w), f32), "v": np.zeros((h, w), f32),
            "mv": np.zeros((h, w, 2), f32), "wq": np.zeros((h, w), f32)}
    with contextlib.ExitStack() as held:
        frame, guides, hin, *outs = (held.enter_context(DeviceBuffers(arrays)) for arrays in (f1, prev, hist0, like, like))
        for t, out in zip((ta, tb), outs):
            table = mm.to_ctypes(t)
            gpu_ctx.temporal_accumulate_device(frame.ptrs(), out.ptrs(PLANES), w, h, c1, hin.ptrs(), guides.ptrs(), c0, out.ptr("v"), id_test=True,
                                               motion=table)
            gpu_ctx.motion_vectors_device(frame.ptr("depth"), out.ptr("mv"), w, h, c1, c0, frame.ptr("instance"), table, out.ptr("wq"))
            del table  # the library has read it
        gpu_ctx.collect_stats()
        for k, out in enumerate(outs):
            got = {n: out.download_like(n, like[n]) for n in like}
            agree(({n: got[n] for n in PLANES}, got["v"]), host[k], k)
            assert same(got["mv"], host_mv[k][0]).all() and same(got["wq"], host_mv[k][1]).all(), k


AOVS = ("normal", "depth", "instance", "variance")


def test_matches_the_cpu_model_bit_for_bit_on_a_rendered_sequence(gpu_ctx):
    """The 128 x 128 Cornell box whose short box (instance 8) turns 4 degrees per frame about its own axis: three frames at 2 x 2 strata,
    render_aovs' buffers in, the model's expectation out.  Not vacuous: the table changes the result, and after the third frame at
    least half of the box's pixels carry a history (with the oracle's first hits the model keeps a tap for 88.0 % of them at 4 degrees)."""
    history = mhistory = plain = prev = scene_prev = None
    for k in range(3):
        hs = pbrs_amd.HostScene(mm.turned_short_box(k))
        gpu_ctx.upload(hs)
        cam = hs.camera
        table = api.instance_motion(hs, scene_prev) if k else None
        img, aov, _ = gpu_ctx.render_aovs(2, 2, 5, 7 + k, aovs=AOVS)
        frame = dict(variance=aov["variance"], normal=aov["normal"], instance=aov["instance"])
        got = gpu_ctx.temporal_accumulate(img, aov["depth"], cam, history=history, prev=prev, camera_prev=cam if k else None, id_test=True, motion=table, **frame)
        want = mm.accumulate(img, aov["depth"], model_camera(cam), history=mhistory, prev=prev, cam_prev=model_camera(cam) if k else None, id_test=True,
                             motion=mm.from_ctypes(table) if k else None, **frame)
        agree(got, want, k)
        plain = gpu_ctx.temporal_accumulate(img, aov["depth"], cam, history=plain, prev=prev, camera_prev=cam if k else None, id_test=True, **frame)[0]
        history, mhistory, scene_prev = got[0], want[0], hs
        prev = {n: aov[n] for n in tm.GUIDE_NAMES}
    box = aov["instance"] == mm.SHORT_BOX
    share, without = float((history["length"][box] > 1.0).mean()), float((plain["length"][box] > 1.0).mean())
    print(f"{int(box.sum())} pixels of the turning box: {share:.3f} carry a history after frame 3 ({without:.3f} without the table)")
    assert box.sum() > 500 and share >= 0.5
    assert sequence_bits([(history, None)]) != sequence_bits([(plain, None)])
    assert all((bits(history[n][~box]) == bits(plain[n][~box])).all() for n in PLANES)


def test_render_animation_is_the_hand_made_chain(gpu_ctx):
    guides = ("albedo", "normal", "depth", "instance")
    scenes_ = [pbrs_amd.HostScene(mm.turned_short_box(k)) for k in range(3)]
    frames = list(gpu_ctx.render_animation([(hs, None, 9 + k) for k, hs in enumerate(scenes_)], 2, 2, 5, temporal=dict(id_test=True, min_temporal=2.0),
                                           motion_vectors=True, iterations=3))
    assert len(frames) == 3
    history = prev = None
    for k, (hs, (den, acc, noisy, st, mv)) in enumerate(zip(scenes_, frames)):
        gpu_ctx.upload(hs)
        cam = hs.camera
        table = api.instance_motion(hs, scenes_[k - 1]) if k else None
        img, aov, _ = gpu_ctx.render_aovs(2, 2, 5, 9 + k, aovs=guides + ("variance",))
        var = aov.pop("variance")
        assert (bits(noisy) == bits(img)).all(), k
        history, v = gpu_ctx.temporal_accumulate(img, aov["depth"], cam, variance=var, normal=aov["normal"], instance=aov["instance"], history=history,
                                                 prev=prev, camera_prev=cam if k else None, id_test=True, min_temporal=2.0, motion=table)
        assert same(acc, history["rgb"]).all(), k
        assert same(den, gpu_ctx.denoise_var(history["rgb"], v, iterations=3, **aov)).all(), k
        assert st["samples"] == img.shape[0] * img.shape[1] * 4
        want_mv = gpu_ctx.motion_vectors(aov["depth"], cam, cam, instance=aov["instance"], motion=table) if k else np.zeros_like(mv)
        assert mv.shape == (128, 128, 2) and same(mv, want_mv).all(), k
        prev = {n: aov[n] for n in tm.GUIDE_NAMES}
    box = aov["instance"] == mm.SHORT_BOX
    assert (history["length"][box] > 1.0).mean() > 0.5 and np.abs(mv[box]).max() > 1.0 and np.abs(mv[~box]).max() < 1e-3  # (a static camera)
    four = next(gpu_ctx.render_animation([(scenes_[0], None, 9)], 2, 2, 5, iterations=3))
    assert len(four) == 4 and (bits(four[2]) == bits(frames[0][2])).all()


def _mse(img, ref, ok):
    return float(((img[ok].astype(np.float64) - ref[ok]) ** 2).mean())


def test_a_table_removes_the_error_of_a_sliding_box(gpu_ctx):
    """The CPU experiment of test_motion_model.py on the GPU's own renders: the 128 x 128 Cornell box, an 8 x 8 two-colour image
    checker on the short box, which slides -12 units in x per frame from x = 330; 8 frames at 2 x 2 strata with seeds 17 .. 24, the depth
    and id tests; the reference is the 32 x 32-strata render (seed 4242) of the last frame.  On the box's pixels the image accumulated
    with the table beats the single frame and the image accumulated without it; the static pixels keep their bits.  The CPU model on
    the oracle's renders: 1.686 / 2.771 / 9.358 ("Moving instances and motion vectors", holds the GPU's figures)."""
    hist = {False: None, True: None}
    prev = scene_prev = None
    for k in range(SLIDE_FRAMES):
        hs = pbrs_amd.HostScene(sliding_box_scene(k))
        gpu_ctx.upload(hs)
        img, aov, _ = gpu_ctx.render_aovs(2, 2, 5, 17 + k, aovs=("depth", "instance"))
        table = api.instance_motion(hs, scene_prev) if k else None
        for follow in (False, True):
            hist[follow], _ = gpu_ctx.temporal_accumulate(img, aov["depth"], hs.camera, instance=aov["instance"], history=hist[follow], prev=prev,
                                                          camera_prev=hs.camera if k else None, id_test=True, motion=table if follow else None)
        prev, scene_prev = {"depth": aov["depth"], "instance": aov["instance"]}, hs
    ref, _, _ = gpu_ctx.render_aovs(32, 32, 5, 4242, aovs=())
    inst = aov["instance"]
    ok = np.isfinite(ref).all(axis=2) & np.isfinite(img).all(axis=2) & np.isfinite(hist[False]["rgb"]).all(axis=2) & np.isfinite(hist[True]["rgb"]).all(axis=2)
    box = (inst == mm.SHORT_BOX) & ok
    e_with, e_single, e_without = _mse(hist[True]["rgb"], ref, box), _mse(img, ref, box), _mse(hist[False]["rgb"], ref, box)
    print(f"{int(box.sum())} pixels of the sliding box: MSE with the table {e_with:.4g}, single frame {e_single:.4g}, without the table {e_without:.4g}; "
          f"{float((hist[True]['length'][box] > 1.0).mean()):.3f} carry a history")
    assert box.sum() > 500
    assert e_with < e_single
    assert e_with < e_without
    assert all((bits(hist[True][n][inst != mm.SHORT_BOX]) == bits(hist[False][n][inst != mm.SHORT_BOX])).all() for n in PLANES)


def test_refusals_leave_the_context_usable(gpu_ctx):
    L = gpu_ctx._L
    w, h = 24, 20
    (cam0, f0, _, _), (cam1, f1, _, table) = list(mm.motion_sequence(w, h, 3, "yaw", 2))
    hist0, _ = tm.accumulate(f0["rgb"], f0["depth"], cam0)
    out = {n: np.empty_like(a) for n, a in hist0.items()}
    vout, mv, wq = np.empty((h, w), f32), np.empty((h, w, 2), f32), np.empty((h, w), f32)
    tab = mm.to_ctypes(table)
    cams = [api_camera(cam1), api_camera(cam0)]

    def accumulate(fn, instance=True, motion=True, n_motion=len(tab)):
        p = api.TemporalParams.make(w, h)
        fs = api._temporal_struct(api.TemporalFrame, api.TEMPORAL_FRAME, {n: a.ctypes.data for n, a in f1.items() if instance or n != "instance"}, "frame")
        gs = api._temporal_struct(api.TemporalGuides, api.TEMPORAL_GUIDES, {n: f0[n].ctypes.data for n in tm.GUIDE_NAMES if instance or n != "instance"},
                                  "previous guide")
        hi = api._temporal_struct(api.TemporalHistory, api.TEMPORAL_HISTORY, {n: a.ctypes.data for n, a in hist0.items()}, "history")
        ho = api._temporal_struct(api.TemporalHistory, api.TEMPORAL_HISTORY, {n: a.ctypes.data for n, a in out.items()}, "history")
        return fn(gpu_ctx._h, C.addressof(p), C.addressof(cams[0]), C.addressof(cams[1]), C.addressof(fs), C.addressof(gs), C.addressof(hi), C.addressof(ho),
                  vout.ctypes.data, C.addressof(tab) if motion else None, n_motion)

    def vectors(fn, cam=True, cam_prev=True, depth=True, instance=True, motion=True, n_motion=len(tab), motion_out=True, size=(w, h)):
        return fn(gpu_ctx._h, size[0], size[1], C.addressof(cams[0]) if cam else None, C.addressof(cams[1]) if cam_prev else None,
                  f1["depth"].ctypes.data if depth else None, f1["instance"].ctypes.data if instance else None, C.addressof(tab) if motion else None,
                  n_motion, mv.ctypes.data if motion_out else None, wq.ctypes.data)
    for fn in (L.pbrs_temporal_accumulate_motion, L.pbrs_temporal_accumulate_motion_device):  # (the device variant refuses before it touches a pointer)
        assert accumulate(fn, instance=False) == -1
        assert b"instance" in L.pbrs_last_error(gpu_ctx._h)
        assert accumulate(fn, n_motion=0) == -1 and accumulate(fn, motion=False) == -1
        assert accumulate(fn, n_motion=(1 << 24) + 1) == -4  # PBRS_E_LIMIT
    for fn in (L.pbrs_motion_vectors, L.pbrs_motion_vectors_device):
        assert vectors(fn, motion_out=False) == -1 and vectors(fn, cam=False) == -1 and vectors(fn, cam_prev=False) == -1 and vectors(fn, depth=False) == -1
        assert vectors(fn, instance=False) == -1 and vectors(fn, n_motion=0) == -1 and vectors(fn, motion=False) == -1
        assert vectors(fn, size=(0, h)) == -1 and vectors(fn, size=(w + 1, h)) == -1
        assert vectors(fn, n_motion=(1 << 24) + 1) == -4
    other = pbrs_amd.HostScene(scenes.sphere_light_scene(width=16, height=16))
    with pytest.raises(ValueError, match="instances beside"):
        api.instance_motion(pbrs_amd.HostScene(mm.turned_short_box(0, 16)), other)
    # what is allowed, and still right after the refusals: the table, no table at all, a table on the first frame of a sequence
    assert accumulate(L.pbrs_temporal_accumulate_motion) == 0
    want, _ = mm.accumulate(f1["rgb"], f1["depth"], cam1, variance=f1["variance"], normal=f1["normal"], instance=f1["instance"], history=hist0,
                            prev={n: f0[n] for n in tm.GUIDE_NAMES}, cam_prev=cam0, motion=table)
    assert all(same(out[n], want[n]).all() for n in PLANES)
    assert accumulate(L.pbrs_temporal_accumulate_motion, motion=False, n_motion=0) == 0
    assert vectors(L.pbrs_motion_vectors) == 0 and same(mv, mm.motion_vectors(f1["depth"], cam1, cam0, f1["instance"], table)[0]).all()
    assert vectors(L.pbrs_motion_vectors, instance=False, motion=False, n_motion=0) == 0
    first, _ = gpu_ctx.temporal_accumulate(f0["rgb"], f0["depth"], cams[1], instance=f0["instance"], motion=tab)
    assert all(same(first[n], hist0[n]).all() for n in PLANES)
