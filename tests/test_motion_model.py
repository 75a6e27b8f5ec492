"""The CPU model of moving instances (tests/motion_model.py) against the properties the header states (include/pbrs_gpu.h, "moving
instances and motion vectors"): the call without motion, the sign convention of the records and of the vectors, f32 against float64,
and the error a table removes on a box that slides through the Cornell box."""
import numpy as np
import pytest

import motion_model as mm
import temporal_model as tm
from common import bits

f32 = np.float32
W, H = 130, 70
# Reprojection with the motion step in f32 against float64, measured over motion_sequence's tables on the 130 x 70 sequences below (seed 3,
# four frames, the moves of tm.MOVES): wq within 3.4e-7 relative, xq within 5.0e-5 and yq within 2.0e-5 of a pixel.  Four times that:
TOL_W, TOL_XY = 1.4e-6, 2.0e-4


def test_a_table_of_identity_records_is_the_call_without_a_table():
    for move in ("none", "yaw"):
        def flagged(*a, motion=None, **kw):
            table = None
            if motion is not None:
                table = dict(motion, flags=np.full_like(motion["flags"], mm.IDENTITY))  # (the garbage and the NaN stay where they are)
            return mm.accumulate(*a, motion=table, **kw)

        def plain(*a, motion=None, **kw):
            return tm.accumulate(*a, **kw)
        for id_test in (False, True):
            got = mm.run_sequence(flagged, W, H, 4, move, id_test=id_test)
            want = mm.run_sequence(plain, W, H, 4, move, id_test=id_test)
            moving = mm.run_sequence(mm.accumulate, W, H, 4, move, id_test=id_test)
            for (g, gv), (m, mv) in zip(got, want):
                assert all((bits(g[n]) == bits(m[n])).all() for n in g) and (bits(gv) == bits(mv)).all()
            assert any((bits(a[0]["rgb"]) != bits(b[0]["rgb"])).any() for a, b in zip(moving, want))  # the records do something


def _plane_frame(cam, z=4.0):
    d = tm.pixel_dirs(cam, np.float64)
    return ((z - float(cam.center[2])) / d[..., 2]).astype(f32)


@pytest.mark.parametrize("how", ("yaw", "translation"))
def test_a_world_that_moves_with_its_camera_has_zero_vectors(how):
    """cam = G . cam_prev and every instance's m = G^-1: the point stands where it stood on the previous film."""
    camp = tm.moved_camera(W, H, "none", 0)
    if how == "yaw":
        about = np.array([0.3, -0.2, 3.0])
        R = mm.rotation((0.0, 1.0, 0.0), 5.0)
        cam = tm.rotated(camp, 5.0, about=about)
        m, n = mm.rigid(R.T, about - R.T @ about)  # G x = about + R (x - about)
    else:
        t = np.array([0.4, -0.1, 0.25])
        cam = tm.Cam(np.asarray(camp.center, dtype=np.float64) + t, camp.c, camp.a, camp.b, W, H)
        m, n = mm.rigid(np.eye(3), -t)
    depth = _plane_frame(cam)
    inst = (np.arange(W * H).reshape(H, W) % 3).astype(np.uint32)
    mv, wq = mm.motion_vectors(depth, cam, camp, inst, mm.table_of([(m, n, 0)] * 3))
    print(f"{how}: largest |vector| {float(np.abs(mv).max()):.3g} px")
    assert np.abs(mv).max() <= TOL_XY and np.abs(wq / depth - 1.0).max() <= TOL_W
    still, _ = mm.motion_vectors(depth, cam, camp)
    assert np.abs(still).max() > 1.0  # without the table the camera's move is all there is


def test_a_translated_instance_has_vectors_that_point_back_along_its_motion():
    """Instance 1 moved by d along the film's x direction since the previous frame (m = translate(-d)), the camera stood still: its
    pixels' vectors point to -x, by d over the pixel's footprint at that depth; everything else keeps the static call's bits."""
    cam = tm.moved_camera(W, H, "none", 0)
    depth = _plane_frame(cam)
    inst = np.zeros((H, W), dtype=np.uint32)
    inst[20:50, 40:90] = 1
    right = tm._unit(cam.a)
    d = 0.25
    m, n = mm.rigid(np.eye(3), -d * right)
    table = mm.table_of([(np.eye(3, 4), np.eye(3), mm.IDENTITY), (m, n, 0)])
    mv, _ = mm.motion_vectors(depth, cam, cam, inst, table)
    still, _ = mm.motion_vectors(depth, cam, cam)
    on = inst == 1
    assert (bits(mv[~on]) == bits(still[~on])).all() and np.abs(still).max() <= TOL_XY
    want = -d / (depth[on].astype(np.float64) * float(np.linalg.norm(cam.a)))  # pixels: the film's step at distance z is |a| * z
    assert np.abs(mv[on][:, 0] - want).max() <= 2 * TOL_XY and (mv[on][:, 0] < -1.0).all()
    assert np.abs(mv[on][:, 1]).max() <= 2 * TOL_XY


def test_invalid_depths_and_points_behind_the_previous_camera_have_no_vector():
    cam = tm.moved_camera(W, H, "none", 0)
    depth = _plane_frame(cam)
    depth[0, 0], depth[1, 1], depth[2, 2], depth[3, 3] = 0.0, np.nan, np.inf, -1.0
    mv, wq = mm.motion_vectors(depth, cam, tm.rotated(cam, 180.0))
    assert (bits(mv) == 0).all() and np.isposinf(wq).all()
    mv, wq = mm.motion_vectors(depth, cam, tm.rotated(cam, 40.0))  # off the previous film, but in front of it: a vector all the same
    bad = np.zeros((H, W), dtype=bool)
    bad[[0, 1, 2, 3], [0, 1, 2, 3]] = True
    assert (bits(mv[bad]) == 0).all() and np.isposinf(wq[bad]).all() and np.isfinite(wq[~bad]).all() and (mv[~bad][:, 0] < -50.0).all() and (mv[~bad][:, 0] < -float(W)).any()


def test_reprojection_with_motion_agrees_with_float64():
    """wq within 1.4e-6 relative, xq and yq within 2.0e-4 of a pixel: four times the largest difference measured here (3.4e-7; 5.0e-5
    and 2.0e-5 of a pixel), the rule of test_temporal_model.py's check without motion."""
    worst, seen, applied = [0.0, 0.0, 0.0], 0, 0
    for move in tm.MOVES:
        frames = list(mm.motion_sequence(W, H, 3, move, 4))
        for (camp, _, _, _), (cam, frame, _, table) in zip(frames, frames[1:]):
            d, inst = frame["depth"], frame["instance"]
            lo, hi = mm.reproject(d, cam, camp, inst, table), mm.reproject(d, cam, camp, inst, table, np.float64)
            with np.errstate(all="ignore"):
                ok = np.isfinite(d) & (d > 0) & np.isfinite(hi[0]) & (hi[0] > 0) & (hi[1] > -1) & (hi[1] < W + 1) & (hi[2] > -1) & (hi[2] < H + 1)
            if move == "away":
                continue
            seen += int(ok.sum())
            applied += int((ok & mm._applies(inst, table)[0]).sum())
            errs = (np.abs(lo[0][ok] / hi[0][ok] - 1.0).max(), np.abs(lo[1][ok] - hi[1][ok]).max(), np.abs(lo[2][ok] - hi[2][ok]).max())
            worst = [max(a, float(b)) for a, b in zip(worst, errs)]
    print(f"f32 against float64 over {seen} reprojected pixels ({applied} through a record): wq {worst[0]:.3g} relative, xq {worst[1]:.3g}, "
          f"yq {worst[2]:.3g} pixels")
    assert seen > 50000 and applied > 20000
    assert worst[0] <= TOL_W and worst[1] <= TOL_XY and worst[2] <= TOL_XY


def test_the_sequences_hold_what_the_gpu_tests_need():
    """Every kind of record meets a pixel, ids reach past the table, and most pixels still find a history."""
    for move in ("none", "yaw"):
        frames = list(mm.motion_sequence(W, H, W + H, move))
        for _, frame, _, table in frames:
            ids = frame["instance"][frame["instance"] != tm.MISS]
            assert {3, 5, 9, 12} <= set(ids.tolist()) and ids.max() >= mm.N_MOTION
            assert table["flags"][5] == mm.IDENTITY and np.isnan(table["m"][5]).any() and np.isnan(table["m"][9]).any() and table["flags"][9] == 0
        last = mm.run_sequence(mm.accumulate, W, H, W + H, move, id_test=True)[-1][0]["length"]
        assert (last > 1.0).mean() > 0.5
        assert (last[frames[-1][1]["instance"] == 9] <= 1.0).all()  # the NaN record: no history


# ---- the sliding box ---------------------------------------------------------------------------------------------------------------------
SLIDE_FRAMES, SLIDE_DX = 8, -12.0


def sliding_box_scene(k, size=128):
    """The Cornell box with an 8 x 8 two-colour image checker on the short box (instance 8), which stands at x = 330 + SLIDE_DX * k."""
    from pbrs_amd import scenes
    from pbrs_amd.spec import SceneBuilder, Transform, deg
    sb = SceneBuilder()
    _, white, _ = scenes._cornell_shell(sb)
    img = np.zeros((8, 8, 3), f32)
    img[...] = (0.1, 0.1, 0.6)
    img[(np.add.outer(np.arange(8), np.arange(8)) & 1) == 1] = (0.8, 0.8, 0.2)
    short_xf = Transform().rotate_y(deg(15.0)).translate((330.0 + SLIDE_DX * k, 0.0, 105.0))
    tall_xf = Transform().rotate_y(deg(-18.0)).translate((130.0, 0.0, 225.0))
    sb.instance(scenes.box_mesh(sb, (0, 0, 0), (165, 165, 165)), sb.lambertian(sb.image(img)), short_xf)
    sb.instance(scenes.box_mesh(sb, (0, 0, 0), (165, 330, 165)), white, tall_xf)
    sb.set_camera(size, size, deg(65.0), (278, 278, 20), (278, 278, 555))
    return sb


def slide_table(n=10):
    """The short box was SLIDE_DX further back along x one frame ago; every other instance stands still."""
    m, nn = mm.rigid(np.eye(3), (-SLIDE_DX, 0.0, 0.0))
    return mm.table_of([(m, nn, 0) if i == 8 else (np.eye(3, 4), np.eye(3), mm.IDENTITY) for i in range(n)])


def test_a_table_removes_the_error_of_a_sliding_box():
    """The oracle's renders (128 x 128, 2 x 2 strata, seeds 17 .. 24) and its first hits at the pixel centres in the place of the depth
    and instance AOVs, the depth and id tests on.  On the moving box's pixels: accumulated with the table < single frame < accumulated
    without it; the static pixels keep their bits.  The reference is the last frame at 8 x 8 strata (seed 4242), not the 32 x 32 of
    DESIGN.md's figures (1.686 / 2.771 / 9.358), to keep this test within seconds: its own noise (about 4 / 64 of the single frame's
    error) adds the same amount to all three, and the order holds with room: measured here 1.849 / 2.909 / 9.435."""
    from oracle import binding
    S = 128
    cam = tm.look_at(S, S, 65.0, (278, 278, 20), (278, 278, 555))
    dirs = tm.pixel_dirs(cam).reshape(-1, 3).astype(f32)
    org = np.broadcast_to(np.asarray(cam.center, f32), dirs.shape).copy()
    frames = []
    for k in range(SLIDE_FRAMES):
        osc = binding.OracleScene(sliding_box_scene(k))
        hits, _, _ = osc.intersect(org, dirs, np.full(len(dirs), np.inf, f32), closest=True, anyhit=False)
        inst = np.asarray(hits["inst"]).reshape(S, S).astype(np.uint32)
        depth = np.where(inst != tm.MISS, np.asarray(hits["t"], f32).reshape(S, S), np.inf).astype(f32)
        out = osc.render(2, 2, 5, 17 + k)
        frames.append((np.asarray(out[0] if isinstance(out, tuple) else out, f32).reshape(S, S, 3), depth, inst))
    out = osc.render(8, 8, 5, 4242)
    ref = np.asarray(out[0] if isinstance(out, tuple) else out, f32).reshape(S, S, 3)
    res = {}
    for table in (None, slide_table()):
        hist = prev = None
        for k, (rgb, depth, inst) in enumerate(frames):
            hist, _ = mm.accumulate(rgb, depth, cam, instance=inst, history=hist, prev=prev, cam_prev=cam if k else None, id_test=True,
                                    motion=table if k else None)
            prev = {"depth": depth, "instance": inst}
        res[table is not None] = hist
    rgb, depth, inst = frames[-1]
    ok = np.isfinite(ref).all(2) & np.isfinite(rgb).all(2) & np.isfinite(res[False]["rgb"]).all(2) & np.isfinite(res[True]["rgb"]).all(2)
    box = (inst == 8) & ok

    def mse(a):
        return float(((a[box].astype(np.float64) - ref[box]) ** 2).mean())
    e_with, e_single, e_without = mse(res[True]["rgb"]), mse(rgb), mse(res[False]["rgb"])
    share = float((res[True]["length"][box] > 1.0).mean())
    print(f"{int(box.sum())} pixels of the sliding box: MSE with the table {e_with:.4g}, single frame {e_single:.4g}, without the table {e_without:.4g}; "
          f"{share:.3f} carry a history")
    assert box.sum() > 500 and share > 0.9
    assert e_with < e_single < e_without
    assert all((bits(res[True][n][inst != 8]) == bits(res[False][n][inst != 8])).all() for n in res[True])
