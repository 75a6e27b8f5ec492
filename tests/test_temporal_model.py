"""The CPU model of temporal accumulation (tests/temporal_model.py) against the properties the header states (include/pbrs_gpu.h,
"temporal accumulation"), and the synthetic sequences of tests/test_gpu_temporal.py against what those tests need from them."""
import numpy as np
import pytest

import temporal_model as tm
from common import bits
from denoise_var_model import lum

f32 = np.float32
W, H = 130, 70
# Reprojection in f32 against float64, measured over the moves of tm.MOVES on the 130 x 70 sequences below (seed 3, four frames): wq
# within 3.1e-7 relative, xq within 4.9e-5 and yq within 1.9e-5 of a pixel.  Four times that for other inputs:
TOL_W, TOL_XY = 1.3e-6, 2.0e-4


def test_the_first_frame_is_rule_c_everywhere():
    cam, frame, _ = next(tm.synthetic_sequence(W, H, 1, "none"))
    hist, vout = tm.accumulate(frame["rgb"], frame["depth"], cam, variance=frame["variance"], normal=frame["normal"], instance=frame["instance"])
    fin = np.isfinite(frame["rgb"]).all(axis=2)
    assert not fin.all()
    y = lum(frame["rgb"])
    assert (bits(hist["rgb"]) == bits(frame["rgb"])).all()
    assert (bits(hist["moments"][fin]) == bits(np.stack([y, (y * y).astype(f32)], axis=2)[fin])).all()
    assert (hist["length"][fin] == 1.0).all()
    # rule A, and rule D below min_temporal: the variance AOV, +inf where it is NaN, negative or +inf
    assert (bits(hist["moments"][~fin]) == 0).all() and (bits(hist["length"][~fin]) == 0).all() and np.isposinf(vout[~fin]).all()
    v = frame["variance"]
    known = fin & np.isfinite(v) & (v >= 0)
    assert (bits(vout[known]) == bits(v[known])).all() and np.isposinf(vout[~known]).all() and (~known & fin).sum() >= 3


@pytest.mark.parametrize("move", ("none", "pan", "yaw"))
def test_a_nan_is_visible_in_its_frame_and_in_no_pixel_of_the_next(move):
    frames = list(tm.synthetic_sequence(W, H, 2, move))
    results = tm.run_sequence(tm.accumulate, W, H, 2, move)
    for (cam, frame, _), (hist, vout) in zip(frames, results):
        bad = ~np.isfinite(frame["rgb"]).all(axis=2)
        assert bad.sum() == 2
        assert (~np.isfinite(hist["rgb"]).all(axis=2) == bad).all()   # this frame's, and nothing of the previous frame's or planted
        assert np.isfinite(hist["moments"]).all() and np.isfinite(hist["length"]).all()
        assert not np.isnan(vout).any()


def _scaled_step(a, b):
    def step(rgb, depth, cam, variance=None, history=None, **kw):
        if history is not None:
            history = dict(history)  # (what the sequence plants is scale-free: 0, NaN, inf)
        return tm.accumulate((rgb * a).astype(f32), depth, cam, variance=(variance * b).astype(f32), history=history, **kw)
    return step


@pytest.mark.parametrize("move", ("none", "yaw"))
def test_the_result_scales_with_the_scene_exactly(move):
    base = tm.run_sequence(tm.accumulate, 56, 44, 5, move, frames=5, min_temporal=3.0)
    assert any((h["length"] >= 3.0).any() for h, _ in base)  # both branches of rule D
    for j in (-6, 6):
        a, b = f32(2.0 ** j), f32(4.0 ** j)
        scaled = tm.run_sequence(_scaled_step(a, b), 56, 44, 5, move, frames=5, min_temporal=3.0)
        for (h0, v0), (h1, v1) in zip(base, scaled):
            assert (bits(h1["rgb"]) == bits((h0["rgb"] * a).astype(f32))).all(), j
            assert (bits(h1["moments"]) == bits((h0["moments"] * np.array([a, b], dtype=f32)).astype(f32))).all(), j
            assert (bits(h1["length"]) == bits(h0["length"])).all(), j
            assert (bits(v1) == bits((v0 * b).astype(f32))).all(), j


def test_the_length_saturates_at_max_history():
    results = tm.run_sequence(tm.accumulate, 40, 30, 4, "none", frames=7, max_history=4.0)
    for k, (hist, _) in enumerate(results):
        assert hist["length"].max() <= 4.0
        assert (hist["length"].max() == 4.0) == (k >= 3)
    assert (results[-1][0]["length"] == 4.0).mean() > 0.9


def test_reprojection_agrees_with_float64():
    """wq within 1.3e-6 relative, xq and yq within 2.0e-4 of a pixel: four times the largest difference measured here over the five
    moves (3.1e-7; 4.9e-5 and 1.9e-5 of a pixel)."""
    worst, seen = [0.0, 0.0, 0.0], 0
    for move in tm.MOVES:
        frames = list(tm.synthetic_sequence(W, H, 3, move, 4))
        for (camp, _, _), (cam, frame, _) in zip(frames, frames[1:]):
            d = frame["depth"]
            lo, hi = tm.reproject(d, cam, camp), tm.reproject(d, cam, camp, np.float64)
            with np.errstate(all="ignore"):
                ok = np.isfinite(d) & (d > 0) & np.isfinite(hi[0]) & (hi[0] > 0) & (hi[1] > -1) & (hi[1] < W + 1) & (hi[2] > -1) & (hi[2] < H + 1)
            if move == "away":
                assert not ok.any()  # every pixel lies behind the previous camera, or sees nothing
                continue
            seen += int(ok.sum())
            errs = (np.abs(lo[0][ok] / hi[0][ok] - 1.0).max(), np.abs(lo[1][ok] - hi[1][ok]).max(), np.abs(lo[2][ok] - hi[2][ok]).max())
            worst = [max(a, float(b)) for a, b in zip(worst, errs)]
    print(f"f32 against float64 over {seen} reprojected pixels: wq {worst[0]:.3g} relative, xq {worst[1]:.3g}, yq {worst[2]:.3g} pixels")
    assert seen > 50000
    assert worst[0] <= TOL_W and worst[1] <= TOL_XY and worst[2] <= TOL_XY


@pytest.mark.parametrize("id_test", (False, True))
def test_a_static_camera_keeps_its_history(id_test):
    """After k frames at least 90 % of the hit pixels have length k (the rest: neighbours of the depth step, which reprojection
    rounding may reject, and of what the sequence plants)."""
    frames = list(tm.synthetic_sequence(W, H, 6, "none", 4))
    results = tm.run_sequence(tm.accumulate, W, H, 6, "none", frames=4, id_test=id_test)
    for k, ((_, frame, _), (hist, _)) in enumerate(zip(frames, results), 1):
        hit = np.isfinite(frame["depth"]) & (frame["depth"] > 0)
        share = float((hist["length"][hit] == k).mean())
        assert share >= 0.9, (k, share)


def test_every_move_of_the_sequences_does_what_it_is_for():
    """What tests/test_gpu_temporal.py relies on: histories survive the small moves, a yaw disoccludes, `away` rejects everything."""
    for move in tm.MOVES:
        det = {}

        def step(*a, **kw):
            return tm.accumulate(*a, details=det, **kw)
        results = tm.run_sequence(step, W, H, 3, move)
        last = results[-1][0]["length"]
        if move == "away":
            assert (last <= 1.0).all()
        else:
            assert (last > 1.0).mean() > 0.5, move
            assert np.isinf(results[-1][1]).any() and np.isfinite(results[-1][1]).any()
        if move == "yaw":
            assert det["rejected"].any(), move
