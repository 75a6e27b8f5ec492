"""The CPU model of history clipping (tests/history_clip_model.py) against the properties the header states (include/pbrs_gpu.h,
"history clipping"), the synthetic sequences of tests/test_gpu_history_clip.py against what that test needs from them, and what the
rule is for: a step in the lighting under a static camera."""
import itertools

import numpy as np
import pytest

import history_clip_model as hc
import motion_model as mm
import temporal_model as tm
from common import bits

f32 = np.float32
PLANES = ("rgb", "moments", "length")
NO_CLIP = dict(radius=2, gamma=2.0 ** 60, clip_history=None)  # a box no colour of these sequences leaves


def same_results(a, b):
    return all((bits(a[0][n]) == bits(b[0][n])).all() for n in PLANES) and (a[1] is None) == (b[1] is None) and \
        (a[1] is None or (bits(a[1]) == bits(b[1])).all())


@pytest.mark.parametrize("move", ("none", "pan", "yaw"))
@pytest.mark.parametrize("with_table", (False, True))
def test_a_box_that_clips_nothing_gives_the_unclipped_result_bit_for_bit(move, with_table):
    """This file's pass through rules A to D is motion_model's (and temporal_model's)."""
    kw = dict(frames=4, with_table=with_table, id_test=True)
    wide = hc.run_sequence(hc.accumulate, 56, 44, 5, move, clip=NO_CLIP, **kw)
    none = hc.run_sequence(hc.accumulate, 56, 44, 5, move, clip=None, **kw)
    plain = (mm.run_sequence(mm.accumulate, 56, 44, 5, move, frames=4, id_test=True) if with_table else
             tm.run_sequence(tm.accumulate, 56, 44, 5, move, frames=4, id_test=True))
    for k, (a, b, c) in enumerate(zip(wide, none, plain)):
        assert same_results(a, c) and same_results(b, c), k
    assert wide[-1][2]["has"].sum() > 1000 and not wide[-1][2]["clipped"].any()


def _scaled_step(a, b):
    def step(rgb, depth, cam, variance=None, history=None, **kw):
        return hc.accumulate((rgb * a).astype(f32), depth, cam, variance=(variance * b).astype(f32), history=history, **kw)
    return step


@pytest.mark.parametrize("radius", (1, 3))
def test_the_result_scales_with_the_scene_exactly(radius):
    """j = +-6 on colours of order 1: no sum or product here comes near the proviso's limits."""
    clip = dict(radius=radius, gamma=1.0, clip_history=2.0)
    kw = dict(frames=5, min_temporal=3.0, clip=clip)
    base = hc.run_sequence(hc.accumulate, 56, 44, 5, "yaw", **kw)
    assert base[-1][2]["clipped"].sum() > 100 and (base[-1][2]["has"] & ~base[-1][2]["clipped"]).sum() > 100
    assert any((h["length"] >= 3.0).any() for h, _, _ in base)
    for j in (-6, 6):
        a, b = f32(2.0 ** j), f32(4.0 ** j)
        scaled = hc.run_sequence(_scaled_step(a, b), 56, 44, 5, "yaw", **kw)
        for (h0, v0, _), (h1, v1, _) in zip(base, scaled):
            assert (bits(h1["rgb"]) == bits((h0["rgb"] * a).astype(f32))).all(), j
            assert (bits(h1["moments"]) == bits((h0["moments"] * np.array([a, b], dtype=f32)).astype(f32))).all(), j
            assert (bits(h1["length"]) == bits(h0["length"])).all(), j
            assert (bits(v1) == bits((v0 * b).astype(f32))).all(), j


def test_a_non_finite_neighbour_is_skipped():
    rng = np.random.default_rng(3)
    rgb = rng.uniform(0.2, 1.0, size=(9, 11, 3)).astype(f32)
    holed = rgb.copy()
    holed[4, 5, 1] = np.nan
    holed[2, 2] = np.inf
    det = {}
    lo, hi = hc.box(holed, 1, 1.5, det)
    assert det["cnt"][4, 4] == 8.0 and det["skipped"][4, 4] == 1 and det["cnt"][0, 0] == 4.0 and det["skipped"][0, 0] == 0
    assert det["cnt"][3, 3] == 8.0 and det["cnt"][6, 8] == 9.0
    # the same numbers as the window's finite pixels summed in the header's order by hand
    taps = [holed[4 + dy, 4 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 1)]
    s1, s2 = np.zeros(3, f32), np.zeros(3, f32)
    for c in taps:
        s1, s2 = (s1 + c).astype(f32), (s2 + (c * c).astype(f32)).astype(f32)
    ic = f32(1.0) / f32(8.0)
    mu = (s1 * ic).astype(f32)
    sd = np.sqrt(np.maximum((s2 * ic).astype(f32) - (mu * mu).astype(f32), f32(0.0))).astype(f32)
    assert (bits(lo[4, 4]) == bits((mu - (f32(1.5) * sd).astype(f32)).astype(f32))).all()
    assert (bits(hi[4, 4]) == bits((mu + (f32(1.5) * sd).astype(f32)).astype(f32))).all()
    assert np.isfinite(lo[np.isfinite(holed).all(axis=2)]).all()
    # an overflowed sum gives a NaN bound, and a NaN bound clips nothing
    big = np.full((3, 3, 3), 3e38, dtype=f32)
    lo, hi = hc.box(big, 1, 1.0)
    assert np.isnan(lo[1, 1]).all()
    H = np.full((3, 3, 3), 7.0, dtype=f32)
    one = np.ones((3, 3), f32)
    Hc, h1, h2, n, changed = hc.clip_history(H, one, one, one, lo, hi, f32(1.0))
    assert (bits(Hc) == bits(H)).all() and not changed.any()


def test_a_window_that_holds_the_pixel_alone_clips_the_history_to_the_pixel():
    """A 1 x 1 image, and a pixel whose neighbours are all non-finite: sd = 0, lo = hi = cur, and the blend of rule C gives cur."""
    cam = tm.moved_camera(1, 1, "none", 0)
    rgb = np.array([[[0.25, 0.5, 0.75]]], dtype=f32)
    depth = np.full((1, 1), 4.0, dtype=f32)
    history = {"rgb": np.array([[[3.0, 0.01, 0.75]]], dtype=f32), "moments": np.array([[[1.0, 1.5]]], dtype=f32), "length": np.full((1, 1), 6.0, dtype=f32)}
    det = {}
    lo, hi = hc.box(rgb, 3, 2.0, det)
    assert det["cnt"][0, 0] == 1.0 and (bits(det["sd"]) == 0).all() and (bits(lo) == bits(rgb)).all() and (bits(hi) == bits(rgb)).all()
    got, _ = hc.accumulate(rgb, depth, cam, history=history, prev={"depth": depth}, cam_prev=cam, clip=dict(radius=3, gamma=2.0, clip_history=2.0), details=det)
    assert det["clipped"].all()
    assert (bits(got["rgb"]) == bits(rgb)).all()
    assert got["length"][0, 0] == 3.0  # min(6, clip_history) + 1
    y = hc.lum(rgb)[0, 0]
    # the mean moved to lum(cur), the spread (1.5 - 1.0 * 1.0) stayed: m1 = y, m2 = (0.5 + y * y) + (y * y - (0.5 + y * y)) / 3
    h2 = f32(0.5) + y * y
    assert bits(got["moments"][0, 0, 0]) == bits(y) and bits(got["moments"][0, 0, 1]) == bits(f32(h2 + (f32(1.0) / f32(3.0)) * (y * y - h2)))
    unclipped, _ = hc.accumulate(rgb, depth, cam, history=history, prev={"depth": depth}, cam_prev=cam, clip=None)
    assert unclipped["length"][0, 0] == 7.0 and abs(unclipped["rgb"][0, 0, 0] - 3.0) < 0.5
    # in a larger image: the neighbours of (2, 2) are all non-finite
    rgb = np.full((5, 5, 3), np.nan, dtype=f32)
    rgb[2, 2] = (0.3, 0.6, 0.9)
    lo, hi = hc.box(rgb, 1, 1.0, det)
    assert det["cnt"][2, 2] == 1.0 and det["skipped"][2, 2] == 8 and (bits(lo[2, 2]) == bits(rgb[2, 2])).all() and (bits(hi[2, 2]) == bits(rgb[2, 2])).all()


@pytest.mark.parametrize("move", ("pan", "yaw"))
def test_the_gpu_tests_sequences_clip_some_pixels_spare_others_and_skip_taps(move):
    """What tests/test_gpu_history_clip.py asserts of its largest size, on the model alone."""
    for radius in (1, 2, 3):
        res = hc.run_sequence(hc.accumulate, 130, 70, 200, move, clip=dict(radius=radius, gamma=1.0, clip_history=2.0))
        det = res[-1][2]
        assert det["clipped"].sum() > 100 and (det["has"] & ~det["clipped"]).sum() > 100 and det["skipped"].sum() >= 1, (move, radius)
        assert (res[-1][0]["length"][det["clipped"]] <= 3.0).all() and (res[-1][0]["length"] > 3.0).sum() == 0


def _step_sequence(noise, clip, w=48, h=24, before=8, after=4, seed=1):
    """Level 1.0 for `before` frames, then the right half at 0.2 for `after` frames, under multiplicative noise of standard deviation
    `noise` (uniform); a static camera over a wall at depth 4 -> (the last accumulated image, the last frame's truth)."""
    cam = tm.moved_camera(w, h, "none", 0)
    depth = np.full((h, w), 4.0, dtype=f32)
    tint = np.array([1.0, 0.8, 0.6])
    rng = np.random.default_rng(seed)
    history = truth = None
    for k in range(before + after):
        level = np.ones((h, w))
        if k >= before:
            level[:, w // 2:] = 0.2
        truth = level[..., None] * tint
        rgb = (truth * (1.0 + noise * rng.uniform(-np.sqrt(3.0), np.sqrt(3.0), size=(h, w, 3)))).astype(f32)
        history, _ = hc.accumulate(rgb, depth, cam, history=history, prev={"depth": depth}, cam_prev=cam, want_variance=False, clip=clip)
    return history["rgb"], truth


def test_the_clip_removes_the_lag_behind_a_step_in_the_lighting():
    """Eight frames at level 1.0, then four in which half the image drops to 0.2 (max_history 32: the running mean still holds 8 / 12 of
    the old level).  Mean absolute error four frames after the step, clipped over unclipped: at most 0.5 in the half that changed and at
    most 1.05 in the half that did not, `radius` columns at the seam left out, for noise 0.1 and 0.5, gamma 1 and 2, radius 1 and 3."""
    w = 48
    for noise in (0.1, 0.5):
        plain, truth = _step_sequence(noise, None)
        for gamma, radius in itertools.product((1.0, 2.0), (1, 3)):
            clipped, _ = _step_sequence(noise, dict(radius=radius, gamma=gamma))
            changed, unchanged = np.s_[:, w // 2 + radius:], np.s_[:, :w // 2 - radius]

            def err(img, where):
                return float(np.abs(img[where].astype(np.float64) - truth[where]).mean())
            r_changed, r_unchanged = err(clipped, changed) / err(plain, changed), err(clipped, unchanged) / err(plain, unchanged)
            print(f"noise {noise} gamma {gamma} radius {radius}: changed half {err(clipped, changed):.4f} / {err(plain, changed):.4f} = {r_changed:.3f}, "
                  f"unchanged half {err(clipped, unchanged):.4f} / {err(plain, unchanged):.4f} = {r_unchanged:.3f}")
            assert r_changed <= 0.5, (noise, gamma, radius, r_changed)
            assert r_unchanged <= 1.05, (noise, gamma, radius, r_unchanged)
