"""The CPU model of the spatial variance estimate (tests/spatial_variance_model.py) against what the header states (include/pbrs_gpu.h,
"spatial variance estimate for short histories"): the pass-through cases, the scale rule, what a constant image, a non-finite
neighbour and a guide edge do, what the estimator estimates, and the error it removes from the filtered image of a short sequence."""
import numpy as np
import pytest

import denoise_model as dm
import denoise_var_model as dvm
import spatial_variance_model as sv
import temporal_model as tm
from common import bits

f32 = np.float32
W, H = 130, 70


def _inputs(move="yaw", frames=3):
    return sv.sequence_inputs(W, H, W + H, move, frames)


def test_the_sequences_hold_what_the_tests_need():
    """Long, short, zero and NaN lengths, non-finite moments, and known and unknown variances among the short pixels."""
    inp = _inputs()
    n = inp["length"]
    short4, short25 = sv.short_pixels(n, 4.0), sv.short_pixels(n, 2.5)
    assert (n == 0).any() and np.isnan(n).any() and (~np.isfinite(inp["moments"])).any()
    assert 0 < short25.sum() < short4.sum() < n.size and (n[~short25 & np.isfinite(n)] > 2.5).any()
    assert sv.known(inp["variance"])[short4].any() and (~sv.known(inp["variance"]))[short4].any()
    assert (sv.short_pixels(_inputs("away")["length"], 2.5) | (_inputs("away")["length"] == 0) | np.isnan(_inputs("away")["length"])).all()


@pytest.mark.parametrize("min_temporal", (2.5, 4.0))
def test_pixels_that_are_not_short_pass_through_bit_for_bit(min_temporal):
    inp = _inputs(frames=5)  # lengths up to 5: long histories at either min_temporal
    v = inp["variance"].copy()
    v.view(np.uint32)[3, 5] = 0x7FC12345  # a NaN with a payload, under a long, a zero and a NaN length
    long_at = np.argwhere(inp["length"] >= 4.0)[7]
    zero_at, nan_at = np.argwhere(inp["length"] == 0)[0], np.argwhere(np.isnan(inp["length"]))[0]
    for at in (long_at, zero_at, nan_at):
        v.view(np.uint32)[tuple(at)] = 0x7FC12345
    inp["variance"] = v
    det = {}
    out = sv.spatial_variance(**inp, min_temporal=min_temporal, id_stop=True, details=det)
    short = sv.short_pixels(inp["length"], min_temporal)
    assert (bits(out[~short]) == bits(v[~short])).all()
    assert all(bits(out)[tuple(at)] == 0x7FC12345 for at in (long_at, zero_at, nan_at))
    assert det["estimated"].sum() > 0 and not (det["estimated"] & ~short).any()
    assert (bits(out[det["estimated"]]) != bits(v[det["estimated"]])).any()
    # a short pixel whose W is 0 (its own depth is NaN or 0: every tap's weight is NaN) passes through as well
    through = short & ~det["estimated"]
    assert through.any() and (bits(out[through]) == bits(v[through])).all() and (det["W"][through] == 0).all()


def test_only_unknown_keeps_the_known_variances_of_short_pixels():
    inp = _inputs()
    every = sv.spatial_variance(**inp, id_stop=True)
    det = {}
    some = sv.spatial_variance(**inp, id_stop=True, only_unknown=True, details=det)
    short, known = sv.short_pixels(inp["length"], 4.0), sv.known(inp["variance"])
    keep = short & known
    assert keep.any() and (bits(some[keep]) == bits(inp["variance"][keep])).all() and (bits(every[keep]) != bits(some[keep])).any()
    assert (bits(some[~keep]) == bits(every[~keep])).all() and det["estimated"].any()
    # -inf, a negative value and a NaN are unknown, +0 is known
    v = np.array([[-np.inf, -1.0, np.nan, 0.0, np.inf, 3.0]], dtype=f32)
    assert sv.known(v).tolist() == [[False, False, False, True, False, True]]


@pytest.mark.parametrize("j", (-6, 6))
def test_the_scale_rule(j):
    for move in ("none", "yaw"):
        inp = _inputs(move)
        base = sv.spatial_variance(**inp, id_stop=True)
        s1, s2 = f32(2.0 ** j), f32(4.0 ** j)
        scaled = dict(inp, moments=(inp["moments"] * np.array([s1, s2], dtype=f32)).astype(f32), variance=(inp["variance"] * s2).astype(f32))
        got = sv.spatial_variance(**scaled, id_stop=True)
        assert (bits(got) == bits((base * s2).astype(f32))).all()


def test_a_constant_image_has_no_variance():
    """Exactly +0 where the sums are exact: luminances 0.75, 2 and 17 (k * c and k * c * c are f32 for every tap count k of the 7 x 7
    window and its clipped forms), no guides.  In general b and a * a round separately and a constant image is only within an ulp of c * c
    of +0; the clamp catches the negative side."""
    for c in (0.75, 2.0, 17.0):
        c = f32(c)
        m = np.empty((20, 23, 2), f32)
        m[..., 0], m[..., 1] = c, c * c
        for radius in (1, 2, 3):
            out = sv.spatial_variance(m, np.ones((20, 23), f32), np.full((20, 23), np.inf, f32), radius=radius)
            assert (bits(out) == 0).all(), (c, radius)
    c = f32(0.3)
    m[..., 0], m[..., 1] = c, c * c
    out = sv.spatial_variance(m, np.ones((20, 23), f32), np.full((20, 23), np.inf, f32))
    assert (out >= 0).all() and out.max() <= np.spacing(c * c) * 2


def test_a_non_finite_neighbour_contaminates_nobody():
    rng = np.random.default_rng(3)
    y = rng.normal(2.0, 0.5, size=(24, 31)).astype(f32)
    m = np.stack([y, y * y], axis=2).astype(f32)
    n = np.ones((24, 31), f32)
    vin = np.full((24, 31), np.inf, f32)
    clean = sv.spatial_variance(m, n, vin)
    bad_m, bad_n = m.copy(), n.copy()
    bad_m[5, 5, 0], bad_m[9, 20, 1], bad_m[15, 3] = np.nan, np.inf, (-np.inf, np.nan)
    bad_n[12, 12], bad_n[20, 25] = 0.0, np.nan
    out = sv.spatial_variance(bad_m, bad_n, vin)
    spots = np.zeros((24, 31), dtype=bool)
    spots[[5, 9, 15, 12, 20], [5, 20, 3, 12, 25]] = True
    assert np.isfinite(clean).all()
    assert np.isfinite(out[~spots]).all()                      # nobody else is touched by them ...
    assert np.isfinite(out[5, 5]) and np.isfinite(out[9, 20])  # ... and a short pixel with a bad moment is estimated from its neighbours
    assert np.isposinf(out[12, 12]) and np.isposinf(out[20, 25])  # lengths 0 and NaN are not short: variance_in
    far = np.ones((24, 31), dtype=bool)
    for yy, xx in np.argwhere(spots):
        far[max(0, yy - 3):yy + 4, max(0, xx - 3):xx + 4] = False
    assert far.any() and (bits(out[far]) == bits(clean[far])).all()


@pytest.mark.parametrize("edge", ("id", "depth"))
def test_an_edge_in_the_guides_cuts_the_window(edge):
    """A step in the moments along a guide edge: the estimate beside it equals the estimate with the other side removed (length 0)."""
    rng = np.random.default_rng(4)
    h, w = 20, 26
    y = rng.normal(2.0, 0.5, size=(h, w)).astype(f32)
    y[:, 13:] += f32(40.0)
    m = np.stack([y, y * y], axis=2).astype(f32)
    n = np.ones((h, w), f32)
    vin = np.full((h, w), np.inf, f32)
    left = np.zeros((h, w), dtype=bool)
    left[:, :13] = True
    if edge == "id":
        guides = dict(instance=np.where(left, 3, 8).astype(np.uint32), id_stop=True)
    else:
        guides = dict(depth=np.where(left, f32(2.0), f32(np.inf)).astype(f32))
    out = sv.spatial_variance(m, n, vin, **guides)
    alone = sv.spatial_variance(m, np.where(left, n, 0).astype(f32), vin)  # no guide, the right side does not count
    blind = sv.spatial_variance(m, n, vin)
    assert (bits(out[left]) == bits(alone[left])).all()
    assert (blind[:, 10:13] > 50.0).all() and (out[:, 10:13] < 1.0).all()  # without the guide the step is counted as variance


def test_the_estimator_on_flat_noise():
    """64 x 64 of N(2, 0.5^2) luminance, length 1, no guides, radius 3: the mean estimate over the pixels at least 3 from the border
    is within 10 % of 0.25 * 48 / 49 (the window's own mean is subtracted).  About 69 independent windows at 20 % each: a standard error
    of about 2.4 %."""
    y = np.random.default_rng(5).normal(2.0, 0.5, size=(64, 64)).astype(f32)
    m = np.stack([y, y * y], axis=2).astype(f32)
    out = sv.spatial_variance(m, np.ones((64, 64), f32), np.full((64, 64), np.inf, f32))
    got, want = float(out[3:-3, 3:-3].astype(np.float64).mean()), 0.25 * 48.0 / 49.0
    print(f"mean estimate {got:.5f}, expected {want:.5f}, ratio {got / want:.4f}")
    assert abs(got / want - 1.0) < 0.10
    # a history of 3 frames divides it by 3
    out3 = sv.spatial_variance(m, np.full((64, 64), 3.0, f32), np.full((64, 64), np.inf, f32))
    assert (bits(out3) == bits((out * (f32(1.0) / f32(3.0))).astype(f32))).all()


def test_the_estimate_removes_error_from_the_filtered_image_of_a_short_sequence():
    """The sliding-box scene of test_motion_model.py at rest (128 x 128, depth 5, 1 x 1 strata, seeds 17, 18, 19: the variance AOV is
    +inf everywhere), the oracle's first hits at the pixel centres in the place of the depth and instance AOVs, no normal guide, the id
    test and the id stop on, denoise_var's defaults (5 iterations, sigma_l 4, sigma_d 0.2).  After frames 1 and 3: the accumulated image
    filtered with the variance unknown against the same filtered with the spatial estimate.  The reference is the scene at 8 x 8 strata
    (seed 4242), not the 16 x 16 of DESIGN.md's figures (0.7917 / 2.232 at frame 1, 0.5388 / 2.234 at frame 3; ratios 0.355 and 0.241), to
    keep this test within seconds, as test_motion_model.py does: its own noise adds the same amount to both sides.  Measured here with the
    8 x 8 reference: frame 1 0.9603 / 2.395 (0.401), frame 3 0.7077 / 2.397 (0.295); on the box's 1104 pixels 5.841 / 10.98 and 3.530 / 10.98."""
    from oracle import binding
    from test_motion_model import sliding_box_scene
    S = 128
    cam = tm.look_at(S, S, 65.0, (278, 278, 20), (278, 278, 555))
    dirs = tm.pixel_dirs(cam).reshape(-1, 3).astype(f32)
    org = np.broadcast_to(np.asarray(cam.center, f32), dirs.shape).copy()
    osc = binding.OracleScene(sliding_box_scene(0))
    hits, _, _ = osc.intersect(org, dirs, np.full(len(dirs), np.inf, f32), closest=True, anyhit=False)
    inst = np.asarray(hits["inst"]).reshape(S, S).astype(np.uint32)
    depth = np.where(inst != tm.MISS, np.asarray(hits["t"], f32).reshape(S, S), np.inf).astype(f32)

    def render(sx, seed):
        out = osc.render(sx, sx, 5, seed)
        return np.asarray(out[0] if isinstance(out, tuple) else out, f32).reshape(S, S, 3)
    ref = render(8, 4242)
    hist, prev, res = None, None, {}
    for k in range(3):
        rgb = render(1, 17 + k)
        hist, vout = tm.accumulate(rgb, depth, cam, instance=inst, history=hist, prev=prev, cam_prev=cam if k else None, id_test=True)
        prev = {"depth": depth, "instance": inst}
        if k in (0, 2):
            assert np.isposinf(vout[np.isfinite(hist["rgb"]).all(2)]).all()  # today's chain: nothing is known
            vest = sv.spatial_variance(hist["moments"], hist["length"], vout, depth=depth, instance=inst, id_stop=True)
            res[k] = tuple(dvm.denoise_var(hist["rgb"], v, 5, 4.0, 0.3, 0.2, flags=dm.ID_STOP, depth=depth, instance=inst)[0] for v in (vout, vest))
            res[k] += (hist["rgb"],)
    ok = np.isfinite(ref).all(2)
    for imgs in res.values():
        for img in imgs:
            ok &= np.isfinite(img).all(2)
    box = ok & (inst == 8)

    def mse(a, where):
        return float(((a[where].astype(np.float64) - ref[where]) ** 2).mean())
    assert box.sum() > 500
    for k, (without, with_estimate, acc) in res.items():
        e_a, e_0, e_1 = mse(acc, ok), mse(without, ok), mse(with_estimate, ok)
        b_a, b_0, b_1 = mse(acc, box), mse(without, box), mse(with_estimate, box)
        print(f"frame {k + 1}: accumulated {e_a:.4g}, filtered with the variance unknown {e_0:.4g}, with the spatial estimate {e_1:.4g} "
              f"(ratio {e_1 / e_0:.3f}); on the box's {int(box.sum())} pixels {b_a:.4g} / {b_0:.4g} / {b_1:.4g}")
        assert e_1 < 0.5 * e_0
        assert b_1 < b_0
