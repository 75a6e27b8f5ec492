"""The depth-of-field arithmetic of include/pbrs_gpu.h ("depth of field") on the CPU, through tests/dof_model.py, the numpy model that
follows the header's text: the four rules the header states, bit for bit; the two occlusion rules on two layers split at a column; the
error bound of a constant image; and api.lens against the formula worked by hand."""
import math

import numpy as np
import pytest

import dof_model as dm
from common import bits
from pbrs_amd import api

f32 = np.float32


def same(got, want, what=""):
    diff = bits(got) != bits(want)
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def noise(w, h, seed=3):
    rng = np.random.default_rng(seed)
    return np.exp2(rng.uniform(-4, 4, (h, w, 3))).astype(f32)


def ramp(w, h, lo=0.5, hi=4.0):
    """A depth that grows along x from lo to hi, the same in every row, with a few rows pulled near."""
    z = np.tile(np.linspace(lo, hi, w, dtype=f32), (h, 1))
    z[h // 3: h // 3 + 3, w // 4: w // 2] = f32(0.75 * lo)
    return z


W_, H_ = 41, 23
KW = dict(max_radius=6, focus=1.5, scale=5.0)


@pytest.fixture(scope="module")
def base():
    rgb, depth = noise(W_, H_), ramp(W_, H_)
    depth[2, 3], depth[H_ - 1, 0], depth[5, W_ - 2], depth[7, 7] = np.inf, 0.0, np.nan, -1.0
    rgb[4, 9] = (np.nan, 1.0, 1.0)
    rgb.flags.writeable = depth.flags.writeable = False
    res = dm.dof(rgb, depth, details=True, **KW)
    assert (res.n > 1).any() and (res.front > 0).any() and (res.partial > 0).any() and (res.r == f32(KW["max_radius"])).any()
    return rgb, depth, res


@pytest.mark.parametrize("j", (5, -5))
def test_rule_a_the_colours_scale(base, j):
    rgb, depth, res = base
    s = f32(2.0) ** j
    scaled = dm.dof(rgb * s, depth, details=True, **KW)
    same(scaled.out, res.out * s, "out")
    same(scaled.coc, res.coc, "coc")
    assert (scaled.n == res.n).all()


@pytest.mark.parametrize("j", (3, -4))
def test_rule_b_depth_and_focus_scale_together(base, j):
    rgb, depth, res = base
    s = f32(2.0) ** j
    scaled = dm.dof(rgb, depth * s, details=True, **{**KW, "focus": float(f32(KW["focus"]) * s)})
    same(scaled.out, res.out, "out")
    same(scaled.coc, res.coc, "coc")


def test_rule_c_small_circles_return_the_image():
    rgb, depth = noise(W_, H_), ramp(W_, H_, 1.0, 2.0)
    rgb[3, 3] = (np.inf, 0.0, -1.0)
    # focus 1.1: |z - F| / z is 0.467 on the near rows (z = 0.75) and at most 0.45 over the ramp: r <= 0.5 with scale 1
    res = dm.dof(rgb, depth, max_radius=16, focus=1.1, scale=1.0, details=True)
    assert res.r.max() <= f32(0.5) and res.r.max() > 0
    same(res.out, rgb)
    assert (res.n[np.isfinite(rgb).all(axis=2)] == 1).all()
    res = dm.dof(rgb, depth, max_radius=16, focus=1.1, scale=0.0, details=True)
    same(res.out, rgb)
    assert (bits(res.coc) == 0).all()


def test_rule_d_a_sharp_pixel_takes_nothing_from_pixels_at_or_behind_it():
    rgb = noise(W_, H_)
    depth = np.full((H_, W_), 4.0, f32)  # everything behind the focus, blurred by the full radius
    depth[10, 20] = 1.0                  # one pixel in focus
    depth[10, 22] = 1.0                  # and a second one at its depth: "at", not behind
    kw = dict(max_radius=8, focus=1.0, scale=40.0)
    res = dm.dof(rgb, depth, details=True, **kw)
    assert res.r[10, 20] == 0 and res.r[10, 21] == 8 and res.n[10, 20] == 1 and res.front[10, 20] == 0
    assert bits(res.out[10, 20]).tolist() == bits(rgb[10, 20]).tolist()
    other = rgb * f32(3.0)  # every other pixel's colour changes
    other[10, 20] = rgb[10, 20]
    again = dm.dof(other, depth, details=True, **kw)
    assert bits(again.out[10, 20]).tolist() == bits(rgb[10, 20]).tolist()
    # its blurred neighbours take from each other, and nothing from it: in front of them, it spreads by its own circle, which is 0
    assert res.front[10, 21] == 0 and res.n[10, 21] > 1


def layers(near_blurred):
    """Two layers split at column 24 of a 48 x 20 image: the left one near (depth 1), the right one far (depth 3).  The focus is on the
    far layer when the near one is to blur, and on the near one otherwise.  scale 12: the blurred layer's r is 8 (near, |1 - 3| / 1 = 2,
    clamped) or 8 (far, |3 - 1| / 3 * 12)."""
    w, h, split = 48, 20, 24
    depth = np.full((h, w), 3.0, f32)
    depth[:, :split] = 1.0
    kw = dict(max_radius=8, focus=3.0 if near_blurred else 1.0, scale=12.0)
    return noise(w, h, 9), depth, split, kw


def test_a_sharp_foreground_keeps_its_edge_against_a_blurred_background():
    rgb, depth, split, kw = layers(near_blurred=False)
    res = dm.dof(rgb, depth, details=True, **kw)
    assert (res.r[:, :split] == 0).all() and (res.r[:, split:] == 8).all()
    same(res.out[:, :split], rgb[:, :split], "the foreground")
    assert (bits(res.out[:, split:]) != bits(rgb[:, split:])).any()
    # the blurred background takes nothing from the sharp foreground either: its colours do not reach across the edge
    louder = rgb.copy()
    louder[:, :split] *= f32(5.0)
    again = dm.dof(louder, depth, **kw)
    same(again[:, split:], res.out[:, split:], "the background")


def test_a_blurred_foreground_spreads_over_a_sharp_background():
    rgb, depth, split, kw = layers(near_blurred=True)
    res = dm.dof(rgb, depth, details=True, **kw)
    assert (res.r[:, :split] == 8).all() and (res.r[:, split:] == 0).all()
    changed = (bits(res.out) != bits(rgb)).any(axis=2)
    # a background pixel at column x has the foreground's nearest column at distance x - split + 1: within the circle (8) it changes,
    # and cov = (8 - dist) + 0.5 > 0 reaches dist = 8 as well
    assert changed[:, split:split + 8].all()
    # further than max_radius from the edge it keeps its bits
    assert not changed[:, split + 8:].any() and split + 8 < rgb.shape[1]
    assert (res.front[:, split:split + 8] > 0).all() and (res.front[:, :split] == 0).all()


def test_a_constant_image_stays_within_the_sums_bound():
    w, h = 57, 31
    v = f32(0.7)
    rgb = np.full((h, w, 3), v, f32)
    depth = ramp(w, h, 0.4, 6.0)
    res = dm.dof(rgb, depth, max_radius=9, focus=1.3, scale=7.0, details=True)
    assert (res.n > 1).any() and res.n.max() > 100
    # a sequential sum of n positive terms, twice (acc and W), and a division: (2 n + 3) 2^-24 relative
    rel = np.abs(res.out.astype(np.float64) - float(v)).max(axis=2) / float(v)
    bound = (2.0 * res.n + 3.0) * 2.0 ** -24
    assert (rel <= bound).all(), (float(rel.max()), float(bound.max()))
    print(f"largest relative error {rel.max():.3g}, its bound {bound[np.unravel_index(rel.argmax(), rel.shape)]:.3g}")


def test_lens_against_the_formula_by_hand():
    # a camera that looks down -z from the origin: the image plane at distance 2, 64 pixels over a width of 2 (a step of 1 / 32)
    cam = api.Camera()
    cam.width, cam.height = 64, 32
    cam.center[:] = (0.0, 0.0, 0.0)
    cam.a[:] = (1.0 / 32.0, 0.0, 0.0)
    cam.b[:] = (0.0, -1.0 / 32.0, 0.0)
    cam.c[:] = (-1.0, 0.5, -2.0)
    got = api.lens(cam, 10.0, 0.25)
    # D = 2: focus = 10 / 2 = 5; one pixel on the plane of focus is 5 / 32; scale = 0.25 / (5 / 32) = 1.6
    assert got == {"focus": 5.0, "scale": float(f32(1.6))}
    half = api.lens(cam, 10.0, 0.125)
    assert half["focus"] == 5.0 and half["scale"] == float(f32(0.8)) and math.isclose(half["scale"] * 2, got["scale"], rel_tol=1e-7)
    assert api.lens(cam, 10.0, 0.0)["scale"] == 0.0
    # a tilted image plane: c along the axis n = (0, 0.6, -0.8) times 3 plus steps within the plane
    cam.a[:] = (0.01, 0.0, 0.0)
    cam.b[:] = (0.0, -0.008, -0.006)
    cam.c[:] = (0.3, 1.8 + 0.16, -2.4 + 0.12)
    got = api.lens(cam, 6.0, 0.06)
    assert got["focus"] == float(f32(6.0 / 3.0)) and got["scale"] == float(f32(0.06 / (0.01 * 2.0)))
    with pytest.raises(ValueError):
        api.lens(cam, 0.0, 0.1)
    with pytest.raises(ValueError):
        api.lens(cam, 1.0, -0.1)
