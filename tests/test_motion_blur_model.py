"""The motion-blur arithmetic of include/pbrs_gpu.h ("motion blur") on the CPU, through tests/motion_blur_model.py, the numpy model that
follows the header's text: the five rules the header states, bit for bit; the tie-break of the dominant velocity; the clamp at
max_radius; shutter 0; non-finite inputs; what the jitter touches; and what the operation is for, a moving square against the mean of
48 instantaneous frames, and a static square in front of a moving background."""
import numpy as np
import pytest

import motion_blur_model as mb
from common import bits

f32 = np.float32


def same(got, want, what=""):
    diff = bits(got) != bits(want)
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def noise(w, h, seed=3):
    rng = np.random.default_rng(seed)
    return np.exp2(rng.uniform(-4, 4, (h, w, 3))).astype(f32)


W_, H_ = 41, 37
KW = dict(max_radius=7, taps=9, shutter=1.0, z_rel=0.25)


def layered(w, h):
    """A far wall (depth 8, growing a little along x), a near block that moves along (-9, 4) and a block between the two (depth 8.8: inside
    z_rel of the wall) that moves along (6, -22), beyond the clamp: the wall itself drifts slowly, below the 0.5 that would make its tiles move."""
    depth = np.tile(np.linspace(8.0, 8.5, w, dtype=f32), (h, 1))
    motion = np.zeros((h, w, 2), f32)
    motion[..., 0] = 0.3
    depth[6:20, 10:24], motion[6:20, 10:24] = 2.0, (-9.0, 4.0)
    depth[22:34, 20:36], motion[22:34, 20:36] = 8.8, (6.0, -22.0)
    return depth, motion


@pytest.fixture(scope="module")
def base():
    rgb = noise(W_, H_)
    depth, motion = layered(W_, H_)
    depth[2, 3], depth[H_ - 1, 0], depth[5, W_ - 2], depth[7, 7] = np.inf, 0.0, np.nan, -1.0
    rgb[9, 12] = (np.nan, 1.0, 1.0)
    for a in (rgb, depth, motion):
        a.flags.writeable = False
    res = mb.motion_blur(rgb, depth, motion, details=True, **KW)
    assert (res.n > 0).any() and (res.front > 0).any() and (res.behind > 0).any() and (res.between > 0).any() and (res.partial > 0).any()
    assert (res.len > f32(KW["max_radius"] - 0.001)).any() and (res.n[np.isfinite(rgb).all(axis=2)] == 0).any()
    return rgb, depth, motion, res


@pytest.mark.parametrize("j", (5, -5))
def test_rule_a_the_colours_scale(base, j):
    rgb, depth, motion, res = base
    s = f32(2.0) ** j
    scaled = mb.motion_blur(rgb * s, depth, motion, details=True, **KW)
    same(scaled.out, res.out * s, "out")
    same(scaled.velocity, res.velocity, "velocity")
    assert (scaled.n == res.n).all()


@pytest.mark.parametrize("j", (3, -4))
def test_rule_b_the_depth_scales(base, j):
    rgb, depth, motion, res = base
    scaled = mb.motion_blur(rgb, depth * f32(2.0) ** j, motion, details=True, **KW)
    same(scaled.out, res.out, "out")
    assert (scaled.n == res.n).all() and (scaled.between == res.between).all()


def test_rule_c_slow_pixels_return_the_image():
    rgb = noise(W_, H_)
    rgb[3, 3] = (np.inf, 0.0, -1.0)
    depth, _ = layered(W_, H_)
    rng = np.random.default_rng(5)
    angle = rng.uniform(0, 2 * np.pi, (H_, W_))
    motion = (np.stack([np.cos(angle), np.sin(angle)], axis=2) * rng.uniform(0, 0.999, (H_, W_, 1))).astype(f32)  # shutter 1: len < 0.5
    res = mb.motion_blur(rgb, depth, motion, max_radius=16, taps=16, shutter=1.0, details=True)
    assert res.len.max() <= f32(0.5) and res.len.max() > 0.4
    same(res.out, rgb)
    assert (res.n == 0).all()
    same(res.velocity, (motion * f32(0.5)).astype(f32))
    res = mb.motion_blur(rgb, depth, np.full((H_, W_, 2), 9.0, f32), shutter=0.0, details=True)  # step 0
    same(res.out, rgb)
    assert (bits(res.velocity) == 0).all()


def test_rule_d_a_still_pixel_takes_nothing_from_pixels_behind_it():
    rgb = noise(W_, H_)
    depth = np.full((H_, W_), 4.0, f32)
    motion = np.full((H_, W_, 2), (10.0, 0.0), f32)  # everything moves, far away
    depth[10, 20], motion[10, 20] = 1.0, (0.0, 0.0)   # but one near, still pixel
    kw = dict(max_radius=8, taps=16, shutter=1.0)
    res = mb.motion_blur(rgb, depth, motion, details=True, **kw)
    assert res.len[10, 20] == 0 and res.len[10, 21] == 5 and res.n[10, 20] == 0
    assert bits(res.out[10, 20]).tolist() == bits(rgb[10, 20]).tolist()
    other = rgb * f32(3.0)  # every other pixel's colour changes
    other[10, 20] = rgb[10, 20]
    again = mb.motion_blur(other, depth, motion, details=True, **kw)
    assert bits(again.out[10, 20]).tolist() == bits(rgb[10, 20]).tolist()
    # its moving neighbours behind it take each other, and nothing from it: in front of them, it spreads by its own speed, which is 0
    assert res.n[10, 21] > 0
    louder = rgb.copy()
    louder[10, 20] *= f32(7.0)
    third = mb.motion_blur(louder, depth, motion, **kw)
    keep = np.ones((H_, W_), bool)
    keep[10, 20] = False
    same(third[keep], res.out[keep], "the still pixel reaches nobody")


def test_rule_e_a_left_out_tap_is_not_added(base):
    """The model keeps a pixel's sums through np.where: with every left-out tap's colour replaced by a huge value or a NaN, nothing
    changes, which a sum that added wgt * rgb with wgt = 0 would not survive."""
    rgb, depth, motion, res = base
    # the pixels no pixel ever takes: poison them
    h, w, _ = rgb.shape
    still = np.zeros((h, w, 2), f32)
    alone = mb.motion_blur(rgb, depth, still, details=True, **KW)
    same(alone.out, rgb)
    far = rgb.copy()
    far[9, 12] = (np.inf, np.nan, -np.inf)  # the non-finite pixel of the base image, made worse: left out by every tap
    again = mb.motion_blur(far, depth, motion, details=True, **KW)
    keep = np.ones((h, w), bool)
    keep[9, 12] = False
    same(again.out[keep], res.out[keep])
    assert np.isfinite(again.out[keep]).all() and (again.n == res.n).all()


@pytest.mark.parametrize("first", ("left", "right"))
def test_the_tie_goes_to_the_lowest_index(first):
    w, h = 40, 20
    rgb = noise(w, h, 11)
    depth = np.full((h, w), 3.0, f32)
    motion = np.zeros((h, w, 2), f32)
    a, b = (6.0, 0.0), (0.0, 6.0)  # equal ll, different directions
    left, right = (a, b) if first == "left" else (b, a)
    motion[5, 14], motion[5, 17] = left, right  # either side of the tile border 15 | 16, both within 4 pixels of both tiles
    res = mb.motion_blur(rgb, depth, motion, max_radius=4, taps=8, shutter=1.0, details=True)
    assert res.winner[0, 0] == res.winner[0, 1] == 5 * w + 14
    want = np.asarray(left, f32) * f32(0.5)
    assert (res.vn[0:16, 0:32] == want).all() and (res.vn_len[0:16, 0:32] == 3).all()
    motion2 = motion.copy()
    motion2[4, 30] = right  # an equal vector in a row above wins the right tile alone (column 30 is outside the left tile's window)
    res2 = mb.motion_blur(rgb, depth, motion2, max_radius=4, taps=8, shutter=1.0, details=True)
    assert res2.winner[0, 0] == 5 * w + 14 and res2.winner[0, 1] == 4 * w + 30
    # the window ends max_radius beyond the tile: a faster pixel five columns outside is not seen
    motion3 = motion.copy()
    motion3[5, 21] = (30.0, 0.0)
    res3 = mb.motion_blur(rgb, depth, motion3, max_radius=4, taps=8, shutter=1.0, details=True)
    assert res3.winner[0, 0] == 5 * w + 14 and res3.winner[0, 1] == 5 * w + 21


def test_the_clamp_at_max_radius():
    m = np.array([[[3.0, 4.0], [30.0, 40.0], [-300.0, 400.0], [0.0, 1e15], [1e25, 1e25], [np.nan, 1.0], [np.inf, 0.0], [8.0, 0.0]]], f32)
    v, ll, ln = mb.velocity(m, 4, 1.0)
    assert v[0, 0].tolist() == [1.5, 2.0] and ln[0, 0] == 2.5 and ll[0, 0] == 6.25
    for k in (1, 2, 3):
        assert ln[0, k] <= 4 and abs(float(ln[0, k]) - 4.0) < 1e-6 and abs(float(np.hypot(*v[0, k])) - 4.0) < 1e-6, k
    assert ll[0, 4] == 0 and ln[0, 4] == 0  # ll overflows: s = R / inf = 0
    assert bits(v[0, 5]).tolist() == [0, 0] and bits(v[0, 6]).tolist() == [0, 0] and ln[0, 5] == 0 and ln[0, 6] == 0
    assert v[0, 7].tolist() == [4.0, 0.0] and ln[0, 7] == 4  # len == R is not clamped
    # every tap of a clamped pixel stays within max_radius (the model asserts it tap by tap)
    rgb, depth = noise(24, 24), np.full((24, 24), 2.0, f32)
    for vec in ((48.0, 0.0), (-33.0, 33.0), (1e6, -3e5)):
        res = mb.motion_blur(rgb, depth, np.full((24, 24, 2), vec, f32), max_radius=16, taps=64, shutter=1.0, details=True)
        assert (res.len <= 16).all() and (res.len > 15.999).all() and (res.n[4:20, 4:20] > 0).all()


def test_non_finite_inputs():
    w, h = 36, 20
    rgb, depth = noise(w, h, 7), np.full((h, w), 2.0, f32)
    motion = np.full((h, w, 2), (8.0, 0.0), f32)
    rgb[4, 10] = (np.nan, 1.0, 1.0)
    rgb[9, 20] = (1.0, np.inf, 1.0)
    motion[12, 5], motion[12, 6] = (np.nan, 3.0), (2.0, -np.inf)
    depth[15, 8], depth[15, 9], depth[15, 10], depth[15, 11] = np.nan, 0.0, -2.0, np.inf
    res = mb.motion_blur(rgb, depth, motion, max_radius=8, taps=16, shutter=1.0, details=True)
    assert bits(res.out[4, 10]).tolist() == bits(rgb[4, 10]).tolist() and bits(res.out[9, 20]).tolist() == bits(rgb[9, 20]).tolist()
    ok = np.isfinite(rgb).all(axis=2)
    assert np.isfinite(res.out[ok]).all()  # a non-finite pixel reaches no neighbour
    assert (bits(res.velocity[12, 5]) == 0).all() and (bits(res.velocity[12, 6]) == 0).all()
    # an unknown depth is far: the pixel is behind its neighbours, level with a miss
    far = depth.copy()
    far[15, 8:12] = np.inf
    same(mb.motion_blur(rgb, far, motion, max_radius=8, taps=16, shutter=1.0), res.out)


def test_jitter_changes_only_tiles_that_move():
    w, h = 64, 48
    rgb, depth = noise(w, h, 13), np.full((h, w), 2.0, f32)
    motion = np.zeros((h, w, 2), f32)
    motion[20:28, 36:44] = (14.0, -6.0)
    plain = mb.motion_blur(rgb, depth, motion, max_radius=8, taps=8, shutter=1.0, details=True)
    jit = mb.motion_blur(rgb, depth, motion, max_radius=8, taps=8, shutter=1.0, jitter=True, details=True)
    moving = plain.vn_len > f32(0.5)
    assert moving.any() and not moving.all() and (moving == (jit.vn_len > f32(0.5))).all()
    same(jit.out[~moving], rgb[~moving])
    same(plain.out[~moving], rgb[~moving])
    assert (bits(jit.out[moving]) != bits(plain.out[moving])).any()
    same(jit.velocity, plain.velocity)


def square_scene():
    """96 x 48, default_rng(3): a background 0.2 + 0.1 U, a 16 x 16 textured square 1 + 2 U at rows 16 .. 31 and columns 40 .. 55, depth
    2 over depth 10 -> (background, square, the frame, its depth)."""
    rng = np.random.default_rng(3)
    bg = (0.2 + 0.1 * rng.uniform(size=(48, 96, 3))).astype(f32)
    sq = (1.0 + 2.0 * rng.uniform(size=(16, 16, 3))).astype(f32)
    frame = bg.copy()
    frame[16:32, 40:56] = sq
    depth = np.full((48, 96), 10.0, f32)
    depth[16:32, 40:56] = 2.0
    return bg, sq, frame, depth


def test_a_moving_square_comes_within_a_tenth_of_the_unblurred_error():
    """What the call is for.  The square moves 12 pixels per frame along x; the truth is the mean of 48 instantaneous frames over the
    exposure (shutter 1).  The bound, a tenth of the unblurred frame's MSE, is a condition set before the model existed, with a threefold
    margin over a prototype's worst ratio (0.031); this model's ratios are 0.0241 and 0.0312
    (8 taps, plain and jittered), 0.0164 and 0.0124 (16), 0.0038 and 0.0056 (32), on an unblurred MSE of 0.03759."""
    bg, sq, frame, depth = square_scene()
    motion = np.zeros((48, 96, 2), f32)
    motion[16:32, 40:56, 0] = -12.0
    truth = np.zeros((48, 96, 3), np.float64)
    for s in range(48):
        o = int(round((s + 0.5) / 48 * 12 - 6))
        f = bg.copy()
        f[16:32, 40 + o:56 + o] = sq
        truth += f
    truth /= 48
    unblurred = float(((frame - truth) ** 2).mean())
    for taps in (8, 16, 32):
        for jitter in (False, True):
            out = mb.motion_blur(frame, depth, motion, max_radius=16, taps=taps, jitter=jitter, shutter=1.0)
            mse = float(((out - truth) ** 2).mean())
            print(f"taps {taps} jitter {jitter}: mse {mse:.3e}, unblurred {unblurred:.3e}, ratio {mse / unblurred:.4f}")
            assert mse <= 0.1 * unblurred, (taps, jitter, mse, unblurred)


def test_a_static_square_keeps_its_bits_in_front_of_a_moving_background():
    _, _, frame, depth = square_scene()
    motion = np.zeros((48, 96, 2), f32)
    motion[..., 0] = -12.0
    motion[16:32, 40:56] = 0.0
    for jitter in (False, True):
        res = mb.motion_blur(frame, depth, motion, max_radius=16, taps=16, jitter=jitter, shutter=1.0, details=True)
        same(res.out[16:32, 40:56], frame[16:32, 40:56], "the square's 256 pixels")
        assert (res.n[16:32, 40:56] == 0).all()
        changed = (bits(res.out) != bits(frame)).any(axis=2)
        assert changed[:, :40].any() and changed[:16].any()  # the background is smeared
