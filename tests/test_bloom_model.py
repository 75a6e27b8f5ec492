"""tests/bloom_model.py, the numpy model of the bloom call (include/pbrs_gpu.h, "bloom"), by the properties the header states for it: the
fixed point, the response to an impulse, the scale rule, strength 0, non-finite pixels, an image below the threshold and the cut of the
level count.  tests/test_gpu_bloom.py holds the device to this model bit for bit."""
import numpy as np
import pytest

import bloom_model as bm
from common import bits

f32 = np.float32


def hdr(w, h, seed=5):
    """Seeded HDR noise, log-uniform over twelve octaves around 1."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    return np.exp2(rng.uniform(-6, 6, (h, w, 3))).astype(f32)


def test_level_sizes_follow_the_header():
    assert bm.level_sizes(1920, 1080, 6) == [(960, 540), (480, 270), (240, 135), (120, 68), (60, 34), (30, 17)]
    assert bm.level_sizes(5, 3, 8) == [(3, 2), (2, 1), (1, 1)]
    assert bm.level_sizes(1, 1, 8) == [(1, 1)] and bm.level_sizes(1, 40, 2) == [(1, 20), (1, 10)]


@pytest.mark.parametrize("size", ((1, 1), (5, 3), (33, 17)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_constant_image_is_its_own_bloom_under_mix(size):
    """0.75 has two significant bits: 0.375f * 0.75f and every partial sum k / 64 * 0.75 are exact."""
    w, h = size
    rgb = np.full((h, w, 3), 0.75, f32)
    for levels, spread, strength in ((6, 0.6, 0.3), (1, 1.0, 1.0), (8, 0.0, 0.05)):
        out = bm.bloom(rgb, levels=levels, threshold=0.0, knee=0.0, strength=strength, spread=spread, mix=True)
        assert (bits(out) == bits(rgb)).all(), (levels, spread, strength)


def _impulse(w, h, x, y):
    rgb = np.zeros((h, w, 3), f32)
    rgb[y, x] = (1.0, 2.0, 0.5)
    return rgb


def test_an_impulses_response_reflects_where_every_level_halves_evenly():
    """The downsample's window 2X - 1 .. 2X + 2 and up()'s two taps mirror onto those of the mirrored pixel only when the source is
    even: w and h must be multiples of 2^N for N effective levels, so that the image and every level but the last have even sizes.
    The sums run in one order, not the mirrored one, so the bits mirror only while every sum is exact: an impulse of powers of two,
    spread and strength 0.5, threshold 0, two levels.  Then: bloom(mirror(image)) == mirror(bloom(image)) for the four reflections."""
    kw = dict(levels=2, threshold=0.0, knee=0.0, strength=0.5, spread=0.5)
    flips = (lambda a: a, lambda a: a[:, ::-1], lambda a: a[::-1], lambda a: a[::-1, ::-1])
    for w, h in ((16, 8), (12, 20)):  # multiples of 2^2
        rgb = _impulse(w, h, 5, 3)
        want = bm.bloom(rgb, **kw)
        assert (want > 0).sum() > 3 * 16  # the glare has spread
        for flip in flips:
            assert (bits(bm.bloom(np.ascontiguousarray(flip(rgb)), **kw)) == bits(np.ascontiguousarray(flip(want)))).all(), (w, h)
    for w, h in ((15, 8), (16, 9), (14, 8)):  # odd, odd, and even with an odd level 0 (7): the reflection about the odd axis does not hold
        rgb = _impulse(w, h, 5, 3)
        want = bm.bloom(rgb, **kw)
        odd_x = w in (15, 14)
        flip = flips[1] if odd_x else flips[2]
        assert (bits(bm.bloom(np.ascontiguousarray(flip(rgb)), **kw)) != bits(np.ascontiguousarray(flip(want)))).any(), (w, h)
        other = flips[2] if odd_x else flips[1]  # the other axis is a multiple of 4 and still mirrors
        assert (bits(bm.bloom(np.ascontiguousarray(other(rgb)), **kw)) == bits(np.ascontiguousarray(other(want)))).all(), (w, h)


@pytest.mark.parametrize("j", (7, -7))
def test_the_scale_rule(j):
    rgb = hdr(21, 13)
    rgb[2, 3] = (0.0, 0.0, 0.0)
    rgb[4, 5] = (-1.0, 2.0, 3.0)
    s = f32(2.0) ** j
    for kw in (dict(), dict(threshold=0.25, knee=1.0, strength=0.7, spread=1.0), dict(threshold=0.0, knee=0.0, strength=0.5, mix=True)):
        base = bm.bloom(rgb, **kw)
        scaled = bm.bloom(rgb * s, **{**bm.DEFAULTS, **kw, "threshold": float(f32({**bm.DEFAULTS, **kw}["threshold"]) * s)})
        assert np.isfinite(base).all() and (np.abs(base[base != 0]) > 1e-30).all()
        assert (bits(scaled) == bits(base * s)).all(), kw


def test_zero_strength_returns_the_inputs_bits():
    rgb = hdr(9, 7)
    rgb[0, 0] = (np.nan, 1.0, -0.0)
    rgb[1, 1] = (-0.0, -0.0, np.inf)
    for mix in (False, True):
        assert (bits(bm.bloom(rgb, strength=0.0, mix=mix)) == bits(rgb)).all()


def test_non_finite_pixels_pass_through_and_poison_nothing():
    rgb = hdr(19, 11)
    payload = np.array([0x7FC12345], np.uint32).view(f32)[0]
    rgb[3, 4] = (payload, 1.0, 2.0)
    rgb[5, 9] = (1.0, np.inf, 2.0)
    rgb[0, 0] = (-np.inf, np.nan, 0.0)
    bad = ~np.isfinite(rgb).all(axis=2)
    for kw in (dict(strength=0.5), dict(threshold=0.0, knee=0.0, strength=0.5, mix=True)):
        out = bm.bloom(rgb, **kw)
        assert (bits(out[bad]) == bits(rgb[bad])).all()
        assert np.isfinite(out[~bad]).all()
        hole = rgb.copy()
        hole[bad] = 0.0  # a non-finite pixel enters the pyramid as +0
        assert (bits(out[~bad]) == bits(bm.bloom(hole, **kw)[~bad])).all()


def test_an_image_below_the_threshold_comes_back():
    rgb = hdr(17, 9) * f32(2.0 ** -7)  # below 2^-1 = t - k
    rgb[2, 2] = (-3.0, 0.0, 0.0)
    assert bm.lum(np.where(rgb > 0, rgb, f32(0))).max() <= 0.5
    assert (bits(bm.bloom(rgb, strength=1.0)) == bits(rgb)).all()
    lit = rgb.copy()
    lit[4, 4] = (8.0, 8.0, 8.0)
    assert (bits(bm.bloom(lit, strength=1.0)) != bits(lit)).any()


def test_levels_beyond_one_by_one_change_nothing():
    rgb = hdr(5, 3)
    assert len(bm.level_sizes(5, 3, 8)) == 3
    want = bm.bloom(rgb, levels=3, strength=0.5)
    for levels in (4, 8):
        assert (bits(bm.bloom(rgb, levels=levels, strength=0.5)) == bits(want)).all()
    assert (bits(bm.bloom(rgb, levels=2, strength=0.5)) != bits(want)).any()
