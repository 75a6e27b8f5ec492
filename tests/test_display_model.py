"""The display transform's CPU model (tests/display_model.py, the text of include/pbrs_gpu.h in numpy) against the properties the header
states: the scale rule, what the histogram counts and where its bin edges lie, the trimming, the adaptation, white, the accuracy and
monotonicity of the encodes, and the reference's settings against the host library's PNG."""
import itertools

import numpy as np
import pytest

import display_model as dm
import pbrs_amd
from test_image_io import read_png

f32 = np.float32


def lognormal(h, w, seed, sigma=2.0, offset=0.0):
    """A log-normal (h, w, 3) f32 image: luminances spread over about +-6 sigma octaves around 2^offset, inside 2^+-10."""
    rs = np.random.RandomState(seed)
    octaves = np.clip(rs.standard_normal((h, w, 1)) * sigma + offset, -9.0, 9.0)
    return (np.exp2(octaves) * rs.uniform(0.5, 1.0, (h, w, 3))).astype(f32)


@pytest.mark.parametrize("j", (3, -3, 10, -10))
def test_the_scale_rule(j):
    """Auto exposure, no exposure_in, the clamp inactive, every luminance inside 2^+-20 at both scales: the image times 2^j gives the
    same bytes, the histogram moves by 8 j bins and the exposure by 2^-j, bit for bit."""
    img = lognormal(37, 29, 5)
    y = dm.lum(img)
    assert y.min() > 2.0 ** -10 and y.max() < 2.0 ** 10
    for curve, encode, quantize in (("aces", "srgb", "round"), ("reinhard", "sqrt", "dither"), ("none", "srgb", "trunc")):
        kw = dict(curve=curve, encode=encode, quantize=quantize, auto=True, white=4.0)
        a, ea, ha = dm.display(img, **kw)
        b, eb, hb = dm.display((img * f32(2.0 ** j)).astype(f32), **kw)
        assert (a == b).all(), (j, curve)
        assert f32(eb * f32(2.0 ** j)).tobytes() == ea.tobytes()
        assert (np.roll(ha, 8 * j) == hb).all() and ha.sum() == hb.sum() == 37 * 29
        assert 2.0 ** -20 < ea < 2.0 ** 20 and 2.0 ** -20 < eb < 2.0 ** 20
        assert len(np.unique(a[:, :, :3])) > 100  # not vacuous: the image is neither black nor white


def specials():
    """Values the histogram must not count, and the two around its lower edge."""
    edge = np.array([0x2F800000], dtype=np.uint32).view(f32)[0]          # 2^-32: counted, bin 0
    below = np.array([0x2F7FFFFF], dtype=np.uint32).view(f32)[0]         # its predecessor: not counted
    return [0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-42, below], edge


def test_the_histogram_total_is_the_counted_pixels():
    img = lognormal(16, 16, 7)
    not_counted, edge = specials()
    for k, v in enumerate(not_counted):
        img[0, k] = v
    img[1, 0] = [edge, edge, edge]          # the luminance of (e, e, e) is below e: the weights sum to 0.99999982
    img[1, 1] = [0.0, f32(2.0 ** -31), 0.0]  # counted
    img[1, 2] = [f32(3e38), f32(3e38), f32(3e38)]  # finite, the largest bins
    img[1, 3] = [np.inf, -np.inf, 0.0]      # NaN luminance
    hist = dm.histogram(img)
    y = dm.lum(img).reshape(-1)
    counted = np.isfinite(y) & (y >= f32(2.0 ** -32))
    assert hist.sum() == counted.sum() == 16 * 16 - len(not_counted) - 2
    assert hist.dtype == np.uint32 and hist.shape == (dm.BINS,)
    assert hist[dm.BINS - 1] == 1  # 3e38 is far above 2^31.875: the last bin holds it
    _, e, h2 = dm.display(img, auto=True)
    assert (h2 == hist).all() and np.isfinite(e) and e > 0
    # nothing counted: the exposure is the previous one if that is valid, else 1
    nothing = np.zeros((3, 5, 3), f32)
    nothing[0, 0] = np.nan
    assert dm.display(nothing, auto=True)[1] == f32(1.0)
    assert dm.display(nothing, auto=True, exposure_in=2.5)[1] == f32(2.5)
    for bad in (np.nan, np.inf, 0.0, -1.0):
        assert dm.display(nothing, auto=True, exposure_in=bad)[1] == f32(1.0)


def test_powers_of_two_and_their_mantissa_steps_land_on_bin_edges():
    for octave in (-32, -31, -7, 0, 1, 13, 31):
        for step in range(8):
            v = f32(2.0 ** octave * (1.0 + step / 8.0))
            want = 8 * (octave + 32) + step
            counted, b = dm.bins_of(np.array([v, np.nextafter(v, f32(0.0)), np.nextafter(v, f32(np.inf))], dtype=f32))
            assert counted[0] and counted[2] and b[0] == want and b[2] == want
            if want > 0:
                assert counted[1] and b[1] == want - 1  # the value just below an edge is the bin before
            else:
                assert not counted[1]
    counted, b = dm.bins_of(np.array([2.0 ** 32, 3e38], dtype=f32))
    assert counted.all() and (b == dm.BINS - 1).all()


def test_outliers_above_the_high_rank_leave_the_exposure_unchanged():
    """The brightest 4 % of the pixels multiplied by 1000 (they stay counted, so N and every kept rank stay): with high_q16 at 95 % they
    lie outside the kept ranks and the exposure does not move; without trimming it does."""
    img = lognormal(50, 40, 11, sigma=1.0)
    y = dm.lum(img)
    order = np.argsort(y.reshape(-1))
    top = order[-int(0.04 * y.size):]
    hot = img.reshape(-1, 3).copy()
    hot[top] *= f32(1000.0)
    hot = hot.reshape(img.shape)
    trim = dict(auto=True, low_q16=0, high_q16=int(0.95 * 65536))
    e0, e1 = dm.display(img, **trim)[1], dm.display(hot, **trim)[1]
    assert e0.tobytes() == e1.tobytes()
    full = dict(auto=True, low_q16=0, high_q16=65536)
    assert dm.display(hot, **full)[1] < dm.display(img, **full)[1] * f32(0.9)


def test_adapt_moves_a_fixed_share_of_the_way_each_frame():
    img = lognormal(20, 20, 13)
    target = dm.display(img, auto=True)[1]
    assert dm.display(img, auto=True, exposure_in=123.0, adapt=1.0)[1] == f32(f32(123.0) + f32(target - f32(123.0)))
    e, adapt = f32(8.0) * target, 0.25
    for _ in range(6):
        nxt = dm.display(img, auto=True, exposure_in=e, adapt=adapt)[1]
        assert nxt.tobytes() == f32(e + f32(f32(target - e) * f32(adapt))).tobytes()
        assert abs((float(nxt) - float(target)) / (float(e) - float(target)) - 0.75) < 1e-5
        e = nxt


@pytest.mark.parametrize("curve", ("none", "reinhard", "aces"))
def test_white_gives_255_under_every_encode_and_quantizer(curve):
    """(1, 1, 1) under no curve; the value the curve maps to 1 under the others (Reinhard: `white`; ACES passes 1 well below 65504)."""
    white = {"none": 1.0, "reinhard": 4.0, "aces": 65504.0}[curve]
    img = np.full((4, 4, 3), white, dtype=f32)
    for encode, quantize in itertools.product(dm.ENCODES, dm.QUANTIZERS):
        out = dm.display(img, curve=curve, encode=encode, quantize=quantize, white=4.0)[0]
        assert (out == 255).all(), (curve, encode, quantize)
    if curve == "none":  # and through the exact branch: t == 1 is not 0.99999994
        assert (dm.display(np.ones((1, 1, 3), f32), curve="none", encode="srgb", quantize="trunc")[0] == 255).all()


def test_srgb_is_within_one_level_of_the_float64_formula():
    """2 000 001 evenly spaced t in [0, 1], sRGB and rounding: against the float64 formula at most one level apart, in at most 1e-4 of the
    values.  Measured: max 1, share 4.5e-6."""
    t = (np.arange(2000001, dtype=np.float64) / 2000000.0).astype(f32)
    got = dm.quantize(dm.curve_encode(t, 0, 1), f32(0.5)).astype(np.int64)
    t64 = t.astype(np.float64)
    g64 = np.where(t64 <= 0.0031308, 12.92 * t64, 1.055 * np.power(t64, 1.0 / 2.4) - 0.055)
    want = np.minimum(np.floor(g64 * 255.0 + 0.5), 255).astype(np.int64)
    diff = np.abs(got - want)
    print(f"sRGB + round against float64: max difference {diff.max()} level(s), share of differing values {np.mean(diff != 0):.3g}")
    assert diff.max() <= 1 and np.mean(diff != 0) <= 1e-4
    assert got[0] == 0 and got[-1] == 255


@pytest.mark.parametrize("encode", ("sqrt", "srgb"))
def test_the_encodes_are_monotone(encode):
    """g does not decrease over 2 000 001 evenly spaced t in [0, 1]; the bytes do not decrease over those and over the 129 floats around
    the sRGB knee, where the two branches meet, and the last float below 1.  (g itself steps down by 3.4e-8 from the knee to the next
    float, 0.040449936 to 0.040449902: the standard's two branches do not meet exactly.  That is 9e-6 of a level, and no byte sees it.)"""
    t = (np.arange(2000001, dtype=np.float64) / 2000000.0).astype(f32)
    g = dm.curve_encode(t, 0, dm.ENCODES[encode])
    assert (np.diff(g) >= 0).all() and g[0] == 0 and g[-1] == 1
    knee = np.array([0.0031308], dtype=f32).view(np.uint32)[0]
    around = (int(knee) + np.arange(-64, 65, dtype=np.int64)).astype(np.uint32).view(f32)
    t = np.unique(np.concatenate([t, around, np.array([np.nextafter(f32(1.0), f32(0.0))], dtype=f32)]))
    g = dm.curve_encode(t, 0, dm.ENCODES[encode])
    for d in (f32(0.0), f32(0.5)):
        assert (np.diff(dm.quantize(g, d).astype(np.int64)) >= 0).all()


def test_the_reference_settings_give_the_bytes_of_the_host_png(tmp_path):
    rs = np.random.RandomState(1)
    img = rs.uniform(-0.2, 1.5, (9, 11, 3)).astype(f32)
    img[0, 0] = [np.nan, 0.0, 1.0]
    img[0, 1] = [4.0, 0.25, 1e-9]
    img[0, 2] = [np.inf, -np.inf, -0.0]
    img[0, 3] = [1e30, np.nextafter(f32(1.0), f32(0.0)), np.nextafter(f32(1.0), f32(2.0))]
    pbrs_amd.write_image(tmp_path / "a.png", img)
    want = read_png(tmp_path / "a.png")
    got = dm.display(img, curve="none", encode="sqrt", quantize="trunc", exposure=1.0)[0]
    assert (got[:, :, :3] == want).all() and (got[:, :, 3] == 255).all()
    # and the 8-bit writer stores bytes as they are
    pbrs_amd.write_image_u8(tmp_path / "b.png", got)
    assert (read_png(tmp_path / "b.png") == got[:, :, :3]).all()
    pbrs_amd.write_image_u8(tmp_path / "c.png", np.ascontiguousarray(got[:, :, :3]))
    assert (read_png(tmp_path / "c.png") == got[:, :, :3]).all()
