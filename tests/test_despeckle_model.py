"""tests/despeckle_model.py, the numpy model of the despeckle call (include/pbrs_gpu.h, "despeckle"), against the header's two rules
and against cases small enough to work out by hand.  The hand cases put their light into the green channel at powers of two: lum(0, g, 0)
is KG * g exactly, so every limit and every scale factor below is an exact f32 and the expected bytes can be written down.
These tests hold the model, the oracle of tests/test_gpu_despeckle.py, to the header's text; only the first one touches the library, so
the others also pass on a tree that has the model and not the feature."""
import itertools

import numpy as np
import pytest

import despeckle_model as dm
import pbrs_amd
from common import bits

f32 = np.float32
NAN, INF = f32(np.nan), f32(np.inf)


def green(values):
    """(h, w) of green levels -> (h, w, 3)."""
    g = np.asarray(values, f32)
    out = np.zeros(g.shape + (3,), f32)
    out[..., 1] = g
    return out


def hdr(w, h, seed=5):
    rng = np.random.default_rng(seed)
    rgb = (rng.random((h, w, 3)) ** 4 * 20 + 1e-3).astype(f32)
    var = (rng.random((h, w)) * 4 + 1e-3).astype(f32)
    return rgb, var


def same(a, b):
    return a.shape == b.shape and (bits(a) == bits(b)).all()


def test_the_models_defaults_are_the_mirrors():
    p = pbrs_amd.DespeckleParams.make(3, 2)
    assert (p.radius, p.rank, p.gain, p.floor, p.flags) == (1, 2, 2.0, 0.0, 0)
    assert dm.despeckle.__defaults__ == (None, 1, 2, 2.0, 0.0)
    assert (dm.CLAMPED, dm.REPAIRED) == (pbrs_amd.DespeckleParams.CLAMPED, pbrs_amd.DespeckleParams.REPAIRED)


def test_pass_through_rule():
    """Every constant image comes back bit for bit with gain >= 1, a negative and a denormal one included; so does an image none of whose
    pixels exceeds its limit."""
    var = np.array([[0.5, INF, 0.0], [NAN, 2.0, 1e-30], [1.0, 1.0, 1.0], [3.0, 0.25, 7.0]], f32)
    for colour in ((0.3, 0.7, 0.1), (0.0, 0.0, 0.0), (-1.0, 0.5, -2.0), (1e-41, 1e-41, 1e-41), (1e30, 1e30, 1e30)):
        img = np.broadcast_to(np.array(colour, f32), (4, 3, 3)).copy()
        for radius, rank, gain in itertools.product((1, 2), (1, 2, 3, 4), (1.0, 2.0)):
            r = dm.despeckle(img, var, radius=radius, rank=rank, gain=gain)
            assert same(r["rgb"], img) and same(r["variance"], var), (colour, radius, rank, gain)
            assert not r["mask"].any() and not bits(r["removed"]).any() and (r["n_clamped"], r["n_repaired"]) == (0, 0)
    rgb, var = hdr(9, 7)
    r = dm.despeckle(rgb, var, gain=1e6)
    assert same(r["rgb"], rgb) and same(r["variance"], var) and not r["mask"].any() and dm.record(r) == bytes(16)


@pytest.mark.parametrize("j", (1, -1, 10, -10))
def test_scale_rule(j):
    """floor == 0: the input times 2^j gives the output and the removed energy times 2^j, the variance times 4^j, the same mask and counts."""
    rgb, var = hdr(11, 9)
    rgb[2, 3] *= f32(300)
    rgb[6, 8:10] *= f32(500)
    rgb[0, 0], rgb[4, 4, 1], rgb[8, 10, 2] = NAN, INF, -INF
    var[1, 1], var[2, 3] = INF, f32(9.0)
    for radius, rank in ((1, 2), (2, 3)):
        base = dm.despeckle(rgb, var, radius=radius, rank=rank)
        assert base["n_clamped"] >= 3 and base["n_repaired"] == 3
        scaled = dm.despeckle(np.ldexp(rgb, j), np.ldexp(var, 2 * j), radius=radius, rank=rank)
        assert same(scaled["rgb"], np.ldexp(base["rgb"], j)) and same(scaled["removed"], np.ldexp(base["removed"], j))
        assert same(scaled["variance"], np.ldexp(base["variance"], 2 * j))
        assert (scaled["mask"] == base["mask"]).all() and dm.record(scaled) == dm.record(base)


def test_a_bright_centre_at_rank_1_and_2():
    """3 x 3 of green 1 around green 64, variance 8 at the centre: S = KG, limit = 2 KG, l' = 64 KG, s = 1 / 32: the centre becomes 2,
    its variance 8 / 1024, 62 is removed.  A corner sees the centre as its largest neighbour and KG as the second: no clamp either way."""
    img = green([[1, 1, 1], [1, 64, 1], [1, 1, 1]])
    var = np.full((3, 3), 8.0, f32)
    want, want_var = img.copy(), var.copy()
    want[1, 1, 1], want_var[1, 1] = 2.0, 8.0 / 1024.0
    for rank in (1, 2):
        r = dm.despeckle(img, var, rank=rank)
        assert same(r["rgb"], want) and same(r["variance"], want_var), rank
        assert (r["mask"] == np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], np.uint32)).all()
        assert same(r["removed"], green([[0, 0, 0], [0, 62, 0], [0, 0, 0]]))
        assert dm.record(r) == np.array([1, 0, 0, 0], np.uint32).tobytes()


def test_two_adjacent_bright_pixels_survive_rank_1_and_are_clamped_at_rank_2():
    img = green([[1, 1, 1, 1], [1, 64, 64, 1], [1, 1, 1, 1]])
    r1 = dm.despeckle(img, rank=1)  # each sees the other: limit = 128 KG
    assert same(r1["rgb"], img) and r1["n_clamped"] == 0 and r1["variance"] is None
    r2 = dm.despeckle(img, rank=2)  # the second largest is the background: limit = 2 KG
    assert same(r2["rgb"], green([[1, 1, 1, 1], [1, 2, 2, 1], [1, 1, 1, 1]])) and r2["n_clamped"] == 2


def test_fewer_neighbours_than_the_rank():
    """1 x 2 at rank 4: n = 1, so k = 1 and S is the other pixel."""
    r = dm.despeckle(green([[64, 1]]), rank=4)
    assert same(r["rgb"], green([[2, 1]])) and (r["mask"] == [[1, 0]]).all() and r["n_clamped"] == 1
    r = dm.despeckle(green([[64, 1]]), rank=4, floor=float(dm.KG) * 2)  # limit = 2 KG + 2 KG = 4 KG, s = 1 / 16
    assert same(r["rgb"], green([[4, 1]]))


def test_a_single_pixel_has_no_window():
    """1 x 1, n = 0: a good pixel stays whatever its value; a NaN becomes zeros, counts as repaired, and its variance becomes +inf."""
    one = np.array([[[5.0, 1e30, 0.25]]], f32)
    r = dm.despeckle(one, np.array([[3.0]], f32))
    assert same(r["rgb"], one) and same(r["variance"], np.array([[3.0]], f32)) and dm.record(r) == bytes(16)
    for bad in (NAN, INF, -INF):
        r = dm.despeckle(np.array([[[1.0, bad, 2.0]]], f32), np.array([[3.0]], f32))
        assert same(r["rgb"], np.zeros((1, 1, 3), f32)) and same(r["variance"], np.array([[INF]], f32))
        assert (r["mask"] == [[2]]).all() and (r["n_clamped"], r["n_repaired"]) == (0, 1) and not bits(r["removed"]).any()


def test_black_neighbours_take_everything_and_an_infinite_variance_stays():
    """Floor 0 among black neighbours: limit = +0, s = 0, the output is +0 in every channel; the centre's variance is +inf, which is not
    finite and is therefore kept: (inf * 0) * 0 would have been a NaN."""
    img = green([[0, 0, 0], [0, 64, 0], [0, 0, 0]])
    img[1, 1] = (3.0, 64.0, 5.0)
    var = np.ones((3, 3), f32)
    var[1, 1] = INF
    r = dm.despeckle(img, var)
    assert not bits(r["rgb"]).any() and same(r["variance"], var) and r["n_clamped"] == 1
    assert same(r["removed"][1, 1], np.array([3.0, 64.0, 5.0], f32))
    var[1, 1] = 4.0
    assert same(dm.despeckle(img, var)["variance"][1, 1], f32(0.0))


def test_a_repair_whose_sum_overflows_gives_zeros():
    """Two good neighbours of 3e38 in red (their luminance, 6.4e37, is finite): their sum is +inf, so is the mean, and c' falls back
    to zeros; a repair that does not overflow is the mean in row-major order."""
    img = np.zeros((1, 3, 3), f32)
    img[0, 0, 0] = img[0, 2, 0] = 3e38
    img[0, 1, 1] = NAN
    r = dm.despeckle(img)
    assert not bits(r["rgb"][0, 1]).any() and (r["mask"] == [[0, 2, 0]]).all() and (r["n_clamped"], r["n_repaired"]) == (0, 1)
    img = green([[1, 2, 4], [8, 0, 16], [32, 64, 128]])
    img[1, 1, 0] = INF
    r = dm.despeckle(img, rank=1, gain=1.0)  # the mean, 255 / 8, lies below the limit of 128
    assert same(r["rgb"][1, 1], np.array([0.0, 255.0 / 8.0, 0.0], f32)) and (r["mask"][1, 1], r["n_repaired"]) == (2, 1)
    r = dm.despeckle(img, rank=4, gain=1.0)  # the fourth largest is 16: the repaired pixel is clamped as well, s = 16 / (255 / 8)
    s = f32(0.71515972) * f32(16) / (f32(0.71515972) * f32(255.0 / 8.0))
    assert r["mask"][1, 1] == 3 and same(r["rgb"][1, 1], np.array([0.0, f32(255.0 / 8.0) * s, 0.0], f32))


def test_a_colour_is_good_only_with_a_finite_luminance():
    """Rule 2 asks the luminance as well as the channels.  The weights sum to less than 1, so the luminance of a finite f32 colour is
    itself finite: 3e38 in all channels has a luminance just below 3e38 and is a good pixel.  It is not repaired; beside a pixel of green
    1 it is a firefly and is clamped to 2 KG like any other, and as the largest neighbour it takes that pixel's limit to +inf.  The clause
    is exercised through the model's own predicate: a luminance that is not finite makes a pixel not good whatever its channels."""
    big = np.array([[[3e38, 3e38, 3e38], [0.0, 1.0, 0.0]]], f32)
    lp = dm.lum(big[0, 0, 0], big[0, 0, 1], big[0, 0, 2])
    assert dm.finite(lp) and lp < f32(3e38)
    r = dm.despeckle(big, rank=1)
    s = (f32(2.0) * dm.KG) / lp
    assert same(r["rgb"], np.array([[[f32(3e38) * s] * 3, [0.0, 1.0, 0.0]]], f32)) and (r["mask"] == [[1, 0]]).all() and r["n_repaired"] == 0
    alone = dm.despeckle(big[:, :1])  # no window: it stays
    assert same(alone["rgb"], big[:, :1]) and dm.record(alone) == bytes(16)
    assert not dm.finite(INF) and not dm.finite(NAN) and dm.finite(f32(3.4028235e38)) and dm.finite(f32(1e-45))
    with np.errstate(over="ignore"):
        assert not dm.finite(dm.lum(f32(3e38), f32(3e38), f32(3e38)) * f32(2))


def test_the_model_on_whole_planes_is_the_model_per_pixel():
    """despeckle_planes, which the GPU tests use where an image is too large for a loop over pixels, gives despeckle's bytes: on the GPU
    tests' planted images of every size (NaN, infinities, 3e38, negative channels, zeros, denormals, NaN payloads in the variance), a
    wholly NaN and a constant one, at both radii and every rank, with a gain of 1 and a floor, and on a window of the tall image."""
    from test_gpu_despeckle import SIZES, inputs, tall
    cases = [(name, rgb, var) for w, h in SIZES for name, (rgb, var) in inputs(w, h).items()]
    rgb, var = tall()
    cases.append(("tall", rgb[16 * 1023:16 * 1025 + 3], var[16 * 1023:16 * 1025 + 3]))
    for name, rgb, var in cases:
        for radius, rank, (gain, floor) in itertools.product((1, 2), (1, 2, 3, 4), ((2.0, 0.0), (1.0, 0.25))):
            if name != "planted" and (rank not in (2, 4) or gain != 2.0):
                continue
            kw = dict(radius=radius, rank=rank, gain=gain, floor=floor)
            a, b = dm.despeckle(rgb, var, **kw), dm.despeckle_planes(rgb, var, **kw)
            what = (name, rgb.shape, kw)
            assert same(a["rgb"], b["rgb"]) and same(a["variance"], b["variance"]) and same(a["removed"], b["removed"]), what
            assert (a["mask"] == b["mask"]).all() and dm.record(a) == dm.record(b), what
    assert dm.despeckle_planes(rgb)["variance"] is None
