"""tests/compare_model.py, the numpy model of pbrsx_compare (include/pbrs_gpu.h, "image comparison"), against what the header promises
and against evaluations that share none of its code: the Gaussian literals, the identities, the scale rule, the summation order's
error bound and SSIM's closed form.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import compare_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIT_FIELDS = ("mse", "mae", "max_abs", "ssim")


def hdr_pair(shape, seed, noise=0.5):
    rng = np.random.default_rng(seed)
    b = (rng.random(shape + (3,)) ** 4 * 20).astype(np.float32)
    return (b + rng.normal(0, noise, b.shape)).astype(np.float32), b


def bits(x):
    return np.float64(x).view(np.uint64)


def test_the_headers_gaussian_literals_are_the_nearest_f32():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    literals = dict(re.findall(r"#define PBRS_COMPARE_G(\d) (\S+)f\n", header))
    assert sorted(literals) == list("012345")
    for k in range(6):
        value = float.fromhex(literals[str(k)])
        assert np.float32(value) == value, k  # an f32 value as written
        assert np.float32(value) == np.float32(np.exp(-k * k / 4.5)) == cm.G[k], k
    assert int(re.search(r"#define PBRS_COMPARE_TILE (\d+)u", header).group(1)) == cm.TILE


@pytest.mark.parametrize("kind", [cm.LINEAR, cm.REINHARD])
def test_an_image_against_itself(kind):
    a, _ = hdr_pair((37, 45), 1)
    r = cm.compare(a, a, kind)
    assert r["mse"] == 0.0 and r["mae"] == 0.0 and r["rel_mse"] == 0.0 and r["max_abs"] == 0.0
    assert r["ssim"] == 1.0 and r["n_ssim"] == r["n_valid"] == 37 * 45 and r["n_invalid"] == 0
    assert (r["ssim_map"] == np.float32(1.0)).all()


@pytest.mark.parametrize("kind", [cm.LINEAR, cm.REINHARD])
def test_swapping_the_arguments_keeps_the_symmetric_fields(kind):
    a, b = hdr_pair((33, 17), 2)
    r, q = cm.compare(a, b, kind, peak=20.0), cm.compare(b, a, kind, peak=20.0)
    for n in BIT_FIELDS:
        assert bits(r[n]) == bits(q[n]), n
    assert r["rel_mse"] != q["rel_mse"]  # the one field that knows which image is the reference
    assert (r["ssim_map"].view(np.uint32) == q["ssim_map"].view(np.uint32)).all()


@pytest.mark.parametrize("j", [-3, 3])
def test_the_linear_scale_rule(j):
    a, b = hdr_pair((20, 50), 3)
    r, q = cm.compare(a, b, cm.LINEAR, ssim=False), cm.compare(np.ldexp(a, j), np.ldexp(b, j), cm.LINEAR, ssim=False)
    assert bits(q["mse"]) == bits(math.ldexp(r["mse"], 2 * j))
    assert bits(q["mae"]) == bits(math.ldexp(r["mae"], j)) and bits(q["max_abs"]) == bits(math.ldexp(r["max_abs"], j))
    assert (q["se"].view(np.uint64) == np.ldexp(r["se"], 2 * j).view(np.uint64)).all()
    assert (q["error_map"].view(np.uint32) == np.ldexp(r["error_map"], 2 * j).view(np.uint32)).all()


def test_the_tile_order_sum_is_within_the_textbook_bound_of_the_exact_sum():
    """Any summation order of n non-negative terms is within n * 2^-53 relative of the exact sum (Higham, Accuracy and Stability of
    Numerical Algorithms, section 4.2, with n - 1 <= n additions)."""
    a, b = hdr_pair((70, 45), 4)
    r = cm.compare(a, b, cm.LINEAR, ssim=False)
    exact = math.fsum(r["se"].ravel())
    n = r["se"].size
    assert abs(cm.ordered_sum(r["se"]) - exact) <= n * 2.0 ** -53 * exact
    assert r["mse"] == cm.ordered_sum(r["se"]) / np.float64(3 * n)


def test_the_order_is_the_tile_tree_and_not_the_row_order():
    """Three tiles: (t0 + t1) + (t2 + 0), each tile an adjacent-pair tree over its 256 row-major entries."""
    rng = np.random.default_rng(5)
    v = rng.random((16, 40))

    def tree(values):
        values = list(values)
        while len(values) > 1:
            values = [values[i] + values[i + 1] for i in range(0, len(values), 2)]
        return values[0]
    tiles = []
    for t in range(3):
        block = np.zeros((16, 16))
        part = v[:, 16 * t:16 * t + 16]
        block[:, :part.shape[1]] = part
        tiles.append(tree(block.ravel()))
    assert cm.ordered_sum(v) == (tiles[0] + tiles[1]) + (tiles[2] + 0.0)


def test_constant_images_give_the_closed_form():
    """Constant luminances ya and yb: the variances vanish and ssim = (2 ya yb + C1) / (ya^2 + yb^2 + C1).  The slack is the cancellation
    of the one-pass variances in f32: a prototype of this model measured 2.5e-5 relative and the bound, 1e-4, is four times that; this
    model measures 1.6e-6."""
    a, b = np.full((40, 40, 3), 0.25, np.float32), np.full((40, 40, 3), 0.5, np.float32)
    r = cm.compare(a, b, cm.LINEAR)
    ya, yb = float(cm.luminance(a)[0, 0]), float(cm.luminance(b)[0, 0])
    C1 = 0.01 ** 2
    closed = (2 * ya * yb + C1) / (ya * ya + yb * yb + C1)
    print(f"constant images: ssim {r['ssim']!r}, closed form {closed!r}, relative gap {abs(r['ssim'] - closed) / closed:.3g}")
    assert abs(r["ssim"] - closed) <= 1e-4 * closed
    assert r["n_ssim"] == 1600


def ssim_f64(a, b, kind, peak):
    """Mean SSIM by the header's formulas wholly in f64, written apart from the model: direct slices, Gaussian weights in f64."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    if kind == cm.REINHARD:
        a, b = np.maximum(a, 0), np.maximum(b, 0)
        a, b = a / (1 + a), b / (1 + b)

    def lum(c):
        return 0.21267127 * c[..., 0] + 0.71515972 * c[..., 1] + 0.07216883 * c[..., 2]
    x, y = lum(a), lum(b)
    g = np.exp(-np.arange(-5, 6) ** 2 / 4.5)

    def win(v):
        h, w = v.shape
        p = np.pad(v, 5)
        r = sum(g[j] * p[:, j:j + w] for j in range(11))
        return sum(g[j] * r[j:j + h, :] for j in range(11))
    W = win(np.ones_like(x))
    mx, my = win(x) / W, win(y) / W
    sxx, syy, sxy = win(x * x) / W - mx * mx, win(y * y) / W - my * my, win(x * y) / W - mx * my
    C1, C2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    return (((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))).mean()


@pytest.mark.parametrize("kind,peak,bound", [(cm.REINHARD, 1.0, 4.9e-8), (cm.LINEAR, 20.0, 4.2e-8)])
def test_the_f32_ssim_is_close_to_the_f64_one(kind, peak, bound):
    """A random 40 x 40 HDR pair (seed 7), the model's mean SSIM against the same formulas in f64.  Measured when this test was written:
    4.9e-9 with REINHARD at peak 1 (ssim 0.92639), 4.2e-9 with LINEAR at peak 20 (ssim 0.99495); the bounds are ten times those."""
    a, b = hdr_pair((40, 40), 7)
    r = cm.compare(a, b, kind, peak=peak)
    ref = ssim_f64(a, b, kind, peak)
    print(f"kind {kind}: model {r['ssim']!r}, f64 {ref!r}, gap {abs(r['ssim'] - ref):.3g}")
    assert r["n_ssim"] == 1600
    assert abs(r["ssim"] - ref) <= bound


@pytest.mark.parametrize("shape", [(1, 1), (5, 7)])
@pytest.mark.parametrize("kind", [cm.LINEAR, cm.REINHARD])
def test_images_smaller_than_the_window_give_finite_results(shape, kind):
    a, b = hdr_pair(shape, 8)
    r = cm.compare(a, b, kind, peak=20.0)
    assert all(math.isfinite(r[n]) for n in ("mse", "rel_mse", "mae", "ssim", "max_abs"))
    assert r["n_valid"] == r["n_ssim"] == shape[0] * shape[1]
    assert np.isfinite(r["ssim_map"]).all() and np.isfinite(r["error_map"]).all()
    assert len(cm.record(r)) == 64


def test_invalid_pixels_count_for_nothing():
    a, b = hdr_pair((20, 20), 9)
    a[3, 4, 1], b[0, 0, 2], a[19, 19, 0] = np.nan, np.inf, -np.inf
    r = cm.compare(a, b, cm.REINHARD)
    assert r["n_invalid"] == 3 and r["n_valid"] == 397 and r["n_ssim"] == 397
    for y, x in ((3, 4), (0, 0), (19, 19)):
        assert r["error_map"].view(np.uint32)[y, x] == 0x7FC00000 and r["ssim_map"].view(np.uint32)[y, x] == 0x7FC00000
    assert math.isfinite(r["mse"]) and math.isfinite(r["ssim"])
    empty = cm.compare(np.full((2, 2, 3), np.nan, np.float32), b[:2, :2], cm.REINHARD)
    assert empty["n_valid"] == 0 and math.isnan(empty["mse"]) and math.isnan(empty["ssim"]) and empty["max_abs"] == 0.0
