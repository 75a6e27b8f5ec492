"""include/pbrs_numeric.h (the f32 libm contract shared by host, kernels and oracle) against the platform
libm, and the RNG contract of SURVEY.md Appendix B."""
import numpy as np
import pytest

from numeric_inputs import around, f32, floats, u32, unary_inputs
from oracle.binding import numeric_eval, rng_stream


def ulp_err(got, want64):
    want32 = want64.astype(np.float32)
    spacing = np.spacing(np.abs(want32)).astype(np.float64)
    spacing[spacing == 0] = np.finfo(np.float32).tiny
    return np.abs(got.astype(np.float64) - want64) / spacing


RS = np.random.RandomState(1)
CASES = [
    ("sin", RS.uniform(-50, 50, 200000), np.sin, 2.0),
    ("cos", RS.uniform(-50, 50, 200000), np.cos, 2.0),
    ("atan", RS.standard_normal(200000) * 20, np.arctan, 3.0),
    ("asin", RS.uniform(-1, 1, 200000), np.arcsin, 3.0),
    ("acos", RS.uniform(-1, 1, 200000), np.arccos, 3.0),
    ("exp", RS.uniform(-80, 80, 200000), np.exp, 2.0),
    ("ln", np.exp(RS.uniform(-80, 80, 200000)), np.log, 2.0),
    ("sqrt", np.exp(RS.uniform(-80, 80, 200000)), np.sqrt, 0.5),
]


@pytest.mark.parametrize("fn,x,ref,max_ulp", CASES, ids=[c[0] for c in CASES])
def test_matches_libm_within_ulps(fn, x, ref, max_ulp):
    x = x.astype(np.float32)
    got = numeric_eval(fn, x)
    err = ulp_err(got, ref(x.astype(np.float64)))
    if fn in ("sin", "cos"):  # absolute accuracy near the zeros of sin/cos is bounded by the 3-part pi/4 reduction
        small = np.abs(ref(x.astype(np.float64))) < 1e-3
        assert np.abs(got.astype(np.float64) - ref(x.astype(np.float64)))[small].max() < 1e-7
        err = err[~small]
    assert err.max() <= max_ulp, (fn, float(err.max()))


@pytest.mark.parametrize("fn,ref", [("sin", np.sin), ("cos", np.cos)])
def test_sin_cos_match_libm_over_the_documented_range(fn, ref):
    """The whole |x| < 8192 that include/pbrs_numeric.h documents, on the sweep's deterministic set: the grid over every exponent
    and every k pi / 4 +- 32 ulp, where the three-part reduction is under the most strain.  Measured on this set against numpy's
    f64 result: sin 1.44 ulp, cos 1.40 ulp away from the zeros, hence the bound 2 (the next power of two); next to the zeros
    1.3e-10 absolute, held to the 1e-7 of the test above."""
    x = unary_inputs(True)
    x = x[np.abs(x) < 8192]
    assert len(x) > 2_500_000
    want = ref(x.astype(np.float64))
    got = numeric_eval(fn, x)
    small = np.abs(want) < 1e-3
    assert np.abs(got.astype(np.float64) - want)[small].max() < 1e-7
    err = ulp_err(got, want)[~small]
    assert err.max() <= 2.0, (fn, float(err.max()))


def test_sin_cos_stay_defined_past_the_i32_range_of_the_reduction():
    """From |x| = 2^31 pi / 4 on, 4 / pi |x| no longer fits an i32: the reduction's conversion saturates (as gfx950's instruction
    does; x86's would return INT_MIN), and everything after it is plain IEEE f32 arithmetic.  The value means nothing there, but it
    is the one this emulation in numpy's f32 arithmetic gives, for every input up to FLT_MAX."""
    x = unary_inputs(True)
    x = x[np.isfinite(x) & (np.abs(x) >= f32(1.0e9))]
    assert len(x) > 400_000 and (np.abs(x) < f32(1.69e9)).any()
    ax = np.abs(x)
    with np.errstate(all="ignore"):
        q = f32(1.27323954473516) * ax
        ji = np.clip(q.astype(np.float64), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)  # toward zero, saturating
        y = ji.astype(f32)
        odd = (ji & 1) == 1
        j = np.where(odd, ji + 1, ji) & 7
        y = np.where(odd, y + f32(1.0), y).astype(f32)
        r = ((ax - y * f32(0.78515625)) - y * f32(2.4187564849853515625e-4)) - y * f32(3.77489497744594108e-8)
        z = r * r
        ps = ((f32(-1.9515295891e-4) * z + f32(8.3321608736e-3)) * z - f32(1.6666654611e-1)) * z * r + r
        pc = ((f32(2.443315711809948e-5) * z - f32(1.388731625493765e-3)) * z + f32(4.166664568298827e-2)) * z * z
        pc = (pc - f32(0.5) * z) + f32(1.0)
    sneg, cneg = (x < 0) ^ (j > 3), (j > 3) ^ ((j & 3) > 1)
    swap = ((j & 3) == 1) | ((j & 3) == 2)
    want_s = np.where(swap, pc, ps).astype(f32)
    want_c = np.where(swap, ps, pc).astype(f32)
    want_s, want_c = np.where(sneg, -want_s, want_s), np.where(cneg, -want_c, want_c)
    for fn, want in (("sin", want_s), ("cos", want_c)):
        got = numeric_eval(fn, x)
        nan = np.isnan(want)
        assert (np.isnan(got) == nan).all() and (got.view(u32)[~nan] == want.view(u32)[~nan]).all(), fn
    assert np.isnan(numeric_eval("sin", np.array([np.inf, -np.inf, np.nan], dtype=f32))).all()


def test_conversions_and_ldexp_bits_at_their_edges():
    """pn_f32_to_i32 is Rust's saturating `as i32` (NaN -> 0), pn_trunc is f32::trunc with the sign of zero kept, pn_ldexp scales
    by 2^n with one rounding at most, at the subnormal end (n in the range exp() produces and well past it)."""
    x = np.concatenate([floats(around([0.5, 1.0, 8388608.0, 2147483648.0, 2147483520.0, 1e-45, 3.4e38], 64)),
                        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, -1.5, 2.5, -2.5], dtype=f32)])
    with np.errstate(all="ignore"):
        want = np.clip(np.trunc(np.nan_to_num(x.astype(np.float64), nan=0.0)), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64).astype(np.int32)
    assert (numeric_eval("f32_to_i32", x).view(np.int32) == want).all()
    t = numeric_eval("trunc", x)
    nan = np.isnan(x)
    assert np.isnan(t[nan]).all() and (t[~nan].view(u32) == np.trunc(x[~nan]).view(u32)).all()
    m = np.repeat(x[np.isfinite(x)], 11)
    n = np.tile(np.array([-300, -252, -150, -126, -24, 0, 1, 127, 128, 254, 300], dtype=f32), len(m) // 11)
    with np.errstate(all="ignore"):
        # pn_ldexp clamps n to [-252, 254]; np.ldexp in f64 then one rounding to f32 is x * 2^n correctly rounded
        want = np.ldexp(m.astype(np.float64), np.clip(n, -252, 254).astype(np.int32)).astype(f32)
    got = numeric_eval("ldexp", m, n)
    # two scalings by 2^(n/2): exact unless the FIRST one already lands among the subnormals (double rounding); those are left out
    first = np.ldexp(m.astype(np.float64), (np.clip(n, -252, 254) / 2).astype(np.int32))
    single = (np.abs(first) >= np.finfo(f32).tiny) | (first == 0)
    assert single.mean() > 0.8
    assert (got.view(u32)[single] == want.view(u32)[single]).all()


def test_tan_atan2_hypot():
    x = RS.uniform(-1.5, 1.5, 100000).astype(np.float32)
    assert ulp_err(numeric_eval("tan", x), np.tan(x.astype(np.float64))).max() <= 4.0
    a = (RS.standard_normal(100000) * 5).astype(np.float32)
    b = (RS.standard_normal(100000) * 5).astype(np.float32)
    got = numeric_eval("atan2", a, b)
    assert np.abs(got.astype(np.float64) - np.arctan2(a.astype(np.float64), b.astype(np.float64))).max() < 1e-6
    assert ulp_err(numeric_eval("hypot", a, b), np.hypot(a.astype(np.float64), b.astype(np.float64))).max() <= 1.5


def test_special_values():
    inf = np.float32(np.inf)
    assert numeric_eval("exp", [-inf, inf, 0.0]).tolist() == [0.0, np.inf, 1.0]
    assert numeric_eval("ln", [0.0, 1.0, inf]).tolist() == [-np.inf, 0.0, np.inf]
    assert np.isnan(numeric_eval("ln", [-1.0])[0])
    assert np.isnan(numeric_eval("acos", [1.5])[0])
    assert numeric_eval("acos", [1.0, -1.0]).tolist() == [0.0, np.float32(np.pi)]
    assert numeric_eval("atan2", [0.0, 1.0, -1.0], [0.0, 0.0, 0.0]).tolist() == [0.0, np.float32(np.pi / 2), -np.float32(np.pi / 2)]
    assert numeric_eval("fract", [1.75, -1.75, 3.0]).tolist() == [0.75, -0.75, 0.0]
    assert numeric_eval("floor", [1.75, -1.75, -3.0]).tolist() == [1.0, -2.0, -3.0]
    # compiler-rt __powisf2 association: powi(x, 5) = x * (x^2)^2
    x = np.float32(1.1)
    assert numeric_eval("powi", [x], [5.0])[0] == np.float32(x * np.float32(np.float32(x * x) * np.float32(x * x)))


def test_division_and_sqrt_are_ieee():
    a = (RS.standard_normal(100000) * np.exp(RS.uniform(-30, 30, 100000))).astype(np.float32)
    b = (RS.standard_normal(100000) * np.exp(RS.uniform(-30, 30, 100000))).astype(np.float32)
    assert (numeric_eval("div", a, b).view(np.uint32) == (a / b).view(np.uint32)).all()
    assert (numeric_eval("sqrt", np.abs(a)).view(np.uint32) == np.sqrt(np.abs(a)).view(np.uint32)).all()


def test_rng_contract():
    """PCG32 keyed by (seed, pixel, sample); f32 = (u32 >> 8) * 2^-24 in [0, 1) (rand 0.8 `Standard`)."""
    a = rng_stream(1, 7, 3, 4096)
    assert (a >= 0).all() and (a < 1).all()
    assert ((a * 2 ** 24) == np.round(a * 2 ** 24)).all()  # 24-bit mantissa grid
    assert (rng_stream(1, 7, 3, 16) == a[:16]).all()
    assert (rng_stream(1, 7, 4, 16) != a[:16]).any() and (rng_stream(1, 8, 3, 16) != a[:16]).any() and (rng_stream(2, 7, 3, 16) != a[:16]).any()
    # golden: first draws of stream (seed=1, pixel=0, sample=0); pins the contract across rounds
    golden = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "rng_seed1_px0_s0.npy"))
    assert (rng_stream(1, 0, 0, len(golden)).view(np.uint32) == golden.view(np.uint32)).all()
    # mean / uniformity sanity
    big = rng_stream(123, 5, 9, 1 << 16)
    assert abs(big.mean() - 0.5) < 5e-3
