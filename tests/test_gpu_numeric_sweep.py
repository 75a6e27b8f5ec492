"""gfx950 evaluates include/pbrs_numeric.h bit for bit like x86 over the WHOLE f32 domain, not only where today's scenes
happen to go: every exponent with both signs, subnormals, infinities, NaNs, the neighbourhood of every constant the header
branches on and of every quadrant boundary of sin / cos / tan.  Inputs are built without random numbers.  A NaN is asked for
exactly where the CPU has one (its payload is not part of the contract); every other result is compared as bits, and results
that are no f32 (integers, halves of an f64) as words, all of them.  NON_NAN pins how many values each comparison covers."""
import functools
import os
import subprocess

import numpy as np
import pytest

from numeric_inputs import MAX_N, around, binary_inputs, bits_of, both_signs, f32, floats, reduced_grid, u32, unary_inputs
from oracle.binding import numeric_eval, numeric_eval_k

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# How many values each comparison covers: the non-NaN results of the CPU, counted on the CPU (deterministic, no GPU involved); for a
# result compared as words, all of them.  A NaN mask cannot grow, and an input set cannot shrink, without this table changing.
NON_NAN = {
    "sin": 3526774, "cos": 2978040, "tan": 2690974, "atan": 2155796, "asin": 1073290, "acos": 1073290, "exp": 2155796, "ln": 1077899,
    "sqrt": 1077899, "fract": 2155794, "floor": 2155796, "trunc": 2155796, "signum": 2155796, "weak_recip": 2155796,
    "f32_to_i32": 2163982, "div": 4163218, "hypot": 4163230, "atan2": 4163226, "max": 4186204, "min": 4186204, "powi": 2218976,
    "ldexp": 2453282, "sincos64": 172032, "mul_add": 3833889, "clamp": 3884806, "slab_filter": 1310720, "rng": 14256,
}
WORDS = {"f32_to_i32"}


def compare(name, cpu, gpu, inputs, words=False):
    cw, gw = cpu.view(u32), gpu.view(u32)
    keep = np.ones(len(cw), dtype=bool) if words else ~np.isnan(cpu.view(f32))
    print(f"{name}: {len(cw)} inputs, {int(keep.sum())} compared as bits")
    assert int(keep.sum()) == NON_NAN[name], (name, int(keep.sum()))
    if not words:
        wrong = ~keep & ~np.isnan(gpu.view(f32))
        assert not wrong.any(), (name, "CPU NaN, GPU not", [tuple(hex(v) for v in a.view(u32)[wrong][:4]) for a in inputs], gw[wrong][:4])
    wrong = keep & (cw != gw)
    assert not wrong.any(), (name, int(wrong.sum()), [tuple(hex(v) for v in a.view(u32)[wrong][:4]) for a in inputs],
                             [hex(v) for v in cw[wrong][:4]], [hex(v) for v in gw[wrong][:4]])


@pytest.mark.parametrize("fn", ["sin", "cos", "tan", "atan", "asin", "acos", "exp", "ln", "sqrt", "fract", "floor", "trunc", "signum",
                                "weak_recip", "f32_to_i32"])
def test_unary_over_the_whole_domain(gpu_ctx, fn):
    x = unary_inputs(fn in ("sin", "cos", "tan"))
    compare(fn, numeric_eval(fn, x), gpu_ctx.numeric_eval(fn, x), [x], words=fn in WORDS)


@pytest.mark.parametrize("fn", ["div", "hypot", "atan2", "max", "min", "powi", "ldexp"])
def test_binary_over_the_exponent_cross_product(gpu_ctx, fn):
    x, y = binary_inputs(fn)
    assert len(x) == len(y) <= MAX_N
    compare(fn, numeric_eval(fn, x, y), gpu_ctx.numeric_eval(fn, x, y), [x, y])


def test_sincos_f64_words(gpu_ctx):
    """pn_sincos_f64 (device/fourier.h's Newton-bisection) on f64 angles (double)x + (double)y: every exponent of x, the
    neighbourhood of k pi / 4 over many turns, with offsets far below an f32 ulp; four words per angle, none masked (the function
    returns (0, 1) outside its range, NaN included)."""
    x = np.concatenate([reduced_grid(), floats(around(np.arange(1, 1025) * (np.pi / 4), 8))])
    offsets = np.array([0.0, 2.0 ** -30, -2.0 ** -30, 1e-12, 2.0 ** -60, 0.1, -3e-9, 7e-17], dtype=f32)
    y = offsets[np.arange(len(x)) % 8]
    with np.errstate(all="ignore"):
        y[1::16] = x[1::16] * f32(2.0 ** -26)
    y[np.isnan(y)] = 0.0
    names = ["sincos64_sin_hi", "sincos64_sin_lo", "sincos64_cos_hi", "sincos64_cos_lo"]
    cpu = np.concatenate([numeric_eval(n, x, y) for n in names])
    gpu = np.concatenate([gpu_ctx.numeric_eval(n, x, y) for n in names])
    s = (cpu[:len(x)].view(u32).astype(np.uint64) << np.uint64(32) | cpu[len(x):2 * len(x)].view(u32)).view(np.float64)
    with np.errstate(all="ignore"):
        angle = x.astype(np.float64) + y
    inside = np.abs(np.nan_to_num(angle, nan=np.inf)) < 1e4
    assert np.abs(s[inside] - np.sin(angle[inside])).max() < 1e-12  # the words are the function's, in this order
    compare("sincos64", cpu, gpu, [np.tile(x, 4), np.tile(y, 4)], words=True)


@functools.lru_cache(None)
def ternary_inputs():
    r = reduced_grid()
    s = np.concatenate([r[::55], floats(both_signs(bits_of([0.0, 1.0, np.inf]))), np.array([np.nan], dtype=f32)])
    a, b, c = (v.reshape(-1) for v in np.meshgrid(s, s, s, indexing="ij"))
    # products whose rounding error is all that is left: c = -RN(a b), which a multiply followed by an add turns into 0
    pa, pb = binary_inputs("div")
    pa, pb = pa[::37][:1 << 17], pb[::37][:1 << 17]
    with np.errstate(all="ignore"):
        pc = -(pa * pb)
    ops = np.stack([np.concatenate([a, pa]), np.concatenate([b, pb]), np.concatenate([c, pc])], axis=1)
    assert len(ops) <= MAX_N
    return np.ascontiguousarray(ops, dtype=f32)


@pytest.mark.parametrize("fn", ["mul_add", "clamp"])
def test_ternary_over_a_cross_product(gpu_ctx, fn):
    ops = ternary_inputs()
    cpu, gpu = numeric_eval_k(fn, ops), gpu_ctx.numeric_eval_k(fn, ops)
    if fn == "mul_add":  # the probe is the fused operation: exact residuals of the products are not all zero
        tail = cpu[-(1 << 17):].view(f32)
        assert (tail[np.isfinite(tail)] != 0).any()
    compare(fn, cpu, gpu, [ops[:, 0], ops[:, 1], ops[:, 2]])


def test_slab_filter_decisions(gpu_ctx, tmp_path):
    """pn_slab_filter prunes in device/traverse.h and device/wide.h: the device's decision equals the CPU's on the cases of
    tests/test_slab_filter.py's generator (random, flat-box, corner, on-face, extent-on-plane, and the unused slots of a wide node)."""
    exe = tmp_path / "slab_filter_check"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe), os.path.join(ROOT, "tests", "slab_filter_check.c"), "-lm"])
    rows = []
    for args, n in ((["dump"], 1 << 20), (["unused"], 1 << 18)):
        path = tmp_path / ("cases_" + args[0])
        subprocess.run([str(exe), str(n)] + args + [str(path)], capture_output=True, check=False)
        rows.append(np.fromfile(path, dtype=u32).reshape(n, 14))
    rows = np.concatenate(rows)
    ops, decided = np.ascontiguousarray(rows[:, :13]), rows[:, 13]
    cpu, gpu = numeric_eval_k("slab_filter", ops), gpu_ctx.numeric_eval_k("slab_filter", ops)
    assert (cpu == decided).all()  # the oracle's build of the function and the generator's agree
    assert 0.05 < cpu[:1 << 20].mean() < 0.95 and not cpu[1 << 20:].any()
    compare("slab_filter", cpu, gpu, [ops.view(f32)[:, j] for j in range(13)], words=True)


def test_rng_streams(gpu_ctx):
    """pn_rng_init / pn_rng_u32 / pn_rng_f32: the first 64 draws of the streams keyed by pixel and sample indices at the ends of
    their ranges, for seeds 0, 1 and 2^63; the initial states too, and one step from those states through the two-operand ids."""
    edge = [0, 1, (1 << 16) - 1, (1 << 16) + 1, 1 << 31, (1 << 32) - 1]
    keys = np.array([(seed & 0xffffffff, seed >> 32, p, s) for seed in (0, 1, 1 << 63) for p in edge for s in edge], dtype=np.uint64).astype(u32)
    draws = np.concatenate([np.repeat(keys, 64, axis=0), np.tile(np.arange(64, dtype=u32), len(keys))[:, None]], axis=1)
    cpu, gpu = [], []
    for fn, ops in (("rng_init_lo", keys), ("rng_init_hi", keys), ("rng_stream_u32", draws), ("rng_stream_f32", draws)):
        cpu.append(numeric_eval_k(fn, ops))
        gpu.append(gpu_ctx.numeric_eval_k(fn, ops))
    lo, hi = floats(cpu[0]), floats(cpu[1])
    for fn in ("rng_u32", "rng_f32"):
        cpu.append(numeric_eval(fn, lo, hi).view(u32))
        gpu.append(gpu_ctx.numeric_eval(fn, lo, hi).view(u32))
    first = cpu[2].reshape(len(keys), 64)
    assert (cpu[4] == first[:, 0]).all() and len(np.unique(first)) > 0.999 * first.size  # draw 0 is one step from the initial state
    assert (cpu[3].view(f32) == (cpu[2] >> 8).astype(f32) * f32(2.0 ** -24)).all()
    compare("rng", np.concatenate(cpu), np.concatenate(gpu), [np.zeros(sum(len(c) for c in cpu), dtype=f32)], words=True)
