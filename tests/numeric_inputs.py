"""Inputs of the numeric sweeps (tests/test_gpu_numeric_sweep.py on the device, tests/test_numeric.py on the CPU), built without
random numbers: a grid over every exponent with both signs, and the neighbourhoods of the constants include/pbrs_numeric.h
branches on and of the quadrant boundaries of sin / cos / tan."""
import functools

import numpy as np

MAX_N = 1 << 22  # the oracle's probe loop is single-threaded: keeps every test at a fraction of a second
u32, f32 = np.uint32, np.float32


def bits_of(x):
    return np.asarray(x, dtype=f32).view(u32)


def floats(b):
    return np.ascontiguousarray(b, dtype=u32).view(f32)


def both_signs(b):
    b = np.asarray(b, dtype=u32)
    return np.concatenate([b, b | u32(0x80000000)])


def around(values, ulps):
    """bit patterns within `ulps` of each positive f32 in `values`, with both signs"""
    centre = bits_of(np.abs(np.asarray(values, dtype=np.float64)).astype(f32)).astype(np.int64)
    return both_signs((centre[:, None] + np.arange(-ulps, ulps + 1)[None, :]).reshape(-1).astype(u32))


# top ten mantissa bits with the low bits all 0 and all 1, the 2^10 smallest and the 2^10 largest mantissas
MANTISSAS = np.unique(np.concatenate([np.arange(1 << 10) << 13, (np.arange(1 << 10) << 13) | 0x1fff, np.arange(1 << 10),
                                      (1 << 23) - 1 - np.arange(1 << 10)])).astype(u32)
# the 16 of the reduced grid; the first eight are the ones ldexp keeps
MANTISSAS16 = np.array([0, 1, 0x7fffff, 0x400000, 0x3fffff, 0x555555, 0x7ffffe, 0x000800,
                        2, 0x400001, 0x200000, 0x600000, 0x2aaaaa, 0x0007ff, 0x7ff800, 0x333333], dtype=u32)
# every constant a function of the header branches on
BRANCH_CONSTANTS = [0.4142135623730950, 2.414213562373095, 1e-4, 0.5, 1.0, 88.72283905206835, 103.278929903431851103, 8388608.0, 2147483648.0]


def grid(mantissas):
    """[sign][exponent 0..255][mantissa]: +-0, every subnormal and normal binade, infinities and NaNs"""
    e = (np.arange(256, dtype=u32) << 23)[:, None] | mantissas[None, :]
    return both_signs(e.reshape(-1))


@functools.lru_cache(None)
def unary_inputs(trig):
    parts = [grid(MANTISSAS), around(BRANCH_CONSTANTS, 64)]
    # the mantissa split 0.70710678 of ln (0x3504f3) at every exponent
    split = ((np.arange(1, 255, dtype=np.int64) << 23) | 0x3504f3)[:, None] + np.arange(-64, 65)[None, :]
    parts.append(both_signs(split.reshape(-1).astype(u32)))
    if trig:  # every k pi / 4 up to 8192 (the documented range), then one per binade up to FLT_MAX
        k = np.arange(1, int(8192 / (np.pi / 4)) + 2, dtype=np.float64)
        parts.append(around(k * (np.pi / 4), 32))
        parts.append(around((np.pi / 4) * 2.0 ** np.arange(13, 128), 32))
    x = floats(np.concatenate(parts))
    assert len(x) <= MAX_N
    return x


@functools.lru_cache(None)
def reduced_grid():
    return floats(grid(MANTISSAS16))  # 8192 values, index = sign * 4096 + exponent * 16 + mantissa


@functools.lru_cache(None)
def binary_inputs(fn):
    r = reduced_grid()
    if fn == "powi":  # every 16th value of the full grid, each with the exponents -8 ... 8
        x = floats(grid(MANTISSAS))[::16]
        return np.repeat(x, 17), np.tile(np.arange(-8, 9, dtype=f32), len(x))
    if fn == "ldexp":  # eight mantissas of the reduced grid, each with n in -300 ... 300
        x = r[(np.arange(len(r)) % 16) < 8]
        return np.repeat(x, 601), np.tile(np.arange(-300, 301, dtype=f32), len(x))
    # the cross product of the reduced grid with itself, cut to the array size: every x of the grid meets every (sign, exponent)
    # of y, with the one mantissa of the sixteen that x's index selects (all 16 x 16 mantissa pairs occur)
    special = floats(both_signs(bits_of([0.0, 1.0, np.inf, 1e-45, 3.4028234663852886e38]))).tolist() + [np.nan]
    sx, sy = (a.reshape(-1).astype(f32) for a in np.meshgrid(special, special))  # the quadrant and zero cases of atan2
    i = np.arange(len(r))
    per_x = (MAX_N - len(sx)) // len(r)
    j = np.arange(per_x)
    yi = j[None, :] * 16 + ((i + i // 16) % 16)[:, None]
    return np.concatenate([np.repeat(r, per_x), sx]), np.concatenate([r[yi.reshape(-1)], sy])
