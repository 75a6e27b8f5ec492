"""The guided upsampling's contract (include/pbrs_gpu.h, pbrs_upsample) on the CPU model tests/upsample_model.py: what the header's
text promises, the ctypes mirror and the exports, and the quality case of the oracle's Cornell box."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pbrs_amd
import upsample_model as um
from oracle.binding import OracleScene
from pbrs_amd import api, scenes
from test_denoise_model import oracle_guides

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 7
CASES = [(f, R) for f in um.FACTORS for R in um.RADII]


def bound(R):
    """The relative error of a constant image: the S side's (2R)^2 products and (2R)^2 additions, the W side's additions (which the
    S side's count covers), the reciprocal and the product, half an ulp each: (2 * (2R)^2 + 2) * 2^-24."""
    return (2 * (2 * R) ** 2 + 2) * 2.0 ** -24


@pytest.mark.parametrize("f,R", CASES)
def test_a_constant_image_stays_constant_under_random_guides(f, R):
    w, h = 23, 17
    _, lo, hi = um.synthetic(w, h, f, 11 + f, plant=False)
    wl, hl = um.low_size(w, h, f)
    value = np.array([0.7, 1.9, 0.031], dtype=f32)
    rgb_lo = np.broadcast_to(value, (hl, wl, 3)).copy()
    for g in (dict(lo=lo, hi=hi, id_stop=True), dict(lo={"depth": lo["depth"]}, hi={"depth": hi["depth"]}), {}):
        for mw in (0.0, 1e-3):
            out = um.upsample(rgb_lo, w, h, f, radius=R, min_weight=mw, **g)
            rel = np.abs(out.astype(np.float64) / value.astype(np.float64) - 1.0).max()
            assert rel <= bound(R), (f, R, mw, rel, bound(R))


@pytest.mark.parametrize("f,R", CASES)
@pytest.mark.parametrize("j", (-6, 6))
def test_the_scale_rule_holds_bit_for_bit(f, R, j):
    w, h = 21, 18
    rgb_lo, lo, hi = um.synthetic(w, h, f, 20 + f, plant=False)
    kw = dict(lo=lo, hi=hi, radius=R, demodulate=True, id_stop=True)
    a = um.upsample(rgb_lo, w, h, f, **kw)
    b = um.upsample((rgb_lo * f32(2.0 ** j)).astype(f32), w, h, f, **kw)
    assert np.array_equal((a * f32(2.0 ** j)).astype(f32).view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("f", um.FACTORS)
def test_no_guides_at_radius_1_is_bilinear_interpolation(f):
    w, h = 19, 14
    rgb_lo, _, _ = um.synthetic(w, h, f, 30 + f, plant=False)
    wl, hl = um.low_size(w, h, f)
    out = um.tent(rgb_lo, w, h, f, radius=1)
    # float64 bilinear interpolation between the low pixels' centres, renormalised over the taps inside the image (clamping the
    # coordinate does the same for a tent of radius 1)
    c = rgb_lo.astype(np.float64)
    u = np.clip((np.arange(w) + 0.5) / f - 0.5, 0.0, wl - 1.0)
    v = np.clip((np.arange(h) + 0.5) / f - 0.5, 0.0, hl - 1.0)
    x0, y0 = np.minimum(np.floor(u).astype(int), max(wl - 2, 0)), np.minimum(np.floor(v).astype(int), max(hl - 2, 0))
    x1, y1 = np.minimum(x0 + 1, wl - 1), np.minimum(y0 + 1, hl - 1)
    ax, ay = (u - x0)[None, :, None], (v - y0)[:, None, None]
    ref = ((c[y0][:, x0] * (1 - ax) + c[y0][:, x1] * ax) * (1 - ay) + (c[y1][:, x0] * (1 - ax) + c[y1][:, x1] * ax) * ay)
    assert np.abs(out - ref).max() <= 12 * 2.0 ** -24 * np.abs(c).max()


@pytest.mark.parametrize("f,edge", ((2, 5), (4, 7), (3, 8)))
@pytest.mark.parametrize("R", um.RADII)
def test_no_bleed_across_an_id_edge_that_is_off_the_low_grid(f, edge, R):
    w, h = 24, 9
    wl, hl = um.low_size(w, h, f)
    left, right = np.array([0.25, 0.5, 1.0], dtype=f32), np.array([3.0, 1.5, 0.125], dtype=f32)
    ids_hi = np.broadcast_to((np.arange(w) >= edge).astype(np.uint32), (h, w)).copy()
    # a low pixel belongs to the side its centre lies on, and holds that side's colour
    ids_lo = np.broadcast_to((((np.arange(wl) + 0.5) * f) >= edge).astype(np.uint32), (hl, wl)).copy()
    rgb_lo = np.where(ids_lo[..., None] == 1, right, left).astype(f32)
    want = np.where(ids_hi[..., None] == 1, right, left).astype(np.float64)
    out = um.upsample(rgb_lo, w, h, f, lo={"instance": ids_lo}, hi={"instance": ids_hi}, radius=R, id_stop=True)
    assert np.abs(out / want - 1.0).max() <= bound(R)
    mixed = um.upsample(rgb_lo, w, h, f, lo={"instance": ids_lo}, hi={"instance": ids_hi}, radius=R, id_stop=False)
    assert np.abs(mixed / want - 1.0).max() > 0.01


@pytest.mark.parametrize("f,R", CASES)
def test_non_finite_inputs_stay_where_they_are(f, R):
    w, h = 22, 20
    rgb_lo, lo, hi = um.synthetic(w, h, f, 40 + f, plant=False)
    wl, hl = um.low_size(w, h, f)
    rgb_lo[2, 3, 1] = np.nan
    rgb_lo[hl - 2, wl - 3] = np.inf
    det = {}
    out = um.upsample(rgb_lo, w, h, f, lo=lo, hi=hi, radius=R, id_stop=True, details=det)
    # the two low pixels stay out of every full pixel that has another tap; one that has none (f = 3, R = 1: the full pixel at a low
    # pixel's very centre has a footprint of that one tap) shows its own low pixel, as the header says
    bad = ~np.isfinite(out).all(axis=2)
    ys, xs = np.nonzero(bad)
    assert (det["V"][bad] == 0).all() and all((y // f, x // f) in ((2, 3), (hl - 2, wl - 3)) for y, x in zip(ys, xs))
    assert bad.sum() == (2 if (f, R) == (3, 1) else 0)
    # a low image of one pixel: the nearest branch shows it
    one = um.upsample(np.full((1, 1, 3), np.nan, dtype=f32), f, f, f, radius=R)
    assert np.isnan(one).all()
    # a non-finite full-resolution guide sends its pixel to the tent branch
    hi2 = {n: a.copy() for n, a in hi.items()}
    hi2["depth"][5, 6] = np.nan
    hi2["normal"][9, 4, 2] = np.nan
    det2 = {}
    out2 = um.upsample(rgb_lo, w, h, f, lo=lo, hi=hi2, radius=R, id_stop=True, details=det2)
    plain = um.tent(rgb_lo, w, h, f, radius=R)
    for y, x in ((5, 6), (9, 4)):
        assert det2["W"][y, x] == 0 and np.array_equal(out2[y, x].view(np.uint32), plain[y, x].view(np.uint32))
    # with a min_weight nothing reaches, the tent branch applies everywhere: the call without guides, bit for bit
    every = um.upsample(rgb_lo, w, h, f, lo=lo, hi=hi2, radius=R, id_stop=True, min_weight=1e30)
    assert np.array_equal(every.view(np.uint32), plain.view(np.uint32))


def test_the_mirror_matches_the_header():
    cls = api.UpsampleParams
    prints = ['printf("%zu\\n", sizeof(pbrs_upsample_params));']
    prints += [f'printf("%zu\\n", offsetof(pbrs_upsample_params, {n}));' for n, _ in cls._fields_]
    consts = ("PBRS_UPSAMPLE_DEMODULATE", "PBRS_UPSAMPLE_ID_STOP", "PBRS_UPSAMPLE_MIN_FACTOR", "PBRS_UPSAMPLE_MAX_FACTOR", "PBRS_UPSAMPLE_MAX_RADIUS")
    prints += [f'printf("%u\\n", {c});' for c in consts]
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "pbrs_gpu.h"\nint main(void) {\n' + "\n".join(prints) + '\nreturn 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        v = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    want = [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_]
    want += [cls.DEMODULATE, cls.ID_STOP, min(cls.FACTORS), max(cls.FACTORS), max(cls.RADII)]
    assert v == want
    assert ctypes.sizeof(cls) == 48
    assert [n for n, _ in cls._fields_] == ["w", "h", "factor", "radius", "flags", "sigma_normal", "sigma_depth", "albedo_floor", "min_weight", "pad"]
    assert (um.DEMODULATE, um.ID_STOP, um.FACTORS, um.RADII) == (cls.DEMODULATE, cls.ID_STOP, cls.FACTORS, cls.RADII)


def test_the_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    for n in ("pbrs_upsample", "pbrs_upsample_device"):
        assert f"int {n}(" in header, n
        assert n in api.GPU_SYMBOLS, n
        assert getattr(lib, n) is not None, n
    assert "void pbrs_upsample_params_default(" in header and "pbrs_upsample_params_default" in api.GPU_SYMBOLS
    assert pbrs_amd.UpsampleParams is api.UpsampleParams and pbrs_amd.scaled_camera is api.scaled_camera
    lib.pbrs_upsample_params_default.argtypes = [ctypes.c_uint32] * 3 + [ctypes.c_void_p]
    lib.pbrs_upsample_params_default.restype = None
    p = api.UpsampleParams()
    ctypes.memset(ctypes.addressof(p), 0xAB, ctypes.sizeof(p))
    lib.pbrs_upsample_params_default(1920, 1080, 3, ctypes.addressof(p))
    assert bytes(p) == bytes(api.UpsampleParams.make(1920, 1080, 3))
    d = {k: um.DEFAULTS[k] for k in ("radius", "sigma_normal", "sigma_depth", "albedo_floor", "min_weight")}
    assert {k: p.as_dict()[k] for k in d} == {k: (f32(v) if isinstance(v, float) else v) for k, v in d.items()}
    assert p.low_size == (640, 360) and api.UpsampleParams.make(5, 7, 2).low_size == (3, 4)


def test_the_scaled_camera_and_the_upscale_argument():
    cam = api.Camera()
    cam.width, cam.height = 13, 8
    cam.center[:], cam.c[:] = (1.0, 2.0, 3.0), (0.1, 0.2, 0.3)
    cam.a[:], cam.b[:] = (0.1, 0.0, 0.7), (0.0, -0.3, 0.0)
    for f in um.FACTORS:
        lo = api.scaled_camera(cam, f)
        assert (lo.width, lo.height) == um.low_size(13, 8, f)
        assert list(lo.center) == list(cam.center) and list(lo.c) == list(cam.c)
        assert [f32(v) for v in lo.a] == [f32(v) * f32(f) for v in cam.a] and [f32(v) for v in lo.b] == [f32(v) * f32(f) for v in cam.b]
    assert (cam.width, cam.height) == (13, 8) and f32(cam.a[0]) == f32(0.1)  # a new camera, the old one untouched
    g = ("albedo", "depth", "instance")
    assert api._upscale_params(None, g) is None
    assert api._upscale_params(3, g) == (3, {})
    assert api._upscale_params({"factor": 4, "radius": 2}, g) == (4, {"radius": 2})
    assert api._upscale_params({"radius": 2}, g) == (2, {"radius": 2})
    with pytest.raises(ValueError):
        api._upscale_params(5, g)
    with pytest.raises(ValueError):
        api._upscale_params(True, g)
    with pytest.raises(TypeError):
        api._upscale_params({"sharpness": 1.0}, g)


@pytest.fixture(scope="module")
def cornell():
    """The oracle's Cornell box at 64 x 64 and at 32 x 32, 16 x 16 strata: the low image with the guides of its own first hits, the
    full-size guides of one sample, and the 64 x 64 reference of another seed."""
    sb_hi, sb_lo = scenes.cornell_scene(width=64, height=64), scenes.cornell_scene(width=32, height=32)
    low, _ = OracleScene(sb_lo).render(16, 16, 5, SEED)
    ref, _ = OracleScene(sb_hi).render(16, 16, 5, SEED + 1000)
    d_lo, i_lo = oracle_guides(sb_lo, 16, 16, SEED)
    d_hi, i_hi = oracle_guides(sb_hi, 1, 1, SEED)
    return dict(low=low, ref=ref, lo={"depth": d_lo, "instance": i_lo}, hi={"depth": d_hi, "instance": i_hi})


@pytest.mark.parametrize("R", um.RADII)
def test_the_guides_beat_the_plain_tent_on_the_oracles_cornell_box(cornell, R):
    guided = um.upsample(cornell["low"], 64, 64, 2, lo=cornell["lo"], hi=cornell["hi"], radius=R, id_stop=True)
    plain = um.tent(cornell["low"], 64, 64, 2, radius=R)
    e_g, e_p = um.display_error(guided, cornell["ref"]), um.display_error(plain, cornell["ref"])
    print(f"cornell 64 x 64 from 32 x 32, 256 spp, radius {R}: display-referred error guided {e_g:.4g}, plain tent {e_p:.4g}, ratio {e_g / e_p:.3f}")
    assert e_g < e_p


def test_the_min_weight_sweep_of_the_default(cornell):
    """The sweep DESIGN.md records (printed; the default is one of the swept values and every result is finite)."""
    errs = {}
    swept = (0.0, 1e-6, 1e-3, 1e-2)
    assert um.DEFAULTS["min_weight"] in swept
    for mw in swept:
        for R in um.RADII:
            out = um.upsample(cornell["low"], 64, 64, 2, lo=cornell["lo"], hi=cornell["hi"], radius=R, id_stop=True, min_weight=mw)
            errs[mw, R] = um.display_error(out, cornell["ref"])
            print(f"min_weight {mw:g}, radius {R}: display-referred error {errs[mw, R]:.5g}")
    assert all(np.isfinite(e) for e in errs.values())
