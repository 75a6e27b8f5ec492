"""The display transform at the C ABI, without a GPU: the ctypes mirrors of pbrs_display_params and pbrs_display_io against a compiled C
file, the entry points, the filler's defaults against DisplayParams.make's, the new export of the host library, and the argument checks
of the Python layer that run before any device call (include/pbrs_gpu.h, include/pbrs_host.h)."""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pbrs_amd
from pbrs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbrs_display", "pbrs_display_device")


def test_the_mirrors_match_the_header():
    cls, io = api.DisplayParams, api.DisplayIO
    prints = ['printf("%zu\\n", sizeof(pbrs_display_params));']
    prints += [f'printf("%zu\\n", offsetof(pbrs_display_params, {n}));' for n, _ in cls._fields_]
    prints += ['printf("%zu\\n", sizeof(pbrs_display_io));']
    prints += [f'printf("%zu\\n", offsetof(pbrs_display_io, {n}));' for n, _ in io._fields_]
    consts = ("PBRS_DISPLAY_BINS", "PBRS_CURVE_NONE", "PBRS_CURVE_REINHARD", "PBRS_CURVE_ACES", "PBRS_ENCODE_SQRT", "PBRS_ENCODE_SRGB",
              "PBRS_QUANT_TRUNC", "PBRS_QUANT_ROUND", "PBRS_QUANT_DITHER", "PBRS_DISPLAY_AUTO_EXPOSURE")
    prints += [f'printf("%u\\n", {c});' for c in consts]
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "pbrs_gpu.h"\nint main(void) {\n' + "\n".join(prints) + '\nreturn 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        v = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    want = [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_]
    want += [ctypes.sizeof(io)] + [getattr(io, n).offset for n, _ in io._fields_]
    want += [cls.BINS, cls.CURVES["none"], cls.CURVES["reinhard"], cls.CURVES["aces"], cls.ENCODES["sqrt"], cls.ENCODES["srgb"],
             cls.QUANTIZERS["trunc"], cls.QUANTIZERS["round"], cls.QUANTIZERS["dither"], cls.AUTO_EXPOSURE]
    assert v == want
    assert ctypes.sizeof(cls) == 64 and ctypes.sizeof(io) == 24
    assert [n for n, _ in cls._fields_] == ["w", "h", "curve", "encode", "quantize", "flags", "exposure", "key", "white", "min_exposure", "max_exposure",
                                            "adapt", "low_q16", "high_q16", "pad"]
    assert [n for n, _ in io._fields_] == ["exposure_in", "exposure_out", "histogram_out"]


def test_the_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    for n in ENTRY_POINTS:
        assert f"int {n}(" in header, n
        assert n in api.GPU_SYMBOLS, n
        assert getattr(lib, n) is not None, n
    assert "void pbrs_display_params_default(" in header and "pbrs_display_params_default" in api.GPU_SYMBOLS
    host_header = open(os.path.join(ROOT, "include", "pbrs_host.h")).read()
    assert "int pbrs_host_write_png_rgba8(" in host_header and "pbrs_host_write_png_rgba8" in api.HOST_SYMBOLS
    assert getattr(ctypes.CDLL(pbrs_amd.lib_paths()[0]), "pbrs_host_write_png_rgba8") is not None
    assert pbrs_amd.write_image_u8 is api.write_image_u8 and pbrs_amd.DisplayParams is api.DisplayParams


def test_the_fillers_defaults_are_makes():
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    lib.pbrs_display_params_default.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.pbrs_display_params_default.restype = None
    p = api.DisplayParams()
    ctypes.memset(ctypes.addressof(p), 0xAB, ctypes.sizeof(p))
    lib.pbrs_display_params_default(1920, 1080, ctypes.addressof(p))
    assert bytes(p) == bytes(api.DisplayParams.make(1920, 1080))
    assert p.as_dict() == {"w": 1920, "h": 1080, "curve": 2, "encode": 1, "quantize": 1, "flags": 0, "exposure": 1.0, "key": np.float32(0.18),
                           "white": math.inf, "min_exposure": 2.0 ** -20, "max_exposure": 2.0 ** 20, "adapt": 1.0, "low_q16": 6554, "high_q16": 62259}
    q = api.DisplayParams.make(7, 5, curve="reinhard", encode="sqrt", quantize="dither", auto=True, exposure=2.0, key=0.25, white=4.0,
                               min_exposure=0.5, max_exposure=8.0, adapt=0.25, low_q16=0, high_q16=65536)
    assert q.as_dict() == {"w": 7, "h": 5, "curve": 1, "encode": 0, "quantize": 2, "flags": 1, "exposure": 2.0, "key": 0.25, "white": 4.0,
                           "min_exposure": 0.5, "max_exposure": 8.0, "adapt": 0.25, "low_q16": 0, "high_q16": 65536}
    assert api._display_params(None) is None and api._display_params(False) is None
    assert api._display_params(True) == {"auto": True}
    assert api._display_params({"curve": "none", "auto": False}) == {"curve": "none", "auto": False}


class _NoDevice:
    """Stands for the library: any call reaching it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_bad_arguments_are_rejected_before_any_device_call():
    ctx = object.__new__(pbrs_amd.Context)  # no pbrs_create: nothing may reach the device
    ctx._L, ctx._h, ctx.scene = _NoDevice(), None, None
    rgb, cam = np.zeros((4, 6, 3), np.float32), api.Camera()
    with pytest.raises(TypeError):
        ctx.display(rgb, gamma=2.2)
    with pytest.raises(KeyError):
        ctx.display(rgb, curve="filmic")
    with pytest.raises(ValueError, match=r"\(h, w, 3\)"):
        ctx.display(np.zeros((4, 6), np.float32))
    with pytest.raises(ValueError, match="unknown display io pointer"):
        ctx.display_device(1, 2, 6, 4, {"exposure": 3})
    with pytest.raises(TypeError):
        next(ctx.render_temporal([cam], 1, 1, 1, [1], display={"gamma": 2.2}))
    with pytest.raises(ValueError, match="display is None, True"):
        next(ctx.render_animation([(None, cam, 1)], 1, 1, 1, display=2.2))
    with pytest.raises(ValueError, match="uint8"):
        api.write_image_u8("unused.png", np.zeros((4, 6, 3), np.float32))
