"""The image comparison at the C ABI, without a GPU: the ctypes mirrors of pbrs_compare_params, pbrs_compare_maps and pbrs_compare_result
against a compiled C file, the entry points, the filler's bytes against CompareParams.make's, and the argument checks of the Python
layer that run before any device call (include/pbrs_gpu.h)."""
import ctypes
import math
import os
import re
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest

import pbrs_amd
from pbrs_amd import api, libs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbrsx_compare", "pbrsx_compare_device")


def test_the_mirrors_match_the_header():
    structs = (("pbrs_compare_params", api.CompareParams), ("pbrs_compare_maps", api.CompareMaps), ("pbrs_compare_result", api.CompareResult))
    prints, want = [], []
    for name, cls in structs:
        prints += [f'printf("%zu\\n", sizeof({name}));'] + [f'printf("%zu\\n", offsetof({name}, {n}));' for n, _ in cls._fields_]
        want += [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_]
    consts = ("PBRS_COMPARE_TILE", "PBRS_COMPARE_LINEAR", "PBRS_COMPARE_REINHARD", "PBRS_COMPARE_SSIM")
    prints += [f'printf("%u\\n", {c});' for c in consts]
    want += [api.CompareParams.TILE, api.CompareParams.TRANSFORMS["linear"], api.CompareParams.TRANSFORMS["reinhard"], api.CompareParams.SSIM]
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "pbrs_gpu.h"\nint main(void) {\n' + "\n".join(prints) + '\nreturn 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        v = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert v == want
    assert ctypes.sizeof(api.CompareParams) == 32 and ctypes.sizeof(api.CompareMaps) == 16 and ctypes.sizeof(api.CompareResult) == 64
    assert [n for n, _ in api.CompareParams._fields_] == ["w", "h", "transform", "flags", "rel_epsilon", "peak", "pad"]
    assert [n for n, _ in api.CompareMaps._fields_] == ["error_out", "ssim_out"]
    assert [n for n, _ in api.CompareResult._fields_] == ["mse", "rel_mse", "mae", "ssim", "max_abs", "n_valid", "n_invalid", "n_ssim", "pad"]
    assert [getattr(api.CompareResult, n).offset for n in ("mse", "rel_mse", "mae", "ssim", "max_abs", "n_valid", "n_invalid", "n_ssim", "pad")] == \
        [0, 8, 16, 24, 32, 40, 44, 48, 52]


def test_the_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    for n in ENTRY_POINTS:
        assert f"int {n}(" in header, n
        assert n in api.GPU_COMPARE_SYMBOLS, n
        assert getattr(lib, n) is not None, n
    assert "void pbrsx_compare_params_default(" in header and "pbrsx_compare_params_default" in api.GPU_COMPARE_SYMBOLS
    assert getattr(lib, "pbrsx_compare_params_default") is not None
    loaded = pbrs_amd.gpu_lib()  # the loader sets the new table's types beside the old one's
    for n, (argtypes, restype) in libs.GPU_COMPARE_FUNCTIONS.items():
        assert list(getattr(loaded, n).argtypes) == list(argtypes) and getattr(loaded, n).restype is restype, n
    assert sorted(libs.GPU_COMPARE_SYMBOLS) == ["pbrsx_compare", "pbrsx_compare_device", "pbrsx_compare_params_default"]
    # what tests/test_abi.py holds for pbrs_: the header's pbrsx_ declarations, the table and the library's pbrsx_ exports are one list
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(pbrsx_[a-z_0-9]+)\s*\(", code))) == sorted(libs.GPU_COMPARE_SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", pbrs_amd.lib_paths()[1]], capture_output=True, text=True, check=True).stdout
    assert sorted(line.split()[-1] for line in nm.splitlines() if line.split() and line.split()[-1].startswith("pbrsx_")) == sorted(libs.GPU_COMPARE_SYMBOLS)
    assert not set(libs.GPU_COMPARE_SYMBOLS) & set(libs.GPU_SYMBOLS)
    assert pbrs_amd.CompareParams is api.CompareParams and pbrs_amd.CompareResult is api.CompareResult


def test_the_fillers_bytes_are_makes():
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    lib.pbrsx_compare_params_default.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.pbrsx_compare_params_default.restype = None
    p = api.CompareParams()
    ctypes.memset(ctypes.addressof(p), 0xAB, ctypes.sizeof(p))
    lib.pbrsx_compare_params_default(1920, 1080, ctypes.addressof(p))
    assert bytes(p) == bytes(api.CompareParams.make(1920, 1080))
    assert p.as_dict() == {"w": 1920, "h": 1080, "transform": 1, "flags": 1, "rel_epsilon": np.float32(1e-2), "peak": 1.0}
    q = api.CompareParams.make(7, 5, transform="linear", ssim=False, rel_epsilon=0.5, peak=4.0)
    assert q.as_dict() == {"w": 7, "h": 5, "transform": 0, "flags": 0, "rel_epsilon": 0.5, "peak": 4.0}


def test_the_result_mirror_reads_a_record():
    r = api.CompareResult.from_buffer_copy(np.array([0.01, 0.5, 0.05, 0.9, 2.0], np.float64).tobytes() + np.array([7, 1, 6, 0, 0, 0], np.uint32).tobytes())
    assert r.as_dict() == {"mse": 0.01, "rel_mse": 0.5, "mae": 0.05, "ssim": 0.9, "max_abs": 2.0, "n_valid": 7, "n_invalid": 1, "n_ssim": 6}
    assert r.psnr() == pytest.approx(20.0) and r.psnr(peak=10.0) == pytest.approx(40.0)
    r.mse = 0.0
    assert r.psnr() == math.inf
    r.mse = math.nan
    assert math.isnan(r.psnr())


class _NoDevice:
    """Stands for the library: any call reaching it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_bad_arguments_are_rejected_before_any_device_call():
    ctx = object.__new__(pbrs_amd.Context)  # no pbrs_create: nothing may reach the device
    ctx._L, ctx._h, ctx.scene = _NoDevice(), None, None
    rgb, cam = np.zeros((4, 6, 3), np.float32), api.Camera()
    with pytest.raises(TypeError):
        ctx.compare(rgb, rgb, gamma=2.2)
    with pytest.raises(KeyError):
        ctx.compare(rgb, rgb, transform="log")
    with pytest.raises(ValueError, match=r"\(h, w, 3\)"):
        ctx.compare(np.zeros((4, 6), np.float32), np.zeros((4, 6), np.float32))
    with pytest.raises(ValueError, match="alike"):
        ctx.compare(rgb, np.zeros((4, 5, 3), np.float32))
    with pytest.raises(ValueError, match="unknown compare map pointer"):
        ctx.compare_device(1, 2, 6, 4, 3, {"error": 4})
    with pytest.raises(TypeError):
        ctx.compare_device(1, 2, 6, 4, 3, gamma=2.2)


def test_a_reference_of_the_wrong_shape_is_refused_before_any_device_call():
    ctx = object.__new__(pbrs_amd.Context)
    ctx._L, ctx._h, ctx.scene = _NoDevice(), None, None
    cam = api.Camera()
    with pytest.raises(ValueError, match=r"the reference is \(h, w, 3\)"):
        next(ctx.render_temporal([cam], 1, 1, 1, [1], reference=np.zeros((4, 6), np.float32)))
    with pytest.raises(ValueError, match=r"the reference is \(h, w, 3\)"):
        next(ctx.render_animation([(None, cam, 1)], 1, 1, 1, reference=np.zeros((4, 6, 4), np.float32)))
    # a single array of another size than the uploaded scene's film: refused by render_temporal itself, before anything is queued
    ctx.scene = SimpleNamespace(width=6, height=8)
    with pytest.raises(ValueError, match=r"frame 0's reference is \(8, 6, 3\), not \(4, 6, 3\)"):
        next(ctx.render_temporal([cam], 1, 1, 1, [1], reference=np.zeros((4, 6, 3), np.float32)))
    # an iterable's frames, and render_animation's (whose film comes with each frame's scene): refused when the frame comes up, before
    # its buffers and its launches
    frames = api._reference_frames([np.zeros((4, 6, 3), np.float32)])
    with pytest.raises(ValueError, match=r"frame 0's reference is \(8, 6, 3\)"):
        api._reference_frame(frames, 0, 6, 8)
    with pytest.raises(ValueError, match="the reference ends before frame 1"):
        api._reference_frame(frames, 1, 6, 8)
    assert api._reference_frames(None) is None
    sizes = api._sequence_buffers(6, 4, 6, 4, ("depth",), False, False, False, True)
    assert sizes["reference"] == 3 * 6 * 4 * 4 and sizes["compare"] == 64
    assert "reference" not in api._sequence_buffers(6, 4, 6, 4, ("depth",), False, False, False)
