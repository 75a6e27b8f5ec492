"""The despeckle call at the C ABI, without a GPU: the ctypes mirrors of pbrs_despeckle_params, pbrs_despeckle_io and
pbrs_despeckle_result against a compiled C file, the entry points and their symbol table, the filler's bytes against
DespeckleParams.make's, and the argument checks of the Python layer that run before any device call (include/pbrs_gpu.h)."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import pbrs_amd
from pbrs_amd import abi, api, libs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbrsi_despeckle", "pbrsi_despeckle_device")
PLANES = ["rgb_in", "rgb_out", "variance_in", "variance_out", "mask_out", "removed_out"]


def test_the_mirrors_match_the_header():
    structs = (("pbrs_despeckle_params", api.DespeckleParams), ("pbrs_despeckle_io", api.DespeckleIO), ("pbrs_despeckle_result", api.DespeckleResult))
    prints, want = [], []
    for name, cls in structs:
        prints += [f'printf("%zu\\n", sizeof({name}));'] + [f'printf("%zu\\n", offsetof({name}, {n}));' for n, _ in cls._fields_]
        want += [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_]
    consts = ("PBRS_DESPECKLE_TILE", "PBRS_DESPECKLE_CLAMPED", "PBRS_DESPECKLE_REPAIRED", "PBRS_DESPECKLE_MAX_RADIUS", "PBRS_DESPECKLE_MAX_RANK")
    prints += [f'printf("%u\\n", {c});' for c in consts]
    want += [api.DespeckleParams.TILE, api.DespeckleParams.CLAMPED, api.DespeckleParams.REPAIRED, 2, 4]
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "pbrs_gpu.h"\nint main(void) {\n' + "\n".join(prints) + '\nreturn 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        v = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert v == want
    assert ctypes.sizeof(api.DespeckleParams) == 32 and ctypes.sizeof(api.DespeckleIO) == 48 and ctypes.sizeof(api.DespeckleResult) == 16
    assert [n for n, _ in api.DespeckleParams._fields_] == ["w", "h", "radius", "rank", "gain", "floor", "flags", "pad"]
    assert [n for n, _ in api.DespeckleIO._fields_] == PLANES == list(abi.DESPECKLE_PLANES)
    assert [n for n, _ in api.DespeckleResult._fields_] == ["n_clamped", "n_repaired", "pad"]
    assert [getattr(api.DespeckleResult, n).offset for n in ("n_clamped", "n_repaired", "pad")] == [0, 4, 8]


def test_the_entry_points_are_declared_exported_and_typed():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    for n in ENTRY_POINTS:
        assert f"int {n}(" in header, n
        assert n in api.GPU_DESPECKLE_SYMBOLS, n
        assert getattr(lib, n) is not None, n
    assert "void pbrsi_despeckle_params_default(" in header and "pbrsi_despeckle_params_default" in api.GPU_DESPECKLE_SYMBOLS
    assert getattr(lib, "pbrsi_despeckle_params_default") is not None
    loaded = pbrs_amd.gpu_lib()  # the loader sets the new table's types beside the others'
    for n, (argtypes, restype) in libs.GPU_DESPECKLE_FUNCTIONS.items():
        assert list(getattr(loaded, n).argtypes) == list(argtypes) and getattr(loaded, n).restype is restype, n
    assert libs.GPU_DESPECKLE_FUNCTIONS["pbrsi_despeckle"] == libs.GPU_DESPECKLE_FUNCTIONS["pbrsi_despeckle_device"] == ([ctypes.c_void_p] * 4, ctypes.c_int)
    assert sorted(libs.GPU_DESPECKLE_SYMBOLS) == ["pbrsi_despeckle", "pbrsi_despeckle_device", "pbrsi_despeckle_params_default"]
    # the header's pbrsi_ declarations, the table and the library's pbrsi_ exports are one list
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(pbrsi_[a-z_0-9]+)\s*\(", code))) == sorted(libs.GPU_DESPECKLE_SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", pbrs_amd.lib_paths()[1]], capture_output=True, text=True, check=True).stdout
    assert sorted(line.split()[-1] for line in nm.splitlines() if line.split() and line.split()[-1].startswith("pbrsi_")) == sorted(libs.GPU_DESPECKLE_SYMBOLS)
    assert not set(libs.GPU_DESPECKLE_SYMBOLS) & set(libs.GPU_SYMBOLS) and not set(libs.GPU_DESPECKLE_SYMBOLS) & set(libs.GPU_COMPARE_SYMBOLS)
    assert pbrs_amd.DespeckleParams is api.DespeckleParams and pbrs_amd.DespeckleResult is api.DespeckleResult


def test_the_fillers_bytes_are_makes():
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    lib.pbrsi_despeckle_params_default.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.pbrsi_despeckle_params_default.restype = None
    p = api.DespeckleParams()
    ctypes.memset(ctypes.addressof(p), 0xAB, ctypes.sizeof(p))
    lib.pbrsi_despeckle_params_default(1920, 1080, ctypes.addressof(p))
    assert bytes(p) == bytes(api.DespeckleParams.make(1920, 1080))
    assert p.as_dict() == {"w": 1920, "h": 1080, "radius": 1, "rank": 2, "gain": 2.0, "floor": 0.0, "flags": 0}
    q = api.DespeckleParams.make(7, 5, radius=2, rank=4, gain=1.5, floor=0.25)
    assert q.as_dict() == {"w": 7, "h": 5, "radius": 2, "rank": 4, "gain": 1.5, "floor": 0.25, "flags": 0}


def test_the_result_mirror_reads_a_record():
    r = api.DespeckleResult.from_buffer_copy(np.array([7, 3, 0, 0], np.uint32).tobytes())
    assert r.as_dict() == {"n_clamped": 7, "n_repaired": 3}


class _NoDevice:
    """Stands for the library: any call reaching it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_bad_arguments_are_rejected_before_any_device_call():
    ctx = object.__new__(pbrs_amd.Context)  # no pbrs_create: nothing may reach the device
    ctx._L, ctx._h, ctx.scene = _NoDevice(), None, None
    rgb, cam = np.zeros((4, 6, 3), np.float32), api.Camera()
    with pytest.raises(TypeError):
        ctx.despeckle(rgb, sigma=2.0)
    with pytest.raises(ValueError, match=r"\(h, w, 3\)"):
        ctx.despeckle(np.zeros((4, 6), np.float32))
    with pytest.raises(ValueError, match=r"the variance is \(4, 6\)"):
        ctx.despeckle(rgb, np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError, match="unknown despeckle plane pointer"):
        ctx.despeckle_device(1, 2, 6, 4, 3, {"mask": 4})
    with pytest.raises(TypeError):
        ctx.despeckle_device(1, 2, 6, 4, 3, sigma=2.0)
    # the sequences take the keyword out of **params and check it before anything is uploaded, allocated or queued
    with pytest.raises(TypeError):
        next(ctx.render_temporal([cam], 1, 1, 1, [1], despeckle={"sigma": 2.0}))
    with pytest.raises(ValueError, match="despeckle is None, True or a dict"):
        next(ctx.render_animation([(None, cam, 1)], 1, 1, 1, despeckle=3))


def test_the_sequences_buffers_with_and_without():
    assert api._despeckle_params(None) is None and api._despeckle_params(False) is None
    assert api._despeckle_params(True) == {} and api._despeckle_params({"rank": 3}) == {"rank": 3}
    plain = api._sequence_buffers(6, 4, 6, 4, ("depth",), False, False, False)
    sizes = api._sequence_buffers(6, 4, 6, 4, ("depth",), False, False, False, False, True)
    assert sizes["despeckled"] == 3 * 6 * 4 * 4 and sizes["despeckle"] == 16
    assert {n: v for n, v in sizes.items() if n not in ("despeckled", "despeckle")} == plain and "despeckled" not in plain
    low = api._sequence_buffers(3, 2, 6, 4, ("depth",), False, True, False, False, True)  # the chain's size, not the film's
    assert low["despeckled"] == 3 * 3 * 2 * 4
