"""The bloom call at the C ABI, without a GPU: the ctypes mirror of pbrs_bloom_params against a compiled C file, the entry points and
their symbol table, the filler's bytes against BloomParams.make's, the argument checks of the Python layer that run before any device
call, and the buffers of a sequence with and without the step (include/pbrs_gpu.h, "bloom")."""
import ctypes
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import pbrs_amd
from pbrs_amd import api, libs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["pbrsb_bloom", "pbrsb_bloom_device", "pbrsb_bloom_params_default"]
FIELDS = ["w", "h", "levels", "flags", "threshold", "knee", "strength", "spread"]


def test_the_mirror_matches_the_header():
    cls = api.BloomParams
    prints = ['printf("%zu\\n", sizeof(pbrs_bloom_params));'] + [f'printf("%zu\\n", offsetof(pbrs_bloom_params, {n}));' for n in FIELDS]
    prints += [f'printf("%u\\n", {c});' for c in ("PBRS_BLOOM_MAX_LEVELS", "PBRS_BLOOM_MIX")]
    want = [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n in FIELDS] + [cls.MAX_LEVELS, cls.MIX]
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "pbrs_gpu.h"\nint main(void) {\n' + "\n".join(prints) + '\nreturn 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        v = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert v == want
    assert ctypes.sizeof(cls) == 32 and [n for n, _ in cls._fields_] == FIELDS
    assert [getattr(cls, n).offset for n in FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28] and (cls.MAX_LEVELS, cls.MIX) == (8, 1)


def test_the_entry_points_are_declared_exported_and_typed():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    for n in SYMBOLS[:2]:
        assert f"int {n}(" in header, n
    assert "void pbrsb_bloom_params_default(" in header
    for n in SYMBOLS:
        assert n in api.GPU_BLOOM_SYMBOLS and getattr(lib, n) is not None, n
    loaded = pbrs_amd.gpu_lib()  # the loader sets the new table's types beside the others'
    for n, (argtypes, restype) in libs.GPU_BLOOM_FUNCTIONS.items():
        assert list(getattr(loaded, n).argtypes) == list(argtypes) and getattr(loaded, n).restype is restype, n
    assert libs.GPU_BLOOM_FUNCTIONS["pbrsb_bloom"] == libs.GPU_BLOOM_FUNCTIONS["pbrsb_bloom_device"] == ([ctypes.c_void_p] * 4, ctypes.c_int)
    assert sorted(libs.GPU_BLOOM_SYMBOLS) == SYMBOLS
    # the header's pbrsb_ declarations, the table and the library's pbrsb_ exports are one list
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(pbrsb_[a-z_0-9]+)\s*\(", code))) == SYMBOLS
    nm = subprocess.run(["nm", "-D", "--defined-only", pbrs_amd.lib_paths()[1]], capture_output=True, text=True, check=True).stdout
    assert sorted(line.split()[-1] for line in nm.splitlines() if line.split() and line.split()[-1].startswith("pbrsb_")) == SYMBOLS
    others = set(libs.GPU_SYMBOLS) | set(libs.GPU_COMPARE_SYMBOLS) | set(libs.GPU_DESPECKLE_SYMBOLS)
    assert not set(SYMBOLS) & others
    assert pbrs_amd.BloomParams is api.BloomParams


def test_gpu_symbols_is_the_pinned_surface():
    """The new functions live in a table of their own: GPU_SYMBOLS stays the list tests/golden/api_surface.json pins, and no pbrs_( function
    of the header is new."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "api_surface.json")))
    pinned = [v for v in golden.values() if isinstance(v, list) and "pbrs_create" in v]
    assert pinned and any(sorted(v) == sorted(libs.GPU_SYMBOLS) for v in pinned)
    assert not any(n.startswith("pbrsb_") for n in libs.GPU_SYMBOLS)


def test_the_fillers_bytes_are_makes():
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    lib.pbrsb_bloom_params_default.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.pbrsb_bloom_params_default.restype = None
    p = api.BloomParams()
    ctypes.memset(ctypes.addressof(p), 0xAB, ctypes.sizeof(p))
    lib.pbrsb_bloom_params_default(1920, 1080, ctypes.addressof(p))
    assert bytes(p) == bytes(api.BloomParams.make(1920, 1080))
    f32 = np.float32
    assert p.as_dict() == {"w": 1920, "h": 1080, "levels": 6, "flags": 0, "threshold": 1.0, "knee": 0.5, "strength": float(f32(0.05)), "spread": float(f32(0.6))}
    q = api.BloomParams.make(7, 5, levels=3, threshold=0.0, knee=0.0, strength=0.5, spread=1.0, mix=True)
    assert q.as_dict() == {"w": 7, "h": 5, "levels": 3, "flags": 1, "threshold": 0.0, "knee": 0.0, "strength": 0.5, "spread": 1.0}


class _NoDevice:
    """Stands for the library: any call reaching it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_bad_arguments_are_rejected_before_any_device_call():
    ctx = object.__new__(pbrs_amd.Context)  # no pbrs_create: nothing may reach the device
    ctx._L, ctx._h, ctx.scene = _NoDevice(), None, None
    rgb, cam = np.zeros((4, 6, 3), np.float32), api.Camera()
    with pytest.raises(TypeError):
        ctx.bloom(rgb, sigma=2.0)
    with pytest.raises(ValueError, match=r"\(h, w, 3\)"):
        ctx.bloom(np.zeros((4, 6), np.float32))
    with pytest.raises(TypeError):
        ctx.bloom_device(1, 2, 6, 4, sigma=2.0)
    # the sequences take the keyword out of **params and check it before anything is uploaded, allocated or queued
    with pytest.raises(TypeError):
        next(ctx.render_temporal([cam], 1, 1, 1, [1], bloom={"sigma": 2.0}))
    with pytest.raises(ValueError, match="bloom is None, True or a dict"):
        next(ctx.render_animation([(None, cam, 1)], 1, 1, 1, bloom=3))


def test_the_sequences_buffers_with_and_without():
    assert api._bloom_params(None) is None and api._bloom_params(False) is None
    assert api._bloom_params(True) == {} and api._bloom_params({"levels": 3}) == {"levels": 3}
    for args in ((6, 4, 6, 4, ("depth",), False, False, False), (6, 4, 6, 4, ("depth", "instance"), True, False, True, True, True),
                 (3, 2, 6, 4, ("depth",), False, True, True)):
        plain = api._sequence_buffers(*args)
        assert api._sequence_buffers(*args, bloom=False) == plain and "bloom" not in plain
        sizes = api._sequence_buffers(*args, bloom=True)
        assert sizes["bloom"] == 3 * 6 * 4 * 4  # the first image's size: the film's, also where the chain runs low
        assert {n: v for n, v in sizes.items() if n != "bloom"} == plain and list(sizes)[:-1] == list(plain)
