"""The depth-of-field call at the C ABI, without a GPU: the ctypes mirror of pbrs_dof_params against a compiled C file, the entry points
and their symbol table, the filler's bytes against DofParams.make's, the argument checks of the Python layer that run before any device
call, and the buffers of a sequence with and without the step (include/pbrs_gpu.h, "depth of field")."""
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
SYMBOLS = ["pbrsf_dof", "pbrsf_dof_device", "pbrsf_dof_params_default"]
FIELDS = ["w", "h", "max_radius", "flags", "focus", "scale", "reserved"]


def test_the_mirror_matches_the_header():
    cls = api.DofParams
    prints = ['printf("%zu\\n", sizeof(pbrs_dof_params));'] + [f'printf("%zu\\n", offsetof(pbrs_dof_params, {n}));' for n in FIELDS]
    prints += ['printf("%u\\n", PBRS_DOF_MAX_RADIUS);']
    want = [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n in FIELDS] + [cls.MAX_RADIUS]
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "pbrs_gpu.h"\nint main(void) {\n' + "\n".join(prints) + '\nreturn 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        v = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert v == want
    assert v[0] == 32 and ctypes.sizeof(cls) == 32 and [n for n, _ in cls._fields_] == FIELDS
    assert [getattr(cls, n).offset for n in FIELDS] == [0, 4, 8, 12, 16, 20, 24] and cls.MAX_RADIUS == 16


def test_the_entry_points_are_declared_exported_and_typed():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    for n in SYMBOLS[:2]:
        assert f"int {n}(" in header, n
    assert "void pbrsf_dof_params_default(" in header
    for n in SYMBOLS:
        assert n in api.GPU_DOF_SYMBOLS and getattr(lib, n) is not None, n
    loaded = pbrs_amd.gpu_lib()  # the loader sets the new table's types beside the others'
    for n, (argtypes, restype) in libs.GPU_DOF_FUNCTIONS.items():
        assert list(getattr(loaded, n).argtypes) == list(argtypes) and getattr(loaded, n).restype is restype, n
    assert libs.GPU_DOF_FUNCTIONS["pbrsf_dof"] == libs.GPU_DOF_FUNCTIONS["pbrsf_dof_device"] == ([ctypes.c_void_p] * 6, ctypes.c_int)
    assert sorted(libs.GPU_DOF_SYMBOLS) == SYMBOLS
    # the header's pbrsf_ declarations, the table and the library's pbrsf_ exports are one list
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(pbrsf_[a-z_0-9]+)\s*\(", code))) == SYMBOLS
    nm = subprocess.run(["nm", "-D", "--defined-only", pbrs_amd.lib_paths()[1]], capture_output=True, text=True, check=True).stdout
    assert sorted(line.split()[-1] for line in nm.splitlines() if line.split() and line.split()[-1].startswith("pbrsf_")) == SYMBOLS
    others = set(libs.GPU_SYMBOLS) | set(libs.GPU_COMPARE_SYMBOLS) | set(libs.GPU_DESPECKLE_SYMBOLS) | set(libs.GPU_BLOOM_SYMBOLS)
    assert not set(SYMBOLS) & others
    assert pbrs_amd.DofParams is api.DofParams and pbrs_amd.lens is api.lens


def test_gpu_symbols_is_the_pinned_surface():
    """The new functions live in a table of their own: GPU_SYMBOLS stays the list tests/golden/api_surface.json pins, and no pbrs_( function
    of the header is new."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "api_surface.json")))
    pinned = [v for v in golden.values() if isinstance(v, list) and "pbrs_create" in v]
    assert pinned and any(sorted(v) == sorted(libs.GPU_SYMBOLS) for v in pinned)
    assert not any(n.startswith("pbrsf_") for n in libs.GPU_SYMBOLS)


def test_the_fillers_bytes_are_makes():
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    lib.pbrsf_dof_params_default.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.pbrsf_dof_params_default.restype = None
    p = api.DofParams()
    ctypes.memset(ctypes.addressof(p), 0xAB, ctypes.sizeof(p))
    lib.pbrsf_dof_params_default(1920, 1080, ctypes.addressof(p))
    assert bytes(p) == bytes(api.DofParams.make(1920, 1080))
    assert p.as_dict() == {"w": 1920, "h": 1080, "max_radius": 8, "flags": 0, "focus": 1.0, "scale": 0.0} and list(p.reserved) == [0, 0]
    q = api.DofParams.make(7, 5, max_radius=16, focus=2.5, scale=12.0)
    assert q.as_dict() == {"w": 7, "h": 5, "max_radius": 16, "flags": 0, "focus": 2.5, "scale": 12.0}


class _NoDevice:
    """Stands for the library: any call reaching it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_bad_arguments_are_rejected_before_any_device_call():
    ctx = object.__new__(pbrs_amd.Context)  # no pbrs_create: nothing may reach the device
    ctx._L, ctx._h, ctx.scene = _NoDevice(), None, None
    rgb, depth, cam = np.zeros((4, 6, 3), np.float32), np.ones((4, 6), np.float32), api.Camera()
    with pytest.raises(TypeError):
        ctx.dof(rgb, depth, sigma=2.0)
    with pytest.raises(ValueError, match=r"\(h, w, 3\)"):
        ctx.dof(np.zeros((4, 6), np.float32), depth)
    with pytest.raises(ValueError, match="like the image"):
        ctx.dof(rgb, np.ones((6, 4), np.float32))
    with pytest.raises(TypeError):
        ctx.dof_device(1, 2, 3, 6, 4, sigma=2.0)
    # focus_pixel reads the depth on the host: outside the image, on a miss, on an unknown depth, and beside `focus`
    for bad in (np.inf, 0.0, -1.0, np.nan):
        d = depth.copy()
        d[2, 5] = bad
        with pytest.raises(ValueError, match="nothing to focus on"):
            ctx.dof(rgb, d, focus_pixel=(5, 2), scale=1.0)
    with pytest.raises(ValueError, match="outside"):
        ctx.dof(rgb, depth, focus_pixel=(6, 2), scale=1.0)
    with pytest.raises(ValueError, match="give one"):
        ctx.dof(rgb, depth, focus_pixel=(1, 1), focus=2.0)
    # the sequences take the keyword out of **params and check it before anything is uploaded, allocated or queued
    with pytest.raises(TypeError):
        next(ctx.render_temporal([cam], 1, 1, 1, [1], dof={"sigma": 2.0}))
    with pytest.raises(TypeError):
        next(ctx.render_temporal([cam], 1, 1, 1, [1], dof=[{"scale": 1.0}, {"sigma": 2.0}]))
    with pytest.raises(ValueError, match="dof is None, a dict"):
        next(ctx.render_animation([(None, cam, 1)], 1, 1, 1, dof=3))
    with pytest.raises(ValueError, match="dof is None, a dict"):
        next(ctx.render_animation([(None, cam, 1)], 1, 1, 1, dof=[]))


def test_the_sequences_buffers_with_and_without():
    assert api._dof_params(None) is None and api._dof_params(False) is None
    one = api._dof_params({"scale": 3.0})
    assert one(0) == one(7) == {"scale": 3.0}
    pull = api._dof_params([{"focus": 1.0, "scale": 3.0}, {"focus": 2.0, "scale": 3.0}])
    assert pull(0)["focus"] == 1.0 and pull(1)["focus"] == 2.0
    with pytest.raises(ValueError, match="none for frame 2"):
        pull(2)
    for args in ((6, 4, 6, 4, ("depth",), False, False, False), (6, 4, 6, 4, ("depth", "instance"), True, False, True, True, True, True),
                 (3, 2, 6, 4, ("depth",), False, True, True)):
        plain = api._sequence_buffers(*args)
        assert api._sequence_buffers(*args, dof=False) == plain and "dof" not in plain
        sizes = api._sequence_buffers(*args, dof=True)
        assert sizes["dof"] == 3 * 6 * 4 * 4  # the first image's size: the film's, also where the chain runs low
        assert {n: v for n, v in sizes.items() if n != "dof"} == plain and list(sizes)[:-1] == list(plain)
