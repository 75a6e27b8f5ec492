"""Temporal accumulation at the C ABI, without a GPU: the ctypes mirrors of the pbrs_temporal_* structs against a compiled C file, the
two entry points, and the argument checks of the Python layer that run before any device call (include/pbrs_gpu.h)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pbrs_amd
from pbrs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbrs_temporal_accumulate", "pbrs_temporal_accumulate_device")
STRUCTS = (("pbrs_temporal_params", api.TemporalParams), ("pbrs_temporal_frame", api.TemporalFrame),
           ("pbrs_temporal_guides", api.TemporalGuides), ("pbrs_temporal_history", api.TemporalHistory))


def test_temporal_mirrors_match_the_header():
    prints = []
    for cname, cls in STRUCTS:
        prints.append(f'printf("%zu\\n", sizeof({cname}));')
        prints += [f'printf("%zu\\n", offsetof({cname}, {n}));' for n, _ in cls._fields_]
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "pbrs_gpu.h"\nint main(void) {\n' + "\n".join(prints) + \
          '\nprintf("%u\\n", PBRS_TEMPORAL_ID_TEST);\nreturn 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        v = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    want = []
    for _, cls in STRUCTS:
        want.append(ctypes.sizeof(cls))
        want += [getattr(cls, n).offset for n, _ in cls._fields_]
    assert v == want + [api.TemporalParams.ID_TEST]
    assert ctypes.sizeof(api.TemporalParams) == 32
    assert [n for n, _ in api.TemporalFrame._fields_] == list(api.TEMPORAL_FRAME)
    assert [n for n, _ in api.TemporalGuides._fields_] == list(api.TEMPORAL_GUIDES)
    assert [n for n, _ in api.TemporalHistory._fields_] == list(api.TEMPORAL_HISTORY)


def test_temporal_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    for n in ENTRY_POINTS:
        assert f"int {n}(" in header, n
        assert n in api.GPU_SYMBOLS, n
        assert getattr(lib, n) is not None, n


def test_the_defaults_are_the_documented_ones():
    p = api.TemporalParams.make(7, 5)
    assert p.as_dict() == {"w": 7, "h": 5, "flags": 0, "max_history": 32.0, "depth_tolerance": np.float32(0.05),
                           "normal_tolerance": np.float32(0.3), "min_temporal": 4.0, "pad": 0}
    assert api.TemporalParams.make(1, 1, id_test=True).flags == 1


class _NoDevice:
    """Stands for the library: any call reaching it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_bad_arguments_are_rejected_before_any_device_call():
    ctx = object.__new__(pbrs_amd.Context)  # no pbrs_create: nothing may reach the device
    ctx._L, ctx._h, ctx.scene = _NoDevice(), None, None
    rgb, z, cam = np.zeros((4, 6, 3), np.float32), np.ones((4, 6), np.float32), api.Camera()
    with pytest.raises(ValueError, match="frame plane normal of shape"):
        ctx.temporal_accumulate(rgb, z, cam, normal=np.zeros((4, 6), np.float32))
    with pytest.raises(ValueError, match="unknown history plane"):
        ctx.temporal_accumulate(rgb, z, cam, history={"colour": rgb}, prev={"depth": z}, camera_prev=cam)
    with pytest.raises(ValueError, match="unknown previous guide plane"):
        ctx.temporal_accumulate_device({"rgb": 1, "depth": 2}, {"rgb": 3, "moments": 4, "length": 5}, 6, 4, cam, {"rgb": 6, "moments": 7, "length": 8},
                                       {"albedo": 9}, cam)
    with pytest.raises(TypeError):
        ctx.temporal_accumulate(rgb, z, cam, sigma_depth=1.0)
    with pytest.raises(ValueError, match="depth"):
        next(ctx.render_temporal([cam], 1, 1, 1, [1], guides=("normal",)))
    with pytest.raises(ValueError, match="seeds"):
        next(ctx.render_temporal([cam, cam], 1, 1, 1, [1]))
