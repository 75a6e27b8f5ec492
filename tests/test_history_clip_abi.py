"""History clipping at the C ABI, without a GPU: the ctypes mirror of pbrs_history_clip_params against a compiled C file, the two entry
points, the defaults, and the argument checks of the Python layer that run before any device call (include/pbrs_gpu.h)."""
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
ENTRY_POINTS = ("pbrs_temporal_accumulate_clip", "pbrs_temporal_accumulate_clip_device")


def test_the_mirror_matches_the_header():
    cls = api.HistoryClipParams
    prints = ['printf("%zu\\n", sizeof(pbrs_history_clip_params));']
    prints += [f'printf("%zu\\n", offsetof(pbrs_history_clip_params, {n}));' for n, _ in cls._fields_]
    prints += ['printf("%zu\\n", sizeof(pbrs_temporal_params));', 'printf("%u\\n", PBRS_CLIP_MAX_RADIUS);']
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "pbrs_gpu.h"\nint main(void) {\n' + "\n".join(prints) + '\nreturn 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        v = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert v == [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_] + [32, cls.MAX_RADIUS]
    assert ctypes.sizeof(cls) == 16 and [n for n, _ in cls._fields_] == ["radius", "gamma", "clip_history", "flags"]
    assert ctypes.sizeof(api.TemporalParams) == 32


def test_the_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    for n in ENTRY_POINTS:
        assert f"int {n}(" in header, n
        assert n in api.GPU_SYMBOLS, n
        assert getattr(lib, n) is not None, n


def test_the_defaults_are_the_documented_ones():
    assert api.HistoryClipParams.make().as_dict() == {"radius": 1, "gamma": 1.0, "clip_history": math.inf, "flags": 0}
    assert api.HistoryClipParams.make(radius=3, gamma=2.0, clip_history=4.0).as_dict() == {"radius": 3, "gamma": 2.0, "clip_history": 4.0, "flags": 0}
    assert pbrs_amd.HistoryClipParams is api.HistoryClipParams
    assert api._history_clip(None) is None and api._history_clip(False) is None
    assert api._history_clip(True).as_dict() == api.HistoryClipParams.make().as_dict()
    assert api._history_clip({"gamma": 1.5}).as_dict() == {"radius": 1, "gamma": 1.5, "clip_history": math.inf, "flags": 0}
    own = api.HistoryClipParams.make(radius=2)
    assert api._history_clip(own) is own
    # the temporal params are as tests/test_temporal_abi.py pins them
    assert api.TemporalParams.make(7, 5).as_dict() == {"w": 7, "h": 5, "flags": 0, "max_history": 32.0, "depth_tolerance": np.float32(0.05),
                                                       "normal_tolerance": np.float32(0.3), "min_temporal": 4.0, "pad": 0}


class _NoDevice:
    """Stands for the library: any call reaching it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_a_bad_clip_is_rejected_before_any_device_call():
    ctx = object.__new__(pbrs_amd.Context)  # no pbrs_create: nothing may reach the device
    ctx._L, ctx._h, ctx.scene = _NoDevice(), None, None
    rgb, z, cam = np.zeros((4, 6, 3), np.float32), np.ones((4, 6), np.float32), api.Camera()
    with pytest.raises(TypeError):
        ctx.temporal_accumulate(rgb, z, cam, clip={"sigma": 1.0})
    with pytest.raises(ValueError, match="clip is None, True"):
        ctx.temporal_accumulate(rgb, z, cam, clip=1.5)
    with pytest.raises(TypeError):
        ctx.temporal_accumulate_device({"rgb": 1, "depth": 2}, {"rgb": 3, "moments": 4, "length": 5}, 6, 4, cam, clip={"width": 2})
    with pytest.raises(TypeError):
        next(ctx.render_temporal([cam], 1, 1, 1, [1], clip={"sigma": 1.0}))
    with pytest.raises(TypeError):
        next(ctx.render_animation([(None, cam, 1)], 1, 1, 1, clip={"sigma": 1.0}))
