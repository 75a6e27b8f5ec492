"""The motion-blur call at the C ABI, without a GPU: the ctypes mirror of pbrs_motion_blur_params against a compiled C file, the entry
points and their symbol table, the filler's bytes against MotionBlurParams.make's, the argument checks of the Python layer that run
before any device call, and the buffers of a sequence with and without the step (include/pbrs_gpu.h, "motion blur")."""
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
SYMBOLS = ["pbrsm_motion_blur", "pbrsm_motion_blur_device", "pbrsm_motion_blur_params_default"]
FIELDS = ["w", "h", "max_radius", "taps", "flags", "shutter", "z_rel", "reserved"]


def test_the_mirror_matches_the_header():
    cls = api.MotionBlurParams
    prints = ['printf("%zu\\n", sizeof(pbrs_motion_blur_params));'] + [f'printf("%zu\\n", offsetof(pbrs_motion_blur_params, {n}));' for n in FIELDS]
    prints += ['printf("%u\\n", PBRS_MOTION_BLUR_MAX_RADIUS);', 'printf("%u\\n", PBRS_MOTION_BLUR_MAX_TAPS);', 'printf("%u\\n", PBRS_MOTION_BLUR_JITTER);']
    want = [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n in FIELDS] + [cls.MAX_RADIUS, cls.MAX_TAPS, cls.JITTER]
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "pbrs_gpu.h"\nint main(void) {\n' + "\n".join(prints) + '\nreturn 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        v = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert v == want
    assert v[0] == 32 and ctypes.sizeof(cls) == 32 and [n for n, _ in cls._fields_] == FIELDS
    assert [getattr(cls, n).offset for n in FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28] and (cls.MAX_RADIUS, cls.MAX_TAPS, cls.JITTER) == (16, 64, 1)


def test_the_entry_points_are_declared_exported_and_typed():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    for n in SYMBOLS[:2]:
        assert f"int {n}(" in header, n
    assert "void pbrsm_motion_blur_params_default(" in header
    for n in SYMBOLS:
        assert n in api.GPU_MOTION_BLUR_SYMBOLS and getattr(lib, n) is not None, n
    loaded = pbrs_amd.gpu_lib()  # the loader sets the new table's types beside the others'
    for n, (argtypes, restype) in libs.GPU_MOTION_BLUR_FUNCTIONS.items():
        assert list(getattr(loaded, n).argtypes) == list(argtypes) and getattr(loaded, n).restype is restype, n
    assert libs.GPU_MOTION_BLUR_FUNCTIONS["pbrsm_motion_blur"] == libs.GPU_MOTION_BLUR_FUNCTIONS["pbrsm_motion_blur_device"] == ([ctypes.c_void_p] * 7, ctypes.c_int)
    assert libs.GPU_MOTION_BLUR_FUNCTIONS["pbrsm_motion_blur_params_default"] == ([ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p], None)
    assert sorted(libs.GPU_MOTION_BLUR_SYMBOLS) == SYMBOLS
    # the header's pbrsm_ declarations, the table and the library's pbrsm_ exports are one list
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(pbrsm_[a-z_0-9]+)\s*\(", code))) == SYMBOLS
    nm = subprocess.run(["nm", "-D", "--defined-only", pbrs_amd.lib_paths()[1]], capture_output=True, text=True, check=True).stdout
    assert sorted(line.split()[-1] for line in nm.splitlines() if line.split() and line.split()[-1].startswith("pbrsm_")) == SYMBOLS
    others = (set(libs.GPU_SYMBOLS) | set(libs.GPU_COMPARE_SYMBOLS) | set(libs.GPU_DESPECKLE_SYMBOLS) | set(libs.GPU_BLOOM_SYMBOLS)
              | set(libs.GPU_DOF_SYMBOLS))
    assert not set(SYMBOLS) & others
    assert pbrs_amd.MotionBlurParams is api.MotionBlurParams


def test_gpu_symbols_is_the_pinned_surface():
    """The new functions live in a table of their own: GPU_SYMBOLS stays the list tests/golden/api_surface.json pins, and no pbrs_( function
    of the header is new."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "api_surface.json")))
    pinned = [v for v in golden.values() if isinstance(v, list) and "pbrs_create" in v]
    assert pinned and any(sorted(v) == sorted(libs.GPU_SYMBOLS) for v in pinned)
    assert not any(n.startswith("pbrsm_") for n in libs.GPU_SYMBOLS)


def test_the_fillers_bytes_are_makes():
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    lib.pbrsm_motion_blur_params_default.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.pbrsm_motion_blur_params_default.restype = None
    p = api.MotionBlurParams()
    ctypes.memset(ctypes.addressof(p), 0xAB, ctypes.sizeof(p))
    lib.pbrsm_motion_blur_params_default(1920, 1080, ctypes.addressof(p))
    assert bytes(p) == bytes(api.MotionBlurParams.make(1920, 1080))
    assert p.as_dict() == {"w": 1920, "h": 1080, "max_radius": 16, "taps": 16, "flags": 0, "shutter": 0.5, "z_rel": float(np.float32(0.05))}
    assert p.reserved == 0
    q = api.MotionBlurParams.make(7, 5, max_radius=4, taps=64, jitter=True, shutter=1.0, z_rel=0.25)
    assert q.as_dict() == {"w": 7, "h": 5, "max_radius": 4, "taps": 64, "flags": 1, "shutter": 1.0, "z_rel": 0.25}


class _NoDevice:
    """Stands for the library: any call reaching it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_bad_arguments_are_rejected_before_any_device_call():
    ctx = object.__new__(pbrs_amd.Context)  # no pbrs_create: nothing may reach the device
    ctx._L, ctx._h, ctx.scene = _NoDevice(), None, None
    rgb, depth, motion, cam = np.zeros((4, 6, 3), np.float32), np.ones((4, 6), np.float32), np.zeros((4, 6, 2), np.float32), api.Camera()
    with pytest.raises(TypeError):
        ctx.motion_blur(rgb, depth, motion, sigma=2.0)
    with pytest.raises(ValueError, match=r"\(h, w, 3\)"):
        ctx.motion_blur(np.zeros((4, 6), np.float32), depth, motion)
    with pytest.raises(ValueError, match="the depth is"):
        ctx.motion_blur(rgb, np.ones((6, 4), np.float32), motion)
    with pytest.raises(ValueError, match="the motion vectors are"):
        ctx.motion_blur(rgb, depth, np.zeros((4, 6, 3), np.float32))
    with pytest.raises(TypeError):
        ctx.motion_blur_device(1, 2, 3, 4, 6, 4, sigma=2.0)
    # the sequences take the keyword out of **params and check it before anything is uploaded, allocated or queued
    with pytest.raises(TypeError):
        next(ctx.render_temporal([cam], 1, 1, 1, [1], motion_blur={"sigma": 2.0}))
    with pytest.raises(TypeError):
        next(ctx.render_temporal([cam], 1, 1, 1, [1], motion_blur=[{"shutter": 1.0}, {"sigma": 2.0}]))
    with pytest.raises(ValueError, match="motion_blur is None, True, a dict"):
        next(ctx.render_animation([(None, cam, 1)], 1, 1, 1, motion_blur=3))
    with pytest.raises(ValueError, match="motion_blur is None, True, a dict"):
        next(ctx.render_animation([(None, cam, 1)], 1, 1, 1, motion_blur=[]))


def test_the_sequences_buffers_with_and_without():
    assert api._motion_blur_params(None) is None and api._motion_blur_params(False) is None
    assert api._motion_blur_params(True)(3) == {}
    one = api._motion_blur_params({"shutter": 1.0})
    assert one(0) == one(7) == {"shutter": 1.0}
    ramp = api._motion_blur_params([{"shutter": 0.25}, {"shutter": 0.5}])
    assert ramp(0)["shutter"] == 0.25 and ramp(1)["shutter"] == 0.5
    with pytest.raises(ValueError, match="none for frame 2"):
        ramp(2)
    # (w, h, fw, fh, guides, motion_vectors, upscale, display, ...) -> does the step need a vector buffer of its own
    for args, own in (((6, 4, 6, 4, ("depth",), False, False, False), True),
                      ((6, 4, 6, 4, ("depth", "instance"), True, False, True, True, True, True, True), False),
                      ((3, 2, 6, 4, ("depth", "instance"), True, True, True), True),
                      ((3, 2, 6, 4, ("depth",), False, True, True), True)):
        plain = api._sequence_buffers(*args)
        assert api._sequence_buffers(*args, motion_blur=False) == plain and "mblur" not in plain and "mblur_motion" not in plain
        sizes = api._sequence_buffers(*args, motion_blur=True)
        assert sizes["mblur"] == 3 * 6 * 4 * 4  # the first image's size: the film's, also where the chain runs low
        assert ("mblur_motion" in sizes) == own and (not own or sizes["mblur_motion"] == 2 * 6 * 4 * 4)
        new = ["mblur", "mblur_motion"] if own else ["mblur"]
        assert {n: v for n, v in sizes.items() if n not in new} == plain and list(sizes)[:-len(new)] == list(plain) and list(sizes)[-len(new):] == new
