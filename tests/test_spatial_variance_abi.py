"""The spatial variance estimate at the C ABI, without a GPU: the ctypes mirrors of the pbrs_spatial_variance_* structs against a
compiled C file, the two entry points, and the argument checks of the Python layer that run before any device call
(include/pbrs_gpu.h)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pbrs_amd
from pbrs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbrs_spatial_variance", "pbrs_spatial_variance_device")
STRUCTS = (("pbrs_spatial_variance_params", api.SpatialVarianceParams), ("pbrs_spatial_variance_guides", api.SpatialVarianceGuides))


def test_spatial_variance_mirrors_match_the_header():
    prints = []
    for cname, cls in STRUCTS:
        prints.append(f'printf("%zu\\n", sizeof({cname}));')
        prints += [f'printf("%zu\\n", offsetof({cname}, {n}));' for n, _ in cls._fields_]
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "pbrs_gpu.h"\nint main(void) {\n' + "\n".join(prints) + \
          '\nprintf("%u %u %u\\n", PBRS_SPATIAL_ID_STOP, PBRS_SPATIAL_ONLY_UNKNOWN, PBRS_SPATIAL_MAX_RADIUS);\nreturn 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        v = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    want = []
    for _, cls in STRUCTS:
        want.append(ctypes.sizeof(cls))
        want += [getattr(cls, n).offset for n, _ in cls._fields_]
    P = api.SpatialVarianceParams
    assert v == want + [P.ID_STOP, P.ONLY_UNKNOWN, P.MAX_RADIUS]
    assert ctypes.sizeof(P) == 32
    assert [n for n, _ in P._fields_] == ["w", "h", "radius", "flags", "sigma_normal", "sigma_depth", "min_temporal", "pad"]
    assert [n for n, _ in api.SpatialVarianceGuides._fields_] == list(api.TEMPORAL_GUIDES)


def test_spatial_variance_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    for n in ENTRY_POINTS:
        assert f"int {n}(" in header, n
        assert n in api.GPU_SYMBOLS, n
        assert getattr(lib, n) is not None, n


def test_the_defaults_are_the_documented_ones():
    p = api.SpatialVarianceParams.make(7, 5)
    assert p.as_dict() == {"w": 7, "h": 5, "radius": 3, "flags": 0, "sigma_normal": np.float32(0.3), "sigma_depth": np.float32(0.2),
                           "min_temporal": 4.0, "pad": 0}
    assert api.SpatialVarianceParams.make(1, 1, id_stop=True).flags == 1
    assert api.SpatialVarianceParams.make(1, 1, only_unknown=True).flags == 2
    assert api.SpatialVarianceParams.make(1, 1, id_stop=True, only_unknown=True, radius=1).flags == 3
    assert pbrs_amd.SpatialVarianceParams is api.SpatialVarianceParams


def test_the_chain_takes_its_parameters_from_its_neighbours():
    sp = pbrs_amd.Context._spatial_params
    assert sp(None, {}, ("depth",)) is None
    assert sp(True, {}, ("depth",)) == {"min_temporal": 4.0, "id_stop": False}
    assert sp(True, {"min_temporal": 2.0}, ("depth", "instance")) == {"min_temporal": 2.0, "id_stop": True}
    assert sp({"radius": 2, "min_temporal": 3.0, "id_stop": False}, {"min_temporal": 2.0}, ("depth", "instance")) == \
        {"radius": 2, "min_temporal": 3.0, "id_stop": False}
    with pytest.raises(TypeError):
        sp({"sigma_luminance": 4.0}, {}, ("depth",))


class _NoDevice:
    """Stands for the library: any call reaching it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_bad_arguments_are_rejected_before_any_device_call():
    ctx = object.__new__(pbrs_amd.Context)  # no pbrs_create: nothing may reach the device
    ctx._L, ctx._h, ctx.scene = _NoDevice(), None, None
    m, n, v, cam = np.zeros((4, 6, 2), np.float32), np.ones((4, 6), np.float32), np.zeros((4, 6), np.float32), api.Camera()
    with pytest.raises(ValueError, match="spatial variance plane moments of shape"):
        ctx.spatial_variance(np.zeros((4, 6), np.float32), n, v)
    with pytest.raises(ValueError, match="spatial variance plane variance of shape"):
        ctx.spatial_variance(m, n, np.zeros((6, 4), np.float32))
    with pytest.raises(ValueError, match="spatial variance plane variance is missing"):
        ctx.spatial_variance(m, n, None)
    with pytest.raises(ValueError, match="length plane"):
        ctx.spatial_variance(m, np.ones(24, np.float32), v)
    with pytest.raises(ValueError, match="spatial variance guide plane normal of shape"):
        ctx.spatial_variance(m, n, v, normal=np.zeros((4, 6), np.float32))
    with pytest.raises(ValueError, match="spatial variance guide plane instance of shape"):
        ctx.spatial_variance(m, n, v, instance=np.zeros((4, 7), np.uint32))
    with pytest.raises(TypeError):
        ctx.spatial_variance(m, n, v, sigma_luminance=1.0)
    with pytest.raises(ValueError, match="unknown spatial variance guide plane 'albedo'"):
        ctx.spatial_variance_device(1, 2, 3, 3, 6, 4, {"albedo": 9})
    for k, name in enumerate(("moments", "length", "variance", "variance_out")):
        ptrs = [1, 2, 3, 4]
        ptrs[k] = 0
        with pytest.raises(ValueError, match=f"plane {name} is a null pointer"):
            ctx.spatial_variance_device(*ptrs, 6, 4)
    with pytest.raises(TypeError):
        ctx.spatial_variance_device(1, 2, 3, 3, 6, 4, iterations=2)
    # the chains: `spatial` changes nothing about what they need, and an unknown keyword fails before anything is allocated
    with pytest.raises(ValueError, match="depth"):
        next(ctx.render_temporal([cam], 1, 1, 1, [1], guides=("normal",), spatial=True))
    with pytest.raises(ValueError, match="depth"):
        next(ctx.render_animation([(None, cam, 1)], 1, 1, 1, guides=("normal", "instance"), spatial={"radius": 2}))
    with pytest.raises(TypeError):
        next(ctx.render_temporal([cam], 1, 1, 1, [1], spatial={"iterations": 3}))
