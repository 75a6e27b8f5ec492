"""Moving instances at the C ABI, without a GPU: the ctypes mirror of pbrs_instance_motion against a compiled C file, the four entry
points, api.instance_motion on two Cornell boxes whose short box differs, and the argument checks of the Python layer that run before
any device call (include/pbrs_gpu.h, "moving instances and motion vectors")."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import motion_model as mm
import pbrs_amd
from pbrs_amd import api, scenes
from pbrs_amd.spec import Transform, deg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbrs_temporal_accumulate_motion", "pbrs_temporal_accumulate_motion_device", "pbrs_motion_vectors", "pbrs_motion_vectors_device")


def test_the_motion_record_matches_the_header():
    cls = api.InstanceMotion
    prints = ['printf("%zu\\n", sizeof(pbrs_instance_motion));'] + [f'printf("%zu\\n", offsetof(pbrs_instance_motion, {n}));' for n, _ in cls._fields_]
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "pbrs_gpu.h"\nint main(void) {\n' + "\n".join(prints) + \
          '\nprintf("%u\\n", PBRS_MOTION_IDENTITY);\nreturn 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        v = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert v == [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_] + [cls.IDENTITY]
    assert v[0] == 96 and v[1:5] == [0, 48, 84, 88]
    t = mm.table_of([(np.arange(12).reshape(3, 4), 100 + np.arange(9).reshape(3, 3), 1), (np.eye(3, 4), np.eye(3), 0)])
    back = mm.from_ctypes(mm.to_ctypes(t))  # the tests' packing is the struct's layout
    assert all((back[n] == t[n]).all() for n in t) and mm.to_ctypes(t)[0].n[2][1] == 107.0


def test_the_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    for n in ENTRY_POINTS:
        assert f"int {n}(" in header, n
        assert n in api.GPU_SYMBOLS, n
        assert getattr(lib, n) is not None, n


def test_instance_motion_of_two_cornell_boxes_whose_short_box_differs():
    xf_prev = Transform().rotate_y(deg(15.0)).translate((265.0, 0.0, 105.0))
    xf_cur = Transform().rotate_y(deg(19.0)).translate((253.0, 0.0, 110.0))
    prev, cur = pbrs_amd.HostScene(mm.cornell_short_box(xf_prev)), pbrs_amd.HostScene(mm.cornell_short_box(xf_cur))
    fwd, inv = cur.instance_transforms()
    assert fwd.shape == inv.shape == (10, 3, 4) and fwd.dtype == np.float32
    table = api.instance_motion(cur, prev)
    assert len(table) == 10 and ctypes.sizeof(table) == 960
    assert [r.flags for r in table] == [0 if i == mm.SHORT_BOX else api.InstanceMotion.IDENTITY for i in range(10)]
    t = mm.from_ctypes(table)
    # the box's corners, where they are and where they were (float64 from the builders' own transforms)
    corners = np.array([[x, y, z, 1.0] for x in (0, 165) for y in (0, 165) for z in (0, 165)], dtype=np.float64)

    def world(xf):
        return (np.array(xf.forward, dtype=np.float64).reshape(4, 4).T @ corners.T).T[:, :3]
    now, was = world(xf_cur), world(xf_prev)
    got = (t["m"][mm.SHORT_BOX].astype(np.float64) @ np.hstack([now, np.ones((8, 1))]).T).T
    assert np.abs(got - was).max() < 1e-3 and np.abs(now - was).max() > 10.0  # f32 records on coordinates of some hundreds
    # n: a rigid motion's inverse transpose is its own rotation, here the box's turn of 4 degrees about y taken back
    lin, n = t["m"][mm.SHORT_BOX][:, :3].astype(np.float64), t["n"][mm.SHORT_BOX].astype(np.float64)
    assert np.abs(n - lin).max() < 1e-6 and np.abs(lin @ lin.T - np.eye(3)).max() < 1e-6
    assert abs(abs(lin[0, 2]) - np.sin(np.radians(4.0))) < 1e-6 and abs(lin[0, 2] + lin[2, 0]) < 1e-6 and lin[1, 1] == 1.0
    turn = np.array(xf_prev.forward, dtype=np.float64).reshape(4, 4).T[:3, :3] @ np.array(xf_cur.inverse, dtype=np.float64).reshape(4, 4).T[:3, :3]
    assert np.abs(lin - turn).max() < 1e-6
    # the same scene twice: every record flagged
    assert all(r.flags == api.InstanceMotion.IDENTITY for r in api.instance_motion(cur, cur))
    other = pbrs_amd.HostScene(scenes.sphere_light_scene(width=16, height=16))
    with pytest.raises(ValueError, match=f"10 instances beside {other.desc.n_instances}"):
        api.instance_motion(cur, other)


class _NoDevice:
    """Stands for the library: any call reaching it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_bad_arguments_are_rejected_before_any_device_call():
    ctx = object.__new__(pbrs_amd.Context)  # no pbrs_create: nothing may reach the device
    ctx._L, ctx._h, ctx.scene = _NoDevice(), None, None
    rgb, z, cam = np.zeros((4, 6, 3), np.float32), np.ones((4, 6), np.float32), api.Camera()
    with pytest.raises(ValueError, match="ctypes array of InstanceMotion"):
        ctx.temporal_accumulate(rgb, z, cam, motion=np.zeros((3, 24), np.float32))
    with pytest.raises(ValueError, match="ctypes array of InstanceMotion"):
        ctx.motion_vectors(z, cam, cam, motion=[api.InstanceMotion()])
    with pytest.raises(ValueError, match="instance plane of shape"):
        ctx.motion_vectors(z, cam, cam, instance=np.zeros((4, 5), np.uint32))
    with pytest.raises(ValueError, match="depth AOV"):
        ctx.motion_vectors(rgb, cam, cam)
    with pytest.raises(ValueError, match="instance"):
        next(ctx.render_animation([], 1, 1, 1, guides=("depth", "normal")))
    with pytest.raises(TypeError):
        next(ctx.render_animation([], 1, 1, 1, temporal=dict(sigma=1.0)))
