"""The pixel filter without a GPU: pbrs_loaded_scene_filter on small pbrt files, the pbrs_pixel_filter mirror, and the test-side
weight model (tests/filter_model.py) at the closed-form points of include/pbrs_gpu.h's table."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pbrs_amd
from pbrs_amd import PixelFilter
import filter_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

HEAD = """LookAt 0 1 -5  0 1 0  0 1 0
Camera "perspective" "float fov" [ 45 ]
Film "image" "integer xresolution" [ 16 ] "integer yresolution" [ 12 ]
"""
WORLD = """WorldBegin
  LightSource "point" "point from" [ 0 3 -2 ] "rgb I" [ 5 5 5 ]
  Material "matte" "rgb Kd" [ .5 .5 .5 ]
  Shape "sphere" "float radius" 1
WorldEnd
"""


def load(tmp_path, filter_line):
    p = tmp_path / "s.pbrt"
    p.write_text(HEAD + filter_line + "\n" + WORLD)
    return pbrs_amd.load_pbrt(str(p))


def as_tuple(f):
    return (int(f.kind), float(f.radius[0]), float(f.radius[1]), float(f.a), float(f.b))


T = f32(1.0) / f32(3.0)


@pytest.mark.parametrize("line, want", [
    ('Filter "box" "float xwidth" [ 0.75 ] "float ywidth" [ 0.25 ]', (PixelFilter.BOX, 0.75, 0.25, 0.0, 0.0)),
    ('Filter "triangle" "float xwidth" 1.5 "float ywidth" 3', (PixelFilter.TRIANGLE, 1.5, 3.0, 0.0, 0.0)),
    ('Filter "gaussian" "float xwidth" 1.25 "float ywidth" 2.5 "float alpha" 3.5', (PixelFilter.GAUSSIAN, 1.25, 2.5, 3.5, 0.0)),
    ('Filter "mitchell" "float xwidth" 2.5 "float ywidth" 1.5 "float B" 0.25 "float C" 0.375', (PixelFilter.MITCHELL, 2.5, 1.5, 0.25, 0.375)),
    ('Filter "sinc" "float xwidth" 3 "float ywidth" 2 "float tau" 2.5', (PixelFilter.LANCZOS, 3.0, 2.0, 2.5, 0.0)),
])
def test_filter_with_explicit_parameters(tmp_path, line, want):
    assert as_tuple(load(tmp_path, line).pixel_filter()) == want


@pytest.mark.parametrize("line, want", [
    ('Filter "box"', (PixelFilter.BOX, 0.5, 0.5, 0.0, 0.0)),
    ('Filter "triangle"', (PixelFilter.TRIANGLE, 2.0, 2.0, 0.0, 0.0)),
    ('Filter "gaussian"', (PixelFilter.GAUSSIAN, 2.0, 2.0, 2.0, 0.0)),
    ('Filter "mitchell"', (PixelFilter.MITCHELL, 2.0, 2.0, float(T), float(T))),
    ('Filter "sinc"', (PixelFilter.LANCZOS, 4.0, 4.0, 3.0, 0.0)),
    ('', (PixelFilter.BOX, 0.5, 0.5, 0.0, 0.0)),  # no Filter: Scene's box 0.5 (loader.rs:73-74)
    ('Filter "mitchell" "float xwidth" 1.0 "string junk" "x"', (PixelFilter.MITCHELL, 1.0, 2.0, float(T), float(T))),  # leftovers ignored
])
def test_filter_defaults(tmp_path, line, want):
    assert as_tuple(load(tmp_path, line).pixel_filter()) == want


def test_python_constructors_carry_the_same_defaults():
    assert as_tuple(PixelFilter.box()) == (0, 0.5, 0.5, 0.0, 0.0)
    assert as_tuple(PixelFilter.triangle()) == (1, 2.0, 2.0, 0.0, 0.0)
    assert as_tuple(PixelFilter.gaussian()) == (2, 2.0, 2.0, 2.0, 0.0)
    assert as_tuple(PixelFilter.mitchell()) == (3, 2.0, 2.0, float(T), float(T))
    assert as_tuple(PixelFilter.lanczos()) == (4, 4.0, 4.0, 3.0, 0.0)
    assert as_tuple(PixelFilter.gaussian(1.5, 2.5, alpha=1.0)) == (2, 1.5, 2.5, 1.0, 0.0)


def test_unknown_filter_is_an_error_of_the_filter_call_only(tmp_path):
    ls = load(tmp_path, 'Filter "catmull-rom" "float xwidth" 2')
    assert ls.spec.n_instances == 1  # pbrs_host_load_pbrt succeeded as before
    with pytest.raises(pbrs_amd.PbrsError, match="catmull-rom"):
        ls.pixel_filter()


def test_scene_spec_does_not_depend_on_the_filter(tmp_path):
    def spec_bytes(line, sub):
        d = tmp_path / sub
        d.mkdir()
        ls = load(d, line)
        s = ls.spec
        cam = bytes(s.camera)
        inst = ctypes.string_at(s.instances, s.n_instances * ctypes.sizeof(pbrs_amd.spec.InstanceSpec))
        mats = ctypes.string_at(s.materials, s.n_materials * ctypes.sizeof(pbrs_amd.spec.MaterialSpec))
        return cam, inst, mats, s.n_instances, s.n_materials, s.n_shapes, s.n_delta_lights
    base = spec_bytes("", "a")
    assert spec_bytes('Filter "mitchell" "float xwidth" 1.5 "float B" 0.5', "b") == base
    assert spec_bytes('Filter "nonsense"', "c") == base


def test_pixel_filter_struct_is_24_bytes():
    src = '#include <stdio.h>\n#include "pbrs_gpu.h"\nint main(void) { printf("%zu\\n", sizeof(pbrs_pixel_filter)); return 0; }\n'
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        size = int(subprocess.check_output([os.path.join(d, "t")]))
    assert size == 24 == ctypes.sizeof(PixelFilter)


def test_model_closed_form_points():
    for B in (f32(1.0) / f32(3.0), f32(0.0), f32(0.5)):
        C = f32(0.25)
        assert fm.factor(fm.MITCHELL, [0.0], 2.0, B, C)[0] == (f32(1.0) / f32(6.0)) * (f32(6.0) - f32(2.0) * B)
    assert fm.factor(fm.LANCZOS, [0.0], 4.0, 3.0)[0] == f32(1.0)
    for r in (0.5, 1.25, 2.0, 4.0):
        assert (fm.factor(fm.TRIANGLE, [r, -r], r) == 0).all()
        assert (fm.factor(fm.GAUSSIAN, [r, -r], r, 2.0) == 0).all()
    assert (fm.factor(fm.BOX, [0.0, 0.3, -0.5], 0.5) == 1).all()
    # Mitchell's two branches meet at |x| = 1 (o = r / 2) and vanish at |x| = 2 (o = r), within rounding
    m = fm.factor(fm.MITCHELL, [1.0, np.nextafter(f32(1.0), f32(2.0)), 2.0], 2.0, T, T)
    assert abs(float(m[0] - m[1])) < 1e-6 and abs(float(m[2])) < 1e-6
    assert fm.halo(0.5) == 1 and fm.halo(0.49) == 0 and fm.halo(2.0) == 2 and fm.halo(4.0) == 4 and fm.halo(1.5) == 2
