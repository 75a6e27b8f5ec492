"""First-hit AOVs at the C ABI, without a GPU: the ctypes mirror of pbrs_aov_buffers, the two entry points, and the name check
of Context.render_aovs (include/pbrs_gpu.h)."""
import ctypes
import os
import subprocess
import tempfile

import pytest

import pbrs_amd
from pbrs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbrs_render_tile_aovs", "pbrs_render_tile_aovs_device")


def test_aov_buffers_mirror_matches_the_header():
    src = r'''
#include <stddef.h>
#include <stdio.h>
#include "pbrs_gpu.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(pbrs_aov_buffers), offsetof(pbrs_aov_buffers, albedo), offsetof(pbrs_aov_buffers, normal),
    offsetof(pbrs_aov_buffers, coverage), offsetof(pbrs_aov_buffers, depth), offsetof(pbrs_aov_buffers, instance),
    offsetof(pbrs_aov_buffers, material), offsetof(pbrs_aov_buffers, prim));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        sizes = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert sizes[0] == ctypes.sizeof(api.AovBuffers) == 7 * ctypes.sizeof(ctypes.c_void_p)
    names = ("albedo", "normal", "coverage", "depth", "instance", "material", "prim")
    assert sizes[1:] == [getattr(api.AovBuffers, n).offset for n in names]
    assert [f for f, _ in api.AovBuffers._fields_] == list(names) == list(api.AOVS)


def test_aov_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    for n in ENTRY_POINTS:
        assert f"int {n}(" in header, n
        assert n in api.GPU_SYMBOLS, n
        assert getattr(lib, n) is not None, n


class _NoDevice:
    """Stands for the library: any call reaching it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_render_aovs_rejects_unknown_names_before_any_device_call():
    ctx = object.__new__(pbrs_amd.Context)  # no pbrs_create: nothing may reach the device
    ctx._L, ctx._h, ctx.scene = _NoDevice(), None, None
    with pytest.raises(ValueError, match="unknown AOV"):
        ctx.render_aovs(1, 1, 1, 1, aovs=("albedo", "position"))
    with pytest.raises(ValueError, match="unknown AOV"):
        ctx.render_aovs_device(0, {"Normal": 0}, 1, 1, 1, 1)
