"""Id mattes at the C ABI, without a GPU: the ctypes mirrors of pbrs_matte_params / pbrs_matte_buffers, the four entry points, and
the argument checks of the Python layer that run before any device call (include/pbrs_gpu.h)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pbrs_amd
from pbrs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbrs_render_tile_matte", "pbrs_render_tile_matte_device", "pbrs_matte_mask", "pbrs_matte_mask_device")


def test_matte_mirrors_match_the_header():
    src = r'''
#include <stddef.h>
#include <stdio.h>
#include "pbrs_gpu.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(pbrs_matte_params), offsetof(pbrs_matte_params, key), offsetof(pbrs_matte_params, slots),
    sizeof(pbrs_matte_buffers), offsetof(pbrs_matte_buffers, ids), offsetof(pbrs_matte_buffers, coverage), offsetof(pbrs_matte_buffers, residual));
  printf("%u %u %u %u\n", PBRS_MATTE_INSTANCE, PBRS_MATTE_MATERIAL, PBRS_MATTE_MAX_SLOTS, PBRS_MATTE_MAX_SELECT);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        v = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert v[0] == ctypes.sizeof(api.MatteParams) == 8
    assert v[1:3] == [api.MatteParams.key.offset, api.MatteParams.slots.offset]
    assert v[3] == ctypes.sizeof(api.MatteBuffers) == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert v[4:7] == [getattr(api.MatteBuffers, n).offset for n in ("ids", "coverage", "residual")]
    assert [f for f, _ in api.MatteBuffers._fields_] == list(api.MATTE_LAYERS)
    assert v[7:] == [api.MatteParams.INSTANCE, api.MatteParams.MATERIAL, api.MatteParams.MAX_SLOTS, api.MatteParams.MAX_SELECT]


def test_matte_entry_points_are_declared_and_exported():
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


def test_bad_arguments_are_rejected_before_any_device_call():
    ctx = object.__new__(pbrs_amd.Context)  # no pbrs_create: nothing may reach the device
    ctx._L, ctx._h, ctx.scene = _NoDevice(), None, None
    with pytest.raises(ValueError, match="unknown matte key"):
        ctx.render_matte(1, 1, 1, 1, key="prim")
    with pytest.raises(ValueError, match="unknown AOV"):
        ctx.render_matte(1, 1, 1, 1, aovs=("position",))
    with pytest.raises(ValueError, match="unknown matte layer"):
        ctx.render_matte_device(0, {"id": 0}, 1, 1, 1, 1)
    with pytest.raises(ValueError, match="slots"):
        ctx.matte_mask(np.zeros((2, 2, 3), np.uint32), np.zeros((2, 2, 2), np.float32), [1])
    with pytest.raises(ValueError, match="u32"):
        ctx.matte_mask(np.zeros((2, 2, 2), np.uint32), np.zeros((2, 2, 2), np.float32), [-1])


def test_the_selection_is_sorted_and_deduplicated():
    assert api._matte_select([7, 3, 7, 0xFFFFFFFF, 0]).tolist() == [0, 3, 7, 0xFFFFFFFF]
    assert api._matte_select([]).size == 0 and api._matte_select([]).dtype == np.uint32
