"""Light passes without a GPU (include/pbrs_gpu.h, "light passes"): the property the feature stands on, on the oracle alone — a path's
radiance after its first vertex is its radiance at depth 1, bit for bit —, the numpy model of tests/passes_model.py at its edge cases,
and the C ABI with its ctypes mirror."""
import ctypes
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest

import passes_model as pm
import pbrs_amd
from common import bits
from oracle.binding import OracleScene
from pbrs_amd import api, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbrs_render_tile_passes", "pbrs_render_tile_passes_device", "pbrs_combine_passes", "pbrs_combine_passes_device")
f32 = np.float32


def _words(v):
    return np.array(list(v), dtype=f32).view(np.uint32).tolist()


@pytest.mark.parametrize("variant", ["diffuse", "specular"])
def test_radiance_after_the_first_vertex_is_the_depth_one_radiance(variant):
    """Neither the draws nor Russian roulette depend on `depth` (src/pathintegrator.rs:9-74): the depth-1 result is a prefix of the
    depth-5 one.  A 6 x 6 window of the 64 x 64 Cornell box, strata 2 x 2."""
    osc = OracleScene(scenes.cornell_scene(64, 64, variant=variant))
    hits = deeper = 0
    for row in range(9, 15):
        for col in range(8, 14):
            for i in range(4):
                full = osc.trace_sample(row, col, i, 2, 2, 5, 3)
                one = osc.trace_sample(row, col, i, 2, 2, 1, 3)
                assert one.n_bounces == 1 and full.bounce[0].hit == one.bounce[0].hit
                if full.bounce[0].hit:
                    hits += 1
                    assert _words(full.bounce[0].radiance_after_nee) == _words(one.radiance), (row, col, i)
                    deeper += _words(full.radiance) != _words(one.radiance)
                else:
                    assert _words(full.radiance) == _words(one.radiance), (row, col, i)
    assert hits > 0 and deeper > 0  # the window sees surfaces, and light that took more than one vertex to arrive


def _samples(values):
    """(spp,) or (spp, 3) values of one pixel -> (spp, 1, 1, 3)."""
    a = np.asarray(values, dtype=f32)
    if a.ndim == 1:
        a = np.repeat(a[:, None], 3, axis=1)
    return a[:, None, None, :]


def test_one_sample_per_pixel_leaves_both_variances_unknown():
    out = pm.passes(_samples([0.5]), _samples([0.75]))
    assert out["direct_variance"][0, 0] == np.inf and out["indirect_variance"][0, 0] == np.inf
    assert out["direct"][0, 0].tolist() == [0.5] * 3 and out["indirect"][0, 0].tolist() == [0.25] * 3


def test_a_path_that_ends_at_its_first_vertex_gives_plus_zero():
    D = _samples([[0.3, 7.0, 1e-30], [2.5, 0.0, 4.0]])
    out = pm.passes(D, D.copy())
    assert (bits(pm.indirect_samples(D, D)) == 0).all()
    assert (bits(out["indirect"]) == 0).all() and bits(out["indirect_variance"])[0, 0] == 0
    assert (bits(out["direct"]) == bits(pm.mean(D))).all()
    assert (bits(pm.combine(out["direct"], out["indirect"])) == bits(out["direct"])).all()


def test_a_nan_sample_is_skipped_by_the_variances_and_poisons_the_sums():
    D = _samples([1.0, np.nan, 3.0, 2.0])
    L = _samples([1.5, 4.0, np.inf, 2.0])
    out = pm.passes(D, L)
    assert np.isnan(out["direct"]).all() and np.isnan(out["indirect"]).all()  # I = (0.5, nan, inf, 0)
    # the finite luminances alone: D over {1, 3, 2}, I over {0.5, 0}
    want_d = pm.vm.variance(_samples([1.0, 3.0, 2.0]))
    want_i = pm.vm.variance(_samples([0.5, 0.0]))
    assert bits(out["direct_variance"]) == bits(want_d) and bits(out["indirect_variance"]) == bits(want_i)
    assert np.isfinite(want_d).all() and want_d > 0 and want_i > 0
    # one finite sample left: unknown
    assert pm.passes(_samples([np.nan, 1.0]), _samples([np.nan, 1.0]))["direct_variance"][0, 0] == np.inf


def test_the_combine_bound_holds_for_the_model_itself():
    rng = np.random.default_rng(2)
    D = rng.random((16, 5, 7, 3)).astype(f32)
    L = (D + rng.random(D.shape).astype(f32) * f32(3)).astype(f32)
    out = pm.passes(D, L)
    err = np.abs(pm.combine(out["direct"], out["indirect"]).astype(np.float64) - pm.mean(L))
    assert (err <= pm.combine_bound(D, L)).all() and err.max() > 0


def test_pass_mirrors_match_the_header():
    src = r'''
#include <stddef.h>
#include <stdio.h>
#include "pbrs_gpu.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(pbrs_pass_buffers), offsetof(pbrs_pass_buffers, direct), offsetof(pbrs_pass_buffers, indirect),
    offsetof(pbrs_pass_buffers, direct_variance), offsetof(pbrs_pass_buffers, indirect_variance));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        v = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert v[0] == ctypes.sizeof(api.PassBuffers) == 32
    assert v[1:] == [getattr(api.PassBuffers, n).offset for n in api.PASSES]
    assert [f for f, _ in api.PassBuffers._fields_] == list(api.PASSES)
    assert api.PASSES == ("direct", "indirect", "direct_variance", "indirect_variance")


def test_pass_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    for n in ENTRY_POINTS:
        assert f"int {n}(" in header, n
        assert n in api.GPU_SYMBOLS, n
        assert getattr(lib, n) is not None, n


def test_the_python_layer_offers_the_passes():
    sig = inspect.signature(pbrs_amd.Context.render_passes)
    assert list(sig.parameters)[:7] == ["self", "strata_x", "strata_y", "depth", "seed", "passes", "aovs"]
    assert sig.parameters["passes"].default == api.PASSES and sig.parameters["aovs"].default == ()
    for name in ("render_passes_device", "combine_passes", "combine_passes_device", "render_denoised_passes"):
        assert callable(getattr(pbrs_amd.Context, name)), name


class _NoDevice:
    """Stands for the library: any call reaching it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_bad_arguments_are_rejected_before_any_device_call():
    ctx = object.__new__(pbrs_amd.Context)  # no pbrs_create: nothing may reach the device
    ctx._L, ctx._h, ctx.scene = _NoDevice(), None, None
    with pytest.raises(ValueError, match="unknown light pass"):
        ctx.render_passes(1, 1, 1, 1, passes=("emission",))
    with pytest.raises(ValueError, match="unknown AOV"):
        ctx.render_passes(1, 1, 1, 1, aovs=("position",))
    with pytest.raises(ValueError, match="unknown light pass"):
        ctx.render_passes_device(0, {"diffuse": 0}, 1, 1, 1, 1)
    with pytest.raises(ValueError, match="both are"):
        ctx.combine_passes(np.zeros((2, 2, 3), f32), np.zeros((2, 3, 3), f32))
