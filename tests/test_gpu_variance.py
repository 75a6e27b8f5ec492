"""The variance AOV on the GPU (include/pbrs_gpu.h, pbrs_render_tile_aovs_var; device/moments.h): bit for bit against the fold of
tests/denoise_var_model.py over the per-sample radiances of Context.sample_radiance (the existing bisect entry, not the code under
test), whatever the passes; the image and the seven AOVs beside it keep the bits of render_aovs."""
import numpy as np
import pytest

import denoise_var_model as vm
import pbrs_amd
from common import bits
from pbrs_amd import api
from test_gpu_pixel_filter import scene

pytestmark = pytest.mark.gpu

SCENES = (("cornell", 5, 7), ("zoo", 5, 7), ("fuzz39", 7, 50))
WITH_VARIANCE = api.AOV_NAMES + ("variance",)


def same(a, b):
    """Equal bits, or a NaN on both sides."""
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def expected(ctx, strata, depth, seed, tile=None):
    samples = np.array([ctx.sample_radiance(i, strata[0], strata[1], depth, seed, tile=tile) for i in range(strata[0] * strata[1])])
    return vm.variance(samples), samples


@pytest.mark.parametrize("strata", ((2, 2), (3, 2)), ids=("2x2", "3x2"))
@pytest.mark.parametrize("name,depth,seed", SCENES)
def test_matches_the_fold_over_the_single_samples_whatever_the_passes(gpu_ctx, name, depth, seed, strata):
    _, hs = scene(name)
    gpu_ctx.upload(hs)
    want, samples = expected(gpu_ctx, strata, depth, seed)
    if name == "fuzz39":
        assert not np.isfinite(samples).all()  # the finite rule is exercised
    img0, aov0, st0 = gpu_ctx.render_aovs(strata[0], strata[1], depth, seed)
    for spp in (1, 2, 0):
        img, aov, st = gpu_ctx.render_aovs(strata[0], strata[1], depth, seed, aovs=WITH_VARIANCE, samples_per_pass=spp)
        got = aov.pop("variance")
        bad = ~same(got, want)
        assert not bad.any(), (name, strata, spp, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        # the image and the seven AOVs of the same call: the bits of render_aovs
        assert same(img, img0).all(), (name, strata, spp)
        for n in api.AOV_NAMES:
            assert same(aov[n], aov0[n]).all(), (name, strata, spp, n)
        assert st["invalid_samples"] == st0["invalid_samples"] and st["samples"] == st0["samples"]
    assert np.isfinite(want).any() and (want[np.isfinite(want)] >= 0).all()
    # the variance alone, without any of the seven
    img, aov, _ = gpu_ctx.render_aovs(strata[0], strata[1], depth, seed, aovs=("variance",))
    assert same(aov["variance"], want).all() and same(img, img0).all()


def test_a_tile_that_is_not_the_full_frame(gpu_ctx):
    _, hs = scene("zoo")
    gpu_ctx.upload(hs)
    tile = (10, 8, 24, 20)
    want, _ = expected(gpu_ctx, (2, 2), 5, 7, tile=tile)
    for spp in (1, 0):
        _, aov, _ = gpu_ctx.render_aovs(2, 2, 5, 7, aovs=("depth", "variance"), tile=tile, samples_per_pass=spp)
        assert aov["variance"].shape == (20, 24) and same(aov["variance"], want).all(), spp


def test_one_sample_per_pixel_is_unknown_everywhere_and_refusals(gpu_ctx):
    _, hs = scene("cornell")
    gpu_ctx.upload(hs)
    _, aov, _ = gpu_ctx.render_aovs(1, 1, 5, 7, aovs=("variance",))
    assert (aov["variance"] == np.inf).all()
    with pytest.raises(api.PbrsError):  # a render that traces no camera ray: refused like the AOVs
        gpu_ctx.render_aovs(2, 2, 0, 7, aovs=("variance",))
    # a plain render afterwards: the bits of a fresh context
    img, _ = gpu_ctx.render(2, 2, 3, 1)
    fresh = pbrs_amd.Context(0)
    try:
        fresh.upload(hs)
        assert (bits(img) == bits(fresh.render(2, 2, 3, 1)[0])).all()
    finally:
        fresh.close()
