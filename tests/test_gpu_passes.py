"""Light passes on the GPU (include/pbrs_gpu.h, pbrs_render_tile_passes*, pbrs_combine_passes*; device/passes.h): bit for bit against
the numpy model of the header's text (tests/passes_model.py) fed with the oracle's per-sample radiances at depth 1 (D_i) and at the
render's depth (L_i), against the same render without passes, and against themselves however the render is cut into passes, tiles
and bands."""
import numpy as np
import pytest

import passes_model as pm
import pbrs_amd
from common import all_ones, bits
from passes_common import SEED, builder, oracle_samples
from pbrs_amd import DeviceBuffers, api

pytestmark = pytest.mark.gpu

TILE = (8, 8, 16, 16)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want, what=""):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].shape == want[k].shape, (what, k)
        bad = _u32(got[k]) != _u32(want[k])
        assert not bad.any(), (what, k, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _no_times(st):
    return {k: v for k, v in st.items() if not k.startswith("ms_")}


def _upload(ctx, name, width, height):
    ctx.upload(pbrs_amd.HostScene(builder(name, width, height)))


def test_cornell_tile_matches_the_model_and_leaves_the_render_alone(gpu_ctx):
    """Case 1.  The image and the statistics beside the passes are those of Context.render: the same passes of the same size."""
    _upload(gpu_ctx, "diffuse", 64, 64)
    D, L, _ = oracle_samples("diffuse", 64, 64, (2, 2), 5, TILE)
    plain, st0 = gpu_ctx.render(2, 2, 5, SEED, tile=TILE)
    rgb, got, aov, st = gpu_ctx.render_passes(2, 2, 5, SEED, tile=TILE)
    assert aov == {} and tuple(got) == api.PASSES
    _same(got, pm.passes(D, L))
    assert (bits(rgb) == bits(plain)).all() and (bits(rgb) == bits(pm.mean(L))).all()
    assert _no_times(st) == _no_times(st0) and st["passes"] == 1
    assert got["indirect"].any() and np.isfinite(got["indirect_variance"]).all() and (got["indirect_variance"] > 0).any()
    # a subset of the passes: the same bits, nothing else written
    _, some, _, _ = gpu_ctx.render_passes(2, 2, 5, SEED, passes=("indirect", "direct_variance"), tile=TILE)
    _same(some, {k: got[k] for k in ("indirect", "direct_variance")})
    # and the plain render afterwards is still the plain render
    again, st1 = gpu_ctx.render(2, 2, 5, SEED, tile=TILE)
    assert (bits(again) == bits(plain)).all() and _no_times(st1) == _no_times(st0)


@pytest.mark.parametrize("overlap", [True, False], ids=["two_streams", "one_stream"])
def test_one_sample_per_pass_gives_the_same_bits(gpu_ctx, overlap):
    """Case 2: four passes that alternate between the two pass sets (each with a D column of its own), their late bounces on the second
    stream; and the same on one stream."""
    _upload(gpu_ctx, "diffuse", 64, 64)
    D, L, _ = oracle_samples("diffuse", 64, 64, (2, 2), 5, TILE)
    gpu_ctx.set_pass_overlap(overlap)
    try:
        rgb, got, _, st = gpu_ctx.render_passes(2, 2, 5, SEED, tile=TILE, samples_per_pass=1)
        plain, st0 = gpu_ctx.render(2, 2, 5, SEED, tile=TILE, samples_per_pass=1)
    finally:
        gpu_ctx.set_pass_overlap(True)
    assert st["passes"] == 4 and _no_times(st) == _no_times(st0)
    _same(got, pm.passes(D, L))
    assert (bits(rgb) == bits(plain)).all() and (bits(rgb) == bits(pm.mean(L))).all()


def test_a_tile_that_is_no_multiple_of_eight(gpu_ctx):
    """Case 3: 13 x 7 takes the row-major pixel order and partial last blocks; three samples per pass of six: two passes."""
    _upload(gpu_ctx, "diffuse", 64, 64)
    tile = (21, 30, 13, 7)
    D, L, _ = oracle_samples("diffuse", 64, 64, (3, 2), 5, tile)
    want = pm.passes(D, L)
    for spp in (0, 3):
        rgb, got, _, st = gpu_ctx.render_passes(3, 2, 5, SEED, tile=tile, samples_per_pass=spp)
        assert got["direct"].shape == (7, 13, 3) and st["passes"] == (2 if spp else 1)
        _same(got, want, spp)
        assert (bits(rgb) == bits(pm.mean(L))).all()


def test_row_bands_are_the_matching_rows(gpu_ctx):
    """Case 4."""
    _upload(gpu_ctx, "diffuse", 64, 64)
    band_rows, band_count, band_index = 2, 3, 1
    _, whole, _, _ = gpu_ctx.render_passes(2, 2, 5, SEED, tile=(8, 0, 16, 48))
    rows = [((r // band_rows) * band_count + band_index) * band_rows + r % band_rows for r in range(16)]
    for spp in (0, 1):
        _, band, _, _ = gpu_ctx.render_passes(2, 2, 5, SEED, tile=(8, 0, 16, 16), bands=(band_rows, band_count, band_index), samples_per_pass=spp)
        _same(band, {k: v[rows] for k, v in whole.items()}, spp)


def test_glass_and_metal_put_emission_behind_specular_bounces_into_indirect(gpu_ctx):
    """Case 5: the whole 16 x 16 film of the specular Cornell box at depth 8."""
    _upload(gpu_ctx, "specular", 16, 16)
    D, L, _ = oracle_samples("specular", 16, 16, (2, 2), 8)
    rgb, got, _, _ = gpu_ctx.render_passes(2, 2, 8, SEED)
    _same(got, pm.passes(D, L))
    assert (bits(rgb) == bits(pm.mean(L))).all() and got["indirect"].any()


@pytest.mark.parametrize("name", ["sphere_light", "light_in_view"])
def test_primary_misses_and_emitter_hits_are_all_direct(gpu_ctx, name):
    """Case 6: a sphere under a spherical light, whole film — scenes.sphere_light_scene, whose camera sees the sphere before a black
    environment, and the same objects on a floor from further back under a constant environment, the light itself on the film.  Where every
    sample of a pixel ends at its first vertex (it misses, or it sees the light) indirect has the bits of +0 and direct those of the
    image."""
    _upload(gpu_ctx, name, 32, 32)
    D, L, ends = oracle_samples(name, 32, 32, (2, 2), 5)
    rgb, got, aov, _ = gpu_ctx.render_passes(2, 2, 5, SEED, aovs=("instance", "coverage"))
    _same(got, pm.passes(D, L))
    done = ends.all(axis=0)
    assert (aov["coverage"][done] == 0).any()  # misses
    if name == "light_in_view":
        assert (aov["instance"][done & (aov["coverage"] == 1)] == 1).any() and rgb[aov["coverage"] == 0].all()  # the light; the environment
    assert (bits(got["indirect"])[done] == 0).all() and (bits(got["indirect_variance"])[done] == 0).all()
    assert (bits(got["direct"])[done] == bits(rgb)[done]).all()
    if name == "light_in_view":
        assert got["indirect"][~done].any()  # (the lone sphere of sphere_light_scene receives no indirect light at all)


def test_depth_one_is_all_direct(gpu_ctx):
    """Case 7."""
    _upload(gpu_ctx, "diffuse", 64, 64)
    D, _, _ = oracle_samples("diffuse", 64, 64, (2, 2), 5, TILE)
    for spp in (0, 1):
        rgb, got, _, _ = gpu_ctx.render_passes(2, 2, 1, SEED, tile=TILE, samples_per_pass=spp)
        _same(got, pm.passes(D, D), spp)
        assert (bits(got["indirect"]) == 0).all() and (bits(got["direct"]) == bits(rgb)).all() and rgb.any()


def test_passes_beside_aovs_and_a_matte_change_no_other_output(gpu_ctx):
    """Case 8: one call with everything against the same call without passes."""
    _upload(gpu_ctx, "specular", 16, 16)
    names = ("albedo", "variance")

    def call(with_passes, spp):
        p = gpu_ctx._params(2, 2, 8, SEED, None, spp)
        mp, mb, pb = api.MatteParams.make("instance", 3), api.MatteBuffers(), api.PassBuffers()
        matte = {"ids": np.empty((p.h, p.w, 3), np.uint32), "coverage": np.empty((p.h, p.w, 3), np.float32), "residual": np.empty((p.h, p.w), np.float32)}
        layers = {n: np.empty((p.h, p.w, api.PASS_CHANNELS[n]), np.float32) for n in api.PASSES}
        for n in api.MATTE_LAYERS:
            setattr(mb, n, matte[n].ctypes.data)
        for n in api.PASSES:
            setattr(pb, n, layers[n].ctypes.data)
        rgb, aov, st = gpu_ctx._render_host(p, names, mp, mb, pb if with_passes else None)
        return {"rgb": rgb, **aov, **matte}, layers, st

    D, L, _ = oracle_samples("specular", 16, 16, (2, 2), 8)
    want = pm.passes(D, L)
    for spp in (0, 1):
        without, _, st0 = call(False, spp)
        beside, layers, st = call(True, spp)
        _same(beside, without, spp)
        assert _no_times(st) == _no_times(st0)
        _same({k: v.reshape(want[k].shape) for k, v in layers.items()}, want, spp)


@pytest.mark.parametrize("shape", [(1, 1), (7, 13), (33, 65), (600, 700)])
def test_combine_is_numpys_f32_add(gpu_ctx, shape):
    """Case 9, first half: 1 x 1 up to an image longer than the kernel's capped grid (it then strides)."""
    rng = np.random.default_rng(shape[0])
    a = (rng.standard_normal(shape + (3,)) * 10).astype(np.float32)
    b = (rng.standard_normal(shape + (3,)) * 1e-3).astype(np.float32)
    a.reshape(-1)[:3] = (np.inf, np.nan, -0.0)
    b.reshape(-1)[:3] = (-np.inf, 1.0, -0.0)
    got, want = gpu_ctx.combine_passes(a, b), pm.combine(a, b)
    nan = np.isnan(want)
    assert got.shape == want.shape and ((bits(got) == bits(want)) | (nan & np.isnan(got))).all()
    assert nan.sum() == 2 and bits(got).reshape(-1)[2] == 0x80000000


def test_direct_plus_indirect_is_the_image_to_rounding(gpu_ctx):
    """Case 9, second half.  Per component |combine - rgb| <= 4 * spp * 2^-24 * mean_i(|L_i| + |D_i|): three sums of spp terms and one
    subtraction per sample, each within an ulp of its operands (passes_model.combine_bound) — derived, not measured."""
    _upload(gpu_ctx, "diffuse", 64, 64)
    D, L, _ = oracle_samples("diffuse", 64, 64, (2, 2), 5, TILE)
    rgb, got, _, _ = gpu_ctx.render_passes(2, 2, 5, SEED, passes=("direct", "indirect"), tile=TILE)
    combined = gpu_ctx.combine_passes(got["direct"], got["indirect"])
    assert (bits(combined) == bits(pm.combine(got["direct"], got["indirect"]))).all()
    err, bound = np.abs(combined.astype(np.float64) - rgb), pm.combine_bound(D, L)
    print("max |combine - rgb| =", err.max(), "; max of bound =", bound.max(), "; max err / bound =", (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all()


def test_refusals_name_the_reason_and_leave_the_context_usable(gpu_ctx):
    """Case 10."""
    _upload(gpu_ctx, "diffuse", 64, 64)
    _, good, _, _ = gpu_ctx.render_passes(1, 1, 3, SEED, tile=TILE)
    for kw, reason in (({"integrator": "direct"}, "path integrator"), ({"integrator": "normals"}, "path integrator"), ({"depth": 0}, "max_depth 0")):
        args = {"depth": 3, **kw}
        with pytest.raises(pbrs_amd.PbrsError, match=reason):
            gpu_ctx.render_passes(1, 1, args.pop("depth"), SEED, tile=TILE, **args)
        _same(gpu_ctx.render_passes(1, 1, 3, SEED, tile=TILE)[1], good, kw)
    # without a pass asked for, the same calls are the plain renders they were
    assert gpu_ctx.render_passes(1, 1, 3, SEED, passes=(), tile=TILE, integrator="direct")[1] == {}
    L, h = gpu_ctx._L, gpu_ctx._h
    a = np.zeros((2, 2, 3), np.float32)
    assert L.pbrs_combine_passes(h, 2, 2, None, a.ctypes.data, a.ctypes.data) == -1
    assert L.pbrs_combine_passes(h, 0, 2, a.ctypes.data, a.ctypes.data, a.ctypes.data) == -1
    assert L.pbrs_combine_passes(h, 2, 2, a.ctypes.data, a.ctypes.data, a.ctypes.data) == 0


def test_the_device_variants_give_the_host_variants_bits(gpu_ctx):
    """Case 11, first half: render_passes_device, then combine_passes_device on the context's stream with nothing in between, read after
    collect_stats(); the sum written over the direct layer's copy."""
    _upload(gpu_ctx, "specular", 16, 16)
    names = ("depth", "variance")
    rgb, layers, aov, _ = gpu_ctx.render_passes(2, 2, 8, SEED, aovs=names, samples_per_pass=1)
    host = {"rgb": rgb, **layers, **aov, "sum": gpu_ctx.combine_passes(layers["direct"], layers["indirect"])}
    with DeviceBuffers(all_ones(host)) as dev:
        gpu_ctx.render_passes_device(dev.ptr("rgb"), dev.ptrs(layers), 2, 2, 8, SEED, aov_device_ptrs=dev.ptrs(names), samples_per_pass=1)
        gpu_ctx.combine_passes_device(dev.ptr("direct"), dev.ptr("indirect"), dev.ptr("sum"), 16, 16)
        gpu_ctx.collect_stats()
        for n, a in host.items():
            assert (_u32(dev.download_like(n, a)) == _u32(a)).all(), n
        # in place: the sum over the direct layer
        gpu_ctx.combine_passes_device(dev.ptr("direct"), dev.ptr("indirect"), dev.ptr("direct"), 16, 16)
        gpu_ctx.collect_stats()
        assert (_u32(dev.download_like("direct", host["sum"])) == _u32(host["sum"])).all()


def test_render_denoised_passes_is_the_chain_of_its_host_steps(gpu_ctx):
    """Case 11, second half: one render, each layer through the variance-guided denoiser with its own variance, the sum — on the device
    without a host step in between, against the same steps through the host entry points (denoise_var is bit-exact against its own
    model: tests/test_gpu_denoise_var.py)."""
    _upload(gpu_ctx, "specular", 16, 16)
    guides = ("albedo", "normal", "depth", "instance")
    rgb, layers, aov, _ = gpu_ctx.render_passes(2, 2, 8, SEED, aovs=guides)
    clean = {n: gpu_ctx.denoise_var(layers[n], layers[n + "_variance"], iterations=3, **aov) for n in ("direct", "indirect")}
    want = gpu_ctx.combine_passes(clean["direct"], clean["indirect"])
    out, noisy, st = gpu_ctx.render_denoised_passes(2, 2, 8, SEED, guides=guides, keep_noisy=True, iterations=3)
    assert (bits(noisy) == bits(rgb)).all() and st["samples"] == 16 * 16 * 4
    assert (bits(out) == bits(want)).all() and (bits(out) != bits(noisy)).any()
    assert (bits(gpu_ctx.render_denoised_passes(2, 2, 8, SEED, guides=guides, iterations=3)[0]) == bits(want)).all()
