"""The filtered film on the GPU (include/pbrs_gpu.h, pbrs_render_tile_filtered[_device]; device/film.h): bit for bit against the CPU
model of tests/filter_model.py, invariant to tiles, passes and the pass overlap, with the plain render's accounting, and refusing
what the header refuses."""
import ctypes as C

import numpy as np
import pytest

import filter_model as fm
import pbrs_amd
from common import all_ones, bits
from oracle.binding import OracleScene
from pbrs_amd import DeviceBuffers, PixelFilter, scenes

pytestmark = pytest.mark.gpu

KINDS = ("box", "triangle", "gaussian", "mitchell", "lanczos")


def _zoo():
    """One small sphere per material kind, a textured one and an emitter (a 64 x 40 film)."""
    from pbrs_amd.spec import SceneBuilder, Transform, deg
    sb = SceneBuilder()
    mats = [sb.lambertian((0.6, 0.5, 0.4)), sb.metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.2), 0.1), sb.glossy((0.7, 0.7, 0.7), 0.2),
            sb.mirror((0.9, 0.9, 0.9)), sb.plastic((0.3, 0.5, 0.2), (0.4, 0.4, 0.4), 0.1), sb.dielectric(1.5),
            sb.diffuse_light((4, 4, 4)), sb.uber(kd=(0.3, 0.3, 0.5), ks=(0.2, 0.2, 0.2)),
            sb.lambertian(sb.checker((0.9, 0.2, 0.2), (0.1, 0.1, 0.8)))]
    for k, m in enumerate(mats):
        sb.instance(sb.sphere((0, 0, 0), 0.45), m, Transform.translater((-2.0 + 1.0 * (k % 5), 0.6 - 1.2 * (k // 5), 0.0)))
    sb.point_light((0, 4, -4), (30, 30, 30))
    sb.set_camera(64, 40, deg(50.0), (0.0, 0.0, -6.0), (0, 0, 0))
    return sb


_SCENES = {}


def scene(name):
    """(scene builder, HostScene) of a small test scene, built once per session."""
    if name not in _SCENES:
        if name == "cornell":
            sb = scenes.cornell_scene(width=48, height=40)
        elif name == "zoo":
            sb = _zoo()
        else:  # a fuzz scene whose path-traced samples include non-finite ones (tests/test_gpu_fuzz.py, seed 39)
            from test_gpu_fuzz import random_scene
            sb = random_scene(39)
        _SCENES[name] = (sb, pbrs_amd.HostScene(sb))
    return _SCENES[name]


def make_filter(kind, aniso=False):
    f = getattr(PixelFilter, kind)()
    if aniso:  # rx != ry (and, for the box, a zero halo in y)
        f.radius[1] = f.radius[0] * 0.5
    return f


def model(ctx, sb, pf, tile, strata, depth, seed, integrator="path"):
    hs = ctx.scene
    return fm.filtered(pf.as_tuple(), tile, (hs.width, hs.height), seed, strata[0], strata[1],
                       lambda i, region: ctx.sample_radiance(i, strata[0], strata[1], depth, seed, tile=region, integrator=integrator))


# (scene, tile or None = full film, strata, depth, integrator, rx != ry)
CASES = {
    "cornell_full": ("cornell", None, (2, 2), 5, "path", False),
    "cornell_interior_3x2": ("cornell", (14, 10, 20, 16), (3, 2), 5, "path", False),
    "cornell_corner_aniso": ("cornell", (0, 0, 16, 12), (2, 2), 5, "path", True),
    "cornell_far_corner_direct": ("cornell", (30, 26, 18, 14), (2, 2), 3, "direct", True),
    "zoo_full": ("zoo", None, (2, 2), 5, "path", False),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("kind", KINDS)
def test_matches_the_cpu_model_bit_for_bit(gpu_ctx, case, kind):
    name, tile, strata, depth, integrator, aniso = CASES[case]
    sb, hs = scene(name)
    gpu_ctx.upload(hs)
    pf = make_filter(kind, aniso)
    tile = tile or (0, 0, hs.width, hs.height)
    img, st = gpu_ctx.render_filtered(pf, strata[0], strata[1], depth, 7, tile=tile, integrator=integrator)
    ref = model(gpu_ctx, sb, pf, tile, strata, depth, 7, integrator)
    assert img.shape == ref.shape
    assert (bits(img) == bits(ref)).all(), (case, kind, int((bits(img) != bits(ref)).sum()))
    region = fm.region_of(tile, (hs.width, hs.height), pf.as_tuple())
    assert st["samples"] == region[2] * region[3] * strata[0] * strata[1]


def test_oracle_radiance_case(gpu_ctx):
    """A tiny tile whose per-sample radiance comes from the CPU oracle's own trace (OracleScene.trace_sample)."""
    sb, hs = scene("cornell")
    gpu_ctx.upload(hs)
    osc = OracleScene(sb)
    strata, depth, seed = (2, 1), 4, 3

    def radiance(i, region):
        x0, y0, w, h = region
        out = np.empty((h, w, 3), dtype=np.float32)
        for y in range(h):
            for x in range(w):
                out[y, x] = np.array(osc.trace_sample(y0 + y, x0 + x, i, strata[0], strata[1], depth, seed).radiance, dtype=np.float32)
        return out
    for kind in ("mitchell", "lanczos"):
        pf = make_filter(kind)
        tile = (20, 17, 5, 4)
        img, _ = gpu_ctx.render_filtered(pf, strata[0], strata[1], depth, seed, tile=tile)
        ref = fm.filtered(pf.as_tuple(), tile, (hs.width, hs.height), seed, strata[0], strata[1], radiance)
        assert (bits(img) == bits(ref)).all(), kind


@pytest.mark.parametrize("kind", ("mitchell", "lanczos", "box"))
def test_tiles_stitch_to_the_full_frame(gpu_ctx, kind):
    _, hs = scene("cornell")
    gpu_ctx.upload(hs)
    pf = make_filter(kind)
    full, _ = gpu_ctx.render_filtered(pf, 2, 2, 5, 11)
    W, H = hs.width, hs.height
    stitched = np.full_like(full, np.nan)
    for (x0, y0, w, h) in ((0, 0, 21, 17), (21, 0, W - 21, 17), (0, 17, 21, H - 17), (21, 17, W - 21, H - 17)):
        stitched[y0:y0 + h, x0:x0 + w], _ = gpu_ctx.render_filtered(pf, 2, 2, 5, 11, tile=(x0, y0, w, h))
    assert (bits(stitched) == bits(full)).all()


def test_passes_overlap_and_the_device_variant_give_the_same_bits(gpu_ctx):
    _, hs = scene("zoo")
    gpu_ctx.upload(hs)
    pf = make_filter("gaussian")
    ref, _ = gpu_ctx.render_filtered(pf, 4, 4, 5, 5)
    try:
        for overlap in (True, False):
            gpu_ctx.set_pass_overlap(overlap)
            for spp_pass in (1, 3, 0):
                img, st = gpu_ctx.render_filtered(pf, 4, 4, 5, 5, samples_per_pass=spp_pass)
                assert (bits(img) == bits(ref)).all(), (overlap, spp_pass)
                if spp_pass == 3:
                    assert st["passes"] == 6
    finally:
        gpu_ctx.set_pass_overlap(True)
    with DeviceBuffers(all_ones({"rgb": ref})) as dev:
        gpu_ctx.render_filtered_device(dev.ptr("rgb"), pf, 4, 4, 5, 5, samples_per_pass=3)
        gpu_ctx.collect_stats()
        assert (bits(dev.download_like("rgb", ref)) == bits(ref)).all()


def test_invalid_samples_count_the_tile_only_and_plain_renders_are_untouched(gpu_ctx):
    _, hs = scene("fuzz39")
    gpu_ctx.upload(hs)
    fresh = pbrs_amd.Context(0)
    try:
        fresh.upload(hs)
        plain_full, plain_st = fresh.render(2, 2, 7, 50)
        assert plain_st["invalid_samples"] > 0  # the scene has them (test_gpu_fuzz.py: the oracle counts 35)
        W, H = hs.width, hs.height
        for tile in ((0, 0, W, H), (10, 8, 24, 20), (0, 0, 17, 13)):
            _, ref_st = fresh.render(2, 2, 7, 50, tile=tile)
            img, st = gpu_ctx.render_filtered(make_filter("mitchell"), 2, 2, 7, 50, tile=tile)
            assert st["invalid_samples"] == ref_st["invalid_samples"], tile
        # a NaN sample stays visible: it reaches every pixel whose support holds it
        if np.isnan(plain_full).any():
            assert np.isnan(gpu_ctx.render_filtered(make_filter("triangle"), 2, 2, 7, 50)[0]).any()
        # plain renders after filtered ones on the same context: the fresh context's bits
        img, st = gpu_ctx.render(2, 2, 7, 50)
        assert (bits(img) == bits(plain_full)).all() and st["invalid_samples"] == plain_st["invalid_samples"]
    finally:
        fresh.close()


def test_refusals_leave_the_context_usable(gpu_ctx):
    _, hs = scene("cornell")
    gpu_ctx.upload(hs)
    good, _ = gpu_ctx.render_filtered(make_filter("mitchell"), 2, 2, 3, 1)
    L = gpu_ctx._L
    p = gpu_ctx._params(2, 2, 3, 1, None)
    out = np.empty((hs.height, hs.width, 3), dtype=np.float32)

    def call(pf, params=p):
        return L.pbrs_render_tile_filtered(gpu_ctx._h, C.addressof(hs.camera), C.addressof(params), None if pf is None else C.byref(pf),
                                           out.ctypes.data, None)
    assert call(None) == -1  # NULL filter
    bands = gpu_ctx._params(2, 2, 3, 1, (0, 0, hs.width, hs.height // 2), bands=(4, 2, 0))
    assert call(make_filter("box"), bands) == -1
    for integ in ("materials", "normals"):
        assert call(make_filter("box"), gpu_ctx._params(1, 1, 3, 1, None, integrator=integ)) == -1
    bad = []
    for r in (0.0, -1.0, float("nan"), float("inf")):
        f = make_filter("triangle")
        f.radius[1] = r
        bad.append(f)
    for k in ("gaussian", "mitchell", "lanczos"):
        f = make_filter(k)
        f.a = float("nan")
        bad.append(f)
    f = make_filter("mitchell")
    f.b = float("inf")
    bad.append(f)
    f = make_filter("box")
    f.kind = 5
    bad.append(f)
    for f in bad:
        assert call(f) == -1, f
    for rx, ry in ((4.5, 1.0), (1.0, 4.25)):
        assert call(PixelFilter.triangle(rx, ry)) == -4  # PBRS_E_LIMIT
    assert call(PixelFilter.lanczos(4.0, 4.0)) == 0  # the limit itself is allowed
    img, _ = gpu_ctx.render_filtered(make_filter("mitchell"), 2, 2, 3, 1)
    assert (bits(img) == bits(good)).all()
