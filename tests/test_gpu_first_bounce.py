"""Bounce 0 runs without a camera path record: k_raygen writes the ray (q[0][0], q[0][1]) and the RNG's high word (the pass set's rng_hi0 column),
bounce 0's k_shade takes origin, beta = 1, L = 0 and slot = queue position without loading them, and L is first written by that k_shade,
by k_class_scatter<2u> for the paths a split queue drops, or by run_pass's memset when the pass has no bounce (device/kernels.h,
pbrs_gpu.hip).  Every case goes through the API of tests/test_gpu_render.py and is compared with the oracle bit for bit: what can go
wrong is a slot nobody wrote (the previous frame's radiance shows through), a wrong RNG word, or a wrong slot."""
import functools

import numpy as np
import pytest

import denoise_var_model as vm
import matte_model
import passes_model as pm
import pbrs_amd
from common import bits
from oracle.binding import OracleScene
from pbrs_amd import api, scenes
from pbrs_amd.spec import SceneBuilder, Transform, deg

pytestmark = pytest.mark.gpu
SEED = 13
MISS = 0xFFFFFFFF


def open_scene(width, height, env=None):
    """A small height field (128 triangles) over nothing under one sphere light: the camera sees sky above the field, nothing below it,
    the light itself, and the field.  One shading class and, without `env`, a black environment: k_extend splits the path integrator's
    queues and drops the misses."""
    sb = SceneBuilder()
    sb.instance(scenes.heightfield_mesh(sb, 8, 8, (20.0, 20.0), 2.0, 3), sb.lambertian((0.55, 0.5, 0.4)), Transform.translater((-10.0, 0.0, 0.0)))
    emit = (12.0, 11.0, 9.0)
    light = sb.sphere((0.0, 8.0, 10.0), 1.5)
    sb.instance(light, sb.diffuse_light(emit))
    sb.area_light(emit, light)
    if env is not None:
        sb.env = env
    sb.set_camera(width, height, deg(38.0), (0.0, 9.0, -16.0), (0.0, 2.0, 10.0))
    return sb


def _textured(width, height):
    from test_gpu_render import _textured_scene
    sb = _textured_scene(None)
    sb.set_camera(width, height, deg(55.0), (0, 2.5, -7), (0, 1, 0))
    return sb


def _specular(width, height):
    from test_gpu_render import _specular_scene
    sb = _specular_scene(0)
    sb.set_camera(width, height, deg(55.0), (0.3, 2.2, -7), (0, 1, 0))
    return sb


def _zoo(width, height):
    from test_gpu_render import _material_zoo
    sb = _material_zoo()  # a sphere of every material kind, a Dielectric among them, in front of nothing
    sb.set_camera(width, height, deg(50.0), (0.0, 0.0, -6.0), (0, 0, 0))
    return sb


BUILDERS = {
    "open": open_scene,
    "open_env": lambda w, h: open_scene(w, h, env=(0.3, 0.4, 0.6)),
    "cornell": lambda w, h: scenes.cornell_scene(w, h, variant="diffuse"),
    "cornell_specular": lambda w, h: scenes.cornell_scene(w, h, variant="specular"),  # several shading classes
    "textured": _textured,
    "specular": _specular,
    "zoo": _zoo,
}


@functools.lru_cache(maxsize=None)
def builder(name, width, height):
    return BUILDERS[name](width, height)


@functools.lru_cache(maxsize=None)
def oracle_image(name, width, height, sx, sy, depth, integrator="path", tile=None):
    """The oracle's frame, computed once per case and kept read-only."""
    osc = OracleScene(builder(name, width, height))
    ref, ost = osc.render(sx, sy, depth, SEED, tile=tile, integrator=integrator)
    osc.close()
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def first_hits(name, width, height, sx, sy):
    """The oracle's camera rays of the render and their closest hits per sample index -> t, inst, prim (spp, P), tie mask (P,)."""
    osc = OracleScene(builder(name, width, height))
    ts, insts, prims, tie = [], [], [], None
    for s in range(sx * sy):
        o, d = osc.camera_rays(s, sx, sy, SEED)
        hits, _, info = osc.intersect(o, d, np.full(len(o), np.inf, dtype=np.float32), anyhit=False)
        ts.append(np.where(hits["inst"] != MISS, hits["t"], np.float32(np.inf)).astype(np.float32))
        insts.append(hits["inst"].astype(np.uint32))
        prims.append(hits["prim"].astype(np.uint32))
        tie = info["tie_mask"].copy() if tie is None else (tie | info["tie_mask"])
    osc.close()
    out = np.array(ts), np.array(insts), np.array(prims), tie
    for a in out:
        a.setflags(write=False)
    return out


def upload(ctx, name, width, height):
    hs = pbrs_amd.HostScene(builder(name, width, height))
    ctx.upload(hs)
    return hs


def same(img, ref):
    """Equal bits, or a NaN on both sides."""
    return bool(((bits(img) == bits(ref)) | (np.isnan(img) & np.isnan(ref))).all())


def sky_of(name, width, height, sx, sy):
    """(h, w) bool: the pixels all of whose camera samples hit nothing."""
    _, insts, _, _ = first_hits(name, width, height, sx, sy)
    return (insts == MISS).all(axis=0).reshape(height, width)


def test_the_open_scene_has_sky_field_and_light():
    """What the other cases rely on: a good part of the open scene's camera samples miss, a good part hits the field, some see the light."""
    _, insts, _, tie = first_hits("open", 64, 48, 2, 2)
    assert not tie.any()
    assert 0.3 < (insts == MISS).mean() < 0.8 and (insts == 0).mean() > 0.1 and (insts == 1).mean() > 0.005
    assert sky_of("open", 64, 48, 2, 2).mean() > 0.3


def test_stale_radiance_does_not_show_through_dropped_paths(gpu_ctx):
    """A bright closed scene first, then the open one in the same context: the pass sets hold the Cornell box's radiance in every slot
    when the open scene's queue split drops its sky paths, which no k_shade lane ever visits.  Their L must be +0.0, frame after frame."""
    upload(gpu_ctx, "cornell", 64, 48)
    for spp_pass in (0, 2):  # one pass, and two that fill both pass sets
        bright, _ = gpu_ctx.render(2, 2, 5, SEED, samples_per_pass=spp_pass)
        assert same(bright, oracle_image("cornell", 64, 48, 2, 2, 5))
    assert (bright > 0).mean() > 0.95
    upload(gpu_ctx, "open", 64, 48)
    ref = oracle_image("open", 64, 48, 2, 2, 5)
    sky = sky_of("open", 64, 48, 2, 2)
    assert (bits(ref)[sky] == 0).all() and ref[~sky].any()
    for spp_pass in (0, 0, 0, 2, 1):  # the repeats run on sets that hold the frame before
        img, st = gpu_ctx.render(2, 2, 5, SEED, samples_per_pass=spp_pass, counters=(spp_pass == 1))
        assert (bits(img)[sky] == 0).all(), spp_pass
        assert same(img, ref), spp_pass
        assert st["invalid_samples"] == 0


@pytest.mark.parametrize("name", ["open", "cornell"])
def test_depth_zero_and_depth_one(gpu_ctx, name):
    """Depth 0 runs no k_shade at all, so nobody stores L but run_pass: all zeros, not what the deeper frame before left; depth 1 runs
    bounce 0 only."""
    upload(gpu_ctx, name, 64, 48)
    deep, _ = gpu_ctx.render(2, 2, 5, SEED)
    assert same(deep, oracle_image(name, 64, 48, 2, 2, 5)) and deep.any()
    for integrator in ("path", "direct"):
        for spp_pass in (0, 1):
            zero, _ = gpu_ctx.render(2, 2, 0, SEED, integrator=integrator, samples_per_pass=spp_pass)
            assert (bits(zero) == 0).all(), (integrator, spp_pass)
            assert same(zero, oracle_image(name, 64, 48, 2, 2, 0, integrator))
        gpu_ctx.render(2, 2, 5, SEED, samples_per_pass=2)  # both sets hold radiance again
    one, _ = gpu_ctx.render(2, 2, 1, SEED)
    assert same(one, oracle_image(name, 64, 48, 2, 2, 1)) and one.any()


@pytest.mark.parametrize("name", ["open", "cornell"])
def test_passes_of_one_three_and_nine_samples(gpu_ctx, name):
    """3 x 3 strata as nine passes, three and one: pass_first_sample is part of the RNG word bounce 0 carries in rng_hi0, and the pass
    sets are reused pass after pass with no store to L but bounce 0's own."""
    upload(gpu_ctx, name, 64, 48)
    ref = oracle_image(name, 64, 48, 3, 3, 5)
    frames = [gpu_ctx.render(3, 3, 5, SEED, samples_per_pass=k, counters=True) for k in (1, 3, 9)]
    assert [st["passes"] for _, st in frames] == [9, 3, 1]
    for img, _ in frames:
        assert same(img, frames[0][0]) and same(img, ref)


def test_pixel_order_row_major_with_a_short_last_chunk(gpu_ctx):
    """37 x 21: no multiple of 8, so the slots go row-major; slot = queue position at bounce 0 whatever the order."""
    upload(gpu_ctx, "open", 37, 21)
    ref = oracle_image("open", 37, 21, 2, 2, 5)
    for spp_pass in (0, 3):
        img, _ = gpu_ctx.render(2, 2, 5, SEED, samples_per_pass=spp_pass)
        assert img.shape == (21, 37, 3) and same(img, ref), spp_pass
    assert (bits(img)[sky_of("open", 37, 21, 2, 2)] == 0).all()


def test_pixel_order_two_interleaved_row_bands(gpu_ctx):
    upload(gpu_ctx, "open", 64, 48)
    ref = oracle_image("open", 64, 48, 2, 2, 5)
    band_rows, band_count = 4, 2
    for band_index in range(band_count):
        rows = [((r // band_rows) * band_count + band_index) * band_rows + r % band_rows for r in range(24)]
        img, _ = gpu_ctx.render(2, 2, 5, SEED, tile=(0, 0, 64, 24), bands=(band_rows, band_count, band_index))
        assert same(img, ref[rows]), band_index


@pytest.mark.parametrize("name,size,depth", [
    ("open_env", (64, 48), 5),          # the misses see the environment: kept and shaded, nothing dropped
    ("cornell_specular", (64, 48), 6),  # several shading classes: class order, no split, every path shaded
    ("textured", (32, 32), 5),          # k_shade<.., TEX = true>
])
def test_scenes_whose_queues_are_not_split(gpu_ctx, name, size, depth):
    upload(gpu_ctx, name, *size)
    ref = oracle_image(name, *size, 2, 2, depth)
    for spp_pass in (0, 1):
        img, _ = gpu_ctx.render(2, 2, depth, SEED, samples_per_pass=spp_pass)
        assert same(img, ref), (name, spp_pass)
    assert np.nanstd(ref) > 0.01
    if name == "open_env":
        assert ref[sky_of("open_env", 64, 48, 2, 2)].all()  # the sky is lit


@pytest.mark.parametrize("name,integrator,strata,depth", [
    ("specular", "direct", 2, 2),  # 1 / mass rides in L.w from bounce 0 to bounce 1
    ("open", "direct", 2, 2),
    ("zoo", "materials", 1, 0),
    ("zoo", "normals", 1, 0),      # the Dielectric's choice draws from rng_in
])
def test_the_other_integrators(gpu_ctx, name, integrator, strata, depth):
    upload(gpu_ctx, name, 32, 32)
    ref = oracle_image(name, 32, 32, strata, strata, depth, integrator)
    for spp_pass in (0, 1):
        img, _ = gpu_ctx.render(strata, strata, depth, SEED, integrator=integrator, samples_per_pass=spp_pass)
        assert same(img, ref), (name, integrator, spp_pass)
    assert len(np.unique(bits(ref).reshape(-1, 3), axis=0)) > 4


@functools.lru_cache(maxsize=None)
def _oracle_samples(name, width, height, strata, depth):
    """Per-sample radiances at depth 1 (D_i) and at `depth` (L_i), (spp, h, w, 3) f32 each, from the oracle's single-sample trace."""
    osc = OracleScene(builder(name, width, height))
    spp = strata * strata
    D = np.empty((spp, height, width, 3), np.float32)
    L = np.empty_like(D)
    for i in range(spp):
        for r in range(height):
            for c in range(width):
                D[i, r, c] = osc.trace_sample(r, c, i, strata, strata, 1, SEED).radiance
                L[i, r, c] = osc.trace_sample(r, c, i, strata, strata, depth, SEED).radiance
    osc.close()
    D.setflags(write=False)
    L.setflags(write=False)
    return D, L


def test_outputs_beside_the_image_on_the_open_scene(gpu_ctx):
    """One render with first-hit AOVs, the variance, the light passes and an instance matte: they read bounce 0's rays and hit records
    (k_aov, the matte fold: the dropped paths count as misses) and L after bounce 0 and after the last (k_pass_direct, k_pass_fold,
    k_moments, k_accumulate).  Each against what its own tests compare it with: the oracle's first hits, the models of the headers' text
    fed with the oracle's per-sample radiances."""
    W = H = 32
    hs = upload(gpu_ctx, "open", W, H)
    gpu_ctx.render(2, 2, 5, SEED)  # the sets hold a frame
    p = gpu_ctx._params(2, 2, 5, SEED, None)
    slots = 3
    mp, mb, pb = api.MatteParams.make("instance", slots), api.MatteBuffers(), api.PassBuffers()
    matte = {"ids": np.empty((H, W, slots), np.uint32), "coverage": np.empty((H, W, slots), np.float32), "residual": np.empty((H, W), np.float32)}
    layers = {n: np.empty((H, W, 3) if api.PASS_CHANNELS[n] > 1 else (H, W), np.float32) for n in api.PASSES}
    for n in api.MATTE_LAYERS:
        setattr(mb, n, matte[n].ctypes.data)
    for n in api.PASSES:
        setattr(pb, n, layers[n].ctypes.data)
    rgb, aov, st = gpu_ctx._render_host(p, api.AOV_NAMES + ("variance",), mp, mb, pb)

    assert same(rgb, oracle_image("open", W, H, 2, 2, 5))
    D, L = _oracle_samples("open", W, H, 2, 5)
    assert same(rgb, pm.mean(L))
    for k, want in pm.passes(D, L).items():
        assert same(layers[k], want), k
    assert same(aov["variance"], vm.variance(L))
    sky = sky_of("open", W, H, 2, 2)
    assert sky.any() and (bits(layers["direct"])[sky] == 0).all() and (bits(layers["indirect"])[sky] == 0).all()

    ts, insts, prims, tie = first_hits("open", W, H, 2, 2)
    assert not tie.any()
    hit = insts != MISS
    n_hit = hit.sum(axis=0)
    best = np.argmin(ts, axis=0)  # the first of equal minima: the lowest sample index
    cols = np.arange(W * H)
    inst = np.where(n_hit > 0, insts[best, cols], MISS).astype(np.uint32)
    want = {"depth": np.where(n_hit > 0, ts[best, cols], np.float32(np.inf)).astype(np.float32), "instance": inst,
            "prim": np.where(n_hit > 0, prims[best, cols], MISS).astype(np.uint32),
            "coverage": (n_hit.astype(np.float32) * (np.float32(1.0) / np.float32(4))).astype(np.float32)}
    for k, v in want.items():
        assert (np.ascontiguousarray(aov[k]).reshape(-1).view(np.uint32) == v.view(np.uint32)).all(), k
    assert (aov["coverage"][sky] == 0).all() and (aov["instance"][sky] == MISS).all()
    ids, coverage, residual, _, _ = matte_model.matte(insts, None, slots)
    for k, v in (("ids", ids), ("coverage", coverage), ("residual", residual)):
        assert (np.ascontiguousarray(matte[k]).view(np.uint32).reshape(W * H, -1) == np.ascontiguousarray(v).view(np.uint32).reshape(W * H, -1)).all(), k
    assert st["invalid_samples"] == 0 and hs.desc.n_instances == 2
