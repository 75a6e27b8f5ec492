"""First-hit AOVs (include/pbrs_gpu.h, pbrs_aov_buffers; device/aov.h) against the oracle's camera rays and closest hits, the scene
description, the oracle-checked normal visualiser, and themselves under every way a render can be cut up."""
import ctypes as C

import numpy as np
import pytest

import pbrs_amd
from oracle.binding import OracleScene
from pbrs_amd import DeviceBuffers, scenes
from common import GOLDEN_NAMES, SEED, all_ones, bits, golden_case

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF


def _material_zoo(textures=True):
    """One sphere of every material kind (as tests/test_gpu_render.py's zoo), plus a checker-textured Lambertian one."""
    from pbrs_amd.spec import SceneBuilder, Transform, deg
    sb = SceneBuilder()
    mats = [sb.lambertian((0.6, 0.5, 0.4)), sb.metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.2), 0.1), sb.glossy((0.7, 0.7, 0.7), 0.2),
            sb.mirror((0.9, 0.9, 0.9)), sb.plastic((0.3, 0.5, 0.2), (0.4, 0.4, 0.4), 0.1), sb.dielectric(1.5),
            sb.diffuse_light((4, 4, 4)), sb.uber(kd=(0.3, 0.3, 0.5), ks=(0.2, 0.2, 0.2)), sb.substrate((0.4, 0.2, 0.2), (0.3, 0.3, 0.3))]
    for k, m in enumerate(mats):
        sb.instance(sb.sphere((0, 0, 0), 0.45), m, Transform.translater((-2.0 + 1.0 * (k % 5), 0.6 - 1.2 * (k // 5), 0.0)))
    if textures:
        sb.instance(sb.sphere((0, 0, 0), 0.45), sb.lambertian(sb.checker((0.9, 0.2, 0.2), (0.1, 0.1, 0.8))), Transform.translater((2.0, -0.6, 0.0)))
    sb.point_light((0, 4, -4), (30, 30, 30))
    sb.set_camera(120, 72, deg(50.0), (0.0, 0.0, -6.0), (0, 0, 0))
    return sb


def _checker_sphere():
    from pbrs_amd.spec import SceneBuilder, Transform, deg
    sb = SceneBuilder()
    sb.instance(sb.sphere((0, 0, 0), 1.0), sb.lambertian(sb.checker((0.9, 0.2, 0.2), (0.1, 0.1, 0.8))), Transform.translater((0.0, 0.0, 0.0)))
    sb.instance(sb.sphere((0, 0, 0), 0.5), sb.lambertian((0.2, 0.7, 0.3)), Transform.translater((1.4, 0.6, 0.5)))
    sb.point_light((0, 4, -4), (30, 30, 30))
    sb.set_camera(64, 48, deg(50.0), (0.0, 0.0, -4.0), (0, 0, 0))
    return sb


def _scene(name):
    """(scene builder, width, height) of a golden case, a small BASELINE config or the zoo."""
    if name in GOLDEN_NAMES:
        sb, (w, h, _, _, _) = golden_case(name)
        return sb, w, h
    if name == "zoo":
        return _material_zoo(), 120, 72
    if name == "zoo_untextured":
        return _material_zoo(textures=False), 120, 72
    if name == "checker":
        return _checker_sphere(), 64, 48
    kw = {"nx": 64, "nz": 64} if name == "c4" else {}
    sb = scenes.build_config(name, width=48, height=32, **kw)[0]
    return sb, 48, 32


def _upload(ctx, name):
    sb, w, h = _scene(name)
    hs = pbrs_amd.HostScene(sb)
    ctx.upload(hs)
    return sb, hs


def _desc_words(hs, field, count, words):
    return np.ctypeslib.as_array(C.cast(getattr(hs.desc, field), C.POINTER(C.c_uint32)), shape=(count, words)).copy()


def _oracle_first_hits(sb, sx, sy):
    """Per sample index: the oracle's camera rays of the render and their closest hits -> t, inst, prim (spp, P), and the pixels
    where some sample met a tie of tlas/src/bvh.rs:94 (deviation 1, docs/design_notes_r1_r2.md)."""
    osc = OracleScene(sb)
    ts, insts, prims, tie = [], [], [], None
    for s in range(sx * sy):
        o, d = osc.camera_rays(s, sx, sy, SEED)
        hits, _, info = osc.intersect(o, d, np.full(len(o), np.inf, dtype=np.float32), anyhit=False)
        ts.append(np.where(hits["inst"] != MISS, hits["t"], np.float32(np.inf)).astype(np.float32))
        insts.append(hits["inst"].copy())
        prims.append(hits["prim"].copy())
        tie = info["tie_mask"] if tie is None else (tie | info["tie_mask"])
    return np.array(ts), np.array(insts), np.array(prims), tie


def _expected_ids(hs, ts, insts, prims):
    spp = np.float32(1.0) / np.float32(ts.shape[0])
    hit = insts != MISS
    n_hit = hit.sum(axis=0)
    best = np.argmin(ts, axis=0)  # the first of equal minima: the lowest sample index
    cols = np.arange(ts.shape[1])
    any_hit = n_hit > 0
    inst = np.where(any_hit, insts[best, cols], MISS).astype(np.uint32)
    mat_of = _desc_words(hs, "instances", hs.desc.n_instances, 32)[:, 26]  # pbrs_instance::material
    return {"depth": np.where(any_hit, ts[best, cols], np.float32(np.inf)).astype(np.float32),
            "instance": inst,
            "material": np.where(any_hit, mat_of[np.minimum(inst, hs.desc.n_instances - 1)], MISS).astype(np.uint32),
            "prim": np.where(any_hit, prims[best, cols], MISS).astype(np.uint32),
            "coverage": (n_hit.astype(np.float32) * spp).astype(np.float32)}


def _sample_albedo(hs):
    """a_s of every material (include/pbrs_gpu.h) from the untextured lobes of the scene description."""
    mats = _desc_words(hs, "materials", hs.desc.n_materials, 8)
    bx = _desc_words(hs, "bxdfs", hs.desc.n_bxdfs, 16)
    out = np.zeros((len(mats), 3), dtype=np.float32)
    for m, rec in enumerate(mats):
        a = np.zeros(3, dtype=np.float32)
        for k in range(rec[3]):
            lobe = bx[rec[4] + k]
            assert lobe[15] == 0, "untextured scenes only"
            colour = np.ones(3, dtype=np.float32) if lobe[0] == 3 else lobe[4:7].view(np.float32)
            a = (a + colour).astype(np.float32)
        out[m] = np.fmin(np.fmax(a, np.float32(0.0)), np.float32(1.0))
    return out


def _check_against_oracle(ctx, name, sx, sy, albedo):
    sb, hs = _upload(ctx, name)
    _, aov, _ = ctx.render_aovs(sx, sy, 4, SEED)
    ts, insts, prims, tie = _oracle_first_hits(sb, sx, sy)
    exp = _expected_ids(hs, ts, insts, prims)
    keep = ~tie
    assert keep.sum() > 0.9 * keep.size
    for k, v in exp.items():
        got = aov[k].reshape(-1)
        assert (got.view(np.uint32)[keep] == v.view(np.uint32)[keep]).all(), (name, k, np.flatnonzero((got.view(np.uint32) != v.view(np.uint32)) & keep)[:8])
    assert (exp["instance"] != MISS).any()
    if albedo:
        a_mat = _sample_albedo(hs)
        mat_of = _desc_words(hs, "instances", hs.desc.n_instances, 32)[:, 26]
        acc = np.zeros((ts.shape[1], 3), dtype=np.float32)
        for s in range(ts.shape[0]):
            hit = insts[s] != MISS
            a_s = np.zeros_like(acc)
            a_s[hit] = a_mat[mat_of[insts[s][hit]]]
            acc = (acc + a_s).astype(np.float32)
        acc = (acc * (np.float32(1.0) / np.float32(ts.shape[0]))).astype(np.float32)
        got = aov["albedo"].reshape(-1, 3)
        assert (bits(got)[keep] == bits(acc)[keep]).all(), name
        assert got[keep].max() > 0


@pytest.mark.parametrize("name", GOLDEN_NAMES + ["zoo"])
@pytest.mark.parametrize("strata", [(2, 2), (4, 4)])
def test_ids_depth_and_coverage_match_the_oracle(gpu_ctx, name, strata):
    """depth / instance / material / prim / coverage from the oracle's per-sample camera rays and closest hits, reduced in numpy.
    The C4 case's k_extend splits its queue (an open scene under a black environment): its dropped misses must count as misses."""
    _check_against_oracle(gpu_ctx, name, *strata, albedo=False)


@pytest.mark.parametrize("name", ["c2_cornell_diffuse", "c3_cornell_specular", "zoo_untextured"])
def test_albedo_matches_the_scene_description(gpu_ctx, name):
    _check_against_oracle(gpu_ctx, name, 2, 2, albedo=True)


@pytest.mark.parametrize("name", ["c2", "c4", "checker"])
def test_albedo_and_normal_match_the_normal_visualizer(gpu_ctx, name):
    """At one un-jittered ray per pixel, on a Lambertian hit, normal_visualizer shows (albedo + normal) / 2 — and that image equals the
    oracle's (tests/test_gpu_render.py, test_normal_visualizer_matches_oracle)."""
    _, hs = _upload(gpu_ctx, name)
    img, aov, _ = gpu_ctx.render_aovs(1, 1, 0, 5, integrator="normals")
    vis_class = _desc_words(hs, "materials", hs.desc.n_materials, 8)[:, 6]
    cov = aov["coverage"] == 1.0
    lam = cov & (vis_class[np.where(cov, aov["material"], 0)] == 8)
    assert lam.sum() > 0.1 * lam.size
    expect = ((aov["albedo"] + aov["normal"]) * np.float32(0.5)).astype(np.float32)
    assert (img[lam] == expect[lam]).all()
    assert ((aov["coverage"] == 0.0) == (aov["instance"] == MISS)).all()


def _same(a, b):
    for k in a:
        assert (a[k].view(np.uint32) == b[k].view(np.uint32)).all(), k


@pytest.mark.parametrize("name", ["c2", "c3", "c5"])
@pytest.mark.parametrize("integrator", ["path", "direct", "materials", "normals"])
def test_the_image_is_unchanged(gpu_ctx, name, integrator):
    _upload(gpu_ctx, name)
    s = (1, 1) if integrator in ("materials", "normals") else (2, 2)
    for counters in (False, True):
        img, st = gpu_ctx.render(*s, 5, 3, counters=counters, integrator=integrator)
        img2, aov, st2 = gpu_ctx.render_aovs(*s, 5, 3, counters=counters, integrator=integrator)
        assert (bits(img) == bits(img2)).all()
        assert {k: v for k, v in st.items() if not k.startswith("ms_")} == {k: v for k, v in st2.items() if not k.startswith("ms_")}
        assert (aov["instance"] != MISS).any()


@pytest.mark.parametrize("name", ["c4", "c2"])
def test_aovs_do_not_depend_on_how_the_render_is_cut(gpu_ctx, name):
    """samples_per_pass 1 / 3 / auto, pass overlap on and off, a tile against the same window of the frame, interleaved bands against
    the matching rows.  C4 splits k_extend's queue."""
    _upload(gpu_ctx, name)
    sx, sy, depth = 3, 2, 5
    ref = gpu_ctx.render_aovs(sx, sy, depth, 7)[1]
    H, W = ref["depth"].shape
    try:
        for overlap in (True, False):
            gpu_ctx.set_pass_overlap(overlap)
            for spp_pass in (1, 3, 0):
                _same(ref, gpu_ctx.render_aovs(sx, sy, depth, 7, samples_per_pass=spp_pass)[1])
                x0, y0, w, h = 5, 3, W - 13, H - 9
                tile = gpu_ctx.render_aovs(sx, sy, depth, 7, tile=(x0, y0, w, h), samples_per_pass=spp_pass)[1]
                _same({k: v[y0:y0 + h, x0:x0 + w] for k, v in ref.items()}, tile)
                band_rows, band_count = 4, 2
                for band_index in range(band_count):
                    rows = [r for r in range(H) if (r // band_rows) % band_count == band_index]
                    band = gpu_ctx.render_aovs(sx, sy, depth, 7, tile=(0, 0, W, len(rows)), bands=(band_rows, band_count, band_index),
                                               samples_per_pass=spp_pass)[1]
                    _same({k: v[rows] for k, v in ref.items()}, band)
    finally:
        gpu_ctx.set_pass_overlap(True)


def test_api_errors_and_the_device_variant(gpu_ctx):
    _upload(gpu_ctx, "c2")
    for integrator in ("path", "direct"):
        with pytest.raises(pbrs_amd.PbrsError, match=r"\(-1\)"):
            gpu_ctx.render_aovs(2, 2, 0, 1, aovs=("depth",), integrator=integrator)
        img, aov, _ = gpu_ctx.render_aovs(2, 2, 0, 1, aovs=(), integrator=integrator)  # nothing requested: the plain call
        assert aov == {} and (bits(img) == bits(gpu_ctx.render(2, 2, 0, 1, integrator=integrator)[0])).all()
    img, aov, _ = gpu_ctx.render_aovs(2, 2, 4, 9, aovs=())
    assert (bits(img) == bits(gpu_ctx.render(2, 2, 4, 9)[0])).all()
    # the device variant: valid after collect_stats()
    img, aov, _ = gpu_ctx.render_aovs(2, 2, 4, 9)
    host = {"rgb": img, **aov}
    with DeviceBuffers(all_ones(host)) as dev:
        gpu_ctx.render_aovs_device(dev.ptr("rgb"), dev.ptrs(aov), 2, 2, 4, 9)
        gpu_ctx.collect_stats()
        for n, a in host.items():
            assert (dev.download_like(n, a).view(np.uint32) == a.view(np.uint32)).all(), n
