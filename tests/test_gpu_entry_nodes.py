"""Entry nodes of the camera rays on the GPU (device/entry_nodes.h; k_entry_nodes, k_extend<.., EntryArgs>): bounce 0's walks enter the terrain's
BLAS at per-pixel entry nodes instead of at its root and must visit the same leaves in the same order with the same extents, so every
image — with the table, without it, and from the instrumented kernels, which never use it — is the oracle's bit for bit, whatever the
tile, the bands, the pixel order, the passes, the depth, the integrator or the film.  The beam test, the refinement and a restatement of
the walk are checked on the CPU (tests/test_entry_nodes.py)."""
import numpy as np
import pytest

import filter_model as fm
import pbrs_amd
from common import bits
from oracle.binding import OracleScene
from pbrs_amd import PixelFilter, scenes
from pbrs_amd.spec import SceneBuilder, Transform, deg

pytestmark = pytest.mark.gpu
W, H, SEED = 96, 64, 7
ZERO = {"pixels_with_entries": 0, "pixels_empty": 0, "pixels_from_root": 0, "entries": 0}


def terrain(width=W, height=H, transform=None, second=None):
    """scenes.terrain_scene at 64 x 128 cells, with the terrain's transform (and a second instance of the mesh) to choose.  Its camera
    stands at x = 0 and looks along +z: the x component of the directions changes sign in the film's two middle columns."""
    sb = SceneBuilder()
    sx, sz = 200.0, 400.0
    mesh = scenes.heightfield_mesh(sb, 64, 128, (sx, sz), 12.0, 4)
    sb.instance(mesh, sb.lambertian((0.55, 0.5, 0.4)), transform if transform is not None else Transform.translater((-sx / 2, 0.0, 0.0)))
    if second is not None:
        sb.instance(mesh, sb.lambertian((0.3, 0.5, 0.6)), second)
    sb.instance(scenes.quad_mesh(sb, (-400, -14, -100), (400, -14, -100), (-400, -14, 600), (400, -14, 600), (0, 1, 0)), sb.lambertian((0.4, 0.4, 0.4)))
    rs = scenes.SplitMix64(4)
    for _ in range(4):
        c = (rs.uniform(-80, 80), rs.uniform(60, 90), rs.uniform(40, 360))
        emit = tuple(rs.uniform(8, 20) for _ in range(3))
        s = sb.sphere(c, rs.uniform(6, 12))
        sb.instance(s, sb.diffuse_light(emit))
        sb.area_light(emit, s)
    sb.set_camera(width, height, deg(45.0), (0, 60, -90), (0, 0, 160))
    return sb


@pytest.fixture(scope="module")
def base():
    """The scene and the render most cases share: terrain_scene(width=96, height=64, nx=64, nz=128), 4 x 4 spp, depth 5 — and the oracle's frame."""
    sb = scenes.terrain_scene(width=W, height=H, nx=64, nz=128)
    osc = OracleScene(sb)
    ref, ost = osc.render(4, 4, 5, SEED)
    assert ost["panics"] == 0
    return sb, pbrs_amd.HostScene(sb), osc, ref, ost


def image_of(result):
    return result[0] if isinstance(result, tuple) else result


def both(ctx, render):
    """render(counters) with the table and without it: (result on, info on, result off, info off).  The instrumented render of the same
    case is made here too: it never takes the table (info all zero) and its image is the one rendered with the table, bit for bit."""
    ctx.set_entry_nodes(True)
    on = render(False)
    info_on = ctx.last_entry_info()
    counted = render(True)
    assert ctx.last_entry_info() == ZERO  # the counting kernels walk from the root
    assert (bits(image_of(counted)) == bits(image_of(on))).all()
    ctx.set_entry_nodes(False)
    try:
        off = render(False)
        info_off = ctx.last_entry_info()
    finally:
        ctx.set_entry_nodes(True)
    return on, info_on, off, info_off


def used(info, pixels, sentinels=True):
    assert info["pixels_with_entries"] > 0 and info["pixels_empty"] > 0, info
    assert info["pixels_with_entries"] + info["pixels_empty"] + info["pixels_from_root"] == pixels, (info, pixels)
    assert info["pixels_with_entries"] <= info["entries"] <= 8 * info["pixels_with_entries"], info
    if sentinels:
        assert info["pixels_from_root"] > 0, info


def test_on_off_and_instrumented_equal_the_oracle(gpu_ctx, base):
    sb, hs, osc, ref, ost = base
    gpu_ctx.upload(hs)
    on, info_on, off, info_off = both(gpu_ctx, lambda c: gpu_ctx.render(4, 4, 5, SEED, counters=c)[0])
    assert (bits(on) == bits(ref)).all() and (bits(off) == bits(ref)).all()
    used(info_on, W * H)  # the middle columns straddle dir.x = 0: no table there
    assert info_on["entries"] > info_on["pixels_with_entries"], info_on  # some pixel forks
    assert info_off == ZERO
    img, cst = gpu_ctx.render(4, 4, 5, SEED, counters=True)
    assert (bits(img) == bits(ref)).all()
    assert gpu_ctx.last_entry_info() == ZERO  # the counting kernels walk from the root
    assert cst["closest_rays"] == ost["closest_rays"] and cst["shadow_rays"] == ost["shadow_rays"]
    assert cst["instances"] + cst["shadow_instances"] == ost["instances"] and cst["tri_shading"] == ost["tri_shading"]


def test_normals_visualiser_and_its_node_counts(gpu_ctx, base):
    """Camera rays only: the instrumented render's BLAS node and triangle counts are the closest-hit walk's alone, hence the oracle's."""
    sb, hs, osc, _, _ = base
    gpu_ctx.upload(hs)
    ref, ost = osc.render(1, 1, 1, SEED, integrator="normals")
    on, info_on, off, info_off = both(gpu_ctx, lambda c: gpu_ctx.render(1, 1, 1, SEED, integrator="normals", counters=c)[0])
    assert (bits(on) == bits(ref)).all() and (bits(off) == bits(ref)).all()
    used(info_on, W * H)
    assert info_off == ZERO
    img, cst = gpu_ctx.render(1, 1, 1, SEED, integrator="normals", counters=True)
    assert (bits(img) == bits(ref)).all()
    assert cst["blas_nodes"] == ost["blas_nodes"] and cst["triangles"] == ost["triangles"] and cst["instances"] == ost["instances"]


def test_depth_one(gpu_ctx, base):
    sb, hs, osc, _, _ = base
    gpu_ctx.upload(hs)
    ref, _ = osc.render(4, 4, 1, SEED)
    on, info_on, off, info_off = both(gpu_ctx, lambda c: gpu_ctx.render(4, 4, 1, SEED, counters=c)[0])
    assert (bits(on) == bits(ref)).all() and (bits(off) == bits(ref)).all()
    used(info_on, W * H)
    assert info_off == ZERO


def test_several_passes(gpu_ctx, base):
    """samples_per_pass: the table is written once and read by every pass's bounce 0, the last pass shorter than the others."""
    sb, hs, osc, ref, _ = base
    gpu_ctx.upload(hs)
    for spp_pass in (1, 5):
        (on, st), info_on, (off, _), info_off = both(gpu_ctx, lambda c: gpu_ctx.render(4, 4, 5, SEED, samples_per_pass=spp_pass, counters=c))
        assert st["passes"] == -(-16 // spp_pass)
        assert (bits(on) == bits(ref)).all() and (bits(off) == bits(ref)).all(), spp_pass
        used(info_on, W * H)
        assert info_off == ZERO


def test_offset_tile_and_width_no_multiple_of_eight(gpu_ctx, base):
    """A tile with an offset in 8 x 8 blocks, and one whose width is no multiple of 8 (row-major pixel order, a short last chunk)."""
    sb, hs, osc, ref, _ = base
    gpu_ctx.upload(hs)
    for tile in ((24, 16, 48, 40), (29, 11, 37, 45)):
        x0, y0, w, h = tile
        on, info_on, off, info_off = both(gpu_ctx, lambda c: gpu_ctx.render(4, 4, 5, SEED, tile=tile, counters=c)[0])
        assert (bits(on) == bits(ref[y0:y0 + h, x0:x0 + w])).all() and (bits(off) == bits(on)).all(), tile
        used(info_on, w * h)
        assert info_off == ZERO


def test_two_interleaved_row_bands(gpu_ctx, base):
    sb, hs, osc, ref, _ = base
    gpu_ctx.upload(hs)
    band_rows, band_count = 4, 2
    for band_index in range(band_count):
        rows = [((r // band_rows) * band_count + band_index) * band_rows + r % band_rows for r in range(H // 2)]
        render = lambda c: gpu_ctx.render(4, 4, 5, SEED, tile=(0, 0, W, H // 2), bands=(band_rows, band_count, band_index), counters=c)[0]
        on, info_on, off, info_off = both(gpu_ctx, render)
        assert (bits(on) == bits(ref[rows])).all() and (bits(off) == bits(on)).all(), band_index
        used(info_on, W * H // 2)
        assert info_off == ZERO


def test_filtered_render(gpu_ctx, base):
    """A filtered tile across the middle columns: its traced region is the tile and the filter's halo; the per-sample radiances of the
    CPU model are the oracle's own (OracleScene.trace_sample)."""
    sb, hs, osc, _, _ = base
    gpu_ctx.upload(hs)
    strata, depth = (2, 2), 5

    def radiance(i, region):
        x0, y0, w, h = region
        out = np.empty((h, w, 3), dtype=np.float32)
        for y in range(h):
            for x in range(w):
                out[y, x] = np.array(osc.trace_sample(y0 + y, x0 + x, i, strata[0], strata[1], depth, SEED).radiance, dtype=np.float32)
        return out
    pf = PixelFilter.mitchell()
    tile = (44, 30, 8, 6)
    region = fm.region_of(tile, (hs.width, hs.height), pf.as_tuple())
    ref = fm.filtered(pf.as_tuple(), tile, (hs.width, hs.height), SEED, strata[0], strata[1], radiance)
    on, info_on, off, info_off = both(gpu_ctx, lambda c: gpu_ctx.render_filtered(pf, strata[0], strata[1], depth, SEED, tile=tile, counters=c)[0])
    assert (bits(on) == bits(ref)).all() and (bits(off) == bits(ref)).all()
    assert info_on["pixels_with_entries"] > 0 and info_on["pixels_from_root"] > 0, info_on
    assert info_on["pixels_with_entries"] + info_on["pixels_empty"] + info_on["pixels_from_root"] == region[2] * region[3], (info_on, region)
    assert info_off == ZERO


def test_rotated_terrain_has_no_table(gpu_ctx):
    sb = terrain(transform=Transform.rotater([0.0, 1.0, 0.0], deg(20.0)).translate((-100.0, 0.0, 0.0)))
    ref, ost = OracleScene(sb).render(4, 4, 5, SEED)
    assert ost["panics"] == 0
    gpu_ctx.upload(pbrs_amd.HostScene(sb))
    for counters in (False, True):
        img, _ = gpu_ctx.render(4, 4, 5, SEED, counters=counters)
        assert (bits(img) == bits(ref)).all()
        assert gpu_ctx.last_entry_info() == ZERO


def test_identity_terrain(gpu_ctx):
    """The terrain under the identity (the walk stays in world space), seen from a camera off the axis: no straddling column."""
    sb = terrain(transform=Transform.translater((0.0, 0.0, 0.0)))
    sb.set_camera(W, H, deg(45.0), (-30, 60, -90), (100, 0, 160))
    ref, ost = OracleScene(sb).render(4, 4, 5, SEED)
    assert ost["panics"] == 0
    gpu_ctx.upload(pbrs_amd.HostScene(sb))
    on, info_on, off, info_off = both(gpu_ctx, lambda c: gpu_ctx.render(4, 4, 5, SEED, counters=c)[0])
    assert (bits(on) == bits(ref)).all() and (bits(off) == bits(ref)).all()
    used(info_on, W * H, sentinels=False)
    assert info_off == ZERO


def test_two_terrain_instances_one_table(gpu_ctx):
    sb = terrain(second=Transform.translater((-60.0, -6.0, 120.0)))
    ref, ost = OracleScene(sb).render(4, 4, 5, SEED)
    assert ost["panics"] == 0
    gpu_ctx.upload(pbrs_amd.HostScene(sb))
    on, info_on, off, info_off = both(gpu_ctx, lambda c: gpu_ctx.render(4, 4, 5, SEED, counters=c)[0])
    assert (bits(on) == bits(ref)).all() and (bits(off) == bits(ref)).all()
    used(info_on, W * H)
    assert info_off == ZERO


def test_a_single_sample_pass_after_a_render_takes_no_table(gpu_ctx, base):
    """pbrs_render_sample_radiance queues a pass of its own, in another pixel order and over another tile than the render before it: it
    must not read that render's table."""
    sb, hs, osc, _, _ = base
    tile = (29, 11, 37, 45)
    gpu_ctx.upload(hs)
    fresh = gpu_ctx.sample_radiance(3, 4, 4, 5, SEED, tile=tile)
    gpu_ctx.render(4, 4, 5, SEED)
    assert gpu_ctx.last_entry_info()["pixels_with_entries"] > 0
    after = gpu_ctx.sample_radiance(3, 4, 4, 5, SEED, tile=tile)
    assert (bits(fresh) == bits(after)).all()
    x0, y0 = tile[:2]
    for x, y in ((0, 40), (20, 30), (36, 44), (18, 20)):  # (the oracle's own trace of a few of its pixels)
        ref = np.array(osc.trace_sample(y0 + y, x0 + x, 3, 4, 4, 5, SEED).radiance, dtype=np.float32)
        assert (bits(after[y, x]) == bits(ref)).all(), (x, y)


def test_closest_hit_queries_take_no_table(gpu_ctx, base):
    """pbrs_intersect_rays walks through the shared xfer_step without a table: 16 000 queries stay the oracle's."""
    sb, hs, osc, _, _ = base
    gpu_ctx.upload(hs)
    rs = np.random.RandomState(3)
    n = 16000
    o = np.empty((n, 3), dtype=np.float32)
    o[:n // 2] = (0.0, 60.0, -90.0)  # the camera's origin
    o[n // 2:] = rs.uniform((-120, 5, -20), (120, 80, 420), (n - n // 2, 3))
    target = rs.uniform((-100, -12, 0), (100, 12, 400), (n, 3))
    d = ((target - o) / 100.0).astype(np.float32)
    d[::37, rs.randint(3)] = 0.0  # a few on the literal divisions
    tmax = np.where(rs.rand(n) < 0.8, np.inf, rs.uniform(0.5, 4.0, n)).astype(np.float32)
    h_ref, _, _ = osc.intersect(o, d, tmax, closest=True, anyhit=False)
    h_gpu, _ = gpu_ctx.intersect(o, d, tmax, closest=True, anyhit=False)
    hit = h_ref["inst"] != 0xFFFFFFFF
    assert hit.sum() > n // 4 and (~hit).sum() > n // 50
    assert (bits(h_ref["t"]) == bits(h_gpu["t"])).all() and (h_ref["inst"] == h_gpu["inst"]).all() and (h_ref["prim"] == h_gpu["prim"]).all()
