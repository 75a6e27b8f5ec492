"""Randomised scenes: every shape kind under random rigid transforms, every material kind (textured ones included), area /
delta / environment lights in random combinations, both integrators — GPU against the oracle, bit for bit.  The scenes are
small so that the oracle takes a fraction of a second; what matters is the variety of code paths that meet in one wave."""
import numpy as np
import pytest

import pbrs_amd
from oracle.binding import OracleScene
from pbrs_amd import scenes, spec
from pbrs_amd.spec import SceneBuilder, Transform, deg

pytestmark = pytest.mark.gpu


def random_scene(seed, quads=True):
    """`quads=False`: the same scene with a disk in the plane of every ParallelQuad (same draws, so everything else stays what it was).  A
    scene with a ParallelQuad next to a mesh renders through the closest-hit walk that follows the reference's extent to the letter
    (PBRS_FEAT_EXTENT); its twin without quads goes through the kernels every benchmark scene takes."""
    rs = np.random.RandomState(1000 + seed)
    sb = SceneBuilder()
    u = rs.uniform

    def colour(lo=0.05, hi=0.9):
        return tuple(u(lo, hi, 3))

    textures = [sb.checker(colour(0.0, 0.3), colour(0.5, 0.95)), sb.checker((0, 0, 0), colour(0.4, 0.9)), sb.perlin(float(u(1, 6)), seed=seed),
                sb.image(rs.rand(int(rs.randint(2, 9)), int(rs.randint(2, 9)), 3))]

    def maybe_tex(p=0.4):
        return textures[rs.randint(len(textures))] if rs.rand() < p else colour()

    def material():
        k = rs.randint(9)
        if k == 0:
            return sb.lambertian(maybe_tex())
        if k == 1:
            return sb.metal(colour(0.1, 1.5), colour(1.5, 4.0), float(u(0.01, 0.4)))
        if k == 2:
            return sb.glossy(colour(0.4, 0.9), float(u(0.001, 0.3)))
        if k == 3:
            return sb.mirror(colour(0.5, 0.95))
        if k == 4:
            return sb.plastic(colour(), colour(0.2, 0.6), float(u(0.02, 0.4)), bool(rs.randint(2)))
        if k == 5:
            return sb.dielectric(float(u(1.2, 1.8)))
        if k == 6:
            return sb.uber(maybe_tex(), maybe_tex(0.3), kr=maybe_tex(0.3) if rs.rand() < 0.6 else None, kt=colour(0.1, 0.6) if rs.rand() < 0.5 else None,
                           rough=(float(u(0.02, 0.3)), float(u(0.02, 0.3))), eta=float(u(1.2, 1.7)), opacity=float(u(0.3, 1.0)))
        if k == 7:
            return sb.substrate(colour(), colour(0.05, 0.3))
        return sb.lambertian(colour())

    def xform(pos):
        t = Transform()
        if rs.rand() < 0.7:
            t = t.rotate_y(deg(u(0, 360)))
        if rs.rand() < 0.3:
            t = t.rotate_x(deg(u(-40, 40)))
        return t.translate(pos)

    sb.instance(scenes.quad_mesh(sb, (-9, 0, -9), (9, 0, -9), (-9, 0, 9), (9, 0, 9), (0, 1, 0)), sb.lambertian(maybe_tex(0.5)))
    for k in range(int(rs.randint(4, 9))):
        pos = (float(u(-4, 4)), float(u(0.4, 2.0)), float(u(-2, 5)))
        kind = rs.randint(6)
        if kind == 5:  # a ParallelQuad instance, defects D1 / D2 included: its mirrored hits lie outside its box
            a = rs.standard_normal(3)
            a = a / np.linalg.norm(a) * u(0.6, 1.4)
            b = np.cross(a, rs.standard_normal(3))
            b = b / np.linalg.norm(b) * u(0.6, 1.4)
            if quads:
                shape = sb.quad((0.0, 0.0, 0.0), tuple(float(x) for x in a), tuple(float(x) for x in b))
            else:
                nrm = np.cross(a, b)
                shape = sb.disk((0.0, 0.0, 0.0), tuple(float(x) for x in nrm / np.linalg.norm(nrm)), tuple(float(x) for x in a))
        elif kind == 0:
            shape = sb.sphere((0, 0, 0), float(u(0.4, 1.1)))
        elif kind == 1:
            shape = sb.cuboid((-u(0.3, 0.9), -0.4, -u(0.3, 0.9)), (u(0.3, 0.9), u(0.4, 1.2), u(0.3, 0.9)))
        elif kind == 2:
            n = rs.standard_normal(3)
            shape = sb.disk((0, 0, 0), tuple(n / np.linalg.norm(n)), tuple(np.cross(n, [0.3, 1, 0.2]) / np.linalg.norm(np.cross(n, [0.3, 1, 0.2])) * u(0.5, 1.0)))
        elif kind == 3:
            shape = scenes.box_mesh(sb, (-u(0.3, 0.8), -0.3, -u(0.3, 0.8)), (u(0.3, 0.8), u(0.5, 1.3), u(0.3, 0.8)))
        else:
            shape = sb.triangle((-1, 0, 0), (1, 0, 0.3), (0, 1.4, 0))
        sb.instance(shape, material(), xform(pos))
    lights = rs.randint(1, 8)  # bit 0 area, bit 1 delta, bit 2 environment
    if lights & 1:
        for k in range(int(rs.randint(1, 3))):
            e = tuple(u(3, 12, 3))
            c = (float(u(-3, 3)), float(u(4, 6)), float(u(-1, 3)))
            which = rs.randint(3)
            if which == 0:
                s = sb.sphere(c, float(u(0.3, 0.8)))
            elif which == 1:
                s = sb.disk(c, (0, -1, 0), (float(u(0.5, 1.2)), 0, 0))
            else:
                s = sb.triangle((c[0] + 1, c[1], c[2] + 1), (c[0] + 1, c[1], c[2] - 1), (c[0] - 1, c[1], c[2]))
            sb.instance(s, sb.diffuse_light(e))
            sb.area_light(e, s)
    if lights & 2:
        sb.point_light((float(u(-3, 3)), float(u(3, 6)), float(u(-4, 0))), tuple(u(15, 40, 3)))
        if rs.rand() < 0.5:
            sb.distant_light((float(u(-0.5, 0.5)), -1.0, float(u(-0.5, 0.5))), tuple(u(0.5, 2, 3)), 15.0)
    if lights & 4:
        which = rs.randint(4)
        if which == 0:
            sb.env = tuple(u(0.1, 0.6, 3))
        elif which == 1:
            sb.env_image(sb.image(rs.rand(4, 8, 3)), tuple(u(0.5, 1.2, 3)))
        else:
            sb.env_sky(spec.ENV_BLUE_SKY if which == 2 else spec.ENV_DUSK)
    sb.set_camera(56, 40, deg(u(40, 65)), (float(u(-2, 2)), float(u(1.5, 4)), -8.0), (0, 1, 0.5))
    return sb


SKIPPED_FOR_TIES = []  # (seed, integrator) of comparisons given up for coincident geometry; asserted empty at the end


@pytest.mark.parametrize("seed", range(48))
def test_random_scene_matches_oracle(gpu_ctx, seed):
    sb = random_scene(seed)
    osc = OracleScene(sb)
    gpu_ctx.upload(pbrs_amd.HostScene(sb))
    for integrator, depth in (("path", 7), ("direct", 3)):
        ref, ost = osc.render(2, 2, depth, 11 + seed, integrator=integrator)
        img, st = gpu_ctx.render(2, 2, depth, 11 + seed, integrator=integrator, counters=True)
        if ost["tlas_ties"]:
            SKIPPED_FOR_TIES.append((seed, integrator))  # coincident geometry from two instances: the one documented deviation
            continue
        assert st["closest_rays"] == ost["closest_rays"] and st["shadow_rays"] == ost["shadow_rays"], (seed, integrator)
        assert st["invalid_samples"] == ost["nonfinite_samples"], (seed, integrator)  # samples whose radiance is not finite
        nan = np.isnan(ref)
        assert (nan == np.isnan(img)).all(), (seed, integrator)
        assert (img.view(np.uint32)[~nan] == ref.view(np.uint32)[~nan]).all(), (seed, integrator)
        # ... and through the shipped kernels (counters=True runs the instrumented ones), the scenes with a ParallelQuad included
        img, st = gpu_ctx.render(2, 2, depth, 11 + seed, integrator=integrator, counters=False)
        assert st["invalid_samples"] == ost["nonfinite_samples"], (seed, integrator, "shipped")
        assert (nan == np.isnan(img)).all(), (seed, integrator, "shipped")
        assert (img.view(np.uint32)[~nan] == ref.view(np.uint32)[~nan]).all(), (seed, integrator, "shipped")


def takes_the_exact_extent_walk(sb):
    built = sb.build()
    kinds = {built.shapes[built.instances[i].shape].kind for i in range(built.n_instances)}
    return spec.SHAPE_QUAD in kinds and spec.SHAPE_MESH in kinds


@pytest.mark.parametrize("seed", [s for s in range(48) if takes_the_exact_extent_walk(random_scene(s))])
def test_random_scene_without_parallel_quads_matches_oracle(gpu_ctx, seed):
    """Two thirds of the randomised scenes hold a ParallelQuad next to a mesh and render through the exact-extent walk; their twins with
    disks for quads take the product's regular kernels (scanned TLAS, scene in LDS) with everything else unchanged.  (The other third
    went through the regular kernels in test_random_scene_matches_oracle.)"""
    sb = random_scene(seed, quads=False)
    assert not takes_the_exact_extent_walk(sb)
    osc = OracleScene(sb)
    gpu_ctx.upload(pbrs_amd.HostScene(sb))
    for integrator, depth in (("path", 7), ("direct", 3)):
        ref, ost = osc.render(2, 2, depth, 11 + seed, integrator=integrator)
        img, st = gpu_ctx.render(2, 2, depth, 11 + seed, integrator=integrator, counters=False)
        assert not st["kernel_features_extend"] & 256
        if ost["tlas_ties"]:
            SKIPPED_FOR_TIES.append((seed, integrator + " (no quads)"))
            continue
        nan = np.isnan(ref)
        assert (nan == np.isnan(img)).all(), (seed, integrator)
        assert (img.view(np.uint32)[~nan] == ref.view(np.uint32)[~nan]).all(), (seed, integrator)


def test_a_raised_extent_reaches_a_mirrored_quad_hit(gpu_ctx):
    """Seed 211699 of tools/soak_fuzz.py (round 4; rounds 1-3 differ on it too).  `ray.set_extent(isect.ray_t)` of tlas/src/bvh.rs:84-88
    takes the LEFT subtree's result, not the best hit so far: a mesh may return a hit beyond the extent it was given (blas.rs:468) and
    the extent then rises.  Boxes the best hit would have pruned are entered; what they hold loses at the compare — unless the shape
    reports hits outside its own box, as a ParallelQuad does in its mirrored quadrants (D1).  This ray (a zero direction component;
    bounce 2 -> 3 of film pixel (18, 43), sample 1) finds a sphere at t = 0.5716, then a mesh returns 0.93 and lifts the extent over the
    quad's box (entered at 0.7666), whose mirrored hit at t = 0.3496 wins.  Scenes with a ParallelQuad next to a mesh therefore walk
    with the extent followed to the letter (PBRS_FEAT_EXTENT, bit 8 of kernel_features_extend)."""
    seed = 211699
    sb = random_scene(seed)
    osc = OracleScene(sb)
    gpu_ctx.upload(pbrs_amd.HostScene(sb))
    o = np.array([[1076550976, 1070745188, 3218686800]], dtype=np.uint32).view(np.float32)
    d = np.array([[0, 3212667273, 1041316617]], dtype=np.uint32).view(np.float32)
    kinds = {sb.build().shapes[i].kind for i in range(sb.build().n_shapes)}
    assert spec.SHAPE_QUAD in kinds
    for tmax in (np.inf, 1e30, 0.6):
        t = np.array([tmax], dtype=np.float32)
        h_ref, occ_ref, st = osc.intersect(o, d, t)
        h_gpu, occ_gpu = gpu_ctx.intersect(o, d, t)
        assert not st["tie_mask"].any()
        assert h_ref["inst"][0] == 2 and h_ref["t"].view(np.uint32)[0] == np.float32(0.34959823).view(np.uint32)  # the quad, behind the raised extent
        assert h_gpu["inst"][0] == h_ref["inst"][0] and h_gpu["t"].view(np.uint32)[0] == h_ref["t"].view(np.uint32)[0]
        assert (occ_ref == occ_gpu).all()
    for integrator, depth in (("path", 7), ("direct", 3)):
        ref, ost = osc.render(2, 2, depth, 11 + seed, integrator=integrator)
        for counters in (True, False):
            img, st = gpu_ctx.render(2, 2, depth, 11 + seed, integrator=integrator, counters=counters)
            assert st["kernel_features_extend"] & 256, st["kernel_features_extend"]
            assert ost["tlas_ties"] == 0
            if counters:
                assert st["closest_rays"] == ost["closest_rays"] and st["shadow_rays"] == ost["shadow_rays"]
                assert st["instances"] + st["shadow_instances"] == ost["instances"]  # what the boxes decide, closest and any-hit walks together
            nan = np.isnan(ref)
            assert (nan == np.isnan(img)).all() and (img.view(np.uint32)[~nan] == ref.view(np.uint32)[~nan]).all(), (integrator, counters)


def test_exact_extent_scene_with_a_stack_above_64_kb_renders(gpu_ctx):
    """A scene with a ParallelQuad next to a mesh walks with the extent followed to the letter (PBRS_FEAT_EXTENT), whose TLAS entries
    take two stack words: its stack has max(T, T - 1 + H) + T + 1 rows of 1 KB for a TLAS of T levels and a BLAS of H.  A TLAS grown
    as a chain (one instance split off per level: spheres at geometrically growing distances) takes it beyond 64 KB, the portable
    default limit of a kernel's dynamic LDS, which configure_kernels raises for every kernel in the tables; upload accepts stacks up to
    80 KB.  Both variants of k_extend for such a scene render it, equal to the oracle bit for bit."""
    def levels(nodes):  # levels of every subtree: children come after their parent
        h = np.ones(len(nodes), dtype=np.int64)
        for i in range(len(nodes) - 1, -1, -1):
            if not nodes[i, 7] & 0x80000000:
                h[i] = max(h[i + 1], h[nodes[i, 3]]) + 1
        return h

    sb = SceneBuilder()
    sb.instance(scenes.quad_mesh(sb, (-4, 0, -4), (4, 0, -4), (-4, 0, 4), (4, 0, 4), (0, 1, 0)), sb.lambertian((0.6, 0.6, 0.5)))
    sb.instance(sb.quad((-1.0, 0.2, 0.5), (0.0, 1.3, 0.0), (1.2, 0.0, 0.0)), sb.lambertian((0.7, 0.3, 0.2)))
    for k in range(32):
        sb.instance(sb.sphere((0, 0, 0), 0.4), sb.lambertian((0.2, 0.5, 0.7)), Transform().translate((5.0 * 2.2 ** k, 0.5, 0.0)))
    light = sb.sphere((-2.0, 4.0, -1.0), 0.5)
    sb.instance(light, sb.diffuse_light((8.0, 8.0, 7.0)))
    sb.area_light((8.0, 8.0, 7.0), light)
    sb.set_camera(64, 48, deg(50), (0.5, 2.5, -6.0), (0.5, 0.5, 0.5))
    assert takes_the_exact_extent_walk(sb)
    hs = pbrs_amd.HostScene(sb)
    T, H = int(levels(hs.nodes("tlas"))[0]), int(levels(hs.nodes("blas")).max())
    rows = max(T, T - 1 + H) + T + 1
    assert 64 < rows <= 80, (T, H, rows)
    gpu_ctx.upload(hs)
    tile = (16, 12, 32, 24)
    ref, ost = OracleScene(sb).render(2, 2, 5, 7, tile=tile)
    assert ost["tlas_ties"] == 0 and ost["panics"] == 0 and np.isfinite(ref).all()
    for counters in (True, False):
        img, st = gpu_ctx.render(2, 2, 5, 7, tile=tile, counters=counters)
        assert st["kernel_features_extend"] & 256, st["kernel_features_extend"]
        if counters:
            assert st["closest_rays"] == ost["closest_rays"] and st["shadow_rays"] == ost["shadow_rays"]
        assert (img.view(np.uint32) == ref.view(np.uint32)).all(), counters


def test_random_scenes_contain_parallel_quads():
    kinds = set()
    for seed in range(48):
        spec_ = random_scene(seed).build()
        kinds |= {spec_.shapes[i].kind for i in range(spec_.n_shapes)}
    assert spec.SHAPE_QUAD in kinds and spec.SHAPE_SPHERE in kinds and spec.SHAPE_CUBOID in kinds and spec.SHAPE_DISK in kinds, kinds


@pytest.mark.parametrize("seed", range(0, 48, 3))
def test_random_scene_rays_match_oracle(gpu_ctx, seed):
    """Hit records and occlusion ray by ray on the randomised scenes (most of them have the 8..16 instances of the shared
    TLAS scan, and ParallelQuads, whose mirrored hits (D1) lie outside their boxes and so expose any box that is passed or
    pruned at the wrong time): camera rays plus rays from points along them, with an infinite extent, a huge finite one,
    and one just past the reference's hit."""
    sb = random_scene(seed)
    osc = OracleScene(sb)
    gpu_ctx.upload(pbrs_amd.HostScene(sb))
    o, d = osc.camera_rays(0, 2, 2, 5)
    rs = np.random.RandomState(seed)
    o2 = (o + d * rs.uniform(0.5, 8, (len(o), 1))).astype(np.float32)
    o, d = np.concatenate([o, o2]), np.concatenate([d, rs.standard_normal(o2.shape).astype(np.float32)])
    t_inf = np.full(len(o), np.inf, dtype=np.float32)
    h_inf, _, st = osc.intersect(o, d, t_inf)
    near = (h_inf["t"] * 1.02).astype(np.float32)
    near[~np.isfinite(near)] = 50.0
    for tmax in (t_inf, np.full(len(o), 1e30, dtype=np.float32), near):
        h_ref, occ_ref, st = osc.intersect(o, d, tmax)
        h_gpu, occ_gpu = gpu_ctx.intersect(o, d, tmax)
        keep = ~st["tie_mask"]  # bit-identical t from two instances: the documented deviation
        assert (h_ref["t"].view(np.uint32) == h_gpu["t"].view(np.uint32)).all(), seed
        assert (h_ref["inst"][keep] == h_gpu["inst"][keep]).all() and (h_ref["prim"][keep] == h_gpu["prim"][keep]).all(), seed
        assert (h_ref["b1"].view(np.uint32)[keep] == h_gpu["b1"].view(np.uint32)[keep]).all(), seed
        assert (occ_ref == occ_gpu).all(), seed


@pytest.mark.parametrize("seed", range(0, 48, 4))
def test_random_scene_with_fourier_materials_matches_oracle(gpu_ctx, seed):
    """The randomised scenes again with two of their objects re-covered by Fourier BSDFs (geometry/src/fourier.rs; one- and
    three-channel tables): the lobe's f64 series sums and Newton loops next to every other material, light and texture, in
    the kernels that carry it (k_shade<.., true, PBRS_SHADE_FOURIER>)."""
    import fourier_scenes
    sb = random_scene(seed)
    for k, name in ((1, "rgb"), (2, "mono")):
        sb.instances[k].material = sb.fourier(sb.fourier_table(fourier_scenes.table(name)))
    osc = OracleScene(sb)
    gpu_ctx.upload(pbrs_amd.HostScene(sb))
    for integrator, depth in (("path", 7), ("direct", 3)):
        ref, ost = osc.render(2, 2, depth, 3 + seed, integrator=integrator)
        img, st = gpu_ctx.render(2, 2, depth, 3 + seed, integrator=integrator, counters=True)
        if ost["tlas_ties"]:
            SKIPPED_FOR_TIES.append((seed, integrator, "fourier"))
            continue
        assert st["closest_rays"] == ost["closest_rays"] and st["shadow_rays"] == ost["shadow_rays"], (seed, integrator)
        assert st["invalid_samples"] == ost["nonfinite_samples"], (seed, integrator)
        nan = np.isnan(ref)
        assert (nan == np.isnan(img)).all(), (seed, integrator)
        assert (img.view(np.uint32)[~nan] == ref.view(np.uint32)[~nan]).all(), (seed, integrator)
        img, st = gpu_ctx.render(2, 2, depth, 3 + seed, integrator=integrator, counters=False)  # the shipped kernels
        assert st["invalid_samples"] == ost["nonfinite_samples"], (seed, integrator, "shipped")
        assert (nan == np.isnan(img)).all(), (seed, integrator, "shipped")
        assert (img.view(np.uint32)[~nan] == ref.view(np.uint32)[~nan]).all(), (seed, integrator, "shipped")


def test_no_random_scene_was_skipped():
    """The tie skip above must stay an exception: a change of scenes or seeds that starts skipping comparisons fails here."""
    assert SKIPPED_FOR_TIES == [], SKIPPED_FOR_TIES
