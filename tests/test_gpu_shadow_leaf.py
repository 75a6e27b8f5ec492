"""The leaf step of the four-wide any-hit walk (device/traverse.h, AnyWalkW) on the GPU: a leaf reference that carries its triangles
(device/scene.h, PBRS_WREF_PACKED) has them tested first and its own box — found through tri_leaf — only once one of them has passed,
so every occlusion answer and every rendered pixel is still the oracle's, bit for bit.  The references, the table and a restatement of
the walk are checked on the CPU (tests/test_shadow_leaf.py).

Every ray test goes through the parity harness's any-hit path with the wide walk asserted (pbrs_last_intersect_info)."""
import numpy as np
import pytest

import pbrs_amd
from oracle.binding import OracleScene
from pbrs_amd import scenes
from pbrs_amd.spec import SceneBuilder, Transform, deg

pytestmark = pytest.mark.gpu
f32 = np.float32
NX, NZ, SIZE, AMP, SEED = 16, 32, (200.0, 400.0), 12.0, 4  # the C4 family's height field at 1 024 triangles
N_TERRAIN = 2 * NX * NZ


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def nested_triangles():
    """13 differently tilted triangles around one midpoint above the terrain: their centroids coincide, recursive_build cannot split them
    (tests/test_gpu_traversal.py, test_leaf_with_many_triangles) — a leaf of 13, which keeps the node form of its reference."""
    pos, idx = [], []
    for k in range(13):
        s, a = 0.25 * (k + 1), 0.125 * ((k * 5) % 7) - 0.25
        pos += [(100.0 - s, 40.0 - s, 200.0 - a * s), (100.0 + s, 40.0 - s, 200.0 - a * s), (100.0, 40.0 + s, 200.0 + a * s)]
        idx.append((3 * k, 3 * k + 1, 3 * k + 2))
    return np.asarray(pos, dtype=f32), np.asarray(idx, dtype=np.uint32)


def terrain_mesh(sb, with_many_triangle_leaf):
    mesh = scenes.heightfield_mesh(sb, NX, NZ, SIZE, AMP, SEED)
    if not with_many_triangle_leaf:
        return mesh
    pos, nrm, uv, idx = (np.asarray(a) for a in sb.meshes.pop())
    pos, nrm, uv, idx = pos.reshape(-1, 3), nrm.reshape(-1, 3), uv.reshape(-1, 2), idx.reshape(-1, 3)
    p2, i2 = nested_triangles()
    n2 = np.tile(np.asarray([(0.0, 0.0, -1.0)], dtype=f32), (len(p2), 1))
    return sb.mesh(np.concatenate([pos, p2]), np.concatenate([nrm, n2]), np.concatenate([uv, np.zeros((len(p2), 2), dtype=f32)]),
                   np.concatenate([idx, i2 + len(pos)]))


INSTANCES = {
    "translated": lambda: [Transform.translater((-100.0, 0.0, 0.0))],
    # one BLAS under two instances: the translated one keeps the world's direction and reciprocals (only the origin moves), the rotated one
    # rebuilds them inside the instance
    "shared": lambda: [Transform.translater((-100.0, 0.0, 0.0)), Transform.rotater([0.2, 1.0, -0.1], deg(31.0)).translate((180.0, 30.0, -40.0))],
}


def build(many, instances):
    sb = SceneBuilder()
    mesh = terrain_mesh(sb, many)
    xfs = INSTANCES[instances]()
    for xf in xfs:
        sb.instance(mesh, sb.lambertian((0.5, 0.5, 0.5)), xf)
    sb.instance(sb.sphere((0.0, 300.0, 200.0), 5.0), sb.lambertian((0.5, 0.5, 0.5)))  # a TLAS of two or three: scanned
    sb.point_light((0.0, 300.0, -50.0), (9e4, 9e4, 9e4))
    sb.set_camera(24, 16, deg(50.0), (0.0, 60.0, -90.0), (0.0, 0.0, 160.0))
    return sb, [xf.forward for xf in xfs]


def local_rays(sb, hs, n):
    """Rays in the mesh's own space: from the surface upward, grazing along it, through corners of leaf boxes, and with t_max equal to
    the distance at which the ray enters a leaf's box (and its two neighbours)."""
    rs = np.random.RandomState(23)
    k = n // 4
    pos, _, _, idx = sb.meshes[0]
    pos, idx = np.asarray(pos, dtype=f32).reshape(-1, 3), np.asarray(idx).reshape(-1, 3)[:N_TERRAIN]
    p0, p1, p2 = pos[idx[:, 0]], pos[idx[:, 1]], pos[idx[:, 2]]
    blas = hs.nodes("blas")
    leaf = blas[((blas[:, 7] & 0x80000000) != 0) & (blas[:, 3] < N_TERRAIN)]
    lo, hi = leaf[:, 0:3].copy().view(f32), leaf[:, 4:7].copy().view(f32)
    box_lo, box_hi = lo.min(axis=0), hi.max(axis=0)
    size = float((box_hi - box_lo).max())

    def on_surface(m):
        t = rs.randint(len(p0), size=m)
        u, v = rs.rand(m), rs.rand(m)
        flip = u + v > 1.0
        u, v = np.where(flip, 1.0 - u, u), np.where(flip, 1.0 - v, v)
        return (p0[t] + u[:, None] * (p1[t] - p0[t]) + v[:, None] * (p2[t] - p0[t])).astype(f32)

    o_up = on_surface(k)
    d_up = np.stack([rs.uniform(-1, 1, k), rs.uniform(0.05, 1.0, k), rs.uniform(-1, 1, k)], axis=1)
    t_up = np.where(np.arange(k) % 4 != 0, np.inf, rs.uniform(0.02, 1.0, k) * size)
    o_gr = on_surface(k) + np.stack([np.zeros(k), rs.uniform(0.0, 0.5, k), np.zeros(k)], axis=1)
    d_gr = np.stack([rs.uniform(-1, 1, k), rs.uniform(-0.08, 0.08, k), rs.uniform(-1, 1, k)], axis=1)
    t_gr = np.where(np.arange(k) % 2 != 0, np.inf, rs.uniform(0.02, 1.0, k) * size)
    pick = rs.randint(len(lo), size=k)
    corner = np.where(rs.randint(2, size=(k, 3)) == 1, hi[pick], lo[pick])
    o_co = 0.5 * (box_lo + box_hi) + rs.uniform(-1, 1, (k, 3)) * size
    o_co[:, 1] = box_hi[1] + rs.uniform(0.1, 0.6, k) * size
    d_co = (corner - o_co.astype(f32)) / size
    t_co = np.where(np.arange(k) % 2 != 0, np.inf, 2.0 * size)
    pick = rs.randint(len(lo), size=k)
    o_en = (0.5 * (box_lo + box_hi) + rs.uniform(-0.7, 0.7, (k, 3)) * (box_hi - box_lo)).astype(f32)
    o_en[:, 1] = box_hi[1] + f32(0.05) * f32(size) + rs.uniform(0.0, 0.45, k).astype(f32) * f32(size)
    d_en = ((lo[pick] + rs.rand(k, 3) * (hi[pick] - lo[pick]) - o_en) / size).astype(f32)
    with np.errstate(all="ignore"):  # the box test's own quotients, in f32: RN((plane - o) / d)
        q0, q1 = (lo[pick] - o_en) / d_en, (hi[pick] - o_en) / d_en
    entry = np.maximum(np.minimum(q0, q1).max(axis=1), f32(0.0)).astype(f32)
    which = np.arange(k) % 3
    t_en = np.where(which == 0, entry, np.where(which == 1, np.nextafter(entry, f32(np.inf)), np.nextafter(entry, f32(0.0)))).astype(f32)
    t_en = np.where(np.isfinite(t_en) & (t_en > 0), t_en, np.inf)
    o = np.concatenate([o_up, o_gr, o_co, o_en]).astype(f32)
    d = np.concatenate([d_up, d_gr, d_co, d_en]).astype(f32)
    return o, d, np.concatenate([t_up, t_gr, t_co, t_en]).astype(f32)


def world_rays(sb, hs, forwards, n=100000):
    """local_rays carried into the world by the instances' transforms in turn ([col][row]: a row vector times the columns).  A translation
    alone leaves every direction bit as it is and moves the origins by whole numbers; t_max stays the mesh-space distance only there."""
    o, d, tmax = local_rays(sb, hs, n)
    wo, wd = np.empty_like(o), np.empty_like(d)
    for i, fwd in enumerate(forwards):
        rows = slice(i, None, len(forwards))
        fwd = np.asarray(fwd, dtype=np.float64)
        wo[rows] = (o[rows] @ fwd[:3, :3] + fwd[3, :3]).astype(f32)
        wd[rows] = (d[rows] @ fwd[:3, :3]).astype(f32)
    return wo, wd, tmax


def check_occlusion(gpu_ctx, many, instances):
    sb, forwards = build(many, instances)
    hs = pbrs_amd.HostScene(sb)
    if many:
        blas = hs.nodes("blas")
        assert (blas[(blas[:, 7] & 0x80000000) != 0][:, 7] & 0x7FFFFFFF).max() == 13
    o, d, tmax = world_rays(sb, hs, forwards)
    assert len(o) >= 100000
    _, occ_ref, _ = OracleScene(sb).intersect(o, d, tmax, closest=False, anyhit=True)
    occ_ref = np.asarray(occ_ref).astype(bool)
    # neither branch of the leaf step can be absent: rays that end on a passing triangle, rays that leave every leaf without one
    print("rays %d, occluded %d (%.1f %%)" % (len(o), occ_ref.sum(), 100.0 * occ_ref.mean()))
    assert occ_ref.mean() >= 0.10 and (~occ_ref).mean() >= 0.30, occ_ref.mean()
    gpu_ctx.upload(hs)
    _, occ_gpu = gpu_ctx.intersect(o, d, tmax, closest=False, anyhit=True)
    info = gpu_ctx.last_intersect_info()
    assert info["wide_any"] == 1, info
    assert info["slow_any"] < len(o) // 100, info  # the rays are the wide walk's own
    wrong = np.flatnonzero(np.asarray(occ_gpu).astype(bool) != occ_ref)
    assert len(wrong) == 0, (len(wrong), wrong[:8], o[wrong[:8]], d[wrong[:8]], tmax[wrong[:8]])


def test_terrain_ray_set_matches_the_oracle(gpu_ctx):
    check_occlusion(gpu_ctx, many=False, instances="translated")


def test_a_many_triangle_leaf_keeps_the_verify_first_path(gpu_ctx):
    check_occlusion(gpu_ctx, many=True, instances="translated")


def test_a_blas_shared_by_a_translated_and_a_rotated_instance(gpu_ctx):
    check_occlusion(gpu_ctx, many=True, instances="shared")


def test_terrain_render_matches_the_oracle(gpu_ctx):
    """The C4 family (the terrain at 32 x 64 cells, the floor, the four sphere lights) through the scene's own kernels: k_shadow's wide walk."""
    sb = scenes.terrain_scene(width=64, height=32, nx=32, nz=64)
    osc = OracleScene(sb)
    gpu_ctx.upload(pbrs_amd.HostScene(sb))
    ref, ost = osc.render(4, 4, 8, 7)
    img, st = gpu_ctx.render(4, 4, 8, 7)
    assert ost["panics"] == 0 and ost["shadow_rays"] > 10000
    assert st["kernel_features_shadow"] & 16, st["kernel_features_shadow"]  # PBRS_FEAT_WIDE
    assert (bits(img) == bits(ref)).all()
