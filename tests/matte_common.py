"""What the matte tests share: the scenes of tests/test_gpu_aov.py's oracle comparison, the oracle's first hits per sample, and the
instance -> material map of a flattened scene."""
import ctypes as C
import functools

import numpy as np

import pbrs_amd
from oracle.binding import OracleScene
from common import GOLDEN_NAMES, SEED, golden_case

MISS = 0xFFFFFFFF
SCENES = GOLDEN_NAMES + ["zoo"]


def zoo():
    """One sphere of every material kind and a checker-textured one: the zoo of tests/test_gpu_aov.py (120 x 72)."""
    from pbrs_amd.spec import SceneBuilder, Transform, deg
    sb = SceneBuilder()
    mats = [sb.lambertian((0.6, 0.5, 0.4)), sb.metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.2), 0.1), sb.glossy((0.7, 0.7, 0.7), 0.2),
            sb.mirror((0.9, 0.9, 0.9)), sb.plastic((0.3, 0.5, 0.2), (0.4, 0.4, 0.4), 0.1), sb.dielectric(1.5),
            sb.diffuse_light((4, 4, 4)), sb.uber(kd=(0.3, 0.3, 0.5), ks=(0.2, 0.2, 0.2)), sb.substrate((0.4, 0.2, 0.2), (0.3, 0.3, 0.3))]
    for k, m in enumerate(mats):
        sb.instance(sb.sphere((0, 0, 0), 0.45), m, Transform.translater((-2.0 + 1.0 * (k % 5), 0.6 - 1.2 * (k // 5), 0.0)))
    sb.instance(sb.sphere((0, 0, 0), 0.45), sb.lambertian(sb.checker((0.9, 0.2, 0.2), (0.1, 0.1, 0.8))), Transform.translater((2.0, -0.6, 0.0)))
    sb.point_light((0, 4, -4), (30, 30, 30))
    sb.set_camera(120, 72, deg(50.0), (0.0, 0.0, -6.0), (0, 0, 0))
    return sb


def scene(name):
    return zoo() if name == "zoo" else golden_case(name)[0]


def material_of_instance(hs):
    """pbrs_instance::material of every instance of a HostScene."""
    n = hs.desc.n_instances
    return np.ctypeslib.as_array(C.cast(hs.desc.instances, C.POINTER(C.c_uint32)), shape=(n, 32))[:, 26].copy()


@functools.lru_cache(maxsize=None)
def first_hits(name, sx, sy):
    """The oracle's camera rays of the render and their closest hits, per sample index: inst (spp, P) u32 (MISS: no hit), the pixels
    where some sample met a traversal tie (the method of tests/test_gpu_aov.py, _oracle_first_hits), and the instance -> material map."""
    sb = scene(name)
    osc = OracleScene(sb)
    insts, tie = [], None
    for s in range(sx * sy):
        o, d = osc.camera_rays(s, sx, sy, SEED)
        hits, _, info = osc.intersect(o, d, np.full(len(o), np.inf, dtype=np.float32), anyhit=False)
        insts.append(hits["inst"].astype(np.uint32))
        tie = info["tie_mask"].copy() if tie is None else (tie | info["tie_mask"])
    return np.array(insts), tie, material_of_instance(pbrs_amd.HostScene(sb))
