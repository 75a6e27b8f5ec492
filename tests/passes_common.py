"""What the light pass tests share: the scenes, and the per-sample radiances D_i (depth 1) and L_i (depth d) of a tile from the oracle's
single-sample trace, computed once per case and kept read-only."""
import functools

import numpy as np

from oracle.binding import OracleScene
from pbrs_amd import scenes
from pbrs_amd.spec import deg

SEED = 11


@functools.lru_cache(maxsize=None)
def builder(name, width, height):
    if name in ("sphere_light", "light_in_view"):
        sb = scenes.sphere_light_scene(width, height)
        if name == "light_in_view":
            # from further back, so that the light itself is on the film, under a constant environment, and on a floor: one convex
            # object alone receives no light that took more than one vertex
            sb.env = (0.2, 0.3, 0.5)
            sb.instance(scenes.quad_mesh(sb, (-4, -1, -4), (4, -1, -4), (-4, -1, 4), (4, -1, 4), (0, 1, 0)), sb.lambertian((0.6, 0.6, 0.6)))
            sb.set_camera(width, height, deg(40.0), (0, 1.5, -9), (0, 1.5, 0))
        return sb
    return scenes.cornell_scene(width, height, variant=name)


@functools.lru_cache(maxsize=None)
def oracle_samples(name, width, height, strata, depth, tile=None, seed=SEED):
    """-> D, L: (spp, h, w, 3) f32 each, and ends: (spp, h, w) bool, the samples whose path ends at its first vertex."""
    osc = OracleScene(builder(name, width, height))
    x0, y0, w, h = tile or (0, 0, width, height)
    spp = strata[0] * strata[1]
    D = np.empty((spp, h, w, 3), np.float32)
    L = np.empty_like(D)
    ends = np.empty((spp, h, w), bool)
    for i in range(spp):
        for r in range(h):
            for c in range(w):
                D[i, r, c] = osc.trace_sample(y0 + r, x0 + c, i, strata[0], strata[1], 1, seed).radiance
                tr = osc.trace_sample(y0 + r, x0 + c, i, strata[0], strata[1], depth, seed)
                L[i, r, c] = tr.radiance
                ends[i, r, c] = tr.n_bounces == 1
    osc.close()
    for a in (D, L, ends):
        a.setflags(write=False)
    return D, L, ends
