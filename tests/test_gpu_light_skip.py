"""The light a shadow ray was aimed at (device/shade.h, light_skip_tag; device/traverse.h, AnyWalk::skip) on the GPU: k_shade runs the
own test of the analytic instance that IS the chosen area light on the lone shadow ray it has just built and, where the value is false,
tags the ray; k_shadow then passes that instance's TLAS leaf over — out of the scan's mask where the TLAS is scanned, in the node step
that pops it where it is walked as a tree.  The term the walk leaves out is false, so every rendered pixel is still the oracle's, bit
for bit; the counting kernels ignore the tag, so the instrumented render equals the timed one and its counts are the oracle's.  The
links and a restatement of the walk with and without the skip are checked on the CPU (tests/test_light_skip.py).

Every case renders through the C ABI (pbrs_render_tile)."""
import numpy as np
import pytest

import pbrs_amd
from oracle.binding import OracleScene
from pbrs_amd import scenes
from pbrs_amd.spec import SceneBuilder, Transform, deg

pytestmark = pytest.mark.gpu
SX, SY, DEPTH, SEED = 2, 2, 4, 11


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def two_identical_lights():
    """A sphere light with two bit-identical instances: the light is linked to the first, which a tagged ray passes over; the second
    is still visited (and, like the first, does not occlude the sample: its own test is the same function of the same floats)."""
    sb = scenes.sphere_light_scene(width=64, height=64)
    sb.instance(sb.sphere((0, 3, 0), 0.5), sb.diffuse_light((10.0, 10.0, 10.0)))
    return sb


def transformed_light():
    """A sphere light whose instance carries a translation (the shape at the origin): no instance has the light's world-space shape
    under identity matrices, so no link is set and every ray walks as before."""
    sb = SceneBuilder()
    grey = sb.lambertian((0.5, 0.5, 0.5))
    emit = (10.0, 10.0, 10.0)
    sb.instance(sb.sphere((0, 0, 0), 1.0), grey)
    sb.instance(sb.sphere((0, 0, 0), 0.5), sb.diffuse_light(emit), Transform.translater((0.0, 3.0, 0.0)))
    sb.area_light(emit, sb.sphere((0, 3, 0), 0.5))
    sb.set_camera(64, 64, deg(40.0), (0, 1, -6), (0, 0, 0))
    return sb


CASES = {
    # name: (scene, shadow kernel feature bits that must be set, ... that must be clear)
    "terrain": (lambda: scenes.terrain_scene(width=96, height=64, nx=16, nz=32), 4 | 16, 0),  # scanned TLAS, the wide walk
    "cornell_diffuse": (lambda: scenes.cornell_scene(width=64, height=64, variant="diffuse"), 4, 16),  # triangle lights: no links
    "cornell_specular": (lambda: scenes.cornell_scene(width=64, height=64, variant="specular"), 4, 16),
    "flat_scan": (lambda: scenes.many_lights_scene(width=96, height=54, n_objects=8, n_lights=8), 4, 0),  # 18 instances: scanned
    "tree_tlas": (lambda: scenes.many_lights_scene(width=96, height=54, n_objects=24, n_lights=24), 0, 4),  # 50 instances: walked
    "c1": (lambda: scenes.sphere_light_scene(width=64, height=64), 4, 0),
    "duplicate": (two_identical_lights, 4, 0),
    "transformed": (transformed_light, 4, 0),
}
RENDERS = [(name, "path") for name in CASES] + [("terrain", "direct"), ("cornell_diffuse", "direct")]


@pytest.mark.parametrize("name,integrator", RENDERS)
def test_render_is_the_oracles_and_the_counts_too(gpu_ctx, name, integrator):
    build, feat_set, feat_clear = CASES[name]
    sb = build()
    hs = pbrs_amd.HostScene(sb)
    gpu_ctx.upload(hs)
    img, st = gpu_ctx.render(SX, SY, DEPTH, SEED, integrator=integrator)
    counted, cst = gpu_ctx.render(SX, SY, DEPTH, SEED, counters=True, integrator=integrator)
    ref, ost = OracleScene(sb).render(SX, SY, DEPTH, SEED, integrator=integrator)
    print("%s/%s: shadow rays %d, shadow kernel features %d" % (name, integrator, ost["shadow_rays"], st["kernel_features_shadow"]))
    # (the case is not vacuous: C1's sphere fills a small part of its 64 x 64 frame, the oracle casts just under a thousand shadow rays there)
    assert ost["panics"] == 0 and ost["shadow_rays"] > 500, ost
    assert st["kernel_features_shadow"] & feat_set == feat_set and st["kernel_features_shadow"] & feat_clear == 0, st["kernel_features_shadow"]
    nan = np.isnan(ref)
    assert (nan == np.isnan(img)).all() and (bits(img)[~nan] == bits(ref)[~nan]).all()
    assert (bits(counted) == bits(img)).all()  # the instrumented frame: kernels that ignore the tag
    assert cst["closest_rays"] == ost["closest_rays"] and cst["shadow_rays"] == ost["shadow_rays"], (cst, ost)
    assert cst["instances"] + cst["shadow_instances"] == ost["instances"], (cst, ost)
