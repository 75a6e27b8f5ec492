"""Every scene of tests/variant_scenes.py on the GPU against the oracle, bit for bit, through the shipped kernels and the instrumented
ones.  tests/test_variant_census.py proves on the CPU that these scenes reach every k_shade instantiation and every traversal key the
planner can yield; the kernel keys a render reports are compared with the probe's here, which ties that census to what ran."""
import numpy as np
import pytest

import pbrs_amd
import plan_probe as pp
import variant_scenes as vs
from oracle.binding import OracleScene

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", list(vs.VARIANTS))
def test_variant_scene_matches_oracle(gpu_ctx, name):
    sb = vs.scene(name)
    hs = pbrs_amd.HostScene(sb)
    facts, choice = pp.probe(hs)
    gpu_ctx.upload(hs)
    for integrator, strata, depth in vs.RENDERS:
        ref, ost = vs.reference(name)[integrator]
        assert ost["tlas_ties"] == 0, (name, integrator)
        nan = np.isnan(ref)
        for counters in (False, True):
            img, st = gpu_ctx.render(strata[0], strata[1], depth, vs.SEED, integrator=integrator, counters=counters)
            what = (name, integrator, "instrumented" if counters else "shipped")
            assert (nan == np.isnan(img)).all(), what
            assert (bits(img)[~nan] == bits(ref)[~nan]).all(), what
            assert st["invalid_samples"] == ost["nonfinite_samples"], what
            if counters:
                assert st["closest_rays"] == ost["closest_rays"] and st["shadow_rays"] == ost["shadow_rays"], what
                assert st["kernel_features_extend"] == 0x80000000 | (choice["extend_stats"][0] & 511), what
            else:  # the kernels the probe names are the kernels that ran
                assert st["kernel_features_extend"] == choice["extend"][0], (what, st["kernel_features_extend"], choice["extend"])
                if st["shadow_rays"] or st["launches_shadow"]:
                    assert st["kernel_features_shadow"] == choice["shadow"][0], (what, st["kernel_features_shadow"], choice["shadow"])
            if st["launches_shade"]:  # one or two k_shade launches per bounce, as planned: the count of bounces is a whole number of passes
                n_shade = len(choice[integrator]["shade"])
                assert 1 <= n_shade <= 2 and st["passes"] >= 1 and st["launches_shade"] % st["passes"] == 0 and st["launches_shade"] == st["launches_extend"], (what, st)


WIDE = [name for name in vs.VARIANTS if vs.plan(name)[1]["wide_shadow"]]


@pytest.mark.parametrize("name", WIDE)
def test_wide_shadow_scenes_answer_occlusion_queries_as_the_oracle(gpu_ctx, name):
    """Occlusion queries through the any-hit walk k_shadow runs for the scene (the four-wide one where the plan says so, with its hand-off to
    the binary walk for rays outside the guarded range of the division-free box test), and closest hits, ray by ray."""
    sb = vs.scene(name)
    hs = pbrs_amd.HostScene(sb)
    _, choice = pp.probe(hs)
    assert choice["wide_shadow"] and choice["shadow"][0] & pp.WIDE
    gpu_ctx.upload(hs)
    osc = OracleScene(sb)
    rng = np.random.default_rng(11)
    n = 384
    # origins above the chain floor (x from -4 to 14.7 about z = 1), half of them over its deep end, where the triangles are small and a
    # walk goes down every level
    o = np.stack([rng.uniform(-4.0, 14.0, n), rng.uniform(0.05, 3.0, n), rng.uniform(-2.0, 4.0, n)], axis=1).astype(np.float32)
    o[: n // 2, 0] = rng.uniform(13.5, 14.8, n // 2)
    o[: n // 2, 1] = rng.uniform(0.05, 0.5, n // 2)
    o[: n // 2, 2] = rng.uniform(0.7, 1.3, n // 2)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[: n // 2, 1] = -np.abs(d[: n // 2, 1]) - 1.0
    d[::7, 0] = 0.0          # axis-parallel, denormal and huge components: refused by the wide walk, traced by the binary one
    d[::11, 2] = 0.0
    d[3::13, 0] = 1e-42
    d[4::17, 1] *= np.float32(2.0 ** 50)
    o[6::19, 2] = 1e-30
    tmax = np.where(rng.uniform(size=n) < 0.5, np.inf, rng.uniform(0.5, 20.0, n)).astype(np.float32)
    gh, gocc = gpu_ctx.intersect(o, d, tmax)
    info = gpu_ctx.last_intersect_info()
    assert info["wide_any"] == 1, (name, info)  # occlusion went through the four-wide any-hit walk, as in k_shadow
    refused = (d == 0).any(axis=1) | (np.abs(d) < 2.0 ** -40).any(axis=1) | (np.abs(d) > 2.0 ** 40).any(axis=1) | ((o != 0) & (np.abs(o) < 2.0 ** -60)).any(axis=1)
    assert n > info["slow_any"] >= int(refused.sum()) > 50, (name, info, int(refused.sum()))
    oh, oocc, st = osc.intersect(o, d, tmax)
    keep = ~st["tie_mask"]  # bit-identical t from two instances: the documented deviation
    assert keep.mean() > 0.95, name
    assert (gocc == oocc).all(), name
    assert (bits(gh["t"]) == bits(oh["t"])).all() and (gh["inst"][keep] == oh["inst"][keep]).all() and (gh["prim"][keep] == oh["prim"][keep]).all(), name
    assert 0.02 < gocc.mean() < 0.98, (name, gocc.mean())
