"""Id mattes (include/pbrs_gpu.h, pbrs_render_tile_matte*, pbrs_matte_mask*; device/matte.h) against the numpy model of the header's
text (tests/matte_model.py) fed with the oracle's camera rays and closest hits, against render_aovs, and against themselves under
every way a render can be cut up.  Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import matte_model
import pbrs_amd
from pbrs_amd import DeviceBuffers, api, scenes
from common import SEED, all_ones, bits
from matte_common import MISS, SCENES, first_hits, scene

pytestmark = pytest.mark.gpu


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and (_u32(a[k]) == _u32(b[k])).all(), k


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("strata", [(2, 2), (4, 4)])
@pytest.mark.parametrize("key", ["instance", "material"])
@pytest.mark.parametrize("slots", [1, 2, 6])
def test_matte_matches_the_model_on_the_oracles_first_hits(gpu_ctx, name, strata, key, slots):
    """ids / coverage / residual from the oracle's per-sample camera rays and closest hits through the model.  Pixels where a sample met
    a traversal tie are left out (at least 90 % kept, as in tests/test_gpu_aov.py).  The C4 case's k_extend splits its queue (an open
    scene under a black environment): its dropped misses must count as misses.  The branches are asserted, not assumed: overflow with 2
    slots and none with 6 on C5 at 4 x 4, pixels with two used ranks on C5 and the Cornell boxes, empty tables in the zoo."""
    insts, tie, mat_of = first_hits(name, *strata)
    gpu_ctx.upload(pbrs_amd.HostScene(scene(name)))
    _, got, aov, _ = gpu_ctx.render_matte(*strata, 4, SEED, key=key, slots=slots, aovs=("coverage",))
    ids, coverage, residual, counts, overflow = matte_model.matte(insts, mat_of if key == "material" else None, slots)
    keep = ~tie
    assert keep.sum() >= 0.9 * keep.size
    P = keep.size
    for k, want in (("ids", ids), ("coverage", coverage), ("residual", residual)):
        g = _u32(got[k]).reshape(P, -1)
        w = _u32(want).reshape(P, -1)
        assert (g[keep] == w[keep]).all(), (name, k, np.flatnonzero((g != w).any(axis=1) & keep)[:8])
    # sum(count) + overflow == n_hit: at a power-of-two spp every term is a multiple of 1 / spp and the sums are exact
    total = (gpu_ctx.matte_mask(got["ids"], got["coverage"], np.unique(got["ids"])) + got["residual"]).astype(np.float32)
    assert (_u32(total) == _u32(aov["coverage"])).all()
    assert (got["ids"] != MISS).any()
    if name == "c5_many_lights" and strata == (4, 4) and key == "instance":
        assert slots != 2 or (got["residual"].reshape(-1)[keep] > 0).any()
        assert slots != 6 or not got["residual"].any()
    if name in ("c5_many_lights", "c2_cornell_diffuse", "c3_cornell_specular") and slots >= 2:
        assert ((got["ids"][..., 1] != MISS) & (got["coverage"][..., 1] > 0)).reshape(-1)[keep].any()
    if name == "zoo":
        empty = (got["ids"] == MISS).all(axis=-1)
        assert empty.mean() > 0.5 and (_u32(got["coverage"])[empty] == 0).all()


@pytest.mark.parametrize("name", ["c2", "c4"])
@pytest.mark.parametrize("integrator", ["path", "direct", "materials", "normals"])
def test_image_aovs_variance_and_stats_are_those_of_render_aovs(gpu_ctx, name, integrator):
    kw = {"nx": 64, "nz": 64} if name == "c4" else {}
    gpu_ctx.upload(pbrs_amd.HostScene(scenes.build_config(name, width=48, height=32, **kw)[0]))
    s = (1, 1) if integrator in ("materials", "normals") else (2, 2)
    names = api.AOV_NAMES + ("variance",)
    for counters in (False, True):
        img, aov, st = gpu_ctx.render_aovs(*s, 5, 3, aovs=names, counters=counters, integrator=integrator)
        img2, matte, aov2, st2 = gpu_ctx.render_matte(*s, 5, 3, aovs=names, counters=counters, integrator=integrator)
        assert (bits(img) == bits(img2)).all()
        _same(aov, aov2)
        assert {k: v for k, v in st.items() if not k.startswith("ms_")} == {k: v for k, v in st2.items() if not k.startswith("ms_")}
        assert (matte["ids"][..., 0] == aov["instance"])[matte["coverage"][..., 0] == 1.0].all() and (matte["ids"] != MISS).any()
        # no AOV requested beside the matte: the image still is the plain render's
        img3, matte3, aov3, _ = gpu_ctx.render_matte(*s, 5, 3, counters=counters, integrator=integrator)
        assert aov3 == {} and (bits(img) == bits(img3)).all()
        _same(matte, matte3)


@pytest.mark.parametrize("name", ["c4", "c2"])
def test_matte_does_not_depend_on_how_the_render_is_cut(gpu_ctx, name):
    """samples_per_pass 1 / 3 / auto, pass overlap on and off, a tile against the same window of the frame, interleaved bands against
    the matching rows (the matrix of tests/test_gpu_aov.py).  C4 splits k_extend's queue.  Few slots, so that where a pixel sees more ids
    than the table holds the order the samples arrive in shows."""
    kw = {"nx": 64, "nz": 64} if name == "c4" else {}
    gpu_ctx.upload(pbrs_amd.HostScene(scenes.build_config(name, width=48, height=32, **kw)[0]))
    sx, sy, depth = 3, 2, 5
    for key, slots in (("instance", 2), ("material", 5)):
        def matte(**cut):
            return gpu_ctx.render_matte(sx, sy, depth, 7, key=key, slots=slots, **cut)[1]
        ref = matte()
        H, W = ref["residual"].shape
        assert (ref["ids"] != MISS).any()
        try:
            for overlap in (True, False):
                gpu_ctx.set_pass_overlap(overlap)
                for spp_pass in (1, 3, 0):
                    _same(ref, matte(samples_per_pass=spp_pass))
                    x0, y0, w, h = 5, 3, W - 13, H - 9
                    _same({k: v[y0:y0 + h, x0:x0 + w] for k, v in ref.items()}, matte(tile=(x0, y0, w, h), samples_per_pass=spp_pass))
                    band_rows, band_count = 4, 2
                    for band_index in range(band_count):
                        rows = [r for r in range(H) if (r // band_rows) % band_count == band_index]
                        band = matte(tile=(0, 0, W, len(rows)), bands=(band_rows, band_count, band_index), samples_per_pass=spp_pass)
                        _same({k: v[rows] for k, v in ref.items()}, band)
        finally:
            gpu_ctx.set_pass_overlap(True)


def _layers(rng, h, w, slots, n_ids):
    ids = rng.integers(0, n_ids, size=(h, w, slots)).astype(np.uint32)
    ids[rng.random((h, w, slots)) < 0.2] = MISS
    coverage = rng.random((h, w, slots)).astype(np.float32)
    return ids, coverage


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 7, 3), (3, 300, 8), (33, 65, 6)])
def test_mask_matches_the_model(gpu_ctx, shape):
    """An empty selection, one id, several, all ids, ids absent from the image, the unused-rank id; 1 x 1 up to sizes that are no
    multiple of the block."""
    rng = np.random.default_rng(11)
    h, w, slots = shape
    ids, coverage = _layers(rng, h, w, slots, 40)
    for select in ([], [int(ids.reshape(-1)[0])], [3, 17, 5, 5, 39], np.unique(ids), [1000, 70000], [MISS], list(range(0, 40, 2)) + [MISS]):
        got = gpu_ctx.matte_mask(ids, coverage, select)
        want = matte_model.mask(ids, coverage, select)
        assert got.shape == (h, w) and (_u32(got) == _u32(want)).all(), select
    assert not gpu_ctx.matte_mask(ids, coverage, []).any()


def test_mask_with_the_largest_selection(gpu_ctx):
    rng = np.random.default_rng(5)
    ids, coverage = _layers(rng, 19, 23, 4, 6000)
    select = rng.choice(6000, size=api.MatteParams.MAX_SELECT, replace=False)
    got = gpu_ctx.matte_mask(ids, coverage, select)
    assert (_u32(got) == _u32(matte_model.mask(ids, coverage, select))).all() and got.any()
    with pytest.raises(pbrs_amd.PbrsError, match=r"\(-1\)"):
        gpu_ctx.matte_mask(ids, coverage, np.arange(api.MatteParams.MAX_SELECT + 1))
    assert (_u32(gpu_ctx.matte_mask(ids, coverage, select)) == _u32(got)).all()


def test_the_device_variants_give_the_host_variants_bits(gpu_ctx):
    """render_matte_device, then matte_mask_device on the context's stream with nothing in between, read after collect_stats()."""
    gpu_ctx.upload(pbrs_amd.HostScene(scenes.build_config("c5", width=48, height=32)[0]))
    slots, names = 2, ("depth", "instance", "variance")
    img, matte, aov, _ = gpu_ctx.render_matte(4, 4, 4, 9, slots=slots, aovs=names)
    select = np.unique(matte["ids"])[::2]
    host = {"rgb": img, **matte, **aov, "mask": gpu_ctx.matte_mask(matte["ids"], matte["coverage"], select)}
    assert host["mask"].any() and matte["residual"].any()
    with DeviceBuffers(all_ones(host)) as dev:
        H, W = host["mask"].shape
        gpu_ctx.render_matte_device(dev.ptr("rgb"), dev.ptrs(matte), 4, 4, 4, 9, slots=slots, aov_device_ptrs=dev.ptrs(names))
        gpu_ctx.matte_mask_device(dev.ptr("ids"), dev.ptr("coverage"), dev.ptr("mask"), W, H, slots, select)
        gpu_ctx.collect_stats()
        for n, a in host.items():
            assert (_u32(dev.download_like(n, a)) == _u32(a)).all(), n


def test_refusals_leave_the_context_usable(gpu_ctx):
    gpu_ctx.upload(pbrs_amd.HostScene(scenes.build_config("c2", width=48, height=32)[0]))
    good = gpu_ctx.render_matte(2, 2, 4, 9, slots=2)[1]
    L, h = gpu_ctx._L, gpu_ctx._h
    p = gpu_ctx._params(2, 2, 4, 9, None)
    rgb = np.empty((p.h, p.w, 3), np.float32)
    ids, cov = np.empty((p.h, p.w, 2), np.uint32), np.empty((p.h, p.w, 2), np.float32)
    cam = C.addressof(gpu_ctx.scene.camera)

    def call(params=p, key=0, slots=2, ids_ptr=ids.ctypes.data, cov_ptr=cov.ctypes.data, mp_null=False):
        mp, mb = api.MatteParams(), api.MatteBuffers()
        mp.key, mp.slots, mb.ids, mb.coverage = key, slots, ids_ptr, cov_ptr
        return L.pbrs_render_tile_matte(h, cam, C.addressof(params), rgb.ctypes.data, None, None, None if mp_null else C.addressof(mp), C.addressof(mb), None)

    def still_works():
        _same(good, gpu_ctx.render_matte(2, 2, 4, 9, slots=2)[1])

    assert call() == 0
    for integrator in ("path", "direct"):
        assert call(params=gpu_ctx._params(2, 2, 0, 9, None, integrator=integrator)) == -1
        still_works()
    for bad in ({"slots": 0}, {"slots": api.MatteParams.MAX_SLOTS + 1}, {"key": 2}, {"ids_ptr": None}, {"cov_ptr": None}, {"mp_null": True}):
        assert call(**bad) == -1, bad
        still_works()
    # the mask
    sel = np.array([1, 2, 5], np.uint32)
    out = np.empty((p.h, p.w), np.float32)

    def mask(w=p.w, hh=p.h, slots=2, ids_ptr=ids.ctypes.data, cov_ptr=cov.ctypes.data, select=sel, n=None, out_ptr=out.ctypes.data):
        return L.pbrs_matte_mask(h, w, hh, slots, ids_ptr, cov_ptr, None if select is None else select.ctypes.data, len(select) if n is None else n, out_ptr)

    ids[:], cov[:] = good["ids"], good["coverage"]
    assert mask() == 0
    first = out.copy()
    big = np.arange(api.MatteParams.MAX_SELECT + 1, dtype=np.uint32)
    for bad in ({"select": np.array([2, 1], np.uint32)}, {"select": np.array([1, 1], np.uint32)}, {"select": big}, {"select": None, "n": 1}, {"slots": 0},
                {"slots": api.MatteParams.MAX_SLOTS + 1}, {"w": 0}, {"hh": 0}, {"ids_ptr": None}, {"cov_ptr": None}, {"out_ptr": None}):
        assert mask(**bad) == -1, list(bad)
        assert mask() == 0 and (_u32(out) == _u32(first)).all()
    assert mask(select=None, n=0) == 0 and not out.any()
