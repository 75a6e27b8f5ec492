"""The spatial variance estimate on the GPU (include/pbrs_gpu.h, pbrs_spatial_variance[_device]; device/spatial_variance.h): bit for bit
against the CPU model of tests/spatial_variance_model.py on the histories synthetic sequences leave, every guide present or absent,
every radius, both flags, in place and out of place, blocks without a short pixel beside blocks with one, the device variant and the
device chain of Context.render_temporal(spatial=...), what the header refuses, and the error the estimate removes."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import pbrs_amd
import spatial_variance_model as sv
import temporal_model as tm
from common import bits
from pbrs_amd import DeviceBuffers, api, scenes
from test_gpu_denoise import same
from test_gpu_temporal import _yawed

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = ((1, 1), (2, 3), (7, 5), (64, 1), (1, 64), (37, 29), (130, 70))  # (w, h)
MOVES = ("none", "yaw", "away")
NAN_BITS = 0x7FC12345  # a NaN with a payload: the pass-through keeps it


@functools.lru_cache(maxsize=None)
def _sequence_inputs(w, h, move):
    inp = sv.sequence_inputs(w, h, w + h, move)
    for a in inp.values():
        a.setflags(write=False)
    return inp


def inputs(w, h, move):
    """The history three frames of `move` leave (shared, read-only), with a NaN payload planted into a copy of its variance."""
    inp = dict(_sequence_inputs(w, h, move))
    v = inp["variance"].copy()
    v.view(np.uint32)[h // 2, w // 3] = NAN_BITS
    inp["variance"] = v
    return inp


def given(inp, depth=True, normal=True, instance=True):
    on = {"depth": depth, "normal": normal, "instance": instance}
    return {n: (a if on.get(n, True) else None) for n, a in inp.items()}


def agree(got, want, what):
    bad = bits(got) != bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def in_place(ctx, inp, **params):
    """pbrs_spatial_variance with variance_out == variance_in at the C ABI -> the plane."""
    h, w = inp["length"].shape
    p = api.SpatialVarianceParams.make(w, h, **params)
    keep = {n: np.ascontiguousarray(a) for n, a in inp.items() if a is not None}
    v = keep["variance"].copy()
    g = api._temporal_struct(api.SpatialVarianceGuides, api.TEMPORAL_GUIDES, {n: keep[n].ctypes.data for n in api.TEMPORAL_GUIDES if n in keep},
                             "spatial variance guide")
    rc = ctx._L.pbrs_spatial_variance(ctx._h, C.addressof(p), keep["moments"].ctypes.data, keep["length"].ctypes.data, C.addressof(g),
                                      v.ctypes.data, v.ctypes.data)
    assert rc == 0, ctx._L.pbrs_last_error(ctx._h)
    return v


@pytest.mark.parametrize("move", MOVES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matches_the_cpu_model_bit_for_bit(gpu_ctx, size, move):
    """All guides and the id stop; min_temporal 2.5 and 4, radius 1, 2 and 3, with and without ONLY_UNKNOWN; out of place, and in
    place for one combination per radius."""
    w, h = size
    inp = inputs(w, h, move)
    estimated = 0
    for mt, radius, only in itertools.product((2.5, 4.0), (1, 2, 3), (False, True)):
        kw = dict(min_temporal=mt, radius=radius, only_unknown=only, id_stop=True)
        det = {}
        want = sv.spatial_variance(**inp, details=det, **kw)
        agree(gpu_ctx.spatial_variance(**inp, **kw), want, (size, move, kw))
        if only == (radius == 2):
            agree(in_place(gpu_ctx, inp, **kw), want, (size, move, kw, "in place"))
        estimated += int(det["estimated"].sum())
    if w * h >= 64:
        assert estimated > 0
        assert bits(want)[h // 2, w // 3] == NAN_BITS or sv.short_pixels(inp["length"], 4.0)[h // 2, w // 3]
    if size == (130, 70) and move == "yaw":  # the two lengths tell apart what is short
        n = inp["length"]
        assert 0 < sv.short_pixels(n, 2.5).sum() < sv.short_pixels(n, 4.0).sum() < n.size
        assert (n == 0).any() and np.isnan(n).any() and not np.isfinite(inp["moments"]).all()


@pytest.mark.parametrize("size", ((37, 29), (130, 70)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_guide_present_or_absent(gpu_ctx, size):
    """normal and instance (with and without the id stop) present or absent, with and without the depth guide, both min_temporal, in
    place and out of place: bit for bit, and a stop that is switched on changes the result."""
    w, h = size
    inp = inputs(w, h, "yaw")
    seen = {}
    for depth, normal, instance in itertools.product((False, True), repeat=3):
        for id_stop in ((False, True) if instance else (False,)):
            g = given(inp, depth, normal, instance)
            for mt in (2.5, 4.0):
                kw = dict(min_temporal=mt, id_stop=id_stop)
                want = sv.spatial_variance(**g, **kw)
                agree(gpu_ctx.spatial_variance(**g, **kw), want, (depth, normal, instance, kw))
                agree(in_place(gpu_ctx, g, **kw), want, (depth, normal, instance, kw, "in place"))
            seen[(depth, normal, instance, id_stop)] = bits(want).tobytes()
    assert len(seen) == 12
    base = seen[(False, False, False, False)]
    assert seen[(False, False, True, False)] == base                  # ids without the flag: not read
    assert seen[(True, False, False, False)] != base and seen[(False, True, False, False)] != base and seen[(False, False, True, True)] != base
    assert len(set(seen.values())) == 8
    # the binding's default: the id stop follows the presence of the ids
    agree(gpu_ctx.spatial_variance(**inp), sv.spatial_variance(**inp, id_stop=True), "default id stop")


def voting_inputs():
    """130 x 70, every history long except one short pixel in a corner of five blocks (one of them the ragged last block): whole
    16 x 16 blocks without a short pixel, beside blocks whose one estimate reads its halo across three block borders."""
    w, h = 130, 70
    rng = np.random.default_rng(21)
    y = rng.normal(2.0, 0.5, size=(h, w)).astype(f32)
    moments = np.stack([y, y * y], axis=2).astype(f32)
    length = np.full((h, w), 8.0, f32)
    corners = [(0, 0), (16, 32), (47, 95), (69, 129), (31, 64)]  # (row, column)
    for at in corners:
        length[at] = 1.0
    variance = rng.uniform(0.0, 1.0, size=(h, w)).astype(f32)
    variance.view(np.uint32)[40, 7] = NAN_BITS
    variance[corners[1]] = np.inf
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    depth = (3.0 + 0.01 * xs + 0.02 * ys).astype(f32)
    normal = np.stack([0.05 * np.sin(xs * 0.3), 0.05 * np.cos(ys * 0.2), -np.ones((h, w))], axis=2).astype(f32)
    instance = ((ys // 24) * 4 + xs // 40).astype(np.uint32)
    return dict(moments=moments, length=length, variance=variance, depth=depth, normal=normal, instance=instance), corners


def test_blocks_without_a_short_pixel_pass_through_beside_blocks_with_one(gpu_ctx):
    inp, corners = voting_inputs()
    for radius, only in itertools.product((1, 3), (False, True)):
        kw = dict(radius=radius, only_unknown=only, id_stop=True)
        det = {}
        want = sv.spatial_variance(**inp, details=det, **kw)
        assert det["estimated"].sum() == (1 if only else len(corners))  # with ONLY_UNKNOWN the pixel whose variance is +inf
        for g in (inp, given(inp, normal=False, instance=False)):
            w_ = want if g is inp else sv.spatial_variance(**g, radius=radius, only_unknown=only)
            agree(gpu_ctx.spatial_variance(**g, **dict(kw, id_stop=g["instance"] is not None)), w_, kw)
            agree(in_place(gpu_ctx, g, **dict(kw, id_stop=g["instance"] is not None)), w_, (kw, "in place"))
        rest = ~det["estimated"]
        assert (bits(want[rest]) == bits(inp["variance"][rest])).all() and bits(want)[40, 7] == NAN_BITS


def test_the_device_variant_on_caller_buffers_equals_the_host_variant(gpu_ctx):
    for (w, h), kw in (((37, 29), dict(min_temporal=2.5, radius=2)), ((130, 70), dict(only_unknown=True))):
        inp = inputs(w, h, "yaw")
        host = gpu_ctx.spatial_variance(**inp, **kw)
        with DeviceBuffers(dict(inp, out=np.zeros((h, w), f32))) as dev:
            guides = dev.ptrs(tm.GUIDE_NAMES)
            gpu_ctx.spatial_variance_device(dev.ptr("moments"), dev.ptr("length"), dev.ptr("variance"), dev.ptr("out"), w, h, guides, **kw)
            gpu_ctx.collect_stats()
            agree(dev.download_like("out", host), host, (w, h, "out of place"))
            agree(dev.download_like("variance", host), inp["variance"], (w, h, "the input is left alone"))
            gpu_ctx.spatial_variance_device(dev.ptr("moments"), dev.ptr("length"), dev.ptr("variance"), dev.ptr("variance"), w, h, guides, **kw)
            gpu_ctx.collect_stats()
            agree(dev.download_like("variance", host), host, (w, h, "in place"))


def test_render_temporal_with_the_estimate_is_the_hand_made_chain(gpu_ctx):
    """64 x 64 Cornell box, three frames, a yaw of 4 degrees per frame: render_temporal(spatial=True) against the three host calls;
    spatial=None and a call that never names the keyword against the two host calls of the chain as it was."""
    hs = pbrs_amd.HostScene(scenes.cornell_scene(width=64, height=64))
    gpu_ctx.upload(hs)
    cams = [_yawed(hs.camera, 4.0 * k) for k in range(3)]
    guides = ("albedo", "normal", "depth", "instance")
    tparams = dict(id_test=True)
    run = lambda **kw: list(gpu_ctx.render_temporal(cams, 1, 1, 5, [9, 10, 11], temporal=tparams, iterations=3, **kw))  # noqa: E731
    with_estimate, none, unnamed = run(spatial=True), run(spatial=None), run()
    tight = run(spatial=dict(radius=1, min_temporal=2.0, only_unknown=True))
    history = prev = cam_prev = None
    changed = 0
    for k, cam in enumerate(cams):
        img, aov, _ = gpu_ctx.render_aovs(1, 1, 5, 9 + k, aovs=guides + ("variance",), camera=cam)
        var = aov.pop("variance")
        history, v = gpu_ctx.temporal_accumulate(img, aov["depth"], cam, variance=var, normal=aov["normal"], instance=aov["instance"], history=history,
                                                 prev=prev, camera_prev=cam_prev, **tparams)
        kept = {n: aov[n] for n in tm.GUIDE_NAMES}
        vest = gpu_ctx.spatial_variance(history["moments"], history["length"], v, **kept)
        changed += int((bits(vest) != bits(v)).sum())
        for frames, variance in ((with_estimate, vest), (none, v), (unnamed, v),
                                 (tight, gpu_ctx.spatial_variance(history["moments"], history["length"], v, radius=1, min_temporal=2.0,
                                                                  only_unknown=True, **kept))):
            den, acc, noisy, st = frames[k]
            assert (bits(noisy) == bits(img)).all() and same(acc, history["rgb"]).all(), k
            assert same(den, gpu_ctx.denoise_var(history["rgb"], variance, iterations=3, **aov)).all(), k
            assert st["samples"] == 64 * 64
        prev, cam_prev = kept, cam
    assert changed > 3 * 64 * 64 // 2  # one sample per pixel: the AOV knows nothing, and every history is shorter than min_temporal
    assert any((bits(a[0]) != bits(b[0])).any() for a, b in zip(with_estimate, none))


def test_refusals_leave_the_context_usable(gpu_ctx):
    L = gpu_ctx._L
    w, h = 24, 20
    inp = inputs(w, h, "yaw")
    out = np.empty((h, w), f32)

    def call(fn=L.pbrs_spatial_variance, params=True, guides=True, drop=(), alias=None, **fields):
        p = api.SpatialVarianceParams.make(w, h, id_stop=True)
        for n, v in fields.items():
            setattr(p, n, v)
        g = api._temporal_struct(api.SpatialVarianceGuides, api.TEMPORAL_GUIDES, {n: inp[n].ctypes.data for n in tm.GUIDE_NAMES if n not in drop},
                                 "spatial variance guide")
        ptr = {n: (None if n in drop else inp[n].ctypes.data) for n in ("moments", "length", "variance")}
        o = None if "out" in drop else inp[alias].ctypes.data if alias else out.ctypes.data
        return fn(gpu_ctx._h, C.addressof(p) if params else None, ptr["moments"], ptr["length"], C.addressof(g) if guides else None,
                  ptr["variance"], o)
    nan, inf = float("nan"), float("inf")
    for fn in (L.pbrs_spatial_variance, L.pbrs_spatial_variance_device):  # (the device variant refuses before it touches a pointer)
        assert call(fn, params=False) == -1
        for n in ("moments", "length", "variance", "out"):
            assert call(fn, drop=(n,)) == -1, n
        assert call(fn, w=0) == -1 and call(fn, h=0) == -1
        assert call(fn, radius=0) == -1 and call(fn, radius=4) == -1
        for n in ("sigma_normal", "sigma_depth"):
            for v in (0.0, -1.0, nan, inf):
                assert call(fn, **{n: v}) == -1, (n, v)
        for v in (0.5, 0.0, -1.0, nan, inf):
            assert call(fn, min_temporal=v) == -1, v
        assert call(fn, flags=4) == -1 and call(fn, flags=0x80000001) == -1
        assert call(fn, drop=("instance",)) == -1 and call(fn, guides=False) == -1  # the id stop without ids
        assert b"instance" in L.pbrs_last_error(gpu_ctx._h)
        assert call(fn, alias="moments") == -1 and call(fn, alias="length") == -1
        assert call(fn, w=1 << 15, h=(1 << 13) + 1) == -4  # PBRS_E_LIMIT
        assert b"2^28" in L.pbrs_last_error(gpu_ctx._h)
    # what is allowed: no guides struct, absent guides, min_temporal 1 (nothing is short), radius 1
    assert call(guides=False, flags=0) == 0
    agree(out, sv.spatial_variance(**given(inp, False, False, False)), "no guides")
    assert call(drop=("instance", "normal"), flags=2, radius=1) == 0
    agree(out, sv.spatial_variance(**given(inp, normal=False, instance=False), radius=1, only_unknown=True), "depth only")
    assert call(min_temporal=1.0) == 0
    agree(out, inp["variance"], "min_temporal 1")
    assert call() == 0
    agree(out, sv.spatial_variance(**inp, id_stop=True), "all guides")
    # a plain render afterwards: the bits of a fresh context, which also grows its staging from nothing
    from test_gpu_pixel_filter import scene
    _, hs = scene("cornell")
    gpu_ctx.upload(hs)
    img, _ = gpu_ctx.render(2, 2, 3, 1)
    fresh = pbrs_amd.Context(0)
    try:
        fresh.upload(hs)
        assert (bits(img) == bits(fresh.render(2, 2, 3, 1)[0])).all()
        for size in ((9, 7), (70, 50), (33, 21)):
            i2 = inputs(size[0], size[1], "yaw")
            agree(fresh.spatial_variance(**i2), sv.spatial_variance(**i2, id_stop=True), size)
    finally:
        fresh.close()


# ---- the error the estimate removes ------------------------------------------------------------------------------------------------------
_CORNELL = {}


def cornell_128(ctx):
    """The 128 x 128 Cornell box uploaded, and its 32 x 32-strata render (seed 4242), rendered once."""
    if not _CORNELL:
        _CORNELL["hs"] = pbrs_amd.HostScene(scenes.cornell_scene(width=128, height=128))
    ctx.upload(_CORNELL["hs"])
    if "ref" not in _CORNELL:
        _CORNELL["ref"] = ctx.render_aovs(32, 32, 5, 4242, aovs=())[0]
    return _CORNELL["hs"], _CORNELL["ref"]


def _mse(img, ref, ok):
    return float(((img[ok].astype(np.float64) - ref[ok]) ** 2).mean())


def filtered_errors(ctx, strata, variants):
    """{name: [MSE of the filtered image after frames 1 and 3]} of render_temporal(spatial=variant) on the 128 x 128 Cornell box, a static
    camera, seeds 17, 18, 19, all guides, against the 32 x 32-strata render; over the pixels finite in all images."""
    hs, ref = cornell_128(ctx)
    cams = [hs.camera] * 3
    den = {name: [f[0] for f in ctx.render_temporal(cams, strata, strata, 5, range(17, 20), spatial=variant)] for name, variant in variants.items()}
    ok = np.isfinite(ref).all(axis=2)
    for imgs in den.values():
        for img in imgs:
            ok &= np.isfinite(img).all(axis=2)
    assert ok.mean() > 0.99
    return {name: [_mse(imgs[k], ref, ok) for k in (0, 2)] for name, imgs in den.items()}


def test_the_estimate_removes_error_on_the_cornell_box(gpu_ctx):
    """128 x 128, 1 x 1 strata (the variance AOV is +inf everywhere), all guides, frames 1 and 3 of render_temporal: the chain as it was
    (spatial=None) against the chain with the estimate, each against the plain 32 x 32-strata render (seed 4242).  The new chain's MSE
    is below the parent's at both frames.  Measured on an MI355X: frame 1 0.4162 against 1.397 (ratio 0.298), frame 3 0.2922 against 1.370
    (ratio 0.213) ("Spatial variance estimate")."""
    e = filtered_errors(gpu_ctx, 1, {"parent": None, "estimate": True})
    for k, frame in enumerate((1, 3)):
        print(f"cornell 128 x 128, 1 spp, frame {frame}: filtered MSE with the variance unknown {e['parent'][k]:.4g}, with the spatial estimate "
              f"{e['estimate'][k]:.4g}, ratio {e['estimate'][k] / e['parent'][k]:.3f}")
    assert e["estimate"][0] < e["parent"][0] and e["estimate"][1] < e["parent"][1]


def test_the_estimate_beside_a_noisy_variance_aov_is_reported(gpu_ctx):
    """The same pair at 2 x 2 strata, where the variance AOV is finite and noisy, with and without ONLY_UNKNOWN (which then keeps the
    AOV wherever it is known).  Reported, not asserted: which of the three wins was not known before it was measured.  Measured on an
    MI355X ("Spatial variance estimate"): the variance AOV wins.  Frame 1: the chain as it was 0.1851, with the estimate 0.2030
    (ratio 1.097), with ONLY_UNKNOWN 0.1851 (four samples leave no pixel unknown: the chain as it was); frame 3: 0.1234, 0.1312 (1.063), 0.1234."""
    e = filtered_errors(gpu_ctx, 2, {"parent": None, "estimate": True, "only_unknown": dict(only_unknown=True)})
    for k, frame in enumerate((1, 3)):
        print(f"cornell 128 x 128, 4 spp, frame {frame}: filtered MSE of the chain as it was {e['parent'][k]:.4g}, with the spatial estimate "
              f"{e['estimate'][k]:.4g} (ratio {e['estimate'][k] / e['parent'][k]:.3f}), with ONLY_UNKNOWN {e['only_unknown'][k]:.4g} "
              f"(ratio {e['only_unknown'][k] / e['parent'][k]:.3f})")
    assert all(np.isfinite(v).all() for v in e.values())
