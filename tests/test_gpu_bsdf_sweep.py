"""device/bsdf.h equals the oracle's src/bsdf.rs bit for bit, lobe by lobe, where renders do not go: every material SceneBuilder can
name, cos theta from 0 over the smallest normal to 1, the axes of the azimuth and their neighbours, four frames, u and v at 0, just below
1 and on every lobe boundary k / n, the critical angle of every dielectric, and a group of degenerate frames and directions
(tests/bsdf_inputs.py).  The device side is pbrs_bsdf_eval, which builds the Bsdf and makes the calls of k_shade; the CPU side is
oracle_bsdf_eval, which tests/test_oracle_bsdf.py anchors to closed forms.

A result word is NaN on the device exactly where the oracle has a NaN (its payload is not part of the contract); every other word,
the flags included, is compared as bits.  PINNED holds, per material and op, how many words that leaves and how many queries reach
a panic site of the reference, counted on the CPU: a NaN mask cannot grow, and an input set cannot shrink, without the table
changing.  In the regular groups at most MAX_NAN_SHARE of the words an op returns may be NaN; the degenerate group has no cap.

Every test here needs the device.  What the oracle alone can show — that it produces the pinned counts, that the cap holds, that the
inputs reach the branches they are there for — runs with the CPU suite: tests/test_oracle_bsdf.py, through oracle_side() below."""
import functools

import numpy as np
import pytest

import bsdf_inputs as B
import pbrs_amd
from oracle.binding import OracleScene

f32, u32 = np.float32, np.uint32
pytestmark = pytest.mark.gpu
MAX_NAN_SHARE = 0.05

# {group: {material: {op: (words compared as bits, queries that reach a panic site of the reference)}}}, from the oracle alone
PINNED = {
    "regular": {
        "lambertian": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2230272, 139200), "sample_specular": (11616, 0)},
        "mirror": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2230272, 0), "sample_specular": (11616, 0)},
        "dielectric_1.5": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2230272, 0), "sample_specular": (11616, 0)},
        "dielectric_1.0": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2230272, 0), "sample_specular": (11616, 0)},
        "dielectric_0.7": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2230272, 0), "sample_specular": (11616, 0)},
        "dielectric_next_above_1": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2230272, 0), "sample_specular": (11616, 0)},
        "dielectric_tinted": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2230272, 0), "sample_specular": (11616, 0)},
        "metal_fuzz_0": {"eval": (2985992, 0), "pdf": (3015120, 672), "sample": (2230272, 0), "sample_specular": (11616, 0)},
        "metal_fuzz_0.0001": {"eval": (2985992, 0), "pdf": (3015120, 672), "sample": (2230272, 0), "sample_specular": (11616, 0)},
        "metal_fuzz_0.5": {"eval": (2987144, 0), "pdf": (3015152, 672), "sample": (2230272, 0), "sample_specular": (11616, 0)},
        "metal_fuzz_1": {"eval": (2987144, 0), "pdf": (3015152, 672), "sample": (2230272, 0), "sample_specular": (11616, 0)},
        "metal_fuzz_2": {"eval": (2987144, 0), "pdf": (3015152, 672), "sample": (2230272, 0), "sample_specular": (11616, 0)},
        "metal_k0": {"eval": (2987144, 0), "pdf": (3015152, 672), "sample": (2229966, 0), "sample_specular": (11616, 0)},
        "glossy_0": {"eval": (2985992, 0), "pdf": (3015120, 672), "sample": (2230272, 0), "sample_specular": (11616, 0)},
        "glossy_0.0001": {"eval": (2985992, 0), "pdf": (3015120, 672), "sample": (2230272, 0), "sample_specular": (11616, 0)},
        "glossy_0.01": {"eval": (2987144, 0), "pdf": (3015152, 672), "sample": (2230272, 0), "sample_specular": (11616, 0)},
        "glossy_0.3": {"eval": (2987144, 0), "pdf": (3015152, 672), "sample": (2229966, 0), "sample_specular": (11616, 0)},
        "glossy_1": {"eval": (2987144, 0), "pdf": (3015152, 672), "sample": (2230272, 0), "sample_specular": (11616, 0)},
        "plastic_remap": {"eval": (2987144, 0), "pdf": (3015152, 672), "sample": (2222079, 63832), "sample_specular": (11616, 0)},
        "plastic_raw": {"eval": (2987144, 0), "pdf": (3015152, 672), "sample": (2222079, 63832), "sample_specular": (11616, 0)},
        "substrate": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2230272, 139200), "sample_specular": (11616, 0)},
        "uber_five": {"eval": (2987144, 0), "pdf": (3015152, 672), "sample": (2224248, 40600), "sample_specular": (11616, 0)},
        "uber_opaque": {"eval": (2987144, 0), "pdf": (3015152, 672), "sample": (2220769, 75436), "sample_specular": (11616, 0)},
        "uber_no_ks": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2230272, 139200), "sample_specular": (11616, 0)},
        "fourier_rgb": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2226576, 34776), "sample_specular": (11616, 0)},
        "fourier_mono": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2228424, 34160), "sample_specular": (11616, 0)},
        "fourier_fine": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2224728, 36544), "sample_specular": (11616, 0)},
        "fourier_translucent": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2228424, 119824), "sample_specular": (11616, 0)},
    },
    "degenerate": {
        "lambertian": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 2184), "sample_specular": (20224, 1896)},
        "mirror": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (8848, 1896), "sample_specular": (8848, 1896)},
        "dielectric_1.5": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (6952, 1896), "sample_specular": (6952, 1896)},
        "dielectric_1.0": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (6952, 1896), "sample_specular": (6952, 1896)},
        "dielectric_0.7": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (6952, 1896), "sample_specular": (6952, 1896)},
        "dielectric_next_above_1": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (6952, 1896), "sample_specular": (6952, 1896)},
        "dielectric_tinted": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (6952, 1896), "sample_specular": (6952, 1896)},
        "metal_fuzz_0": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 1896), "sample_specular": (20224, 1896)},
        "metal_fuzz_0.0001": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 1896), "sample_specular": (20224, 1896)},
        "metal_fuzz_0.5": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 1896), "sample_specular": (20224, 1896)},
        "metal_fuzz_1": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 1896), "sample_specular": (20224, 1896)},
        "metal_fuzz_2": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 1896), "sample_specular": (20224, 1896)},
        "metal_k0": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 1896), "sample_specular": (20224, 1896)},
        "glossy_0": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 1896), "sample_specular": (20224, 1896)},
        "glossy_0.0001": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 1896), "sample_specular": (20224, 1896)},
        "glossy_0.01": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 1896), "sample_specular": (20224, 1896)},
        "glossy_0.3": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 1896), "sample_specular": (20224, 1896)},
        "glossy_1": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 1896), "sample_specular": (20224, 1896)},
        "plastic_remap": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16384, 1968), "sample_specular": (20224, 1896)},
        "plastic_raw": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16384, 1968), "sample_specular": (20224, 1896)},
        "substrate": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 2184), "sample_specular": (20224, 1896)},
        "uber_five": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (12640, 2040), "sample_specular": (8848, 1896)},
        "uber_opaque": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16396, 2112), "sample_specular": (20224, 1896)},
        "uber_no_ks": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 2184), "sample_specular": (20224, 1896)},
        "fourier_rgb": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16384, 2040), "sample_specular": (20224, 1896)},
        "fourier_mono": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16408, 2032), "sample_specular": (20224, 1896)},
        "fourier_fine": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16384, 2056), "sample_specular": (20224, 1896)},
        "fourier_translucent": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16408, 2198), "sample_specular": (20224, 1896)},
    },
    "lambert": {
        "lambert_red": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2230272, 139200), "sample_specular": (11616, 0)},
        "lambert_grey": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2230272, 139200), "sample_specular": (11616, 0)},
        "lambert_black": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2230272, 139200), "sample_specular": (11616, 0)},
        "substrate": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2230272, 139200), "sample_specular": (11616, 0)},
        "emitter": {"eval": (3015968, 0), "pdf": (3015968, 0), "sample": (2230272, 0), "sample_specular": (11616, 0)},
    },
    "lambert_degenerate": {
        "lambert_red": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 2184), "sample_specular": (20224, 1896)},
        "lambert_grey": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 2184), "sample_specular": (20224, 1896)},
        "lambert_black": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 2184), "sample_specular": (20224, 1896)},
        "substrate": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (16432, 2184), "sample_specular": (20224, 1896)},
        "emitter": {"eval": (20224, 2528), "pdf": (20224, 2528), "sample": (20224, 1896), "sample_specular": (20224, 1896)},
    },
}


@functools.lru_cache(None)
def setup(which):
    """-> (SceneBuilder, {material: index}, OracleScene) of the sweep's scene ("all") or of the Lambert-only scene ("lambert")."""
    sb, index = B.scene() if which == "all" else B.lambert_scene()
    return sb, index, OracleScene(sb)


def group_queries(group, material, op):
    return B.degenerate_queries(material) if group.endswith("degenerate") else B.queries(material, op)


def nan_words(r):
    nan = np.zeros(r.shape, dtype=bool)
    nan[:, :7] = np.isnan(r[:, :7].view(f32))
    return nan


def oracle_side(group, name, op):
    """The oracle's results for one (group, material, op), checked against the table and the cap."""
    _, index, osc = setup("lambert" if group.startswith("lambert") else "all")
    q = group_queries(group, index[name], op)
    cpu, panics = osc.bsdf_eval(op, q)
    nan = nan_words(cpu)
    got = (int(cpu.size - nan.sum()), int((panics > 0).sum()))
    share = float(nan[:, list(B.RETURNED[op])].mean())
    print(f"{group} {name} {op}: {len(q)} queries, {got[0]} words compared as bits, {got[1]} queries with panics, NaN share {share:.4f}")
    assert got == PINNED[group][name][op], (group, name, op, got)
    if not group.endswith("degenerate"):
        assert share <= MAX_NAN_SHARE, (group, name, op, share)
    return q, cpu


def compare(what, q, cpu, dev):
    nan, dev_nan = nan_words(cpu), nan_words(dev)
    wrong = (nan != dev_nan).any(axis=1)
    assert not wrong.any(), (what, "NaN on one side only", int(wrong.sum()), [hex(v) for v in q[wrong][0]], [hex(v) for v in cpu[wrong][0]],
                             [hex(v) for v in dev[wrong][0]])
    wrong = (~nan & (cpu != dev)).any(axis=1)
    assert not wrong.any(), (what, int(wrong.sum()), [hex(v) for v in q[wrong][0]], [hex(v) for v in cpu[wrong][0]], [hex(v) for v in dev[wrong][0]])


GROUPS = [(g, n) for g in ("regular", "degenerate") for n in B.MATERIALS] + [(g, n) for g in ("lambert", "lambert_degenerate") for n in B.LAMBERT_MATERIALS]


# ---- the device against the oracle --------------------------------------------------------------------------------------------------
def upload(gpu_ctx, which):
    sb, index, _ = setup(which)
    gpu_ctx.upload(pbrs_amd.HostScene(sb))
    return index


@pytest.mark.parametrize("name", B.MATERIALS)
def test_device_equals_the_oracle(gpu_ctx, name):
    upload(gpu_ctx, "all")
    for group in ("regular", "degenerate"):
        for op in B.OPS:
            q, cpu = oracle_side(group, name, op)
            compare((group, name, op), q, cpu, gpu_ctx.bsdf_eval(op, q))


@pytest.mark.parametrize("name", B.LAMBERT_MATERIALS)
def test_lambert_specialisation_equals_the_generic_code_and_the_oracle(gpu_ctx, name):
    """On a scene the planner gives PBRS_SHADE_LAMBERT, lam = true (the lobe's kind is never read) and lam = false agree with each
    other and with the oracle, for all four ops; an emitter's empty lobe list included."""
    upload(gpu_ctx, "lambert")
    for group in ("lambert", "lambert_degenerate"):
        for op in B.OPS:
            q, cpu = oracle_side(group, name, op)
            generic, special = gpu_ctx.bsdf_eval(op, q), gpu_ctx.bsdf_eval(op, q, lambert=True)
            compare((group, name, op, "generic"), q, cpu, generic)
            compare((group, name, op, "lambert"), q, cpu, special)
            nan = nan_words(cpu)
            assert (generic[~nan] == special[~nan]).all()


def test_refusals_leave_the_context_usable(gpu_ctx):
    from pbrs_amd.libs import PbrsError
    L, bits = gpu_ctx._L, lambda a: a.ctypes.data
    index = upload(gpu_ctx, "all")
    q = B.specular_queries(index["mirror"])
    out = np.zeros((len(q), B.RESULT_WORDS), dtype=u32)

    def refused(rc, words):
        message = L.pbrs_last_error(gpu_ctx._h).decode()
        assert rc == -1 and words in message, (rc, message)  # PBRS_E_INVALID

    refused(L.pbrs_bsdf_eval(gpu_ctx._h, 0, 0, len(q), None, bits(out)), "null")
    refused(L.pbrs_bsdf_eval(gpu_ctx._h, 0, 0, len(q), bits(q), None), "null")
    refused(L.pbrs_bsdf_eval(gpu_ctx._h, 4, 0, len(q), bits(q), bits(out)), "unknown op")
    refused(L.pbrs_bsdf_eval(gpu_ctx._h, 0, 1, len(q), bits(q), bits(out)), "Lambert")
    for u in (1.0, np.nextafter(f32(0), f32(-1)), -1.0, 2.0 ** 31, np.inf, -np.inf, np.nan):  # BSDF::sample's lobe index is (u * n) as usize
        off = q.copy()
        off.view(f32)[len(q) // 2, 13] = u
        refused(L.pbrs_bsdf_eval(gpu_ctx._h, 2, 0, len(q), bits(off), bits(out)), "u outside [0, 1)")
        assert L.pbrs_bsdf_eval(gpu_ctx._h, 0, 0, len(q), bits(off), bits(out)) == 0  # (eval does not read u)
        out[:] = 0
    assert not out.any()
    assert L.pbrs_bsdf_eval(gpu_ctx._h, 0, 0, 0, None, None) == 0  # n = 0: nothing to touch
    for bad in (len(index), 0xffffffff):
        far = q.copy()
        far[len(q) // 2, 0] = bad
        with pytest.raises(PbrsError, match="material index out of range"):
            gpu_ctx.bsdf_eval("sample", far)
    fresh = pbrs_amd.Context(0)
    try:
        assert len(fresh.bsdf_eval("eval", q[:0])) == 0
        with pytest.raises(PbrsError, match="no scene uploaded"):
            fresh.bsdf_eval("eval", q)
    finally:
        fresh.close()
    tsb, textured = B.textured_scene()
    gpu_ctx.upload(pbrs_amd.HostScene(tsb))
    tq = q.copy()
    tq[:, 0] = textured
    with pytest.raises(PbrsError, match="textured materials are out of scope"):
        gpu_ctx.bsdf_eval("eval", tq)
    # and after all that the context renders a frame as before: the Cornell box, bit for bit the oracle's
    from pbrs_amd import scenes
    sb, _ = scenes.build_config("c2", width=48, height=48)
    gpu_ctx.upload(pbrs_amd.HostScene(sb))
    img, _ = gpu_ctx.render(2, 2, 4, 5)
    ref, stats = OracleScene(sb).render(2, 2, 4, 5)
    assert stats["panics"] == 0 and np.isfinite(ref).all() and ref.max() > 0
    assert (img.view(u32) == ref.view(u32)).all()
