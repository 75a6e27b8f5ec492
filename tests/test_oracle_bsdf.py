"""oracle_bsdf_eval is wired to the right functions in the right argument order: closed forms of src/bsdf.rs and geometry/src/bxdf.rs
that need no second model.  The device's pbrs_bsdf_eval is compared with this entry bit for bit (tests/test_gpu_bsdf_sweep.py); these
cases keep the two from being wrong together through one wiring mistake.  f32 arithmetic is numpy's, operation by operation, in the
order of the source; the functions of include/pbrs_numeric.h come from the oracle's own build of that header (numeric_eval).

Below the anchors: what the oracle alone says about the sweep of tests/test_gpu_bsdf_sweep.py — the counts pinned there are the ones it
produces, few words are NaN, and the inputs reach the branches they are there for."""
import functools

import numpy as np

import pytest

import bsdf_inputs as B
import test_gpu_bsdf_sweep as S  # the pinned table and oracle_side(), which the device's comparisons go through as well
from oracle.binding import OracleScene, lib, numeric_eval

f32, u32 = np.float32, np.uint32
FRAC_1_PI = f32(0.318309886183790671538)
EXACT_FRAMES = ("identity", "mirrored")  # world = +-local exactly: the local direction is hat() of the query's


@functools.lru_cache(None)
def main_scene():
    sb, index = B.scene()
    return OracleScene(sb), index


def local(q, cols, frame):
    """The local direction of a query's wo (cols 7:10) or wi (10:13) in one of EXACT_FRAMES."""
    w = B.hat(q.view(f32)[:, cols])
    return w * np.array([-1, -1, 1], dtype=f32) if frame == "mirrored" else w


def exact_rows(q):
    fr = B.frame_of(q)
    names = list(B.FRAMES)
    return [(name, fr == names.index(name)) for name in EXACT_FRAMES]


def test_lambert_eval_and_pdf_are_the_closed_forms():
    osc, index = main_scene()
    albedo = np.array([0.7, 0.4, 0.2], dtype=f32)
    q = B.pair_queries(index["lambertian"])
    f, panics = osc.bsdf_eval("eval", q)
    p, _ = osc.bsdf_eval("pdf", q)
    assert not panics.any()
    for frame, rows in exact_rows(q):
        wo, wi = local(q[rows], slice(7, 10), frame), local(q[rows], slice(10, 13), frame)
        # BSDF::eval (src/bsdf.rs:43-51): black where wo lies in the surface, else the lobe's albedo * FRAC_1_PI whatever the directions
        want = np.where((wo[:, 2] == 0)[:, None], f32(0), (albedo * FRAC_1_PI)[None, :]).astype(f32)
        assert (wo[:, 2] == 0).any() and (f[rows, :3] == want.view(u32)).all(), frame
        assert not f[rows, 3:].any()
        # DiffuseReflect::prob (bxdf.rs:566-572): wi.z / pi on wo's side (a negative number below the surface), 0 across
        want = np.where(wo[:, 2] * wi[:, 2] >= 0, wi[:, 2] * FRAC_1_PI, f32(0)).astype(f32)
        assert (want < 0).any() and (want == 0).any()
        assert (p[rows, 6].view(f32) == want).all(), frame
        assert not p[rows, :6].any() and not p[rows, 7].any()
    # the rotated frames: the local wo is known only as far as the rotation's rounding, so eval is the closed form wherever the
    # direction was built with |cos theta| >= 1e-3 (rounding moves a cosine by 1e-7), and one of the two values everywhere
    rotated = ~np.isin(B.frame_of(q), [list(B.FRAMES).index(n) for n in EXACT_FRAMES])
    lit = (f[:, :3] == (albedo * FRAC_1_PI).view(u32)).all(axis=1)
    cos_o = np.tile(np.repeat(B.local_directions()[:, 2], len(B.local_directions())), len(B.FRAMES))
    assert rotated.sum() == len(q) // 2 and (lit | ~f[:, :3].any(axis=1))[rotated].all()
    assert lit[rotated & (np.abs(cos_o) >= 1e-3)].all() and (rotated & (np.abs(cos_o) >= 1e-3)).sum() > 100000


def test_lambert_sample_takes_v_then_the_remapped_u():
    """BSDF::sample hands the lobe rnd2 = (v, fract(u n)) (Q8): with one lobe, B.cos_sample_hemisphere(v, u), in the identity frame
    the world wi itself.  u and v differ in the grid, so a swap shows."""
    osc, index = main_scene()
    q = B.sample_queries(index["lambertian"])
    q = q[B.frame_of(q) == 0]
    r, _ = osc.bsdf_eval("sample", q)
    u, v = q.view(f32)[:, 13], q.view(f32)[:, 14]
    want = B.cos_sample_hemisphere(v, numeric_eval("fract", u))
    assert (want != B.cos_sample_hemisphere(u, v)).any()
    assert (r[:, 3:6].view(f32) == want).all()
    assert not (r[:, 7] & B.FLAG_IS_MASS).any()


def test_mirror_sample_reflects_about_the_normal():
    osc, index = main_scene()
    q = B.sample_queries(index["mirror"])
    q = q[B.frame_of(q) == 0]
    r, panics = osc.bsdf_eval("sample", q)
    wo = local(q, slice(7, 10), "identity")
    want = wo * np.array([-1, -1, 1], dtype=f32)
    got = r[:, 3:6].view(f32)
    assert (got == want).all()  # (a zero may differ in its sign: local_to_world adds the three columns)
    nz = want != 0
    assert (got.view(u32)[nz] == want.view(u32)[nz]).all()
    assert (r[:, 7] == B.FLAG_IS_MASS).all() and (r[:, 6].view(f32) == 1).all()
    # sample_specular is the same lobe with rnd2 = (0, 0), and says that it found one; a Lambertian has none
    s, _ = osc.bsdf_eval("sample_specular", q)
    assert (s[:, 7] == (B.FLAG_IS_MASS | B.FLAG_FOUND)).all() and (s[:, :7] == r[:, :7]).all()
    none, _ = osc.bsdf_eval("sample_specular", B.specular_queries(index["lambertian"]))
    assert not none.any()


def one_query(material, wo, u=0.0, v=0.0, wi=(0.0, 0.0, 1.0)):
    return B._rows(material, "identity", np.array([wo], dtype=f32), np.array([wi], dtype=f32), np.array([u], dtype=f32), np.array([v], dtype=f32))


def ulps(a, b):
    return abs(int(f32(a).view(u32)) - int(f32(b).view(u32)))


def test_dielectric_at_normal_incidence_and_beyond_the_critical_angle():
    """Fresnel at cos theta = 1 is ((eta - 1) / (eta + 1))^2 to a few f32 roundings of a value near 0.04: 16 ulp would cover them, the
    largest distance observed over these materials is 1 ulp, and 1 is what is asked.  The hybrid lobe reflects for rnd2.0 below that
    value — rnd2.0 is the query's v (Q8) — and refracts from it on; beyond the critical angle reflection is certain."""
    osc, index = main_scene()
    worst = 0
    for name in ("dielectric_1.5", "dielectric_0.7", "dielectric_tinted"):
        m, eta = index[name], float(f32(B.DIELECTRIC_IORS[name]))
        r, _ = osc.bsdf_eval("sample", one_query(m, (0, 0, 1)))
        assert r[0, 7] == B.FLAG_IS_MASS
        mass = r[0, 6].view(f32)
        worst = max(worst, ulps(mass, ((eta - 1.0) / (eta + 1.0)) ** 2))
        below, _ = osc.bsdf_eval("sample", one_query(m, (0, 0, 1), u=0.75, v=np.nextafter(mass, f32(0))))
        at, _ = osc.bsdf_eval("sample", one_query(m, (0, 0, 1), u=0.0, v=mass))
        assert below[0, 6].view(f32) == mass and below[0, 5].view(f32) == 1.0, name            # reflected: wi = +z
        assert at[0, 6].view(f32) == f32(1) - mass and at[0, 5].view(f32) == -1.0, name         # refracted: wi = -z
        assert below[0, 7] == at[0, 7] == B.FLAG_IS_MASS
        # total internal reflection: from inside for eta > 1, from outside for eta < 1 (sin theta = 0.866 > 0.7)
        z = -0.5 if eta > 1 else 0.5
        tir, _ = osc.bsdf_eval("sample", one_query(m, (np.sqrt(0.75), 0, z), u=0.5, v=B.ONE_BELOW))
        assert tir[0, 7] == B.FLAG_IS_MASS and tir[0, 6].view(f32) == 1.0 and np.sign(tir[0, 5].view(f32)) == np.sign(z), name
    print("largest distance of the reflection mass from its closed form:", worst, "ulp")
    assert worst <= 1, worst


def test_lobe_choice_follows_u_times_n_at_the_boundaries():
    """The Uber material of five lobes: u = k / 5 one ulp down and up picks lobe (uint32_t)(u * 5) — the product rounded to f32 — and
    the Lambertian's direction shows that the lobe was handed (v, fract(u * 5)).  Each lobe has a colour of its own
    (bsdf_inputs.uber_five_lobe)."""
    osc, index = main_scene()
    m = index["uber_five"]
    us = [f32(0.0)] + [np.nextafter(f32(k / 5), f32(t)) for k in range(1, 5) for t in (0.0, 1.0)] + [f32(B.ONE_BELOW)]
    q = np.concatenate([one_query(m, (0.6, 0.0, 0.8), u=u, v=v) for u in us for v in (0.0, 0.3, 0.9)])
    r, _ = osc.bsdf_eval("sample", q)
    want = np.array([int(f32(u * f32(5))) for u in us for _ in range(3)])
    assert (B.uber_five_lobe(q, r) == want).all(), (B.uber_five_lobe(q, r), want)
    assert want.tolist() == [k for k in (0, 0, 1, 1, 2, 2, 3, 3, 4, 4) for _ in range(3)]


def test_u_outside_the_unit_interval_is_refused():
    """`bxdfs.swap_remove((u * n) as usize)` panics upstream for u >= 1; a std::vector would read past its end."""
    osc, index = main_scene()
    out = np.zeros((1, 8), dtype=u32)
    for u in (1.0, np.nextafter(f32(0), f32(-1)), -1.0, 2.0 ** 31, np.inf, -np.inf, np.nan):
        q = one_query(index["uber_five"], (0.6, 0.0, 0.8), u=u)
        assert lib().oracle_bsdf_eval(osc._h, 2, 1, q.ctypes.data, out.ctypes.data, None) == -1, u
        assert lib().oracle_bsdf_eval(osc._h, 0, 1, q.ctypes.data, out.ctypes.data, None) == 0, u  # eval does not read u
    assert lib().oracle_bsdf_eval(osc._h, 2, 1, one_query(index["uber_five"], (0.6, 0.0, 0.8), u=B.ONE_BELOW).ctypes.data, out.ctypes.data, None) == 0


# ---- the sweep, as far as the oracle alone can show it --------------------------------------------------------------------------------
@pytest.mark.parametrize("group,name", S.GROUPS)
def test_oracle_counts_are_the_pinned_ones_and_few_words_are_nan(group, name):
    for op in B.OPS:
        S.oracle_side(group, name, op)


def identity_samples(name):
    _, index, osc = S.setup("all")
    q = B.sample_queries(index[name])
    q = q[B.frame_of(q) == 0]
    r, _ = osc.bsdf_eval("sample", q)
    return q, r


def specular_outcomes(q, r):
    """Of identity-frame samples: (reflected, refracted, the zero wi of specular_refract's total internal reflection), masses only."""
    wo, wi = q.view(f32)[:, 7:10], r[:, 3:6].view(f32)
    is_mass = (r[:, 7] & B.FLAG_IS_MASS) != 0
    zero = is_mass & (wi == 0).all(axis=1) & (r[:, :3] == 0).all(axis=1)
    return is_mass & ~zero & (wi[:, 2] * wo[:, 2] > 0), is_mass & ~zero & (wi[:, 2] * wo[:, 2] < 0), zero


@pytest.mark.parametrize("name", B.DIELECTRICS)
def test_every_dielectric_reflects_refracts_and_reflects_totally(name):
    """From the oracle's results.  The Dielectric material is one Hybrid lobe: beyond the critical angle its Fresnel coefficient is 1 and
    the lobe reflects with mass 1 whatever rnd2.0 is, so specular_refract — and its zero wi — is never reached there; both sides of the
    angle decide alike down to the ulp (test_no_dielectric_returns_a_zero_wi_near_its_critical_angle).  So total internal reflection is asked for as what the reference does: a certain reflection, on
    the side of the surface where the angle exists, and not one zero wi.  The zero wi itself is asked of the Transmission lobes below."""
    q, r = identity_samples(name)
    reflected, refracted, zero = specular_outcomes(q, r)
    assert reflected.any() and refracted.any() and not zero.any()
    ior = float(f32(B.DIELECTRIC_IORS[name]))
    certain = reflected & (r[:, 6].view(f32) == 1)
    below_v = q.view(f32)[:, 14] == f32(B.ONE_BELOW)  # rnd2.0 = v at its largest still reflects
    side = q.view(f32)[:, 9] < 0 if ior > 1 else q.view(f32)[:, 9] > 0
    if ior != 1.0:
        assert (certain & below_v & side).any()


def test_transmission_lobes_return_the_zero_wi_of_total_internal_reflection():
    q, r = identity_samples("uber_five")
    lobe = B.uber_five_lobe(q, r)
    reflected, refracted, zero = specular_outcomes(q, r)
    chosen = (q.view(f32)[:, 13] * f32(5)).astype(f32).astype(np.int64)
    for k in (0, 4):  # the opacity's lobe and kt
        assert (zero & (chosen == k)).any() and (refracted & (lobe == k)).any(), k
    assert (lobe[zero] == -1).all() and (q.view(f32)[zero, 9] <= 0).all()  # from inside only (eta = 1.4); wo.z = 0 counts as inside


def test_each_of_the_five_uber_lobes_is_chosen():
    q, r = identity_samples("uber_five")
    lobe = B.uber_five_lobe(q, r)
    assert sorted(set(lobe[lobe >= 0].tolist())) == [0, 1, 2, 3, 4]
    # ... the masses by the u that names them (the transcription of `(u * n) as usize` is anchored in tests/test_oracle_bsdf.py; a
    # density's direction may coincide with the other density's, so those two are told apart there, on a direction where it cannot)
    chosen = (q.view(f32)[:, 13] * f32(5)).astype(f32).astype(np.int64)
    masses = np.isin(lobe, (0, 3, 4))
    assert (lobe[masses] == chosen[masses]).all()


@pytest.mark.parametrize("name", list(B.MICROFACET_LOBE))
def test_every_microfacet_material_has_samples_rejected_by_same_hemisphere(name):
    """MicrofacetReflection::sample's `!same_hemisphere(wo, wi)` arm returns wi = +z with a density: in the identity frame the world wi
    is (0, 0, 1) to the bit where the microfacet lobe was the chosen one; alone in its material it also returns black at density 0.
    (The `a >= 1.6` return of beckmann_lambda is not asked for here: g and d are not visible from outside one by one.)"""
    q, r = identity_samples(name)
    chosen = (q.view(f32)[:, 13] * f32(B.LOBES[name])).astype(f32).astype(np.int64) == B.MICROFACET_LOBE[name]
    up = (r[:, 3:6] == np.array([0.0, 0.0, 1.0], dtype=f32).view(u32)).all(axis=1) & ((r[:, 7] & B.FLAG_IS_MASS) == 0)
    assert (chosen & up).sum() > 100
    if B.LOBES[name] == 1:
        assert (chosen & up & (r[:, :3] == 0).all(axis=1) & (r[:, 6] == 0)).sum() > 100


@pytest.mark.parametrize("name", [n for n in B.DIELECTRICS if float(f32(B.DIELECTRIC_IORS[n])) != 1.0])
def test_no_dielectric_returns_a_zero_wi_near_its_critical_angle(name):
    """Every f32 cosine within 3000 ulps of the critical one, on the side where the angle exists, on all 16 azimuths, with rnd2.0 at its
    largest and at 0.5: where the Fresnel coefficient leaves room to refract, refract() transmits — not one zero wi."""
    osc, index = main_scene()
    ior = float(f32(B.DIELECTRIC_IORS[name]))
    c = f32(np.sqrt(1.0 - 1.0 / (ior * ior)) if ior > 1.0 else np.sqrt(1.0 - ior * ior))
    z = (int(c.view(u32)) + np.arange(-3000, 3001)).astype(u32).view(f32).astype(np.float64) * (-1.0 if ior > 1.0 else 1.0)
    d = np.concatenate([np.stack([np.sqrt(1.0 - z * z) * x, np.sqrt(1.0 - z * z) * y, z], axis=1) for x, y in B.azimuths()]).astype(f32)
    for v in (B.ONE_BELOW, 0.5):
        q = B._rows(index[name], "identity", d, d, np.zeros(1, dtype=f32), np.full(1, v, dtype=f32))
        r, _ = osc.bsdf_eval("sample", q)
        reflected, refracted, zero = specular_outcomes(q, r)
        assert not zero.any() and reflected.any(), (name, v)
        # both sides of the angle are inside the scan: with rnd2.0 at its largest the far side refracts (at 0.5 the coefficient, above 0.5
        # this close to the angle, reflects throughout; and for the ior one ulp above 1 the whole scan rounds to sin theta_t >= 1)
        assert refracted.any() or v == 0.5 or abs(ior - 1.0) < 1e-6, name
