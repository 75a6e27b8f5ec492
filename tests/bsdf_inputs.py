"""Inputs of the BSDF sweep (tests/test_gpu_bsdf_sweep.py on the device, tests/test_oracle_bsdf.py on the CPU), built without random
numbers: one scene that holds every material SceneBuilder can name, a Lambert-only scene for k_shade's Lambert specialisation, and the
16-word queries of pbrs_bsdf_eval / oracle_bsdf_eval (material, normal, tangent, wo, wi, u, v, spare) over grids of directions,
frames and random numbers that reach the edges: cos theta = 0, the smallest normal, one ulp below 1, the axes of the azimuth and
their neighbours, u = 0, u just below 1, the lobe boundaries k / n, the critical angle of every dielectric."""
import functools

import numpy as np

from fourier_scenes import table
from oracle.binding import numeric_eval
from pbrs_amd.spec import SceneBuilder, deg

u32, f32, f64 = np.uint32, np.float32, np.float64
QUERY_WORDS, RESULT_WORDS = 16, 8
OPS = ("eval", "pdf", "sample", "sample_specular")
# the float words of a result an op returns (include/pbrs_gpu.h): f, wi_out, pr; word 7 is the flags
RETURNED = {"eval": (0, 1, 2), "pdf": (6,), "sample": (0, 1, 2, 3, 4, 5, 6), "sample_specular": (0, 1, 2, 3, 4, 5, 6)}
FLAG_IS_MASS, FLAG_FOUND = 1, 2

ONE_BELOW = 1.0 - 2.0 ** -24
COS_THETA = [0.0] + [s * c for c in (2.0 ** -126, 1e-20, 1e-7, 1e-3, 0.1, 0.5, 0.9, ONE_BELOW, 1.0) for s in (1.0, -1.0)]
DIELECTRIC_IORS = {"dielectric_1.5": 1.5, "dielectric_1.0": 1.0, "dielectric_0.7": 0.7,
                   "dielectric_next_above_1": float(np.nextafter(f32(1.0), f32(2.0))), "dielectric_tinted": 1.5}
METAL_FUZZ = (0.0, 1e-4, 0.5, 1.0, 2.0)
GLOSSY_ROUGHNESS = (0.0, 1e-4, 0.01, 0.3, 1.0)
UBER_ETA = 1.4
FOURIER_TABLES = ("rgb", "mono", "fine", "translucent")
# "uber_five": the five-lobe form of tests/test_gpu_render.py's Uber material (anisotropic roughness, opacity below 1, kr and kt), with a
# colour of its own per lobe so that a sample says which lobe produced it: the opacity's transmission lobe is grey by construction
KD, KS, KR, KT = (0.3, 0.2, 0.1), (0.1, 0.4, 0.2), (0.5, 0.1, 0.1), (0.1, 0.2, 0.6)
UBER_FIVE = dict(kd=KD, ks=KS, kr=KR, kt=KT, rough=(0.05, 0.2), eta=UBER_ETA, opacity=0.7)


def material_makers():
    """name -> function of a SceneBuilder that adds the material and returns its index; the order is the scene's."""
    m = {"lambertian": lambda sb: sb.lambertian((0.7, 0.4, 0.2)), "mirror": lambda sb: sb.mirror((0.9, 0.8, 0.7))}
    for name, ior in DIELECTRIC_IORS.items():
        tinted = name == "dielectric_tinted"
        m[name] = lambda sb, ior=ior, tinted=tinted: sb.dielectric(ior, (0.9, 0.5, 0.2), (0.2, 0.5, 0.9)) if tinted else sb.dielectric(ior)
    for fz in METAL_FUZZ:  # a real conductor (gold-like eta, k)
        m[f"metal_fuzz_{fz:g}"] = lambda sb, fz=fz: sb.metal((0.18, 0.42, 1.37), (3.42, 2.35, 1.77), fz)
    m["metal_k0"] = lambda sb: sb.metal((1.5, 1.3, 1.1), (0.0, 0.0, 0.0), 0.3)
    for r in GLOSSY_ROUGHNESS:
        m[f"glossy_{r:g}"] = lambda sb, r=r: sb.glossy((0.9, 0.8, 0.7), r)
    m["plastic_remap"] = lambda sb: sb.plastic((0.2, 0.6, 0.3), (0.4, 0.5, 0.6), 0.15, True)
    m["plastic_raw"] = lambda sb: sb.plastic((0.2, 0.6, 0.3), (0.4, 0.5, 0.6), 0.15, False)
    m["substrate"] = lambda sb: sb.substrate((0.4, 0.5, 0.3), (0.1, 0.1, 0.1))
    m["uber_five"] = lambda sb: sb.uber(**UBER_FIVE)
    m["uber_opaque"] = lambda sb: sb.uber((0.5, 0.1, 0.1), (0.2, 0.3, 0.4), rough=(0.3, 0.3), opacity=1.0)
    m["uber_no_ks"] = lambda sb: sb.uber((0.5, 0.1, 0.1), (0, 0, 0), rough=(0.3, 0.3), opacity=1.0)
    for t in FOURIER_TABLES:
        m[f"fourier_{t}"] = lambda sb, t=t: sb.fourier(sb.fourier_table(table(t)))
    return m


MATERIALS = tuple(material_makers())
DIELECTRICS = tuple(DIELECTRIC_IORS)
# materials with a MicrofacetReflection lobe, and the index of that lobe among the material's
MICROFACET_LOBE = {**{n: 0 for n in MATERIALS if n.startswith(("metal_", "glossy_", "plastic_"))}, "uber_five": 2, "uber_opaque": 1}
LOBES = {**{n: 1 for n in MATERIALS}, "plastic_remap": 2, "plastic_raw": 2, "uber_five": 5, "uber_opaque": 2}


def _finish(sb, mats):
    """One unit sphere per material in a row (a flattener may drop what no instance names), a light, a camera."""
    for k, m in enumerate(mats):
        sb.instance(sb.sphere((2.5 * (k % 8) - 8.75, 1.0 + 2.5 * (k // 8), 0.0), 1.0), m)
    sb.point_light((0, 12, -9), (300, 300, 300))
    sb.env = (0.2, 0.25, 0.3)
    sb.set_camera(48, 32, deg(60), (0, 4, -16), (0, 4, 0))
    return sb


def scene():
    """-> (SceneBuilder, {material name: index})"""
    sb = SceneBuilder()
    index = {name: make(sb) for name, make in material_makers().items()}
    return _finish(sb, list(index.values())), index


LAMBERT_MATERIALS = ("lambert_red", "lambert_grey", "lambert_black", "substrate", "emitter")


def lambert_scene():
    """Every lobe an untextured Lambertian DiffuseReflect, at most one per material (Substrate degenerates to one, Q18; an emitter
    has none): the scenes k_shade's PBRS_SHADE_LAMBERT variants render."""
    sb = SceneBuilder()
    index = {"lambert_red": sb.lambertian((0.7, 0.2, 0.1)), "lambert_grey": sb.lambertian((0.5, 0.5, 0.5)),
             "lambert_black": sb.lambertian((0.0, 0.0, 0.0)), "substrate": sb.substrate((0.4, 0.5, 0.3), (0.1, 0.1, 0.1)),
             "emitter": sb.diffuse_light((4.0, 4.0, 4.0))}
    return _finish(sb, list(index.values())), index


def textured_scene():
    """-> (SceneBuilder, index of a material whose colour is a checker texture)"""
    sb = SceneBuilder()
    m = sb.lambertian(sb.checker((0.1, 0.1, 0.1), (0.8, 0.8, 0.8)))
    return _finish(sb, [m, sb.lambertian((0.5, 0.5, 0.5))]), m


# ---- directions ------------------------------------------------------------------------------------------------------------
def azimuths():
    """16 unit (x, y): the four axes, each with its two neighbours one ulp of 1 off the axis, and the four diagonals."""
    tiny = 2.0 ** -24
    out = []
    for ax, ay in ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)):
        out += [(ax, ay), (ax + tiny * -ay, ay + tiny * ax), (ax - tiny * -ay, ay - tiny * ax)]
    r = np.sqrt(0.5)
    return out + [(r, r), (-r, r), (-r, -r), (r, -r)]


# beckmann_lambda returns 0 from `a >= 1.6` on, a = 1 / (alpha |tan theta|): directions (x, 0, z), as bits, whose a IS the f32 1.6 in the
# identity frame, found by running the oracle's own lambda over the f32 neighbourhood of tan theta = 0.625 / alpha for the alphas of
# "plastic_raw" (0.15, two neighbours) and "metal_fuzz_0.5" (roughness_to_alpha(0.5)).  Without them a `>` in place of the `>=` computes
# the same bits on every other input of the sweep.
LAMBDA_THRESHOLD = [(0x3f78ee60, 0, 0x3e6ef952), (0x3f78ee60, 0, 0x3e6ef953), (0x3ef7ab11, 0, 0x3f600e59)]


@functools.lru_cache(None)
def local_directions(every=1):
    """(19 * 16 / every + 3, 3) f32 unit vectors, cos theta outermost, then LAMBDA_THRESHOLD; `every` thins the azimuths, never the
    cosines."""
    az = azimuths()[::every]
    rows = [(np.sqrt(max(1.0 - c * c, 0.0)) * x, np.sqrt(max(1.0 - c * c, 0.0)) * y, c) for c in COS_THETA for x, y in az]
    d = np.concatenate([np.array(rows, dtype=f64).astype(f32), np.array(LAMBDA_THRESHOLD, dtype=u32).view(f32)])
    assert np.isfinite(d).all() and (np.abs(d).max(axis=1) > 0).all()
    return d


def critical_cosines():
    """Local wo.z around every dielectric's critical angle, on the side the angle exists: inside (wo.z < 0) for ior > 1, where
    ior sin theta = 1; outside for ior < 1, where sin theta = ior.  The exact f32 cosine and 1, 2 and 8 ulps to each side."""
    out = []
    for ior in sorted(set(list(DIELECTRIC_IORS.values()) + [UBER_ETA])):
        i = float(f32(ior))
        if i == 1.0:
            continue
        c = f32(np.sqrt(1.0 - 1.0 / (i * i)) if i > 1.0 else np.sqrt(1.0 - i * i))
        bits = int(c.view(u32))
        sign = -1.0 if i > 1.0 else 1.0
        out += [sign * float(np.array(bits + k, dtype=u32).view(f32)) for k in (-8, -2, -1, 0, 1, 2, 8)]
    return out


@functools.lru_cache(None)
def sample_directions(every=1):
    """local_directions plus the critical-angle neighbourhoods on two azimuths (an axis and a diagonal)."""
    extra = [(np.sqrt(1.0 - c * c) * x, np.sqrt(1.0 - c * c) * y, c) for c in critical_cosines() for x, y in ((1.0, 0.0), (np.sqrt(0.5), -np.sqrt(0.5)))]
    return np.concatenate([local_directions(every), np.array(extra, dtype=f64).astype(f32)])


# ---- frames ----------------------------------------------------------------------------------------------------------------
def _rotation():
    a, b, c = 0.7, 1.1, -0.4
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
    return rz @ ry @ rx


# name -> (normal, tangent, the 3 x 3 matrix that takes a local direction to the world, length given to wo, to wi).  bsdf_new_frame
# normalises the normal and rebuilds the tangent, world_to_local normalises the direction: the lengths must not matter.
FRAMES = {
    "identity": (np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]), np.eye(3), 1.0, 1.0),
    "rotated_short_normal": (_rotation()[:, 2] * 1e-3, _rotation()[:, 0], _rotation(), 1.0, 1.0),
    "rotated_long_normal": (_rotation()[:, 2] * 1e3, _rotation()[:, 0] * 0.5, _rotation(), 3.0, 0.25),
    # the mirror image: the tangent of a left-handed parametrisation, which bsdf_new_frame answers with a frame turned about the normal
    "mirrored": (np.array([0.0, 0.0, 1.0]), np.array([-1.0, 0.0, 0.0]), np.diag([-1.0, -1.0, 1.0]), 1.0, 1.0),
}


def _rows(material, frame, wo_local, wi_local, u, v):
    """Queries for broadcastable local directions (n, 3) and random numbers (n,) in one frame."""
    normal, tangent, to_world, len_o, len_i = FRAMES[frame]
    n = max(len(wo_local), len(wi_local), len(u), len(v))
    q = np.zeros((n, QUERY_WORDS), dtype=f32)
    q[:, 1:4] = normal.astype(f32)
    q[:, 4:7] = tangent.astype(f32)
    q[:, 7:10] = ((wo_local.astype(f64) @ to_world.T) * len_o).astype(f32)
    q[:, 10:13] = ((wi_local.astype(f64) @ to_world.T) * len_i).astype(f32)
    q[:, 13], q[:, 14] = u, v
    w = q.view(u32)
    w[:, 0] = material
    return w


def u_values():
    base = [0.0, 2.0 ** -24, 2.0 ** -12, 0.25, 0.5 - 2.0 ** -25, 0.5, 0.5 + 2.0 ** -24, ONE_BELOW]
    edges = [float(np.nextafter(f32(k / n), f32(t))) for n in range(2, 6) for k in range(1, n) for t in (0.0, 1.0)]
    return np.unique(np.array(base + edges, dtype=f32))


def v_values():
    return np.array([0.0, 2.0 ** -24, 2.0 ** -12, 0.25, 0.5 - 2.0 ** -25, 0.5, 0.5 + 2.0 ** -24, ONE_BELOW], dtype=f32)


@functools.lru_cache(None)
def _pair_grid(every):
    d = local_directions(every)
    o, i = np.meshgrid(np.arange(len(d)), np.arange(len(d)), indexing="ij")
    zero = np.zeros(1, dtype=f32)
    return np.concatenate([_rows(0, fr, d[o.reshape(-1)], d[i.reshape(-1)], zero, zero) for fr in FRAMES])


def pair_queries(material, every=1):
    """eval and pdf: every direction as wo crossed with every direction as wi, in every frame."""
    q = _pair_grid(every).copy()
    q[:, 0] = material
    return q


@functools.lru_cache(None)
def _sample_grid(every):
    d, us, vs = sample_directions(every), u_values(), v_values()
    o, a, b = (x.reshape(-1) for x in np.meshgrid(np.arange(len(d)), np.arange(len(us)), np.arange(len(vs)), indexing="ij"))
    return np.concatenate([_rows(0, fr, d[o], d[o], us[a], vs[b]) for fr in FRAMES])


def sample_queries(material, every=1):
    """sample: every direction (and the critical-angle neighbourhoods) as wo, crossed with u and v, in every frame."""
    q = _sample_grid(every).copy()
    q[:, 0] = material
    return q


def specular_queries(material):
    d = sample_directions()
    zero = np.zeros(1, dtype=f32)
    return np.concatenate([_rows(material, fr, d, d, zero, zero) for fr in FRAMES])


def queries(material, op, every=1):
    if op in ("eval", "pdf"):
        return pair_queries(material, every)
    return sample_queries(material, every) if op == "sample" else specular_queries(material)


def frame_of(q):
    """Which frame each row of pair_queries / sample_queries / specular_queries is in, as an index into FRAMES."""
    return np.repeat(np.arange(len(FRAMES)), len(q) // len(FRAMES))


def degenerate_queries(material):
    """Kept apart from the grids: wo or wi the zero vector, a tangent parallel to the normal, a zero normal, an infinite or NaN
    component in a direction or in the frame.  Each against every cos theta on four azimuths and a few (u, v); one set for all ops."""
    d = local_directions(4)
    us, vs = u_values()[[0, 5, 9, -1]], v_values()[[0, 3, 5, 7]]
    o, a = (x.reshape(-1) for x in np.meshgrid(np.arange(len(d)), np.arange(4), indexing="ij"))
    base = _rows(material, "identity", d[o], d[o][::-1], us[a], vs[a])
    inf, nan = f32(np.inf).view(u32), f32(np.nan).view(u32)
    out = []

    def case(cols, words):
        q = base.copy()
        q[:, cols] = np.asarray(words, dtype=u32)
        out.append(q)
    case(slice(7, 10), [0, 0, 0])        # wo = 0
    case(slice(10, 13), [0, 0, 0])       # wi = 0
    case(slice(4, 7), base[0, 1:4])      # tangent parallel to the normal
    case(slice(1, 4), [0, 0, 0])         # normal = 0
    case(slice(7, 8), [inf])             # wo.x infinite
    case(slice(12, 13), [nan])           # wi.z NaN
    case(slice(3, 4), [inf])             # normal.z infinite
    case(slice(5, 6), [nan])             # tangent.y NaN
    return np.concatenate(out)


# ---- closed forms the tests share ------------------------------------------------------------------------------------------------
def hat(v):
    """math/src/vector.rs hat(): a * (1 / sqrt(x x + y y + z z)), f32 operation by operation."""
    v = np.asarray(v, dtype=f32)
    inv = f32(1.0) / np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    return v * inv[:, None]


def cos_sample_hemisphere(r0, r1):
    """bxdf.rs:187-206 in f32; pn_hypot and pn_sqrt from the oracle's build of the numeric header."""
    x, y = r0 * f32(2) - f32(1), r1 * f32(2) - f32(1)
    r = np.abs(np.where(np.abs(x) > np.abs(y), x, y))
    h = numeric_eval("hypot", x, y)
    with np.errstate(all="ignore"):
        dx, dy = r * (x / h), r * (y / h)
    centre = (x == 0) & (y == 0)
    dx, dy = np.where(centre, f32(0), dx).astype(f32), np.where(centre, f32(0), dy).astype(f32)
    z = numeric_eval("sqrt", np.maximum(f32(1) - dx * dx - dy * dy, f32(0)))
    return np.stack([dx, dy, z], axis=1)


def uber_five_lobe(q, r):
    """Which lobe of "uber_five" produced each sample of identity-frame queries q (results r): the transmission lobe of the opacity (0)
    is grey, kr (3) and kt (4) have colours of their own, and a mass's f is its lobe's colour times a number; of the two densities the
    Lambertian's (1) direction is cos_sample_hemisphere(v, fract(5 u)) and the microfacet's (2) is not.  -1: a black mass (total
    internal reflection of a transmission lobe), which carries no colour."""
    f, wi = r[:, :3].view(f32).astype(f64), r[:, 3:6].view(f32)
    is_mass = (r[:, 7] & FLAG_IS_MASS) != 0
    total = f.sum(axis=1)
    out = np.full(len(q), -1)
    with np.errstate(all="ignore"):
        chroma = f / total[:, None]
    for lobe, colour in ((0, (1, 1, 1)), (3, KR), (4, KT)):
        c = np.asarray(colour, dtype=f64) / sum(colour)
        out[is_mass & (total > 0) & (np.abs(chroma - c).max(axis=1) < 1e-5)] = lobe
    u, v = q.view(f32)[:, 13], q.view(f32)[:, 14]
    lambert = (wi == cos_sample_hemisphere(v, numeric_eval("fract", u * f32(5)))).all(axis=1)
    out[~is_mass] = np.where(lambert[~is_mass], 1, 2)
    return out
