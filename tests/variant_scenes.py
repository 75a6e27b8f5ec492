"""Scenes that reach every kernel the planner can name (pbrs_amd/csrc/host/kernel_choice.cpp): one generator over the axes that
prepare_scene turns into SceneFacts, and VARIANTS, the named points of that grid which tests/test_variant_census.py proves (on the CPU,
through tests/plan_probe.py) to cover every k_shade instantiation and every reachable traversal key, and which
tests/test_gpu_variants.py renders against the oracle.  Every entry of VARIANTS was picked by tools/search_variants.py, which walks the
grid with the probe; none by hand.

Axes of build():
  analytic      spheres, cuboids and disks among the objects (PBRS_FEAT_ANALYTIC); without them every object is a mesh
  mesh          None, "box" (objects of 12 triangles, a BLAS of three levels), "quad" (of two triangles: a BLAS of one leaf) or an int T:
                a floor of T triangles whose BLAS is a chain of T - 3 levels (areas fall by more than half from one triangle to the
                next, so the area-median split peels one off per level): 11 gives the four wide levels of PBRS_WIDE_MIN_LEVELS, 15 the
                twelve levels of PBRS_LONG_WALK_HEIGHT
  tangent_check the floor mesh's vertex normals are such that hits need the tangent check (PBRS_FEAT_SHADING_CHECK)
  quad          a ParallelQuad; next to a mesh it makes the closest-hit walks follow the extent (PBRS_FEAT_EXTENT)
  instances     objects on the grid in view (lights and the floor come on top)
  tlas_chain    further objects at geometrically growing distances: each adds a level to the TLAS
  tiny          a coordinate of 1e-30, outside the guarded range of the division-free box test (full steps)
  spare_mesh    T triangles of a chain mesh that no instance uses: its levels count for PBRS_LONG_WALK_HEIGHT, no walk enters it
  materials     "lambert", "mixed", "glossy", "one_glossy", "textured", "fourier", "fourier_mixed", "fourier_textured", or
                ("signatures", n, special, position): n different lobe signatures, `special` ("lambert", "fourier" or None) at the
                1-based `position` among them
  lights        a tuple out of "sphere", "triangle", "disk" (area lights), "point", "distant", "env"
  pad_triangles a strip mesh of that many triangles (k_shade's triangle records); pad_materials: further materials (its shading records)
  seed          jitter of the grid positions
"""
import functools
import math

import numpy as np

import fourier_scenes
from oracle.binding import OracleScene
from pbrs_amd import scenes
from pbrs_amd.spec import SceneBuilder, Transform, deg

DEFAULTS = dict(analytic=True, mesh=None, tangent_check=False, quad=False, instances=6, tlas_chain=0, tiny=False, spare_mesh=0, materials="lambert",
                lights=("sphere",), pad_triangles=0, pad_materials=0, seed=0, camera=(64, 48))

CHAIN_RATIO = 0.68  # side of a chain triangle over its predecessor's: areas fall to 0.46, the first of any tail holds more than half of its area


def chain_mesh(sb, n_triangles, first=6.0, tangent_check=False, tiny=False):
    """A floor strip along +x from x = -first / 2: triangle k has side first * CHAIN_RATIO^k and rises a little towards +x."""
    pos, nrm, uv, idx = [], [], [], []
    x, s = -0.5 * first, first
    for k in range(n_triangles):
        y0 = 1e-30 if (tiny and k == 1) else 0.0
        pos += [(x, y0, -0.5 * s), (x, 0.0, 0.5 * s), (x + s, 0.05 * s, 0.0)]
        # normals that lean against each other across a triangle: no bound on the tangent check holds (flatten.cpp, smooth_shading_bound)
        nrm += [(0.8, 0.6, 0.0), (-0.8, 0.6, 0.0), (0.0, 0.6, 0.8)] if tangent_check else [(0.0, 1.0, 0.0)] * 3
        uv += [(0, 0), (0, 1), (1, 0.5)]
        idx.append((3 * k, 3 * k + 1, 3 * k + 2))
        x, s = x + s, s * CHAIN_RATIO
    return sb.mesh(pos, nrm, uv, idx)


def strip_mesh(sb, n_triangles):
    """A zigzag strip of n triangles in a plane, one unit wide and n / 8 long."""
    pos = [((i // 2) * 0.25, 0.0, float(i % 2)) for i in range(n_triangles + 2)]
    idx = [(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(n_triangles)]
    return sb.mesh(pos, [(0.0, 1.0, 0.0)] * len(pos), [(p[0], p[2]) for p in pos], idx)


def signature_pool(sb):
    """Untextured materials of pairwise different lobe signatures, none of them Lambert's or Fourier's (flatten.cpp, flatten_material)."""
    pool = [lambda: sb.metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.2), 0.1), lambda: sb.glossy((0.7, 0.6, 0.5), 0.1), lambda: sb.mirror((0.9, 0.9, 0.9)),
            lambda: sb.plastic((0.2, 0.3, 0.7), (0.4, 0.4, 0.4), 0.1), lambda: sb.dielectric(1.5)]

    def uber(transmit, kd, ks, aniso, kr, kt):
        return lambda: sb.uber((0.5, 0.4, 0.3) if kd else (0, 0, 0), (0.3, 0.3, 0.3) if ks else (0, 0, 0), kr=(0.4, 0.4, 0.4) if kr else None,
                               kt=(0.3, 0.3, 0.3) if kt else None, rough=(0.1, 0.25 if aniso else 0.1), opacity=0.7 if transmit else 1.0)
    for bits in range(1, 32):
        transmit, kd, ks, kr, kt = (bits >> 4 & 1, bits & 1, bits >> 1 & 1, bits >> 2 & 1, bits >> 3 & 1)
        if (transmit, kd, ks, kr, kt) in ((0, 1, 0, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1)):
            continue  # one lobe that another material has: Lambert's, the dielectric's hybrid one, the transmission of opacity < 1
        pool.append(uber(transmit, kd, ks, False, kr, kt))
        if ks:
            pool.append(uber(transmit, kd, ks, True, kr, kt))
    return pool


def _materials(sb, kind):
    fourier = lambda: sb.fourier(sb.fourier_table(fourier_scenes.table("mono")))  # noqa: E731
    if isinstance(kind, tuple):
        _, n, special, position = kind
        pool = signature_pool(sb)
        mats = []
        for at in range(1, n + 1):
            if special and at == position:
                mats.append(sb.lambertian((0.6, 0.5, 0.4)) if special == "lambert" else fourier())
            else:
                mats.append(pool.pop(0)())
        return mats
    if kind == "lambert":
        return [sb.lambertian(c) for c in ((0.6, 0.6, 0.5), (0.7, 0.3, 0.2), (0.2, 0.5, 0.7))]
    if kind == "mixed":
        return [sb.lambertian((0.6, 0.6, 0.5)), sb.mirror((0.9, 0.9, 0.9)), sb.glossy((0.7, 0.6, 0.5), 0.1), sb.plastic((0.2, 0.3, 0.7), (0.4, 0.4, 0.4), 0.1),
                sb.lambertian((0.2, 0.5, 0.7))]
    if kind == "glossy":
        return [sb.glossy((0.7, 0.6, 0.5), 0.2), sb.mirror((0.9, 0.9, 0.9)), sb.metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.2), 0.1)]
    if kind == "one_glossy":
        return [sb.glossy((0.7, 0.6, 0.5), 0.2), sb.glossy((0.3, 0.6, 0.4), 0.05)]
    if kind == "textured":
        return [sb.lambertian(sb.checker((0.1, 0.1, 0.1), (0.8, 0.8, 0.8))), sb.lambertian((0.7, 0.3, 0.2)), sb.mirror((0.9, 0.9, 0.9)),
                sb.uber(sb.perlin(3.0, seed=3), (0.3, 0.3, 0.3))]
    if kind == "fourier":
        return [fourier(), fourier()]
    if kind == "fourier_mixed":
        return [sb.lambertian((0.6, 0.6, 0.5)), fourier(), sb.mirror((0.9, 0.9, 0.9))]
    if kind == "fourier_textured":
        return [sb.lambertian(sb.checker((0.1, 0.1, 0.1), (0.8, 0.8, 0.8))), fourier(), sb.glossy((0.7, 0.6, 0.5), 0.1)]
    raise ValueError(kind)


def build(**axes):
    a = dict(DEFAULTS, **axes)
    unknown = set(a) - set(DEFAULTS)
    assert not unknown, unknown
    assert a["analytic"] or a["mesh"] is not None, "a scene needs objects of some kind"
    sb = SceneBuilder()
    rs = np.random.RandomState(77 + a["seed"])
    mats = _materials(sb, a["materials"])
    for _ in range(a["pad_materials"]):
        sb.lambertian((0.5, 0.5, 0.5)) if a["materials"] in ("lambert", "mixed") else sb.glossy((0.5, 0.5, 0.5), 0.3)
    used = [0]

    def next_material():
        used[0] += 1
        return mats[(used[0] - 1) % len(mats)]

    # the floor
    chain = isinstance(a["mesh"], int)
    if chain:
        sb.instance(chain_mesh(sb, a["mesh"], tangent_check=a["tangent_check"], tiny=a["tiny"]), next_material(), Transform().translate((-1.0, 0.0, 1.0)))
    elif a["mesh"] in ("box", "quad"):
        floor = scenes.quad_mesh(sb, (-9, 0, -9), (9, 0, -9), (-9, 0, 9), (9, 0, 9), (0, 1, 0))
        if a["tangent_check"] or a["tiny"]:
            pos, nrm = sb.meshes[-1][0], sb.meshes[-1][1]
            if a["tangent_check"]:
                nrm[:] = [(0.8, 0.6, 0.0), (-0.8, 0.6, 0.0), (0.0, 0.6, 0.8), (0.0, 0.6, -0.8)]
            if a["tiny"]:
                pos[1, 1] = 1e-30
        sb.instance(floor, next_material())
    else:
        sb.instance(sb.disk((0, 1e-30 if a["tiny"] else 0.0, 0), (0, 1, 0), (12, 0, 0)), next_material())
    if a["spare_mesh"]:
        chain_mesh(sb, a["spare_mesh"])
    # the objects: shapes shared by kind, one instance per grid cell and per link of the TLAS chain
    n = a["instances"]
    cols = max(1, int(math.ceil(math.sqrt(1.5 * max(n, 1)))))
    pitch = min(1.7, 10.0 / cols)
    size = 0.3 * pitch
    shapes = {}

    def shape(kind):
        if kind not in shapes:
            shapes[kind] = sb.add_shape({"sphere": lambda: sb.sphere((0, 0, 0), size), "cuboid": lambda: sb.cuboid((-size, -size, -size), (size, size, size)),
                                         "disk": lambda: sb.disk((0, 0, 0), (0.0, 0.6, -0.8), (size, 0, 0)),
                                         "box": lambda: scenes.box_mesh(sb, (-size, -size, -size), (size, 1.2 * size, size)),
                                         "quad": lambda: scenes.quad_mesh(sb, (-size, -size, 0.3 * size), (size, -size, 0.3 * size), (-size, size, -0.3 * size),
                                                                          (size, size, -0.3 * size), (0.0, 0.2873479, 0.9578263))}[kind]())
        return shapes[kind]
    kinds = (["sphere", "cuboid", "disk"] if a["analytic"] else []) + (["quad" if a["mesh"] == "quad" else "box"] if a["mesh"] is not None else [])
    for i in range(n + a["tlas_chain"]):
        if i < n:
            c, r = i % cols, i // cols
            p = ((c - 0.5 * (cols - 1)) * pitch + rs.uniform(-0.1, 0.1) * pitch, size + 0.05 + rs.uniform(0.0, 0.5) * pitch, -1.5 + r * pitch + rs.uniform(-0.1, 0.1) * pitch)
        else:
            p = (20.0 * 2.2 ** (i - n), 0.5, 0.0)
        t = Transform().rotate_y(deg(rs.uniform(0, 360))) if i % 3 == 1 else Transform()
        sb.instance(shape(kinds[i % len(kinds)]), next_material(), t.translate(tuple(float(x) for x in p)))
    if a["quad"]:
        sb.instance(sb.quad((-3.0, 0.2, 5.5), (0.0, 2.5, 0.0), (2.5, 0.0, 0.3)), next_material())
    # lights: area lights are objects too where the scene has analytic shapes (an IsolatedTriangle is no analytic shape to the walks)
    for k, light in enumerate(a["lights"]):
        e = (9.0 + k, 8.0, 7.0)
        c = (-2.0 + 2.5 * k, 5.0, -1.0 + 0.7 * k)
        if light in ("sphere", "disk", "triangle"):
            s = {"sphere": lambda: sb.sphere(c, 0.6), "disk": lambda: sb.disk(c, (0, -1, 0), (0.8, 0, 0)),
                 "triangle": lambda: sb.triangle((c[0] + 1, c[1], c[2] + 1), (c[0] + 1, c[1], c[2] - 1), (c[0] - 1, c[1], c[2]))}[light]()
            if a["analytic"] or light == "triangle":
                sb.instance(s, sb.diffuse_light(e))
            sb.area_light(e, s)
        elif light == "point":
            sb.point_light((2.0, 5.0, -3.0), (40, 38, 36))
        elif light == "distant":
            sb.distant_light((0.2, -1.0, 0.3), (1.5, 1.4, 1.3), 15.0)
        elif light == "env":
            sb.env = (0.4, 0.5, 0.7)
        else:
            raise ValueError(light)
    if a["pad_triangles"]:
        sb.instance(strip_mesh(sb, a["pad_triangles"]), next_material(), Transform().rotate_x(deg(-60)).translate((-4.0, 0.3, 4.0)))
    sb.set_camera(a["camera"][0], a["camera"][1], deg(50), (0.5, 3.5, -8.0), (0.0, 0.5, 1.0))
    return sb


# How the scenes are rendered, on the CPU and on the GPU: (integrator, strata, depth) — the visualisers take one sample per pixel — and one seed
SEED = 5
RENDERS = (("path", (2, 2), 6), ("direct", (2, 2), 3), ("materials", (1, 1), 1), ("normals", (1, 1), 1))


@functools.lru_cache(maxsize=None)
def scene(name):
    return build(**VARIANTS[name])


@functools.lru_cache(maxsize=None)
def plan(name):
    """(facts, choice) of the plan probe for the scene: what pbrs_upload_scene finds out about it and which kernels it picks."""
    import pbrs_amd
    import plan_probe
    return plan_probe.probe(pbrs_amd.HostScene(scene(name)))


@functools.lru_cache(maxsize=None)
def reference(name):
    """{integrator: (image, stats)} of the oracle, computed once per process; do not write to the images."""
    osc = OracleScene(scene(name))
    return {integrator: osc.render(strata[0], strata[1], depth, SEED, integrator=integrator) for integrator, strata, depth in RENDERS}


# name -> the axes that differ from DEFAULTS; the pairs of scenes on either side of an LDS budget (tools/search_variants.py prints both)
VARIANTS = {
    'n55': {'instances': 55},
    'n56': {'instances': 56},
    'chain8_n92': {'tlas_chain': 8, 'instances': 92},
    'chain8_n93': {'tlas_chain': 8, 'instances': 93},
    'meshbox_n12_tri107': {'mesh': 'box', 'instances': 12, 'pad_triangles': 107},
    'meshbox_n12_tri108': {'mesh': 'box', 'instances': 12, 'pad_triangles': 108},
    'n100_tri40_mat14': {'instances': 100, 'pad_triangles': 40, 'pad_materials': 14},
    'n100_tri40_mat15': {'instances': 100, 'pad_triangles': 40, 'pad_materials': 15},
    'n18_sig14_fourier14': {'instances': 18, 'materials': ('signatures', 14, 'fourier', 14)},
    'n18_sig17_fourier15': {'instances': 18, 'materials': ('signatures', 17, 'fourier', 15)},
    'mesh11_tan_mixed_point+env': {'mesh': 11, 'tangent_check': True, 'materials': 'mixed', 'lights': ('point', 'env')},
    'noan_mesh11_textured': {'analytic': False, 'mesh': 11, 'materials': 'textured'},
    'mesh15_fourier_point+env': {'mesh': 15, 'materials': 'fourier', 'lights': ('point', 'env')},
    'noan_mesh15_fourier_textured': {'analytic': False, 'mesh': 15, 'materials': 'fourier_textured'},
    'meshquad_tiny_spare15_n100_mixed_triangle': {'mesh': 'quad', 'tiny': True, 'spare_mesh': 15, 'instances': 100, 'materials': 'mixed', 'lights': ('triangle',)},
    'noan_meshquad_triangle': {'analytic': False, 'mesh': 'quad', 'lights': ('triangle',)},
    'noan_mesh11_n100_sphere+disk+triangle+point': {'analytic': False, 'mesh': 11, 'instances': 100, 'lights': ('sphere', 'disk', 'triangle', 'point')},
    'noan_meshquad_tan_tiny_mixed': {'analytic': False, 'mesh': 'quad', 'tangent_check': True, 'tiny': True, 'materials': 'mixed'},
    'n18_sig15_lambert15': {'instances': 18, 'materials': ('signatures', 15, 'lambert', 15)},
    'spare15_one_glossy_point+env': {'spare_mesh': 15, 'materials': 'one_glossy', 'lights': ('point', 'env')},
    'tiny_spare15_point+env': {'tiny': True, 'spare_mesh': 15, 'lights': ('point', 'env')},
    'noan_meshquad_spare15': {'analytic': False, 'mesh': 'quad', 'spare_mesh': 15},
    'noan_meshquad_tiny_spare15': {'analytic': False, 'mesh': 'quad', 'tiny': True, 'spare_mesh': 15},
    'meshquad_tan_spare15_sphere+disk+triangle+point': {'mesh': 'quad', 'tangent_check': True, 'spare_mesh': 15, 'lights': ('sphere', 'disk', 'triangle', 'point')},
    'tiny_n36_point+env': {'tiny': True, 'instances': 36, 'lights': ('point', 'env')},
    'noan_meshbox_tan_spare15_triangle': {'analytic': False, 'mesh': 'box', 'tangent_check': True, 'spare_mesh': 15, 'lights': ('triangle',)},
    'noan_meshquad_n36': {'analytic': False, 'mesh': 'quad', 'instances': 36},
    'noan_meshquad_tiny_n36': {'analytic': False, 'mesh': 'quad', 'tiny': True, 'instances': 36},
    'noan_meshquad_n30_chain8': {'analytic': False, 'mesh': 'quad', 'instances': 30, 'tlas_chain': 8},
    'noan_meshquad_tiny_n30_chain8': {'analytic': False, 'mesh': 'quad', 'tiny': True, 'instances': 30, 'tlas_chain': 8},
    'meshbox_n36_point+env': {'mesh': 'box', 'instances': 36, 'lights': ('point', 'env')},
    'noan_meshbox_n36': {'analytic': False, 'mesh': 'box', 'instances': 36},
    'noan_meshquad_n60_triangle': {'analytic': False, 'mesh': 'quad', 'instances': 60, 'lights': ('triangle',)},
    'meshquad_tan_point+env': {'mesh': 'quad', 'tangent_check': True, 'lights': ('point', 'env')},
    'noan_meshquad_tan': {'analytic': False, 'mesh': 'quad', 'tangent_check': True},
    'meshquad_quad_point+env': {'mesh': 'quad', 'quad': True, 'lights': ('point', 'env')},
    'n18_sig14_lambert14': {'instances': 18, 'materials': ('signatures', 14, 'lambert', 14)},
    'meshquad_tan_spare15_point+env': {'mesh': 'quad', 'tangent_check': True, 'spare_mesh': 15, 'lights': ('point', 'env')},
    'meshquad_tan_tiny_spare15_point+env': {'mesh': 'quad', 'tangent_check': True, 'tiny': True, 'spare_mesh': 15, 'lights': ('point', 'env')},
    'noan_meshquad_tan_spare15': {'analytic': False, 'mesh': 'quad', 'tangent_check': True, 'spare_mesh': 15},
    'noan_meshquad_tan_tiny_spare15': {'analytic': False, 'mesh': 'quad', 'tangent_check': True, 'tiny': True, 'spare_mesh': 15},
    'meshquad_tan_n24_point+env': {'mesh': 'quad', 'tangent_check': True, 'instances': 24, 'lights': ('point', 'env')},
    'meshquad_tan_tiny_n24_point+env': {'mesh': 'quad', 'tangent_check': True, 'tiny': True, 'instances': 24, 'lights': ('point', 'env')},
    'noan_meshquad_tan_n24': {'analytic': False, 'mesh': 'quad', 'tangent_check': True, 'instances': 24},
    'noan_meshquad_tan_tiny_n24': {'analytic': False, 'mesh': 'quad', 'tangent_check': True, 'tiny': True, 'instances': 24},
    'meshquad_tan_n30_chain8_point+env': {'mesh': 'quad', 'tangent_check': True, 'instances': 30, 'tlas_chain': 8, 'lights': ('point', 'env')},
    'meshquad_tan_tiny_n30_chain8_point+env': {'mesh': 'quad', 'tangent_check': True, 'tiny': True, 'instances': 30, 'tlas_chain': 8, 'lights': ('point', 'env')},
    'noan_meshquad_tan_n30_chain8': {'analytic': False, 'mesh': 'quad', 'tangent_check': True, 'instances': 30, 'tlas_chain': 8},
    'noan_meshquad_tan_tiny_n30_chain8': {'analytic': False, 'mesh': 'quad', 'tangent_check': True, 'tiny': True, 'instances': 30, 'tlas_chain': 8},
    'meshquad_tan_spare15_n24_point+env': {'mesh': 'quad', 'tangent_check': True, 'spare_mesh': 15, 'instances': 24, 'lights': ('point', 'env')},
    'noan_meshquad_tan_spare15_n24': {'analytic': False, 'mesh': 'quad', 'tangent_check': True, 'spare_mesh': 15, 'instances': 24},
    'meshbox_tan_n36_point+env': {'mesh': 'box', 'tangent_check': True, 'instances': 36, 'lights': ('point', 'env')},
    'noan_meshbox_tan_n36': {'analytic': False, 'mesh': 'box', 'tangent_check': True, 'instances': 36},
    'meshquad_tan_n60': {'mesh': 'quad', 'tangent_check': True, 'instances': 60},
    'noan_meshquad_tan_n60_triangle': {'analytic': False, 'mesh': 'quad', 'tangent_check': True, 'instances': 60, 'lights': ('triangle',)},
    'n130_triangle': {'instances': 130, 'lights': ('triangle',)},
    'n130_sphere+disk': {'instances': 130, 'lights': ('sphere', 'disk')},
}
BOUNDARY_PAIRS = {
    'scene': ('n55', 'n56'),
    'top': ('chain8_n92', 'chain8_n93'),
    'shade_all': ('meshbox_n12_tri107', 'meshbox_n12_tri108'),
    'shade_records': ('n100_tri40_mat14', 'n100_tri40_mat15'),
}
