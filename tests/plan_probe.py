"""What pbrs_upload_scene plans for a scene, asked on the CPU: tests/plan_probe.cpp, compiled with the library's own host/scene_prepare.cpp
and host/kernel_choice.cpp (plain g++, no sanitizer: the code is loaded into python) into a temporary directory, once per process.  It is
the planner's own source under default DevOverrides, so what it reports is what bind_kernels looks up."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pbrs_amd", "csrc", "host")
SOURCES = [os.path.join(ROOT, "tests", "plan_probe.cpp"), os.path.join(HOST, "scene_prepare.cpp"), os.path.join(HOST, "kernel_choice.cpp")]

# PBRS_FEAT_* and the k_shade template arguments (pbrs_amd/csrc/device/scene.h)
ANALYTIC, SHADING_CHECK, FLAT_TLAS, LONG_WALKS, WIDE, FULL_STEPS, LDS_SCENE, LDS_TOP, EXTENT = 1, 2, 4, 8, 16, 32, 64, 128, 256
SHADE_LAMBERT, SHADE_LIGHT_SPHERE, SHADE_LIGHT_TRIANGLE, SHADE_FOURIER, SHADE_FOURIER_ONLY, SHADE_LDS_RECORDS, SHADE_LDS_TRIS = 1, 2, 4, 8, 16, 32, 64
SHADE_LDS_ALL = SHADE_LDS_RECORDS | SHADE_LDS_TRIS
SHADE_FOURIER_ALONE = SHADE_FOURIER | SHADE_FOURIER_ONLY
MAX_CLASSES = 16
LDS_BYTES_PER_CU = 160 * 1024
SCENE_BUDGET, TOP_BUDGET, SHADE_BUDGET = LDS_BYTES_PER_CU // 8, LDS_BYTES_PER_CU // 7, 16 << 10  # stack + scene; stack + top + 512; records (+ triangles)
INTEGRATORS = ("path", "direct", "materials", "normals")
TABLES = ("extend", "shadow", "shadow_slow")

# plan_probe_scene's `facts`: SceneFacts in declaration order, then the levels and the signature census of the probe itself
FACTS = ("features", "tlas_scanned", "exact_extent", "long_walks", "full_steps", "wide_ok", "stack_bytes", "wide_stack_bytes", "scene_bytes", "top_bytes",
         "n_classes", "lambert_class", "fourier_class", "textured", "fourier", "lambert", "light_spec", "shade_lds", "shade_rec_bytes", "shade_tri_bytes",
         "tlas_levels", "blas_levels", "stack_levels", "wide_levels", "n_signatures", "lambert_position", "fourier_position", "overflow_signatures",
         "max_instance_class", "n_instances", "n_triangles", "n_materials")


@functools.lru_cache(maxsize=None)
def lib():
    with tempfile.TemporaryDirectory(prefix="pbrs_plan_probe_") as tmp:  # (the loaded library outlives its file)
        out = os.path.join(tmp, "libplan_probe.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-shared", "-fPIC", "-o", out] + SOURCES)
        L = C.CDLL(out)
    L.plan_probe_scene.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.plan_probe_scene.restype = C.c_int
    for fn in (L.plan_probe_shade_keys, L.plan_probe_reachable):
        fn.argtypes = [C.POINTER(C.c_uint32), C.c_uint32]
        fn.restype = C.c_uint32
    return L


def probe(host_scene):
    """-> (facts, choice) of a pbrs_amd.HostScene.  facts: dict over FACTS.  choice: extend / extend_stats / shadow / shadow_stats / shadow_slow
    as (key, lds bytes), wide_shadow, split_queue, lds_staging, and per integrator name a dict order / last_class / shade, the latter a list of
    (integrator, textured, spec, lds bytes, range)."""
    facts, words = (C.c_uint64 * 32)(), (C.c_uint64 * 80)()
    rc = lib().plan_probe_scene(C.addressof(host_scene.desc), facts, words)
    if rc != 0:
        raise ValueError(f"check_scene refuses the scene ({rc})")
    w = [int(x) for x in words]
    choice = {name: (w[2 * i], w[2 * i + 1]) for i, name in enumerate(("extend", "extend_stats", "shadow", "shadow_stats", "shadow_slow"))}
    choice["wide_shadow"], choice["split_queue"], choice["lds_staging"] = bool(w[10]), bool(w[11]), w[12]
    for i, name in enumerate(INTEGRATORS):
        o = 13 + 13 * i
        choice[name] = {"order": w[o], "last_class": w[o + 1],
                        "shade": [(w[o + 3 + 5 * k], bool(w[o + 4 + 5 * k]), w[o + 5 + 5 * k], w[o + 6 + 5 * k], w[o + 7 + 5 * k]) for k in range(w[o + 2])]}
    return dict(zip(FACTS, (int(x) for x in facts))), choice


@functools.lru_cache(maxsize=None)
def shade_keys():
    """The k_shade instantiations of PBRS_SHADE_KERNELS: (integrator index, textured, spec)."""
    buf = (C.c_uint32 * (3 * 64))()
    n = lib().plan_probe_shade_keys(buf, 64)
    assert n <= 64
    return tuple((int(buf[3 * i]), bool(buf[3 * i + 1]), int(buf[3 * i + 2])) for i in range(n))


@functools.lru_cache(maxsize=None)
def reachable_keys():
    """The traversal keys choose_kernels yields over the producible fact combinations (tests/kernel_choice_sweep.h): (table name, key)."""
    buf = (C.c_uint32 * (2 * 256))()
    n = lib().plan_probe_reachable(buf, 256)
    assert n <= 256
    return tuple((TABLES[buf[2 * i]], int(buf[2 * i + 1])) for i in range(n))


def planned_keys(choice):
    """The traversal keys of a choice, as reachable_keys names them."""
    keys = {("extend", choice["extend"][0]), ("shadow", choice["shadow"][0])}
    if choice["wide_shadow"]:
        keys.add(("shadow_slow", choice["shadow_slow"][0]))
    return keys


def feature_names(key):
    names = ("ANALYTIC", "SHADING_CHECK", "FLAT_TLAS", "LONG_WALKS", "WIDE", "FULL_STEPS", "LDS_SCENE", "LDS_TOP", "EXTENT")
    return "|".join(n for i, n in enumerate(names) if key >> i & 1) or "0"


def shade_name(key):
    integ, tex, spec = key
    names = ("LAMBERT", "LIGHT_SPHERE", "LIGHT_TRIANGLE", "FOURIER", "FOURIER_ONLY", "LDS_RECORDS", "LDS_TRIS")
    return f"({INTEGRATORS[integ].upper()}, {str(tex).lower()}, {'|'.join(n for i, n in enumerate(names) if spec >> i & 1) or '0'})"
