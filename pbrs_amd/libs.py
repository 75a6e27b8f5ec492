"""The native libraries: libpbrs_host.so, libpbrs_gpu.so and the HIP runtime the latter is linked against.  Each exported function has
one entry in its library's table, (argtypes, restype); a loader sets them all, so a symbol the library lacks, or an entry the table
lacks, fails at load and not at the first call.  There is no CPU fallback: a missing library raises."""
import ctypes as C
import os

from .abi import Camera, SceneDesc
from .spec import SceneSpec

_LIBDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")


class PbrsError(RuntimeError):
    pass


P, U32, INT, STR = C.c_void_p, C.c_uint32, C.c_int, C.c_char_p


def _table(functions, with_device=()):
    """{symbol: argtypes, or (argtypes, restype)} -> {symbol: (argtypes, restype)}: the restype is ctypes' default, c_int, unless given;
    a symbol of `with_device` is entered again as symbol + "_device", which the header declares with the same signature."""
    full = {n: v if isinstance(v, tuple) else (v, INT) for n, v in {**functions, **dict(with_device)}.items()}
    return {**full, **{n + "_device": full[n] for n in with_device}}


GPU_FUNCTIONS = _table({
    "pbrs_create": [INT, C.POINTER(P)],
    "pbrs_destroy": [P],
    "pbrs_last_error": ([P], STR),
    "pbrs_set_stream": [P, P],
    "pbrs_set_pass_overlap": [P, INT],
    "pbrs_upload_scene": [P, P],
    "pbrs_collect_stats": [P, P],
    "pbrs_intersect_rays": [P, U32] + [P] * 5,
    "pbrs_last_intersect_info": [P, P],
    "pbrs_camera_rays": [P, P, P, U32, P, P],
    "pbrs_numeric_eval": [P, U32, U32, P, P, P],
    "pbrs_numeric_eval_k": [P, U32, U32, U32, P, P],
    "pbrs_bsdf_eval": [P, U32, U32, U32, P, P],
    "pbrs_render_sample_radiance": [P, P, P, U32, P],
    "pbrs_display_params_default": ([U32, U32, P], None),
    "pbrs_upsample_params_default": ([U32, U32, U32, P], None),
}, with_device={
    "pbrs_render_tile": [P] * 5,
    "pbrs_render_tile_aovs": [P] * 6,
    "pbrs_render_tile_filtered": [P] * 6,
    "pbrs_denoise": [P] * 5,
    "pbrs_render_tile_aovs_var": [P] * 7,
    "pbrs_denoise_var": [P] * 6,
    "pbrs_render_tile_matte": [P] * 9,
    "pbrs_matte_mask": [P, U32, U32, U32, P, P, P, U32, P],
    "pbrs_render_tile_passes": [P] * 10,
    "pbrs_combine_passes": [P, U32, U32, P, P, P],
    "pbrs_temporal_accumulate": [P] * 9,
    "pbrs_temporal_accumulate_motion": [P] * 10 + [U32],
    "pbrs_temporal_accumulate_clip": [P] * 10 + [U32, P],
    "pbrs_motion_vectors": [P, U32, U32] + [P] * 5 + [U32, P, P],
    "pbrs_spatial_variance": [P] * 7,
    "pbrs_display": [P] * 5,
    "pbrs_upsample": [P] * 7,
})
# The image comparison's entry points (include/pbrs_gpu.h, "image comparison"), in a table of their own: GPU_FUNCTIONS and GPU_SYMBOLS are
# the surface tests/golden/api_surface.json pins name for name.  gpu_lib() loads both tables, so a missing symbol fails at load here too.
GPU_COMPARE_FUNCTIONS = _table({
    "pbrsx_compare_params_default": ([U32, U32, P], None),
}, with_device={
    "pbrsx_compare": [P] * 6,
})
# The despeckle call's entry points (include/pbrs_gpu.h, "despeckle"), likewise in a table of their own, under the prefix pbrsi_.
GPU_DESPECKLE_FUNCTIONS = _table({
    "pbrsi_despeckle_params_default": ([U32, U32, P], None),
}, with_device={
    "pbrsi_despeckle": [P] * 4,
})
# The bloom call's entry points (include/pbrs_gpu.h, "bloom"), likewise, under the prefix pbrsb_.
GPU_BLOOM_FUNCTIONS = _table({
    "pbrsb_bloom_params_default": ([U32, U32, P], None),
}, with_device={
    "pbrsb_bloom": [P] * 4,
})
# The depth-of-field call's entry points (include/pbrs_gpu.h, "depth of field"), likewise, under the prefix pbrsf_.
GPU_DOF_FUNCTIONS = _table({
    "pbrsf_dof_params_default": ([U32, U32, P], None),
}, with_device={
    "pbrsf_dof": [P] * 6,
})
# The motion-blur call's entry points (include/pbrs_gpu.h, "motion blur"), likewise, under the prefix pbrsm_.
GPU_MOTION_BLUR_FUNCTIONS = _table({
    "pbrsm_motion_blur_params_default": ([U32, U32, P], None),
}, with_device={
    "pbrsm_motion_blur": [P] * 7,
})
# The entry nodes' switch and report (include/pbrs_gpu.h, "entry nodes of the camera rays"), likewise, under the prefix pbrse_.
GPU_ENTRY_FUNCTIONS = _table({
    "pbrse_set_entry_nodes": [P, INT],
    "pbrse_last_entry_info": [P, P],
})
HOST_FUNCTIONS = _table({
    "pbrs_host_scene_build": [P, C.POINTER(P)],
    "pbrs_host_scene_free": [P],
    "pbrs_host_scene_desc": ([P], C.POINTER(SceneDesc)),
    "pbrs_host_scene_camera": ([P], C.POINTER(Camera)),
    "pbrs_host_scene_stack_depth": ([P], U32),
    "pbrs_host_last_error": ([], STR),
    "pbrs_host_load_pbrt": [STR, C.POINTER(P)],
    "pbrs_loaded_scene_spec": ([P], C.POINTER(SceneSpec)),
    "pbrs_loaded_scene_free": [P],
    "pbrs_host_load_error": ([], STR),
    "pbrs_loaded_scene_filter": [P, P],
    "pbrs_host_write_exr": [STR, P, U32, U32],
    "pbrs_host_write_png": [STR, P, U32, U32],
    "pbrs_host_write_png_rgba8": [STR, P, U32, U32],
    "pbrs_host_io_error": ([], STR),
})
GPU_SYMBOLS, HOST_SYMBOLS = list(GPU_FUNCTIONS), list(HOST_FUNCTIONS)
GPU_COMPARE_SYMBOLS = list(GPU_COMPARE_FUNCTIONS)
GPU_DESPECKLE_SYMBOLS = list(GPU_DESPECKLE_FUNCTIONS)
GPU_BLOOM_SYMBOLS = list(GPU_BLOOM_FUNCTIONS)
GPU_DOF_SYMBOLS = list(GPU_DOF_FUNCTIONS)
GPU_MOTION_BLUR_SYMBOLS = list(GPU_MOTION_BLUR_FUNCTIONS)
GPU_ENTRY_SYMBOLS = list(GPU_ENTRY_FUNCTIONS)
_host = _gpu = _hip = None


def _load(path, functions):
    L = C.CDLL(path)
    for name, (argtypes, restype) in functions.items():
        fn = getattr(L, name)  # AttributeError: the library does not export it
        fn.argtypes, fn.restype = argtypes, restype
    return L


def lib_paths():
    return os.path.join(_LIBDIR, "libpbrs_host.so"), os.path.join(_LIBDIR, "libpbrs_gpu.so")


def host_lib():
    global _host
    if _host is None:
        # PBRS_HOST_LIB: the sanitizer build of the host library (tools/cpu_asan.sh: make -C pbrs_amd/csrc host-asan)
        path = os.environ.get("PBRS_HOST_LIB") or lib_paths()[0]
        if not os.path.exists(path):
            raise PbrsError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (make -C pbrs_amd/csrc)")
        _host = _load(path, HOST_FUNCTIONS)
    return _host


def gpu_lib():
    """Loads the HIP library. Raises (never falls back) when it is absent or cannot be loaded."""
    global _gpu
    if _gpu is None:
        # PBRS_GPU_LIB: developer override to A/B two builds of the HIP library in one session (tools/ablate.sh)
        path = os.environ.get("PBRS_GPU_LIB") or lib_paths()[1]
        if not os.path.exists(path):
            raise PbrsError(f"{path} is missing: the HIP extension must be built (make -C pbrs_amd/csrc); there is no CPU fallback")
        _gpu = _load(path, {**GPU_FUNCTIONS, **GPU_COMPARE_FUNCTIONS, **GPU_DESPECKLE_FUNCTIONS, **GPU_BLOOM_FUNCTIONS, **GPU_DOF_FUNCTIONS,
                            **GPU_MOTION_BLUR_FUNCTIONS, **GPU_ENTRY_FUNCTIONS})
    return _gpu


def hip_runtime():
    """The HIP runtime libpbrs_gpu.so is linked against (already loaded with it), for the device buffers of devmem.DeviceBuffers."""
    global _hip
    if _hip is None:
        gpu_lib()
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        _hip = _load(path, _table({"hipMalloc": [C.POINTER(P), C.c_size_t], "hipMemcpy": [P, P, C.c_size_t, INT], "hipFree": [P]}))
    return _hip
