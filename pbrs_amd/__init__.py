"""pbrs_amd — MI355X-native wavefront path tracer behind the pbrs integrator seam.

Only the path-integrator hot path of plumer/pbrs: the HIP kernels + C ABI
(csrc/, include/pbrs_gpu.h), the host-side scene flattener (csrc/host, include/pbrs_host.h),
their ctypes mirrors (abi.py), loaders (libs.py) and driver (api.py, device buffers in devmem.py),
and the synthetic scene generators (scenes.py).
"""
from .api import BloomParams, CompareParams, CompareResult, Context, DenoiseGuides, DenoiseParams, DenoiseVarGuides, DenoiseVarParams, DespeckleParams, DespeckleResult, DeviceBuffers, DisplayParams, DofParams, HistoryClipParams, HostScene, LoadedScene, MatteBuffers, MatteParams, MotionBlurParams, PassBuffers, PbrsError, PixelFilter, SpatialVarianceParams, UpsampleParams, gpu_lib, host_lib, lens, lib_paths, load_pbrt, scaled_camera, write_image, write_image_u8  # noqa: F401
from . import scenes, spec  # noqa: F401
