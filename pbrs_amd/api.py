"""ctypes bindings of the product path: libpbrs_host.so (include/pbrs_host.h) and libpbrs_gpu.so
(include/pbrs_gpu.h).

`HostScene` mirrors the reference's `Scene::new(*tlas::build_bvh(instances), camera)
.with_lights(..)` (scene/src/lib.rs:36-63, :118-126); `Context.render` replaces the frame loop of
src/main.rs:192-231 for one tile.  There is no CPU fallback: if the HIP library is missing or the
device call fails, these raise.
"""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np

from .abi import (AOV_NAMES, AOVS, BSDF_OPS, BSDF_QUERY_WORDS, BSDF_RESULT_WORDS, DENOISE_GUIDES, HIT_DTYPE, INTEGRATORS, MATTE_LAYERS, NUMERIC_FNS, NUMERIC_K_FNS, PASS_CHANNELS, PASSES,  # noqa: F401
                  SPATIAL_VARIANCE_PLANES, TEMPORAL_FRAME, TEMPORAL_GUIDES, TEMPORAL_HISTORY, VARIANCE, AovBuffers, BloomParams, Camera, CompareMaps, CompareParams, CompareResult,
                  DenoiseGuides, DenoiseParams, DespeckleIO, DespeckleParams, DespeckleResult, DofParams,
                  DenoiseVarGuides, DenoiseVarParams, DisplayIO, DisplayParams, HistoryClipParams, InstanceMotion, MatteBuffers, MatteParams, MotionBlurParams, Node, PassBuffers,
                  PixelFilter, RenderParams, SceneDesc, SpatialVarianceGuides, SpatialVarianceParams, Stats, TemporalFrame, TemporalGuides, TemporalHistory,
                  TemporalParams, UpsampleParams, _aov_names, _bloom_params, _DenoiseParamsMixin, _despeckle_params, _display_params, _dof_params, _history_clip, _matte_select, _motion_args, _motion_blur_params, _pass_names,
                  _reference_frame, _reference_frames, _temporal_struct, _upscale_params, lens, scaled_camera)
from .devmem import DeviceBuffers
from .libs import GPU_BLOOM_SYMBOLS, GPU_COMPARE_SYMBOLS, GPU_DESPECKLE_SYMBOLS, GPU_DOF_SYMBOLS, GPU_ENTRY_SYMBOLS, GPU_MOTION_BLUR_SYMBOLS, GPU_SYMBOLS, HOST_SYMBOLS, PbrsError, gpu_lib, hip_runtime, host_lib, lib_paths  # noqa: F401
from .spec import SceneSpec  # noqa: F401


def orbited(camera, about, axis, degrees):
    """`camera` (a Camera) turned by `degrees` about the line through the point `about` along `axis`: a frame of a turntable or of an
    orbit about the look-at point -> a new Camera of the same film."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    t = np.radians(degrees)

    def rot(v):
        return v * np.cos(t) + np.cross(k, v) * np.sin(t) + k * np.dot(k, v) * (1.0 - np.cos(t))
    about = np.asarray(about, dtype=np.float64)
    out = Camera()
    out.width, out.height = camera.width, camera.height
    out.center[:] = [float(v) for v in about + rot(np.array(list(camera.center), dtype=np.float64) - about)]
    for n in ("c", "a", "b"):
        getattr(out, n)[:] = [float(v) for v in rot(np.array(list(getattr(camera, n)), dtype=np.float64))]
    return out


def instance_motion(scene, scene_prev):
    """The motion table (a ctypes array of InstanceMotion, one per instance) that carries a surface point of `scene` to where it was in
    `scene_prev`, two HostScenes of the same instances in the same order: m = fwd_prev . inv_cur and n = transpose(lin(fwd_cur) .
    lin(inv_prev)) (the inverse transpose of m's linear part), computed in float64 from the scenes' f32 records and rounded once.  An
    instance whose fwd and inv are bitwise equal in both scenes is flagged IDENTITY."""
    fwd, inv = scene.instance_transforms()
    fwd_p, inv_p = scene_prev.instance_transforms()
    if len(fwd) != len(fwd_p):
        raise ValueError(f"instance_motion: {len(fwd)} instances beside {len(fwd_p)} in the previous scene")
    table = (InstanceMotion * max(len(fwd), 1))()
    bottom = np.array([[0.0, 0.0, 0.0, 1.0]])
    for i in range(len(fwd)):
        r = table[i]
        if fwd[i].tobytes() == fwd_p[i].tobytes() and inv[i].tobytes() == inv_p[i].tobytes():
            m, n, r.flags = np.eye(3, 4), np.eye(3), InstanceMotion.IDENTITY
        else:
            m = (np.vstack([fwd_p[i].astype(np.float64), bottom]) @ np.vstack([inv[i].astype(np.float64), bottom]))[:3]
            n = (fwd[i, :, :3].astype(np.float64) @ inv_p[i, :, :3].astype(np.float64)).T
        for a in range(3):
            r.m[a][:] = [float(v) for v in m[a].astype(np.float32)]
            r.n[a][:] = [float(v) for v in n[a].astype(np.float32)]
    return table


def _guide_bytes(guides, w, h, suffix=""):
    """{guide + suffix: bytes of its w x h plane}."""
    return {n + suffix: DENOISE_GUIDES[n][0] * w * h * 4 for n in guides}


def _sequence_buffers(w, h, fw, fh, guides, motion_vectors, upscale, display, reference=False, despeckle=False, bloom=False, dof=False,
                      motion_blur=False):
    """{name: bytes} of the device buffers of a frame sequence (Context._temporal_frames) that runs at w x h and shows fw x fh: the
    frame's image, the filtered one, the two variances; two ping-pong halves ("0", "1") of the guides the next frame is tested against
    and of the history; the other guides once; and what each option that is on adds."""
    kept = [n for n in TEMPORAL_GUIDES if n in guides]
    sizes = {"rgb": 3 * w * h * 4, "out": 3 * w * h * 4, VARIANCE: w * h * 4, "acc_variance": w * h * 4}
    for k in ("0", "1"):
        sizes.update(_guide_bytes(kept, w, h, k))
        sizes.update({f"h_{n}{k}": ch * w * h * 4 for n, (ch, _) in TEMPORAL_HISTORY.items()})
    sizes.update(_guide_bytes([n for n in guides if n not in kept], w, h))
    if motion_vectors:
        sizes["motion"], sizes["prev_depth"] = 2 * w * h * 4, w * h * 4
    if upscale:
        sizes["up"] = 3 * fw * fh * 4
        sizes.update(_guide_bytes(guides, fw, fh, "_hi"))
    if display:
        sizes["display"], sizes["exposure"] = fw * fh * 4, 4
    if reference:
        sizes["reference"], sizes["compare"] = 3 * fw * fh * 4, C.sizeof(CompareResult)
    if despeckle:
        sizes["despeckled"], sizes["despeckle"] = 3 * w * h * 4, C.sizeof(DespeckleResult)
    if bloom:
        sizes["bloom"] = 3 * fw * fh * 4
    if dof:
        sizes["dof"] = 3 * fw * fh * 4
    if motion_blur:
        sizes["mblur"] = 3 * fw * fh * 4
        if upscale or not motion_vectors:  # the step needs vectors of the full size: the "motion" buffer is the chain's, at its size
            sizes["mblur_motion"] = 2 * fw * fh * 4
    return sizes


class LoadedScene:
    """A scene read from a pbrt-v3 file by the host library (include/pbrs_host.h, pbrs_host_load_pbrt).  Stands where a
    SceneBuilder stands: `build()` returns the scene spec, so HostScene(...) and the oracle take it as they take a builder."""

    def __init__(self, path):
        h = C.c_void_p()
        rc = host_lib().pbrs_host_load_pbrt(os.fsencode(path), C.byref(h))
        if rc != 0:
            raise PbrsError(f"pbrs_host_load_pbrt({path}) failed ({rc}): {host_lib().pbrs_host_load_error().decode()}")
        self._h = h
        self.spec = host_lib().pbrs_loaded_scene_spec(h).contents

    def build(self):
        return self.spec

    def pixel_filter(self):
        """The file's `Filter` as a PixelFilter (pbrs_loaded_scene_filter: parse_filter's defaults; none: box 0.5)."""
        f = PixelFilter()
        rc = host_lib().pbrs_loaded_scene_filter(self._h, C.byref(f))
        if rc != 0:
            raise PbrsError(f"pbrs_loaded_scene_filter failed ({rc}): {host_lib().pbrs_host_load_error().decode()}")
        return f

    def close(self):
        if getattr(self, "_h", None):
            host_lib().pbrs_loaded_scene_free(self._h)
            self._h = None

    def __del__(self):
        self.close()


def load_pbrt(path):
    return LoadedScene(path)


def write_image(path, rgb):
    """`write_exr` (path ending in .exr: f32 RGB) or `write_image` (.png: 8-bit, sqrt-gamma) of src/main.rs:28-53 for an
    (h, w, 3) radiance array."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w, _ = rgb.shape
    fn = host_lib().pbrs_host_write_exr if str(path).lower().endswith(".exr") else host_lib().pbrs_host_write_png
    rc = fn(os.fsencode(path), rgb.ctypes.data, w, h)
    if rc != 0:
        raise PbrsError(f"writing {path} failed ({rc}): {host_lib().pbrs_host_io_error().decode()}")


def write_image_u8(path, rgba8):
    """The 8-bit PNG of an (h, w, 4) or (h, w, 3) uint8 image that is display-ready already (Context.display): the bytes go into the
    file as they are, alpha is dropped."""
    img = np.asarray(rgba8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in (3, 4):
        raise ValueError(f"an 8-bit image is (h, w, 4) or (h, w, 3) uint8, not {img.dtype} {img.shape}")
    h, w, ch = img.shape
    if ch == 3:
        img = np.concatenate([img, np.full((h, w, 1), 255, dtype=np.uint8)], axis=2)
    words = np.ascontiguousarray(img).view("<u4")
    rc = host_lib().pbrs_host_write_png_rgba8(os.fsencode(path), words.ctypes.data, w, h)
    if rc != 0:
        raise PbrsError(f"writing {path} failed ({rc}): {host_lib().pbrs_host_io_error().decode()}")


class HostScene:
    """Flattened scene: TLAS/BLAS built with the reference's algorithms, linearised for HBM."""

    def __init__(self, scene_builder):
        self._sb = scene_builder
        self._spec = scene_builder.build()
        h = C.c_void_p()
        rc = host_lib().pbrs_host_scene_build(C.addressof(self._spec), C.byref(h))
        if rc != 0:
            raise PbrsError(f"pbrs_host_scene_build failed ({rc}): {host_lib().pbrs_host_last_error().decode()}")
        self._h = h
        self.desc = host_lib().pbrs_host_scene_desc(h).contents
        self.camera = host_lib().pbrs_host_scene_camera(h).contents
        self.width, self.height = self.camera.width, self.camera.height

    @property
    def stack_depth(self):
        return host_lib().pbrs_host_scene_stack_depth(self._h)

    @property
    def nbytes(self):
        """Bytes of the flattened scene as it sits in HBM (record sizes of include/pbrs_gpu.h)."""
        d = self.desc
        return (32 * (d.n_tlas_nodes + d.n_blas_nodes) + 128 * d.n_instances + 48 * d.n_shapes + 32 * d.n_meshes +
                (48 + 64) * d.n_triangles + 32 * d.n_materials + 64 * d.n_bxdfs + 64 * d.n_area_lights + 32 * d.n_delta_lights +
                48 * d.n_textures + 4 * (d.n_tex_floats + d.n_tex_words) + 48 * d.n_fourier_tables)

    def instance_transforms(self):
        """(fwd, inv): the instances' object-to-world and world-to-object transforms as (n, 3, 4) f32 arrays, rows of the affine
        matrices as pbrs_instance holds them, in the order of the scene spec (the `instance` AOV indexes them)."""
        n = self.desc.n_instances
        if n == 0 or not self.desc.instances:
            return np.zeros((0, 3, 4), dtype=np.float32), np.zeros((0, 3, 4), dtype=np.float32)
        rec = np.ctypeslib.as_array(C.cast(self.desc.instances, C.POINTER(C.c_float)), shape=(n, 32))  # pbrs_instance: 128 B, inv then fwd
        return rec[:, 12:24].reshape(n, 3, 4).copy(), rec[:, :12].reshape(n, 3, 4).copy()

    def nodes(self, which="tlas"):
        n, p = (self.desc.n_tlas_nodes, self.desc.tlas_nodes) if which == "tlas" else (self.desc.n_blas_nodes, self.desc.blas_nodes)
        if n == 0 or not p:
            return np.zeros((0, 8), dtype=np.uint32)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n, 8)).copy()

    def close(self):
        if getattr(self, "_h", None):
            host_lib().pbrs_host_scene_free(self._h)
            self._h = None

    def __del__(self):
        self.close()


class Context:
    """One per GPU (the per-thread state of the reference's rayon row loop, src/main.rs:219-224)."""

    def __init__(self, device=0):
        self._L = gpu_lib()
        h = C.c_void_p()
        rc = self._L.pbrs_create(device, C.byref(h))
        if rc != 0:
            raise PbrsError(f"pbrs_create(device={device}) failed ({rc}): no usable HIP device; there is no CPU fallback")
        self._h = h
        self.scene = None

    def _check(self, rc, what):
        if rc != 0:
            raise PbrsError(f"{what} failed ({rc}): {self._L.pbrs_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None):
            self._L.pbrs_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def set_stream(self, hip_stream_ptr):
        self._check(self._L.pbrs_set_stream(self._h, C.c_void_p(hip_stream_ptr)), "pbrs_set_stream")

    def set_pass_overlap(self, enabled):
        """Late bounces of a pass beside the next pass's first bounces, on a second stream (default on; include/pbrs_gpu.h)."""
        self._check(self._L.pbrs_set_pass_overlap(self._h, int(bool(enabled))), "pbrs_set_pass_overlap")

    def set_entry_nodes(self, enabled):
        """Camera rays enter the scene's deep mesh at per-pixel entry nodes instead of at its root (default on; include/pbrs_gpu.h)."""
        self._check(self._L.pbrse_set_entry_nodes(self._h, int(bool(enabled))), "pbrse_set_entry_nodes")

    def last_entry_info(self):
        """What the entry-node pre-pass of the last render found (include/pbrs_gpu.h, pbrs_entry_info); waits for that render."""
        v = (C.c_uint32 * 4)()
        self._check(self._L.pbrse_last_entry_info(self._h, C.addressof(v)), "pbrse_last_entry_info")
        return {"pixels_with_entries": int(v[0]), "pixels_empty": int(v[1]), "pixels_from_root": int(v[2]), "entries": int(v[3])}

    def upload(self, host_scene):
        self._check(self._L.pbrs_upload_scene(self._h, C.addressof(host_scene.desc)), "pbrs_upload_scene")
        self.scene = host_scene

    def _params(self, strata_x, strata_y, depth, seed, tile, samples_per_pass=0, counters=False, timing=False, bands=None,
                integrator="path"):
        x0, y0, w, h = tile or (0, 0, self.scene.width, self.scene.height)
        p = RenderParams()
        if bands:
            p.band_rows, p.band_count, p.band_index = bands
        p.x0, p.y0, p.w, p.h = x0, y0, w, h
        p.strata_x, p.strata_y, p.max_depth, p.samples_per_pass = strata_x, strata_y, depth, samples_per_pass
        p.seed, p.collect_counters, p.time_stages = seed, int(counters), int(timing)
        p.integrator = INTEGRATORS[integrator]
        return p

    def render(self, strata_x, strata_y, depth, seed, tile=None, samples_per_pass=0, counters=False, timing=False, bands=None,
               integrator="path"):
        """-> (h, w, 3) f32 radiance, stats dict.  Host output (one D2H copy at the end).
        bands = (band_rows, band_count, band_index): the tile's rows are interleaved row bands.
        integrator: "path" (src/pathintegrator.rs) or "direct" (direct_lighting_integrator, src/directlighting.rs:14-47)."""
        p = self._params(strata_x, strata_y, depth, seed, tile, samples_per_pass, counters, timing, bands, integrator)
        out = np.empty((p.h, p.w, 3), dtype=np.float32)
        st = Stats()
        self._check(self._L.pbrs_render_tile(self._h, C.addressof(self.scene.camera), C.addressof(p), out.ctypes.data, C.addressof(st)),
                    "pbrs_render_tile")
        return out, st.as_dict()

    def render_device(self, rgb_device_ptr, strata_x, strata_y, depth, seed, tile=None, samples_per_pass=0, counters=False,
                      timing=False, bands=None, integrator="path"):
        """Asynchronous: the result lands in caller-owned device memory on the context's own NON-BLOCKING stream.  It is valid
        after `collect_stats()` (which waits for that stream), not merely after work queued later on torch's or the default
        stream: those are not ordered against it (include/pbrs_gpu.h, "Stream ordering")."""
        p = self._params(strata_x, strata_y, depth, seed, tile, samples_per_pass, counters, timing, bands, integrator)
        self._check(self._L.pbrs_render_tile_device(self._h, C.addressof(self.scene.camera), C.addressof(p), C.c_void_p(rgb_device_ptr), None),
                    "pbrs_render_tile_device")

    @staticmethod
    def _aov_arrays(names, p):
        """The host arrays of the AOVs named ("variance" among them) for the tile of `p`, and the AovBuffers that points at them."""
        bufs, arrays = AovBuffers(), {}
        for n in names:
            ch, dt = AOVS.get(n, (1, np.float32))
            arrays[n] = np.empty((p.h, p.w, ch) if ch > 1 else (p.h, p.w), dtype=dt)
            if n != VARIANCE:
                setattr(bufs, n, arrays[n].ctypes.data)
        return bufs, arrays

    @staticmethod
    def _aov_device(aov_device_ptrs):
        """{name: device pointer} -> the AovBuffers of the first-hit AOVs and the pointer of "variance" (None: not asked for)."""
        ptrs = dict(aov_device_ptrs or {})
        _aov_names(ptrs)
        variance = ptrs.pop(VARIANCE, None)
        bufs = AovBuffers()
        for n, ptr in ptrs.items():
            setattr(bufs, n, ptr)
        return bufs, variance

    def _render_host(self, p, names, mp=None, mb=None, pb=None, camera=None):
        """A host render of `p` with the AOVs named and, with `mp` and `mb`, a matte, with `pb`, light passes -> (rgb, {name: array},
        stats).  One entry point serves all of them: the library forwards the AOV and matte ones to it."""
        out = np.empty((p.h, p.w, 3), dtype=np.float32)
        bufs, arrays = self._aov_arrays(names, p)
        st = Stats()
        self._check(self._L.pbrs_render_tile_passes(self._h, C.addressof(camera or self.scene.camera), C.addressof(p), out.ctypes.data, C.addressof(bufs),
                                                    arrays[VARIANCE].ctypes.data if VARIANCE in names else None, C.addressof(mp) if mp else None,
                                                    C.addressof(mb) if mb else None, C.addressof(pb) if pb else None, C.addressof(st)),
                    "pbrs_render_tile_passes")
        return out, arrays, st.as_dict()

    def _render_device(self, p, rgb_device_ptr, bufs, variance, mp=None, mb=None, pb=None, camera=None):
        """`camera`: a Camera in the place of the scene's own (render_temporal's moving camera)."""
        self._check(self._L.pbrs_render_tile_passes_device(self._h, C.addressof(camera or self.scene.camera), C.addressof(p), C.c_void_p(rgb_device_ptr),
                                                           C.addressof(bufs), C.c_void_p(variance), C.addressof(mp) if mp else None,
                                                           C.addressof(mb) if mb else None, C.addressof(pb) if pb else None, None),
                    "pbrs_render_tile_passes_device")

    def render_aovs(self, strata_x, strata_y, depth, seed, aovs=AOV_NAMES, tile=None, samples_per_pass=0, counters=False,
                    timing=False, bands=None, integrator="path", camera=None):
        """render() plus first-hit AOVs of the same camera samples (include/pbrs_gpu.h, pbrs_aov_buffers) -> (rgb, {name: array},
        stats).  albedo / normal: (h, w, 3) f32; coverage / depth: (h, w) f32; instance / material / prim: (h, w) u32.  The name
        "variance" (not in the default) adds the variance of the pixel's mean luminance, (h, w) f32, +inf where fewer than two samples
        are finite (pbrs_render_tile_aovs_var).  `camera`: a Camera of the film's size in the place of the scene's own (a frame of a
        camera move, as render_temporal renders it)."""
        names = _aov_names(aovs)
        return self._render_host(self._params(strata_x, strata_y, depth, seed, tile, samples_per_pass, counters, timing, bands, integrator), names,
                                 camera=camera)

    def render_aovs_device(self, rgb_device_ptr, aov_device_ptrs, strata_x, strata_y, depth, seed, tile=None, samples_per_pass=0,
                           counters=False, timing=False, bands=None, integrator="path"):
        """render_device() plus first-hit AOVs into caller-owned device memory: `aov_device_ptrs` = {name: pointer} (e.g.
        tensor.data_ptr(); sizes as render_aovs returns them).  Asynchronous like render_device: valid after `collect_stats()`."""
        bufs, variance = self._aov_device(aov_device_ptrs)
        self._render_device(self._params(strata_x, strata_y, depth, seed, tile, samples_per_pass, counters, timing, bands, integrator),
                            rgb_device_ptr, bufs, variance)

    def render_aovs_var_device(self, rgb_device_ptr, aov_device_ptrs, variance_device_ptr, strata_x, strata_y, depth, seed, tile=None,
                               samples_per_pass=0, counters=False, timing=False, bands=None, integrator="path"):
        """render_aovs_device() plus the variance AOV into `variance_device_ptr` (w * h f32; pbrs_render_tile_aovs_var_device)."""
        unknown = [n for n in aov_device_ptrs if n not in AOVS]
        if unknown:
            raise ValueError(f"unknown AOV name(s) {unknown}; known: {sorted(AOVS)}")
        bufs, _ = self._aov_device(aov_device_ptrs)
        self._render_device(self._params(strata_x, strata_y, depth, seed, tile, samples_per_pass, counters, timing, bands, integrator),
                            rgb_device_ptr, bufs, variance_device_ptr)

    def render_matte(self, strata_x, strata_y, depth, seed, key="instance", slots=6, aovs=(), tile=None, samples_per_pass=0, counters=False,
                     timing=False, bands=None, integrator="path"):
        """render_aovs() plus the id matte of the same camera samples (include/pbrs_gpu.h, pbrs_render_tile_matte) -> (rgb, matte, aovs,
        stats).  matte = {"ids": (h, w, slots) u32, "coverage": (h, w, slots) f32, "residual": (h, w) f32}: per pixel the ids ranked by the
        share of the pixel's samples each covers (an unused rank: 0xffffffff, +0), and the share of the hits the table had no entry for.
        key: "instance" or "material"; aovs: names as render_aovs takes them ("variance" included)."""
        names = _aov_names(aovs)
        mp = MatteParams.make(key, slots)
        p = self._params(strata_x, strata_y, depth, seed, tile, samples_per_pass, counters, timing, bands, integrator)
        layers = max(int(slots), 0)  # (a refused `slots` still reaches the library: it is the one that refuses)
        matte = {"ids": np.empty((p.h, p.w, layers), dtype=np.uint32), "coverage": np.empty((p.h, p.w, layers), dtype=np.float32),
                 "residual": np.empty((p.h, p.w), dtype=np.float32)}
        mb = MatteBuffers()
        for n in MATTE_LAYERS:
            setattr(mb, n, matte[n].ctypes.data)
        out, arrays, stats = self._render_host(p, names, mp, mb)
        return out, matte, arrays, stats

    def render_matte_device(self, rgb_device_ptr, matte_device_ptrs, strata_x, strata_y, depth, seed, key="instance", slots=6,
                            aov_device_ptrs=None, tile=None, samples_per_pass=0, counters=False, timing=False, bands=None, integrator="path"):
        """render_matte() into caller-owned device memory: `matte_device_ptrs` = {"ids", "coverage"[, "residual"]: pointer}, `aov_device_ptrs`
        as render_aovs_device takes them ("variance" included).  Asynchronous like render_device: valid after `collect_stats()`."""
        unknown = [n for n in matte_device_ptrs if n not in MATTE_LAYERS]
        if unknown:
            raise ValueError(f"unknown matte layer(s) {unknown}; known: {list(MATTE_LAYERS)}")
        bufs, variance = self._aov_device(aov_device_ptrs)
        mp, mb = MatteParams.make(key, slots), MatteBuffers()
        for n, ptr in matte_device_ptrs.items():
            setattr(mb, n, ptr)
        self._render_device(self._params(strata_x, strata_y, depth, seed, tile, samples_per_pass, counters, timing, bands, integrator),
                            rgb_device_ptr, bufs, variance, mp, mb)

    def render_passes(self, strata_x, strata_y, depth, seed, passes=PASSES, aovs=(), tile=None, samples_per_pass=0, counters=False,
                      timing=False, bands=None, integrator="path"):
        """render_aovs() plus the light passes of the same camera samples (include/pbrs_gpu.h, pbrs_render_tile_passes) -> (rgb,
        {pass: array}, {aov: array}, stats).  "direct" / "indirect": (h, w, 3) f32, the light that reaches the camera after one path
        vertex and after more; "direct_variance" / "indirect_variance": (h, w) f32, the variance of each one's pixel-mean luminance, +inf
        where fewer than two samples are finite.  The path integrator at depth >= 1 only."""
        pnames, names = _pass_names(passes), _aov_names(aovs)
        p = self._params(strata_x, strata_y, depth, seed, tile, samples_per_pass, counters, timing, bands, integrator)
        layers = {n: np.empty((p.h, p.w, 3) if PASS_CHANNELS[n] > 1 else (p.h, p.w), dtype=np.float32) for n in pnames}
        pb = PassBuffers()
        for n in pnames:
            setattr(pb, n, layers[n].ctypes.data)
        out, arrays, stats = self._render_host(p, names, pb=pb)
        return out, layers, arrays, stats

    def render_passes_device(self, rgb_device_ptr, pass_device_ptrs, strata_x, strata_y, depth, seed, aov_device_ptrs=None, tile=None,
                             samples_per_pass=0, counters=False, timing=False, bands=None, integrator="path"):
        """render_passes() into caller-owned device memory: `pass_device_ptrs` = {pass: pointer}, `aov_device_ptrs` as render_aovs_device
        takes them ("variance" included).  Asynchronous like render_device: valid after `collect_stats()`."""
        _pass_names(pass_device_ptrs)
        bufs, variance = self._aov_device(aov_device_ptrs)
        pb = PassBuffers()
        for n, ptr in pass_device_ptrs.items():
            setattr(pb, n, ptr)
        self._render_device(self._params(strata_x, strata_y, depth, seed, tile, samples_per_pass, counters, timing, bands, integrator),
                            rgb_device_ptr, bufs, variance, pb=pb)

    def combine_passes(self, direct, indirect):
        """direct + indirect per component on the device (include/pbrs_gpu.h, pbrs_combine_passes) -> (h, w, 3) f32."""
        direct = np.ascontiguousarray(direct, dtype=np.float32)
        indirect = np.ascontiguousarray(indirect, dtype=np.float32)
        if direct.ndim != 3 or direct.shape[2] != 3 or direct.shape != indirect.shape:
            raise ValueError(f"a direct layer of shape {direct.shape} beside an indirect one of {indirect.shape}; both are (h, w, 3)")
        h, w, _ = direct.shape
        out = np.empty_like(direct)
        self._check(self._L.pbrs_combine_passes(self._h, w, h, direct.ctypes.data, indirect.ctypes.data, out.ctypes.data), "pbrs_combine_passes")
        return out

    def combine_passes_device(self, direct_device_ptr, indirect_device_ptr, rgb_out_device_ptr, w, h):
        """combine_passes() on caller-owned device memory; the output pointer may be either input's.  Runs on the context's stream behind
        whatever was queued there and does not wait: valid after `collect_stats()`."""
        self._check(self._L.pbrs_combine_passes_device(self._h, w, h, C.c_void_p(direct_device_ptr), C.c_void_p(indirect_device_ptr),
                                                       C.c_void_p(rgb_out_device_ptr)), "pbrs_combine_passes_device")

    def matte_mask(self, ids, coverage, select):
        """The mask of the ids in `select` (any order, duplicates allowed: sorted here) from the layers render_matte returns -> (h, w) f32:
        per pixel the coverages of the selected ids, summed in rank order (include/pbrs_gpu.h, pbrs_matte_mask)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        coverage = np.ascontiguousarray(coverage, dtype=np.float32)
        if ids.ndim != 3 or ids.shape != coverage.shape:
            raise ValueError(f"ids of shape {ids.shape} beside a coverage of {coverage.shape}; both are (h, w, slots)")
        h, w, slots = ids.shape
        sel = _matte_select(select)
        out = np.empty((h, w), dtype=np.float32)
        self._check(self._L.pbrs_matte_mask(self._h, w, h, slots, ids.ctypes.data, coverage.ctypes.data, sel.ctypes.data if sel.size else None,
                                            sel.size, out.ctypes.data), "pbrs_matte_mask")
        return out

    def matte_mask_device(self, ids_device_ptr, coverage_device_ptr, mask_device_ptr, w, h, slots, select):
        """matte_mask() on caller-owned device memory.  Runs on the context's stream behind whatever was queued there (a
        render_matte_device needs no synchronisation in between) and does not wait: valid after `collect_stats()`."""
        sel = _matte_select(select)
        self._check(self._L.pbrs_matte_mask_device(self._h, w, h, slots, C.c_void_p(ids_device_ptr), C.c_void_p(coverage_device_ptr),
                                                   sel.ctypes.data if sel.size else None, sel.size, C.c_void_p(mask_device_ptr)),
                    "pbrs_matte_mask_device")

    def render_filtered(self, pixel_filter, strata_x, strata_y, depth, seed, tile=None, samples_per_pass=0, counters=False, timing=False,
                        integrator="path"):
        """render() through a pixel reconstruction filter (PixelFilter; include/pbrs_gpu.h, pbrs_render_tile_filtered) -> (h, w, 3) f32
        radiance, stats dict.  The tile traces a halo of floor(r + 0.5) pixels around it (stats["samples"] counts it)."""
        p = self._params(strata_x, strata_y, depth, seed, tile, samples_per_pass, counters, timing, None, integrator)
        out = np.empty((p.h, p.w, 3), dtype=np.float32)
        st = Stats()
        self._check(self._L.pbrs_render_tile_filtered(self._h, C.addressof(self.scene.camera), C.addressof(p), C.byref(pixel_filter),
                                                      out.ctypes.data, C.addressof(st)), "pbrs_render_tile_filtered")
        return out, st.as_dict()

    def render_filtered_device(self, rgb_device_ptr, pixel_filter, strata_x, strata_y, depth, seed, tile=None, samples_per_pass=0,
                               counters=False, timing=False, integrator="path"):
        """render_filtered() into caller-owned device memory; asynchronous like render_device: valid after `collect_stats()`."""
        p = self._params(strata_x, strata_y, depth, seed, tile, samples_per_pass, counters, timing, None, integrator)
        self._check(self._L.pbrs_render_tile_filtered_device(self._h, C.addressof(self.scene.camera), C.addressof(p), C.byref(pixel_filter),
                                                             C.c_void_p(rgb_device_ptr), None), "pbrs_render_tile_filtered_device")

    @staticmethod
    def _denoise_guide_names(names):
        unknown = [n for n in names if n not in DENOISE_GUIDES]
        if unknown:
            raise ValueError(f"unknown denoise guide(s) {unknown}; known: {sorted(DENOISE_GUIDES)}")

    @staticmethod
    def _host_guides(g, rgb, given):
        """Fills the guides struct `g` from the arrays of `given` that are there, checked against the image; returns the arrays to keep."""
        h, w, _ = rgb.shape
        keep = []
        for n, a in given.items():
            if a is None:
                continue
            ch, dt = DENOISE_GUIDES.get(n, (1, np.float32))  # (the variance)
            a = np.ascontiguousarray(a, dtype=dt)
            if a.shape != ((h, w, ch) if ch > 1 else (h, w)):
                raise ValueError(f"{n} guide of shape {a.shape} beside an image of {rgb.shape}")
            keep.append(a)
            setattr(g, n, a.ctypes.data)
        return keep

    def _device_guides(self, g, guide_device_ptrs):
        ptrs = dict(guide_device_ptrs or {})
        self._denoise_guide_names(ptrs)
        for n, ptr in ptrs.items():
            setattr(g, n, ptr)
        return ptrs

    def denoise(self, rgb, albedo=None, normal=None, depth=None, instance=None, **params):
        """The edge-avoiding a-trous denoiser (include/pbrs_gpu.h, pbrs_denoise) over an (h, w, 3) f32 image and the guides given
        (arrays as render_aovs returns them; None = that stop is off) -> (h, w, 3) f32.  params: DenoiseParams.make's keywords; by
        default the image is demodulated when there is an albedo and taps stop at instance edges when there are ids."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        h, w, _ = rgb.shape
        p = DenoiseParams.for_guides(w, h, albedo is not None, instance is not None, **params)
        g = DenoiseGuides()
        keep = self._host_guides(g, rgb, {"albedo": albedo, "normal": normal, "depth": depth, "instance": instance})  # noqa: F841
        out = np.empty_like(rgb)
        self._check(self._L.pbrs_denoise(self._h, C.addressof(p), rgb.ctypes.data, C.addressof(g), out.ctypes.data), "pbrs_denoise")
        return out

    def denoise_device(self, rgb_in_device_ptr, rgb_out_device_ptr, w, h, guide_device_ptrs=None, **params):
        """denoise() on caller-owned device memory: `guide_device_ptrs` = {name: pointer} of albedo / normal / depth / instance.  Runs on
        the context's stream behind whatever was queued there (a render_aovs_device needs no synchronisation in between) and does not
        wait: valid after `collect_stats()`.  The output pointer may be the input's."""
        g = DenoiseGuides()
        ptrs = self._device_guides(g, guide_device_ptrs)
        p = DenoiseParams.for_guides(w, h, bool(ptrs.get("albedo")), bool(ptrs.get("instance")), **params)
        self._check(self._L.pbrs_denoise_device(self._h, C.addressof(p), C.c_void_p(rgb_in_device_ptr), C.addressof(g),
                                                C.c_void_p(rgb_out_device_ptr)), "pbrs_denoise_device")

    def _render_denoised(self, name, with_variance, strata_x, strata_y, depth, seed, guides, samples_per_pass, integrator, keep_noisy, params):
        """render_denoised / render_denoised_var: the frame's device buffers (with_variance: and the variance's), the render with its
        guides, the denoise behind it on the same stream, one copy back."""
        self._denoise_guide_names(guides)
        w, h = self.scene.width, self.scene.height
        n_rgb = 3 * w * h * 4
        sizes = {"rgb": n_rgb, "out": n_rgb, **({VARIANCE: w * h * 4} if with_variance else {}), **_guide_bytes(guides, w, h)}
        with DeviceBuffers(sizes, name) as dev:
            gp = dev.ptrs(guides)
            if with_variance:
                self.render_aovs_var_device(dev.ptr("rgb"), gp, dev.ptr(VARIANCE), strata_x, strata_y, depth, seed,
                                            samples_per_pass=samples_per_pass, integrator=integrator)
                self.denoise_var_device(dev.ptr("rgb"), dev.ptr("out"), w, h, dev.ptr(VARIANCE), gp, **params)
            else:
                self.render_aovs_device(dev.ptr("rgb"), gp, strata_x, strata_y, depth, seed, samples_per_pass=samples_per_pass,
                                        integrator=integrator)
                self.denoise_device(dev.ptr("rgb"), dev.ptr("out"), w, h, gp, **params)
            return self._denoised_frame(dev, "out", (h, w, 3), keep_noisy, self.collect_stats())  # (which waits for the stream)

    @staticmethod
    def _denoised_frame(dev, denoised, shape, keep_noisy, stats):
        """The one copy back of the render_denoised family -> (denoised, stats) or (denoised, noisy, stats)."""
        out = dev.download(denoised, shape, np.float32, "the denoised image")
        if not keep_noisy:
            return out, stats
        return out, dev.download("rgb", shape, np.float32, "the plain image"), stats

    def render_denoised(self, strata_x, strata_y, depth, seed, guides=("albedo", "normal", "depth", "instance"), samples_per_pass=0,
                        integrator="path", keep_noisy=False, **params):
        """The whole frame rendered with its guides and denoised in device memory (render_aovs_device, then denoise_device on the same
        stream, no synchronisation in between), copied back once -> (h, w, 3) f32 denoised radiance, stats dict; with keep_noisy the
        plain image comes too: (denoised, noisy, stats)."""
        return self._render_denoised("render_denoised", False, strata_x, strata_y, depth, seed, guides, samples_per_pass, integrator,
                                     keep_noisy, params)

    def denoise_var(self, rgb, variance, albedo=None, normal=None, depth=None, instance=None, return_variance=False, **params):
        """The variance-guided a-trous denoiser (include/pbrs_gpu.h, pbrs_denoise_var) over an (h, w, 3) f32 image, its (h, w) f32
        variance (render_aovs(..., aovs=(..., "variance"))) and the guides given -> (h, w, 3) f32; with return_variance also the
        filtered variance: (denoised, variance_out).  params: DenoiseVarParams.make's keywords, flags by default as denoise()."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        h, w, _ = rgb.shape
        p = DenoiseVarParams.for_guides(w, h, albedo is not None, instance is not None, **params)
        g = DenoiseVarGuides()
        keep = self._host_guides(g, rgb, {"albedo": albedo, "normal": normal, "depth": depth, "instance": instance,  # noqa: F841
                                          VARIANCE: variance})
        out = np.empty_like(rgb)
        vout = np.empty((h, w), dtype=np.float32) if return_variance else None
        self._check(self._L.pbrs_denoise_var(self._h, C.addressof(p), rgb.ctypes.data, C.addressof(g), out.ctypes.data,
                                             vout.ctypes.data if return_variance else None), "pbrs_denoise_var")
        return (out, vout) if return_variance else out

    def denoise_var_device(self, rgb_in_device_ptr, rgb_out_device_ptr, w, h, variance_device_ptr, guide_device_ptrs=None,
                           variance_out_device_ptr=None, **params):
        """denoise_var() on caller-owned device memory, asynchronous on the context's stream like denoise_device.  The output pointers
        may be the inputs'."""
        g = DenoiseVarGuides()
        ptrs = self._device_guides(g, guide_device_ptrs)
        p = DenoiseVarParams.for_guides(w, h, bool(ptrs.get("albedo")), bool(ptrs.get("instance")), **params)
        g.variance = variance_device_ptr
        self._check(self._L.pbrs_denoise_var_device(self._h, C.addressof(p), C.c_void_p(rgb_in_device_ptr), C.addressof(g),
                                                    C.c_void_p(rgb_out_device_ptr), C.c_void_p(variance_out_device_ptr)),
                    "pbrs_denoise_var_device")

    def render_denoised_var(self, strata_x, strata_y, depth, seed, guides=("albedo", "normal", "depth", "instance"), samples_per_pass=0,
                            integrator="path", keep_noisy=False, **params):
        """render_denoised() through the variance AOV and the variance-guided denoiser (render_aovs_var_device, then denoise_var_device
        on the same stream, no synchronisation in between), copied back once -> (denoised, stats) or (denoised, noisy, stats)."""
        return self._render_denoised("render_denoised_var", True, strata_x, strata_y, depth, seed, guides, samples_per_pass, integrator,
                                     keep_noisy, params)

    def render_denoised_passes(self, strata_x, strata_y, depth, seed, guides=("albedo", "normal", "depth", "instance"), samples_per_pass=0,
                               keep_noisy=False, **params):
        """The whole frame rendered once with its guides and the four light passes, direct and indirect light each through the
        variance-guided denoiser with its own variance, the two summed again (render_passes_device, denoise_var_device twice,
        combine_passes_device: one stream, no synchronisation in between), copied back once -> (denoised, stats) or (denoised, noisy,
        stats).  params: DenoiseVarParams.make's keywords, for both layers."""
        self._denoise_guide_names(guides)
        w, h = self.scene.width, self.scene.height
        sizes = {"rgb": 3 * w * h * 4, **{n: PASS_CHANNELS[n] * w * h * 4 for n in PASSES}, **_guide_bytes(guides, w, h)}
        with DeviceBuffers(sizes, "render_denoised_passes") as dev:
            gp = dev.ptrs(guides)
            self.render_passes_device(dev.ptr("rgb"), dev.ptrs(PASSES), strata_x, strata_y, depth, seed, aov_device_ptrs=gp,
                                      samples_per_pass=samples_per_pass)
            for layer in ("direct", "indirect"):  # each in place
                self.denoise_var_device(dev.ptr(layer), dev.ptr(layer), w, h, dev.ptr(layer + "_variance"), gp, **params)
            self.combine_passes_device(dev.ptr("direct"), dev.ptr("indirect"), dev.ptr("direct"), w, h)
            return self._denoised_frame(dev, "direct", (h, w, 3), keep_noisy, self.collect_stats())  # (which waits for the stream)

    @staticmethod
    def _temporal_host(layout, arrays, shape, what):
        """{name: array or None} -> ({name: pointer}, the contiguous arrays to keep alive), each checked against the (h, w) image."""
        ptrs, keep = {}, []
        for n, a in arrays.items():
            if n not in layout:
                raise ValueError(f"unknown {what} plane {n!r}; known: {list(layout)}")
            if a is None:
                continue
            ch, dt = layout[n]
            a = np.ascontiguousarray(a, dtype=dt)
            if a.shape != (shape + (ch,) if ch > 1 else shape):
                raise ValueError(f"{what} plane {n} of shape {a.shape} beside an image of {shape}")
            keep.append(a)
            ptrs[n] = a.ctypes.data
        return ptrs, keep

    def temporal_accumulate(self, rgb, depth, camera, variance=None, normal=None, instance=None, history=None, prev=None, camera_prev=None,
                            return_variance=True, motion=None, clip=None, **params):
        """Temporal accumulation (include/pbrs_gpu.h, pbrs_temporal_accumulate) of an (h, w, 3) f32 image, its depth AOV and what else
        of its variance, normal and instance AOVs is given, rendered through `camera`.  `history` = the dict an earlier call returned
        (None: the first frame of a sequence), `prev` = {"depth", "normal", "instance"} of that earlier frame, `camera_prev` its Camera.
        -> ({"rgb": (h, w, 3), "moments": (h, w, 2), "length": (h, w)}, variance (h, w)), all f32: the new history, whose rgb is the
        accumulated image, and the variance of its pixels' luminance (None with return_variance=False).  `motion`: the table of
        api.instance_motion for sequences in which instances move (pbrs_temporal_accumulate_motion; needs `instance`); None is the call
        without one.  `clip`: True, a dict of HistoryClipParams.make's keywords or a HistoryClipParams clips the reprojected history to
        the colour box of this frame's neighbourhood (pbrs_temporal_accumulate_clip: shadows and lights that move); None is the call
        without it.  params: TemporalParams.make's keywords."""
        table = _motion_args(motion)
        cp = _history_clip(clip)
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        h, w, _ = rgb.shape
        p = TemporalParams.make(w, h, **params)
        fp, keep = self._temporal_host(TEMPORAL_FRAME, {"rgb": rgb, "variance": variance, "depth": depth, "normal": normal, "instance": instance},
                                       (h, w), "frame")
        frame = _temporal_struct(TemporalFrame, TEMPORAL_FRAME, fp, "frame")
        hin = guides = None
        if history is not None:
            hp, k2 = self._temporal_host(TEMPORAL_HISTORY, history, (h, w), "history")
            gp, k3 = self._temporal_host(TEMPORAL_GUIDES, prev or {}, (h, w), "previous guide")
            keep += k2 + k3
            hin = _temporal_struct(TemporalHistory, TEMPORAL_HISTORY, hp, "history")
            guides = _temporal_struct(TemporalGuides, TEMPORAL_GUIDES, gp, "previous guide")
        out = {n: np.empty((h, w, ch) if ch > 1 else (h, w), dtype=dt) for n, (ch, dt) in TEMPORAL_HISTORY.items()}
        hout = _temporal_struct(TemporalHistory, TEMPORAL_HISTORY, {n: a.ctypes.data for n, a in out.items()}, "history")
        vout = np.empty((h, w), dtype=np.float32) if return_variance else None
        args = (self._h, C.addressof(p), C.addressof(camera), C.addressof(camera_prev) if camera_prev else None, C.addressof(frame),
                C.addressof(guides) if guides else None, C.addressof(hin) if hin else None, C.addressof(hout),
                vout.ctypes.data if return_variance else None)
        if cp is not None:
            self._check(self._L.pbrs_temporal_accumulate_clip(*args, *table, C.addressof(cp)), "pbrs_temporal_accumulate_clip")
        elif motion is None:
            self._check(self._L.pbrs_temporal_accumulate(*args), "pbrs_temporal_accumulate")
        else:
            self._check(self._L.pbrs_temporal_accumulate_motion(*args, *table), "pbrs_temporal_accumulate_motion")
        return out, vout

    def temporal_accumulate_device(self, frame_device_ptrs, history_out_device_ptrs, w, h, camera, history_in_device_ptrs=None,
                                   prev_device_ptrs=None, camera_prev=None, variance_out_device_ptr=None, motion=None, clip=None, **params):
        """temporal_accumulate() on caller-owned device memory: {name: pointer} dicts with the names of TemporalFrame, TemporalHistory
        and TemporalGuides.  Runs on the context's stream behind whatever was queued there (a render_aovs_var_device before it and a
        denoise_var_device after it need no synchronisation in between) and does not wait: valid after `collect_stats()`.  The history
        written must not share a plane with the history read.  `motion` (host memory, as in temporal_accumulate) is copied on that
        stream before the call returns.  `clip`: as temporal_accumulate's; the history written must then not be the frame's rgb plane."""
        table = _motion_args(motion)
        cp = _history_clip(clip)
        p = TemporalParams.make(w, h, **params)
        frame = _temporal_struct(TemporalFrame, TEMPORAL_FRAME, frame_device_ptrs, "frame")
        hout = _temporal_struct(TemporalHistory, TEMPORAL_HISTORY, history_out_device_ptrs, "history")
        hin = guides = None
        if history_in_device_ptrs is not None:
            hin = _temporal_struct(TemporalHistory, TEMPORAL_HISTORY, history_in_device_ptrs, "history")
            guides = _temporal_struct(TemporalGuides, TEMPORAL_GUIDES, prev_device_ptrs or {}, "previous guide")
        args = (self._h, C.addressof(p), C.addressof(camera), C.addressof(camera_prev) if camera_prev else None, C.addressof(frame),
                C.addressof(guides) if guides else None, C.addressof(hin) if hin else None, C.addressof(hout), C.c_void_p(variance_out_device_ptr))
        if cp is not None:
            self._check(self._L.pbrs_temporal_accumulate_clip_device(*args, *table, C.addressof(cp)), "pbrs_temporal_accumulate_clip_device")
        elif motion is None:
            self._check(self._L.pbrs_temporal_accumulate_device(*args), "pbrs_temporal_accumulate_device")
        else:
            self._check(self._L.pbrs_temporal_accumulate_motion_device(*args, *table), "pbrs_temporal_accumulate_motion_device")

    def motion_vectors(self, depth, camera, camera_prev, instance=None, motion=None, return_prev_depth=False):
        """The motion vector AOV (include/pbrs_gpu.h, pbrs_motion_vectors) of an (h, w) f32 depth AOV rendered through `camera`: per
        pixel where its surface point was on `camera_prev`'s film minus where it is, in pixels -> (h, w, 2) f32, and with
        return_prev_depth also the depth the previous frame would have recorded, (h, w) f32.  `motion` (api.instance_motion) with the
        `instance` AOV follows moving instances; without them only the camera moves."""
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        if depth.ndim != 2:
            raise ValueError(f"the depth AOV is (h, w), not {depth.shape}")
        h, w = depth.shape
        if instance is not None:
            instance = np.ascontiguousarray(instance, dtype=np.uint32)
            if instance.shape != (h, w):
                raise ValueError(f"instance plane of shape {instance.shape} beside a depth of {(h, w)}")
        out = np.empty((h, w, 2), dtype=np.float32)
        wq = np.empty((h, w), dtype=np.float32) if return_prev_depth else None
        mp, n = _motion_args(motion)
        self._check(self._L.pbrs_motion_vectors(self._h, w, h, C.addressof(camera), C.addressof(camera_prev) if camera_prev else None,
                                                depth.ctypes.data, instance.ctypes.data if instance is not None else None, mp, n,
                                                out.ctypes.data, wq.ctypes.data if return_prev_depth else None), "pbrs_motion_vectors")
        return (out, wq) if return_prev_depth else out

    def motion_vectors_device(self, depth_device_ptr, motion_out_device_ptr, w, h, camera, camera_prev, instance_device_ptr=None, motion=None,
                              prev_depth_out_device_ptr=None):
        """motion_vectors() on caller-owned device memory, on the context's stream without waiting: valid after `collect_stats()`.  The
        table stays host memory."""
        mp, n = _motion_args(motion)
        self._check(self._L.pbrs_motion_vectors_device(self._h, w, h, C.addressof(camera), C.addressof(camera_prev) if camera_prev else None,
                                                       C.c_void_p(depth_device_ptr), C.c_void_p(instance_device_ptr), mp, n,
                                                       C.c_void_p(motion_out_device_ptr), C.c_void_p(prev_depth_out_device_ptr)),
                    "pbrs_motion_vectors_device")

    def spatial_variance(self, moments, length, variance, depth=None, normal=None, instance=None, **params):
        """The spatial variance estimate for pixels with a short history (include/pbrs_gpu.h, pbrs_spatial_variance): the (h, w, 2)
        moments and (h, w) length of the history temporal_accumulate returned, the (h, w) variance it returned beside them, and the
        frame's guides (None = that stop is off) -> (h, w) f32: `variance` with the short pixels' entries replaced by the estimate
        over their neighbourhood.  params: SpatialVarianceParams.make's keywords; by default taps stop at instance edges when there
        are ids."""
        length = np.ascontiguousarray(length, dtype=np.float32)
        if length.ndim != 2:
            raise ValueError(f"the length plane is (h, w), not {length.shape}")
        h, w = length.shape
        params.setdefault("id_stop", instance is not None)
        p = SpatialVarianceParams.make(w, h, **params)
        ptrs, keep = self._temporal_host(SPATIAL_VARIANCE_PLANES, {"moments": moments, "length": length, "variance": variance}, (h, w),  # noqa: F841
                                         "spatial variance")
        for n in SPATIAL_VARIANCE_PLANES:
            if n not in ptrs:
                raise ValueError(f"spatial variance plane {n} is missing")
        gp, k2 = self._temporal_host(TEMPORAL_GUIDES, {"depth": depth, "normal": normal, "instance": instance}, (h, w), "spatial variance guide")  # noqa: F841
        g = _temporal_struct(SpatialVarianceGuides, TEMPORAL_GUIDES, gp, "spatial variance guide")
        out = np.empty((h, w), dtype=np.float32)
        self._check(self._L.pbrs_spatial_variance(self._h, C.addressof(p), ptrs["moments"], ptrs["length"], C.addressof(g), ptrs["variance"],
                                                  out.ctypes.data), "pbrs_spatial_variance")
        return out

    def spatial_variance_device(self, moments_device_ptr, length_device_ptr, variance_in_device_ptr, variance_out_device_ptr, w, h,
                                guide_device_ptrs=None, **params):
        """spatial_variance() on caller-owned device memory: `guide_device_ptrs` = {name: pointer} of depth / normal / instance.  Runs on
        the context's stream behind whatever was queued there (a temporal_accumulate_device before it and a denoise_var_device after
        it need no synchronisation in between) and does not wait: valid after `collect_stats()`.  The output pointer may be the
        variance input's."""
        for n, ptr in (("moments", moments_device_ptr), ("length", length_device_ptr), ("variance", variance_in_device_ptr),
                       ("variance_out", variance_out_device_ptr)):
            if not ptr:
                raise ValueError(f"spatial variance plane {n} is a null pointer")
        ptrs = {n: ptr for n, ptr in dict(guide_device_ptrs or {}).items() if ptr}
        g = _temporal_struct(SpatialVarianceGuides, TEMPORAL_GUIDES, ptrs, "spatial variance guide")
        params.setdefault("id_stop", "instance" in ptrs)
        p = SpatialVarianceParams.make(w, h, **params)
        self._check(self._L.pbrs_spatial_variance_device(self._h, C.addressof(p), C.c_void_p(moments_device_ptr), C.c_void_p(length_device_ptr),
                                                         C.addressof(g), C.c_void_p(variance_in_device_ptr), C.c_void_p(variance_out_device_ptr)),
                    "pbrs_spatial_variance_device")

    def display(self, rgb, exposure_in=None, return_exposure=False, return_histogram=False, **params):
        """The display transform (include/pbrs_gpu.h, pbrs_display) of an (h, w, 3) f32 image -> an (h, w, 4) uint8 array, RGBA with alpha
        255: exposure, tone curve, transfer function, quantiser.  params: DisplayParams.make's keywords (auto=True: the exposure follows
        the image's trimmed log-average luminance; `exposure_in`, a float, is then the previous frame's exposure, which `adapt` eases
        from).  With return_exposure and / or return_histogram the result is a tuple: the image, then the applied auto exposure e (a
        float32; 1 without auto), then the 512 counts of the luminance histogram (uint32)."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"the image is (h, w, 3), not {rgb.shape}")
        h, w, _ = rgb.shape
        p = DisplayParams.make(w, h, **params)
        out = np.empty((h, w), dtype="<u4")
        e_in = np.array([exposure_in], dtype=np.float32) if exposure_in is not None else None
        e_out = np.zeros(1, dtype=np.float32) if return_exposure else None
        hist = np.zeros(DisplayParams.BINS, dtype=np.uint32) if return_histogram else None
        io = DisplayIO(*(a.ctypes.data if a is not None else None for a in (e_in, e_out, hist)))
        self._check(self._L.pbrs_display(self._h, C.addressof(p), rgb.ctypes.data, C.addressof(io), out.ctypes.data), "pbrs_display")
        img = out.view(np.uint8).reshape(h, w, 4)
        if not (return_exposure or return_histogram):
            return img
        return (img,) + ((e_out[0],) if return_exposure else ()) + ((hist,) if return_histogram else ())

    def display_device(self, rgb_device_ptr, rgba8_device_ptr, w, h, io_device_ptrs=None, **params):
        """display() on caller-owned device memory: `io_device_ptrs` = {name: pointer} of exposure_in / exposure_out / histogram_out (one
        float, one float, 512 words).  Runs on the context's stream behind whatever was queued there and does not wait: valid after
        `collect_stats()`.  exposure_out may be exposure_in: a sequence carries its exposure in one device word."""
        p = DisplayParams.make(w, h, **params)
        io = DisplayIO()
        for n, ptr in dict(io_device_ptrs or {}).items():
            if n not in ("exposure_in", "exposure_out", "histogram_out"):
                raise ValueError(f"unknown display io pointer {n!r}; known: exposure_in, exposure_out, histogram_out")
            setattr(io, n, ptr)
        self._check(self._L.pbrs_display_device(self._h, C.addressof(p), C.c_void_p(rgb_device_ptr), C.addressof(io), C.c_void_p(rgba8_device_ptr)),
                    "pbrs_display_device")

    def upsample(self, rgb_lo, w, h, factor=2, lo=None, hi=None, return_weight=False, **params):
        """Guided upsampling (include/pbrs_gpu.h, pbrs_upsample) of an (hl, wl, 3) f32 image to w x h, hl = ceil(h / factor) and wl
        likewise -> (h, w, 3) f32; with return_weight also the (h, w) f32 guided weight sums: (out, weight).  `lo`, `hi`: dicts of the
        guides at the low and at the full size (albedo / normal / depth / instance arrays as render_aovs returns them; a guide counts
        when both give it).  params: UpsampleParams.make's keywords; by default the image is demodulated when there is an albedo pair and
        taps stop at instance edges when there is an instance pair."""
        rgb_lo = np.ascontiguousarray(rgb_lo, dtype=np.float32)
        lo, hi = {n: a for n, a in dict(lo or {}).items() if a is not None}, {n: a for n, a in dict(hi or {}).items() if a is not None}
        self._denoise_guide_names(list(lo) + list(hi))
        p = UpsampleParams.for_guides(w, h, factor, "albedo" in lo and "albedo" in hi, "instance" in lo and "instance" in hi, **params)
        wl, hl = p.low_size
        if rgb_lo.shape != (hl, wl, 3):
            raise ValueError(f"the low image is ({hl}, {wl}, 3) for {w} x {h} at factor {factor}, not {rgb_lo.shape}")
        gl, gh = DenoiseGuides(), DenoiseGuides()
        keep = self._host_guides(gl, rgb_lo, lo) + self._host_guides(gh, np.empty((h, w, 0), dtype=np.float32), hi)  # noqa: F841
        out = np.empty((h, w, 3), dtype=np.float32)
        weight = np.empty((h, w), dtype=np.float32) if return_weight else None
        self._check(self._L.pbrs_upsample(self._h, C.addressof(p), rgb_lo.ctypes.data, C.addressof(gl), C.addressof(gh), out.ctypes.data,
                                          weight.ctypes.data if return_weight else None), "pbrs_upsample")
        return (out, weight) if return_weight else out

    def upsample_device(self, rgb_lo_device_ptr, out_device_ptr, w, h, factor=2, lo_device_ptrs=None, hi_device_ptrs=None,
                        weight_out_device_ptr=None, **params):
        """upsample() on caller-owned device memory: `lo_device_ptrs`, `hi_device_ptrs` = {name: pointer} of albedo / normal / depth /
        instance at the low and at the full size.  Runs on the context's stream behind whatever was queued there (the filter of the low
        image and the render of the full-size guides need no synchronisation in between) and does not wait: valid after
        `collect_stats()`."""
        gl, gh = DenoiseGuides(), DenoiseGuides()
        lo, hi = self._device_guides(gl, lo_device_ptrs), self._device_guides(gh, hi_device_ptrs)
        p = UpsampleParams.for_guides(w, h, factor, bool(lo.get("albedo")) and bool(hi.get("albedo")),
                                      bool(lo.get("instance")) and bool(hi.get("instance")), **params)
        self._check(self._L.pbrs_upsample_device(self._h, C.addressof(p), C.c_void_p(rgb_lo_device_ptr), C.addressof(gl), C.addressof(gh),
                                                 C.c_void_p(out_device_ptr), C.c_void_p(weight_out_device_ptr)), "pbrs_upsample_device")

    def compare(self, a, b, maps=False, **params):
        """The comparison (include/pbrs_gpu.h, pbrsx_compare) of the (h, w, 3) f32 image `a` with the reference `b` -> CompareResult: mse,
        rel_mse, mae, ssim, max_abs over the valid pixels and the counts.  With maps=True a tuple: the result, the (h, w) f32 squared
        error of every pixel and, where SSIM is on, its (h, w) f32 SSIM (None where it is off); NaN at invalid pixels.  params:
        CompareParams.make's keywords."""
        a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
        if a.ndim != 3 or a.shape[2] != 3 or b.shape != a.shape:
            raise ValueError(f"the image and the reference are (h, w, 3) and alike, not {a.shape} and {b.shape}")
        h, w, _ = a.shape
        p = CompareParams.make(w, h, **params)
        result = CompareResult()
        error = np.empty((h, w), dtype=np.float32) if maps else None
        ssim = np.empty((h, w), dtype=np.float32) if maps and p.flags & CompareParams.SSIM else None
        m = CompareMaps(*(x.ctypes.data if x is not None else None for x in (error, ssim)))
        self._check(self._L.pbrsx_compare(self._h, C.addressof(p), a.ctypes.data, b.ctypes.data, C.addressof(m) if maps else None, C.addressof(result)),
                    "pbrsx_compare")
        return (result, error, ssim) if maps else result

    def compare_device(self, a_ptr, b_ptr, w, h, result_ptr, map_ptrs=None, **params):
        """compare() on caller-owned device memory: `result_ptr` receives the 64 bytes of CompareResult, `map_ptrs` = {name: pointer} of
        error_out / ssim_out.  Runs on the context's stream behind whatever was queued there and does not wait: valid after
        `collect_stats()`."""
        p = CompareParams.make(w, h, **params)
        m = CompareMaps()
        for n, ptr in dict(map_ptrs or {}).items():
            if n not in ("error_out", "ssim_out"):
                raise ValueError(f"unknown compare map pointer {n!r}; known: error_out, ssim_out")
            setattr(m, n, ptr)
        self._check(self._L.pbrsx_compare_device(self._h, C.addressof(p), C.c_void_p(a_ptr), C.c_void_p(b_ptr), C.addressof(m), C.c_void_p(result_ptr)),
                    "pbrsx_compare_device")

    def despeckle(self, rgb, variance=None, mask=False, removed=False, **params):
        """The (h, w, 3) f32 image `rgb` despeckled (include/pbrs_gpu.h, pbrsi_despeckle): fireflies scaled down to gain times the rank-th
        brightest neighbour, non-finite pixels rebuilt from their neighbours -> a tuple: the image; with `variance`, the (h, w) f32 variance
        AOV, what becomes of it; with mask=True the (h, w) u32 mask (DespeckleParams.CLAMPED | REPAIRED); with removed=True the (h, w, 3)
        f32 energy taken out; and, last, the DespeckleResult with the two counts.  params: DespeckleParams.make's keywords."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"the image is (h, w, 3), not {rgb.shape}")
        h, w, _ = rgb.shape
        p = DespeckleParams.make(w, h, **params)
        if variance is not None:
            variance = np.ascontiguousarray(variance, dtype=np.float32)
            if variance.shape != (h, w):
                raise ValueError(f"the variance is ({h}, {w}), not {variance.shape}")
        out = np.empty((h, w, 3), dtype=np.float32)
        vout = np.empty((h, w), dtype=np.float32) if variance is not None else None
        m = np.empty((h, w), dtype=np.uint32) if mask else None
        rm = np.empty((h, w, 3), dtype=np.float32) if removed else None
        io = DespeckleIO(*(x.ctypes.data if x is not None else None for x in (rgb, out, variance, vout, m, rm)))
        result = DespeckleResult()
        self._check(self._L.pbrsi_despeckle(self._h, C.addressof(p), C.addressof(io), C.addressof(result)), "pbrsi_despeckle")
        return tuple(x for x in (out, vout, m, rm) if x is not None) + (result,)

    def despeckle_device(self, rgb_in_ptr, rgb_out_ptr, w, h, result_ptr=None, plane_ptrs=None, **params):
        """despeckle() on caller-owned device memory: `plane_ptrs` = {name: pointer} of variance_in / variance_out (both or neither; they
        may be one plane) / mask_out / removed_out, `result_ptr` receives the 16 bytes of DespeckleResult (None: not wanted).  Runs on the
        context's stream behind whatever was queued there and does not wait: valid after `collect_stats()`."""
        p = DespeckleParams.make(w, h, **params)
        io = DespeckleIO(rgb_in_ptr, rgb_out_ptr)
        for n, ptr in dict(plane_ptrs or {}).items():
            if n not in ("variance_in", "variance_out", "mask_out", "removed_out"):
                raise ValueError(f"unknown despeckle plane pointer {n!r}; known: variance_in, variance_out, mask_out, removed_out")
            setattr(io, n, ptr)
        self._check(self._L.pbrsi_despeckle_device(self._h, C.addressof(p), C.addressof(io), C.c_void_p(result_ptr)), "pbrsi_despeckle_device")

    def bloom(self, rgb, **params):
        """The (h, w, 3) f32 image `rgb` with its glare (include/pbrs_gpu.h, pbrsb_bloom): the bright part of the image down a pyramid
        of half-size levels, back up, and added to (mix=True: mixed into) the image -> the (h, w, 3) f32 image.  params: BloomParams.make's
        keywords."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"the image is (h, w, 3), not {rgb.shape}")
        h, w, _ = rgb.shape
        p = BloomParams.make(w, h, **params)
        out = np.empty((h, w, 3), dtype=np.float32)
        self._check(self._L.pbrsb_bloom(self._h, C.addressof(p), rgb.ctypes.data, out.ctypes.data), "pbrsb_bloom")
        return out

    def bloom_device(self, src_ptr, dst_ptr, w, h, **params):
        """bloom() on caller-owned device memory, (h, w, 3) f32 each; `dst_ptr` may be `src_ptr`.  Runs on the context's stream behind
        whatever was queued there and does not wait: valid after `collect_stats()`."""
        p = BloomParams.make(w, h, **params)
        self._check(self._L.pbrsb_bloom_device(self._h, C.addressof(p), C.c_void_p(src_ptr), C.c_void_p(dst_ptr)), "pbrsb_bloom_device")

    def dof(self, rgb, depth, return_coc=False, focus_pixel=None, **params):
        """The (h, w, 3) f32 image `rgb` through a thin lens (include/pbrs_gpu.h, pbrsf_dof): every pixel's circle of confusion from the
        (h, w) f32 depth AOV `depth`, then one gather under the header's occlusion rules -> the (h, w, 3) f32 image; with return_coc
        also the (h, w) f32 signed circles (near field negative).  params: DofParams.make's keywords (api.lens gives focus and scale).
        `focus_pixel`: (x, y), takes `focus` from depth[y, x], which must be finite and positive."""
        rgb, depth = np.ascontiguousarray(rgb, dtype=np.float32), np.ascontiguousarray(depth, dtype=np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"the image is (h, w, 3), not {rgb.shape}")
        h, w, _ = rgb.shape
        if depth.shape != (h, w):
            raise ValueError(f"the depth is ({h}, {w}) like the image, not {depth.shape}")
        if focus_pixel is not None:
            if "focus" in params:
                raise ValueError("focus_pixel and focus are two ways to say the same thing: give one")
            x, y = (int(v) for v in focus_pixel)
            if not (0 <= x < w and 0 <= y < h):
                raise ValueError(f"focus_pixel {(x, y)} is outside the {w} x {h} image")
            z = float(depth[y, x])
            if not (np.isfinite(z) and z > 0.0):
                raise ValueError(f"the depth at focus_pixel {(x, y)} is {z}: nothing to focus on")
            params["focus"] = z
        p = DofParams.make(w, h, **params)
        out = np.empty((h, w, 3), dtype=np.float32)
        coc = np.empty((h, w), dtype=np.float32) if return_coc else None
        self._check(self._L.pbrsf_dof(self._h, C.addressof(p), rgb.ctypes.data, depth.ctypes.data, out.ctypes.data, coc.ctypes.data if return_coc else None),
                    "pbrsf_dof")
        return (out, coc) if return_coc else out

    def dof_device(self, rgb_ptr, depth_ptr, out_ptr, w, h, coc_ptr=None, **params):
        """dof() on caller-owned device memory: (h, w, 3) f32 in and out, which must differ, the (h, w) f32 depth, and the optional
        (h, w) f32 signed circles.  Runs on the context's stream behind whatever was queued there and does not wait: valid after
        `collect_stats()`."""
        p = DofParams.make(w, h, **params)
        self._check(self._L.pbrsf_dof_device(self._h, C.addressof(p), C.c_void_p(rgb_ptr), C.c_void_p(depth_ptr), C.c_void_p(out_ptr), C.c_void_p(coc_ptr)),
                    "pbrsf_dof_device")

    def motion_blur(self, rgb, depth, motion, return_velocity=False, **params):
        """The (h, w, 3) f32 image `rgb` through a shutter (include/pbrs_gpu.h, pbrsm_motion_blur): smeared along the (h, w, 2) f32
        motion vector AOV `motion` of the same frame (motion_vectors(): where each surface point was one frame ago minus where it is,
        in pixels), with the (h, w) f32 depth AOV `depth` deciding what covers what -> the (h, w, 3) f32 image; with return_velocity
        also the (h, w, 2) f32 clamped half-exposure vectors.  params: MotionBlurParams.make's keywords."""
        rgb, depth = np.ascontiguousarray(rgb, dtype=np.float32), np.ascontiguousarray(depth, dtype=np.float32)
        motion = np.ascontiguousarray(motion, dtype=np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"the image is (h, w, 3), not {rgb.shape}")
        h, w, _ = rgb.shape
        if depth.shape != (h, w):
            raise ValueError(f"the depth is ({h}, {w}) like the image, not {depth.shape}")
        if motion.shape != (h, w, 2):
            raise ValueError(f"the motion vectors are ({h}, {w}, 2) like the image, not {motion.shape}")
        p = MotionBlurParams.make(w, h, **params)
        out = np.empty((h, w, 3), dtype=np.float32)
        vel = np.empty((h, w, 2), dtype=np.float32) if return_velocity else None
        self._check(self._L.pbrsm_motion_blur(self._h, C.addressof(p), rgb.ctypes.data, depth.ctypes.data, motion.ctypes.data, out.ctypes.data,
                                              vel.ctypes.data if return_velocity else None), "pbrsm_motion_blur")
        return (out, vel) if return_velocity else out

    def motion_blur_device(self, rgb_ptr, depth_ptr, motion_ptr, out_ptr, w, h, velocity_ptr=None, **params):
        """motion_blur() on caller-owned device memory: (h, w, 3) f32 in and out, which must differ, the (h, w) f32 depth, the
        (h, w, 2) f32 motion vectors and the optional (h, w, 2) f32 velocities.  Runs on the context's stream behind whatever was
        queued there and does not wait: valid after `collect_stats()`."""
        p = MotionBlurParams.make(w, h, **params)
        self._check(self._L.pbrsm_motion_blur_device(self._h, C.addressof(p), C.c_void_p(rgb_ptr), C.c_void_p(depth_ptr), C.c_void_p(motion_ptr),
                                                     C.c_void_p(out_ptr), C.c_void_p(velocity_ptr)), "pbrsm_motion_blur_device")

    def _render_guides_device(self, rgb_device_ptr, guide_device_ptrs, seed, camera=None):
        """The full-size first-hit guides of guided upsampling: a one-sample render of `seed` through the path integrator at depth 1 (the
        cheapest route whose first hits are the jittered ones the low-resolution AOVs average; the visualisers shoot through the
        pixel's corner), its image into `rgb_device_ptr`."""
        bufs, _ = self._aov_device(guide_device_ptrs)
        self._render_device(self._params(1, 1, 1, seed, None), rgb_device_ptr, bufs, None, camera=camera)

    def render_upscaled(self, strata_x, strata_y, depth, seed, factor=2, guides=("albedo", "normal", "depth", "instance"), samples_per_pass=0,
                        upsample=None, **params):
        """The frame traced and filtered at 1 / factor of the resolution per axis and rebuilt at full size: render_denoised_var's chain
        through scaled_camera(camera, factor) on the low-resolution tile, the full-size guides as a one-sample render of the same seed
        (the path integrator at depth 1), then upsample_device; one stream, no synchronisation in between, copied back once ->
        (h, w, 3) f32 full-size image, (hl, wl, 3) f32 filtered low-resolution image, stats dict (the guide render's, plus "low_res":
        (wl, hl)).  `upsample`: a dict of UpsampleParams.make's keywords; params: DenoiseVarParams.make's."""
        self._denoise_guide_names(guides)
        factor, up = _upscale_params(dict(upsample or {}, factor=factor), guides)
        w, h = self.scene.width, self.scene.height
        cam_lo = scaled_camera(self.scene.camera, factor)
        wl, hl = cam_lo.width, cam_lo.height
        sizes = {"rgb": 3 * wl * hl * 4, "out": 3 * wl * hl * 4, VARIANCE: wl * hl * 4, "up": 3 * w * h * 4, **_guide_bytes(guides, wl, hl, "_lo"),
                 **_guide_bytes(guides, w, h, "_hi")}
        with DeviceBuffers(sizes, "render_upscaled") as dev:
            gl = {n: dev.ptr(f"{n}_lo") for n in guides}
            self._render_var_device(dev, gl, self._params(strata_x, strata_y, depth, seed, (0, 0, wl, hl), samples_per_pass), cam_lo)
            self.denoise_var_device(dev.ptr("rgb"), dev.ptr("out"), wl, hl, dev.ptr(VARIANCE), gl, **params)
            self._upsample_out_device(dev, gl, guides, seed, w, h, factor, up)
            stats = self.collect_stats()  # waits for the stream
            stats["low_res"] = (wl, hl)
            full = dev.download("up", (h, w, 3), np.float32, "the upscaled image")
            return full, dev.download("out", (hl, wl, 3), np.float32, "the upscaled image"), stats

    def _render_var_device(self, dev, guide_device_ptrs, p, camera):
        """What render_upscaled and a frame sequence both begin with: the render of `p` through `camera` into dev's "rgb", its variance
        into dev's "variance", its guides where `guide_device_ptrs` says."""
        bufs, _ = self._aov_device(guide_device_ptrs)
        self._render_device(p, dev.ptr("rgb"), bufs, dev.ptr(VARIANCE), camera=camera)

    def _upsample_out_device(self, dev, lo_device_ptrs, guides, seed, w, h, factor, up, camera=None):
        """What both end with: the full-size guides rendered into dev's "*_hi" (the image of that render into "up"), then dev's filtered
        low image "out" upsampled over it into "up"."""
        gh = {n: dev.ptr(f"{n}_hi") for n in guides}
        self._render_guides_device(dev.ptr("up"), gh, seed, camera=camera)
        self.upsample_device(dev.ptr("out"), dev.ptr("up"), w, h, factor, lo_device_ptrs, gh, **up)

    @staticmethod
    def _spatial_params(spatial, tparams, guides):
        """render_temporal's / render_animation's `spatial` -> SpatialVarianceParams.make's keywords, or None: min_temporal follows the
        temporal params unless given, the id stop the presence of the instance guide.  An unknown keyword fails here."""
        if spatial is None or spatial is False:
            return None
        sp = {} if spatial is True else dict(spatial)
        sp.setdefault("min_temporal", tparams.get("min_temporal", TemporalParams.make(1, 1).min_temporal))
        sp.setdefault("id_stop", "instance" in guides)
        SpatialVarianceParams.make(1, 1, **sp)
        return sp

    def render_temporal(self, cameras, strata_x, strata_y, depth, seeds, guides=("albedo", "normal", "depth", "instance"), samples_per_pass=0,
                        temporal=None, spatial=None, clip=None, display=None, upscale=None, **params):
        """A sequence of frames of the uploaded scene, one per Camera of `cameras` with the seed of `seeds` at the same place, each
        rendered with its guides and its variance, accumulated against the generator's own history (temporal_accumulate_device; the
        history and the guides it is tested against live in ping-pong device buffers) and filtered (denoise_var_device on the
        accumulated image with the accumulated variance): one stream, no synchronisation inside a frame, the images copied back behind
        one wait per frame.  A generator of (denoised, accumulated, noisy, stats), (h, w, 3) f32 each; its device buffers are freed when
        it ends or is closed.  `guides` must hold "depth"; `temporal`: TemporalParams.make's keywords; params: DenoiseVarParams.make's.
        `spatial`: None is that chain; True, or a dict of SpatialVarianceParams.make's keywords, queues spatial_variance_device in place on
        the accumulated variance between the accumulation and the filter, so that pixels with a history shorter than min_temporal are
        filtered with an estimated variance instead of an unknown one (min_temporal follows `temporal` unless given, the id stop the
        presence of the instance guide).  `clip`: None is that chain; True, a dict of HistoryClipParams.make's keywords or a
        HistoryClipParams makes every accumulation after the first the clipped one (temporal_accumulate's `clip`).  `display`: None is
        that chain; True, or a dict of DisplayParams.make's keywords (auto=True unless it says otherwise), queues display_device on each
        frame's filtered image on the same stream, the exposure carried from frame to frame in a device word: the frame's stats gain
        "display", the (h, w, 4) uint8 image, and "exposure", the auto exposure applied to it.  `upscale`: None is that chain; a factor
        (2, 3 or 4), or a dict of UpsampleParams.make's keywords plus "factor", runs the chain unchanged at 1 / factor of the resolution
        per axis through scaled_camera of each Camera (which are still given at full size) and queues two more calls per frame on the
        same stream, the render of the full-size guides and upsample_device behind the filter: the first image of a frame is then the
        full-size one, the accumulated and the noisy ones stay low, `display` acts on the full-size image, and the stats gain
        "low_res", (wl, hl).  `reference` (a keyword taken out of `params`; the signature is the one callers know): None is that chain; an iterable of one (h, w, 3) image per frame at full size, or a single such
        array for every frame, queues compare_device of each frame's first image against it on the same stream (CompareParams' defaults)
        and yields the CompareResult, read back behind the frame's one wait, as a fifth entry.  `despeckle` (a keyword taken out of
        `params` likewise): None is that chain, with its allocations and tuples; True, or a dict of DespeckleParams.make's keywords, queues
        despeckle_device on the frame's rendered image and its variance between the render and the accumulation, on the same stream, into
        one more colour buffer and the variance in place: the accumulation then reads the despeckled colour, the stats gain "despeckle",
        the DespeckleResult read back behind the frame's one wait, and the "noisy" image stays the render's own.  `bloom` (a keyword
        taken out of `params` likewise): None is that chain, with its allocations and tuples; True, or a dict of BloomParams.make's
        keywords, queues bloom_device on the frame's first image (the full-size one with `upscale`) behind the filter, on the same stream,
        into one more colour buffer: `display` then reads the bloomed image, `reference` keeps scoring the first image as it was, and
        the stats gain "bloom", the (h, w, 3) f32 bloomed image.  `dof` (a keyword taken out of `params` likewise): None is that chain,
        with its allocations and tuples; a dict of DofParams.make's keywords (api.lens gives focus and scale), or a list of such dicts,
        one per frame (a focus pull), queues dof_device on the frame's first image and the depth of its size (the frame's depth guide;
        with `upscale` the full-size guide render's) behind the filter and the upsample, on the same stream, into one more colour
        buffer: a lens blurs before the sensor glares, so `bloom` then reads the defocused image and `display` reads bloom's or,
        without bloom, the defocused one; `reference` keeps scoring the first image as it was, and the stats gain "dof", the (h, w, 3)
        f32 defocused image.  `motion_blur` (a keyword taken out of `params` likewise): None is that chain, with its allocations and
        tuples; True, a dict of MotionBlurParams.make's keywords, or a list of such dicts, one per frame, queues motion_blur_device
        between the depth of field and the bloom, on the same stream, into one more colour buffer: it reads the defocused image (or the
        first one), the depth of its size and the motion vectors of its size against the previous frame's camera (the chain's own
        where render_animation's motion_vectors is on and there is no `upscale`; otherwise motion_vectors_device into a buffer of the
        step's, with `upscale` from the full-size guide render's depth and instance ids through the full-size cameras), `bloom` and
        `display` then read the blurred image, and the stats gain "motion_blur", the (h, w, 3) f32 image.  The first frame has no
        previous one: its "motion_blur" is a copy of what the step read."""
        reference, despeckle, bloom, dof = params.pop("reference", None), params.pop("despeckle", None), params.pop("bloom", None), params.pop("dof", None)
        motion_blur = params.pop("motion_blur", None)
        self._denoise_guide_names(guides)
        if "depth" not in guides:
            raise ValueError("render_temporal reprojects through the depth AOV: guides must hold \"depth\"")
        cameras, seeds = list(cameras), list(seeds)
        if len(cameras) != len(seeds):
            raise ValueError(f"{len(cameras)} cameras beside {len(seeds)} seeds")
        if isinstance(reference, np.ndarray) and self.scene is not None:  # the scene is uploaded: its film is the size every frame has
            _reference_frame(_reference_frames(reference), 0, self.scene.width, self.scene.height)
        frames = [(None, cam, seed) for cam, seed in zip(cameras, seeds)]
        for out in self._temporal_frames(frames, strata_x, strata_y, depth, guides, samples_per_pass, temporal, params, False, spatial, clip, display,
                                         upscale, reference, despeckle, bloom, dof, motion_blur):
            yield out[:4] if reference is None else out[:4] + out[5:]

    def render_animation(self, frames, strata_x, strata_y, depth, guides=("albedo", "normal", "depth", "instance"), samples_per_pass=0,
                         temporal=None, motion_vectors=False, spatial=None, clip=None, display=None, upscale=None, **params):
        """render_temporal for sequences in which instances move.  `frames` yields (HostScene, Camera or None, seed): every frame's scene
        is uploaded (the same instances in the same order as the frame before, moved: instance ids are stable), rendered through the
        Camera (None: the scene's own) with its guides and its variance, accumulated with the table of instance_motion(scene, previous
        scene), and filtered: one stream, one wait per frame.  A generator of (denoised, accumulated, noisy, stats), and with
        motion_vectors=True a fifth entry, the (h, w, 2) motion vector AOV of the frame (zeros for the first one, which has no previous
        frame; motion_vectors="prev_depth": (h, w, 3), the depth the previous frame would have recorded as the third channel, +inf where
        there is none).  `guides` must hold "depth" and "instance"; every scene must have the first one's film size.  Lights that move and the
        shadows of moving instances are not followed (include/pbrs_gpu.h) unless `clip` bounds their lag: as render_temporal's, and so
        are `spatial`, `display`, `upscale` (the motion vectors are then the low-resolution chain's) and the keyword `reference`, whose
        CompareResult is the last entry, and the keywords `despeckle`, `bloom`, `dof` and `motion_blur` (whose vectors follow the
        instances through the frame's motion table)."""
        reference, despeckle, bloom, dof = params.pop("reference", None), params.pop("despeckle", None), params.pop("bloom", None), params.pop("dof", None)
        motion_blur = params.pop("motion_blur", None)
        self._denoise_guide_names(guides)
        if "depth" not in guides or "instance" not in guides:
            raise ValueError("render_animation reprojects through the depth AOV and the instance ids: guides must hold \"depth\" and \"instance\"")
        for out in self._temporal_frames(frames, strata_x, strata_y, depth, guides, samples_per_pass, temporal, params, motion_vectors, spatial, clip, display,
                                         upscale, reference, despeckle, bloom, dof, motion_blur):
            yield (out[:5] if motion_vectors else out[:4]) + (() if reference is None else out[5:])

    def _temporal_frames(self, frames, strata_x, strata_y, depth, guides, samples_per_pass, temporal, params, motion_vectors, spatial=None,
                         clip=None, display=None, upscale=None, reference=None, despeckle=None, bloom=None, dof=None, motion_blur=None):
        """The device chain of render_temporal and render_animation over (HostScene or None, Camera or None, seed) -> (denoised,
        accumulated, noisy, stats, motion vectors or None, CompareResult or None) per frame.  A scene that is given is uploaded and, from the second one on,
        brings its motion table; None keeps the uploaded scene (no table: only the camera moves).  The options are checked here, before
        anything is allocated; the first frame fixes the sizes (_sequence_buffers: with `upscale` the chain runs at the low size w x h,
        fw x fh is the full one); every frame is queued (_queue_frame), waited for once and read back (_read_frame)."""
        s = SimpleNamespace(guides=guides, kept=[n for n in TEMPORAL_GUIDES if n in guides], motion_vectors=motion_vectors, params=params,
                            tparams=dict(temporal or {}))
        TemporalParams.make(1, 1, **s.tparams)  # an unknown keyword fails here
        s.clip = _history_clip(clip)
        s.sparams = self._spatial_params(spatial, s.tparams, guides)
        s.dparams = _display_params(display)
        s.uparams = _upscale_params(upscale, guides)
        s.shown = "out" if s.uparams is None else "up"  # the buffer of a frame's first image
        s.reference, s.one_reference = _reference_frames(reference), isinstance(reference, np.ndarray)
        s.despeckle = _despeckle_params(despeckle)
        s.bloom = _bloom_params(bloom)
        s.dof = _dof_params(dof)
        s.mblur = _motion_blur_params(motion_blur)
        dev = None
        try:
            cam_prev = cam_full_prev = scene_prev = None
            for i, (scene, cam, seed) in enumerate(frames):
                table = None
                if scene is not None:
                    self.upload(scene)
                    if scene_prev is not None:
                        table = instance_motion(scene, scene_prev)
                    scene_prev = scene
                cam = Camera.from_buffer_copy(cam if cam is not None else self.scene.camera)  # (a scene's own camera lives in the scene)
                cam_full, tile = cam, None
                if s.uparams is not None:
                    cam = scaled_camera(cam_full, s.uparams[0])
                    tile = (0, 0, cam.width, cam.height)
                if dev is None:
                    s.fw, s.fh = self.scene.width, self.scene.height
                    s.w, s.h = (s.fw, s.fh) if s.uparams is None else (cam.width, cam.height)
                elif (self.scene.width, self.scene.height) != (s.fw, s.fh):
                    raise ValueError(f"frame {i} has a film of {self.scene.width} x {self.scene.height}, the sequence {s.fw} x {s.fh}")
                ref = None
                if s.reference is not None and not (s.one_reference and i):  # checked before anything is allocated or queued
                    ref = _reference_frame(s.reference, i, s.fw, s.fh)
                if s.dof is not None:
                    s.dof(i)  # a list shorter than the sequence fails here, before the frame is queued
                if s.mblur is not None:
                    s.mblur(i)  # likewise
                if dev is None:
                    dev = DeviceBuffers(_sequence_buffers(s.w, s.h, s.fw, s.fh, guides, motion_vectors, s.uparams is not None, s.dparams is not None,
                                                          s.reference is not None, s.despeckle is not None, s.bloom is not None, s.dof is not None,
                                                          s.mblur is not None), "a temporal sequence")
                if ref is not None:
                    dev.upload("reference", ref)  # the frame before has been waited for: nothing reads the buffer
                self._queue_frame(s, dev, i, self._params(strata_x, strata_y, depth, seed, tile, samples_per_pass), cam, cam_full, cam_prev, table,
                                  cam_full_prev)
                stats = self.collect_stats()  # waits for the stream
                cam_prev, cam_full_prev = cam, cam_full
                yield self._read_frame(s, dev, i, stats)
        finally:
            if dev is not None:
                dev.free()

    def _queue_frame(self, s, dev, i, p, cam, cam_full, cam_prev, table, cam_full_prev=None):
        """Frame i of the sequence `s` on the context's stream, nothing waits: the render of `p` with its guides and its variance; the
        despeckle step, into a colour buffer of its own and in place on the variance; the accumulation into this frame's ping-pong half against the other one; the motion vectors; the spatial variance estimate, in place
        on the accumulated variance; the filter; the full-size guides and the upsample; the depth of field of the frame's first image, into a
        colour buffer of its own; the motion blur of that (without the step: of the first image), into a colour buffer of its own, from
        the vectors against `cam_prev` (with `upscale`: `cam_full_prev`), a copy for the first frame; the bloom of that (without those
        steps: of the first image), into a colour buffer of its own; the display
        transform, which reads the last of the four that exists and whose exposure word is
        read from the second frame on and written by every one; the comparison of the frame's first image with its reference."""
        w, h, cur, old = s.w, s.h, i & 1, (i & 1) ^ 1
        gp = {n: dev.ptr(f"{n}{cur}" if n in s.kept else n) for n in s.guides}
        kept = {n: gp[n] for n in s.kept}  # what the next frame is tested against
        hist = [{n: dev.ptr(f"h_{n}{k}") for n in TEMPORAL_HISTORY} for k in (0, 1)]
        acc_variance = dev.ptr("acc_variance")
        self._render_var_device(dev, gp, p, cam)
        rgb = dev.ptr("rgb")
        if s.despeckle is not None:
            rgb = dev.ptr("despeckled")
            self.despeckle_device(dev.ptr("rgb"), rgb, w, h, dev.ptr("despeckle"), {"variance_in": dev.ptr(VARIANCE), "variance_out": dev.ptr(VARIANCE)},
                                  **s.despeckle)
        self.temporal_accumulate_device({"rgb": rgb, "variance": dev.ptr(VARIANCE), **kept}, hist[cur], w, h, cam, hist[old] if i else None,
                                        {n: dev.ptr(f"{n}{old}") for n in s.kept} if i else None, cam_prev, acc_variance,
                                        motion=table if i else None, clip=s.clip, **s.tparams)
        if s.motion_vectors and i:
            self.motion_vectors_device(gp["depth"], dev.ptr("motion"), w, h, cam, cam_prev, gp.get("instance") if table else None, table,
                                       dev.ptr("prev_depth"))
        if s.sparams is not None:
            self.spatial_variance_device(hist[cur]["moments"], hist[cur]["length"], acc_variance, acc_variance, w, h, kept, **s.sparams)
        self.denoise_var_device(hist[cur]["rgb"], dev.ptr("out"), w, h, acc_variance, gp, **s.params)
        if s.uparams is not None:
            self._upsample_out_device(dev, gp, s.guides, p.seed, s.fw, s.fh, *s.uparams, camera=cam_full)
        lit = s.shown  # what the next step of the chain reads: the first image, then the defocused one, then the bloomed one
        if s.dof is not None:
            self.dof_device(dev.ptr(lit), dev.ptr("depth_hi") if s.uparams is not None else gp["depth"], dev.ptr("dof"), s.fw, s.fh, **s.dof(i))
            lit = "dof"
        if s.mblur is not None:
            full = s.uparams is not None
            depth_ptr = dev.ptr("depth_hi") if full else gp["depth"]
            own = full or not s.motion_vectors  # (otherwise the chain's own vectors are this size and have been queued above)
            vectors = dev.ptr("mblur_motion" if own else "motion")
            if i and own:
                if full:
                    self.motion_vectors_device(depth_ptr, vectors, s.fw, s.fh, cam_full, cam_full_prev,
                                               (dev.ptr("instance_hi") if "instance" in s.guides else None) if table else None, table)
                else:
                    self.motion_vectors_device(depth_ptr, vectors, w, h, cam, cam_prev, gp.get("instance") if table else None, table)
            # frame 0 has no previous frame and no vectors: shutter 0 is the call's copy, which reads neither the depth nor the vectors
            self.motion_blur_device(dev.ptr(lit), depth_ptr, vectors, dev.ptr("mblur"), s.fw, s.fh, **(s.mblur(i) if i else dict(s.mblur(i), shutter=0.0)))
            lit = "mblur"
        if s.bloom is not None:
            self.bloom_device(dev.ptr(lit), dev.ptr("bloom"), s.fw, s.fh, **s.bloom)
            lit = "bloom"
        if s.dparams is not None:
            self.display_device(dev.ptr(lit), dev.ptr("display"), s.fw, s.fh,
                                {"exposure_in": dev.ptr("exposure") if i else None, "exposure_out": dev.ptr("exposure")}, **s.dparams)
        if s.reference is not None:
            self.compare_device(dev.ptr(s.shown), dev.ptr("reference"), s.fw, s.fh, dev.ptr("compare"))

    @staticmethod
    def _read_frame(s, dev, i, stats):
        """Frame i copied back, behind the wait -> (first image, accumulated, noisy, stats, motion vectors or None, CompareResult or
        None); the display image, its exposure and the low size go into `stats`."""
        w, h = s.w, s.h
        if s.dparams is not None:
            stats["display"] = dev.download("display", (s.fh, s.fw, 4), np.uint8, "a temporal sequence's display image")
            stats["exposure"] = dev.download("exposure", 1, np.float32, "a temporal sequence's display image")[0]
        if s.uparams is not None:
            stats["low_res"] = (w, h)
        if s.despeckle is not None:
            stats["despeckle"] = DespeckleResult.from_buffer_copy(dev.download("despeckle", C.sizeof(DespeckleResult), np.uint8, "a temporal sequence's despeckle record"))
        if s.dof is not None:
            stats["dof"] = dev.download("dof", (s.fh, s.fw, 3), np.float32, "a temporal sequence's defocused image")
        if s.mblur is not None:
            stats["motion_blur"] = dev.download("mblur", (s.fh, s.fw, 3), np.float32, "a temporal sequence's motion-blurred image")
        if s.bloom is not None:
            stats["bloom"] = dev.download("bloom", (s.fh, s.fw, 3), np.float32, "a temporal sequence's bloomed image")
        shapes = {s.shown: (h, w, 3) if s.uparams is None else (s.fh, s.fw, 3), f"h_rgb{i & 1}": (h, w, 3), "rgb": (h, w, 3)}
        shown, accumulated, noisy = (dev.download(n, shape, np.float32, "a temporal sequence's image") for n, shape in shapes.items())
        mv = None
        if s.motion_vectors:
            mv, wq = np.zeros((h, w, 2), dtype=np.float32), np.full((h, w), np.inf, dtype=np.float32)  # the first frame has no previous one
            if i:
                mv = dev.download("motion", mv.shape, np.float32, "the motion vectors")
                wq = dev.download("prev_depth", wq.shape, np.float32, "the motion vectors")
            if s.motion_vectors == "prev_depth":
                mv = np.concatenate([mv, wq[:, :, None]], axis=2)
        record = None
        if s.reference is not None:
            record = CompareResult.from_buffer_copy(dev.download("compare", C.sizeof(CompareResult), np.uint8, "a temporal sequence's comparison"))
        return shown, accumulated, noisy, stats, mv, record

    def collect_stats(self):
        st = Stats()
        self._check(self._L.pbrs_collect_stats(self._h, C.addressof(st)), "pbrs_collect_stats")
        return st.as_dict()

    def intersect(self, origins, dirs, tmax, closest=True, anyhit=True):
        origins = np.ascontiguousarray(origins, dtype=np.float32)
        dirs = np.ascontiguousarray(dirs, dtype=np.float32)
        tmax = np.ascontiguousarray(tmax, dtype=np.float32)
        n = len(tmax)
        hits = np.empty(n, dtype=HIT_DTYPE) if closest else None
        occ = np.empty(n, dtype=np.uint8) if anyhit else None
        self._check(self._L.pbrs_intersect_rays(self._h, n, origins.ctypes.data, dirs.ctypes.data, tmax.ctypes.data,
                                                hits.ctypes.data if closest else None, occ.ctypes.data if anyhit else None),
                    "pbrs_intersect_rays")
        return hits, occ

    def last_intersect_info(self):
        """Which walks the last intersect() went through (include/pbrs_gpu.h, pbrs_intersect_info)."""
        v = (C.c_uint32 * 4)()
        self._check(self._L.pbrs_last_intersect_info(self._h, C.addressof(v)), "pbrs_last_intersect_info")
        return {"wide_any": int(v[0]), "wide_closest": int(v[1]), "slow_any": int(v[2]), "slow_closest": int(v[3])}

    def camera_rays(self, sample, strata_x, strata_y, seed, tile=None):
        p = self._params(strata_x, strata_y, 1, seed, tile)
        o = np.empty((p.w * p.h, 3), dtype=np.float32)
        d = np.empty((p.w * p.h, 3), dtype=np.float32)
        self._check(self._L.pbrs_camera_rays(self._h, C.addressof(self.scene.camera), C.addressof(p), sample, o.ctypes.data, d.ctypes.data),
                    "pbrs_camera_rays")
        return o, d

    def sample_radiance(self, sample, strata_x, strata_y, depth, seed, tile=None, integrator="path"):
        p = self._params(strata_x, strata_y, depth, seed, tile, integrator=integrator)
        out = np.empty((p.h, p.w, 3), dtype=np.float32)
        self._check(self._L.pbrs_render_sample_radiance(self._h, C.addressof(self.scene.camera), C.addressof(p), sample, out.ctypes.data),
                    "pbrs_render_sample_radiance")
        return out

    def numeric_eval(self, fn, x, y=None):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(x)
        yp = None
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.float32)
            yp = y.ctypes.data
        self._check(self._L.pbrs_numeric_eval(self._h, NUMERIC_FNS[fn], x.size, x.ctypes.data, yp, out.ctypes.data), "pbrs_numeric_eval")
        return out

    def numeric_eval_k(self, fn, ops):
        """A function of more than two operands on the rows of `ops` (n x k, 32-bit words: float32 or uint32) -> n uint32 words."""
        ops = np.ascontiguousarray(ops)
        assert ops.ndim == 2 and ops.dtype.itemsize == 4
        out = np.empty(len(ops), dtype=np.uint32)
        self._check(self._L.pbrs_numeric_eval_k(self._h, NUMERIC_K_FNS[fn], ops.shape[0], ops.shape[1], ops.ctypes.data, out.ctypes.data),
                    "pbrs_numeric_eval_k")
        return out

    def bsdf_eval(self, op, queries, lambert=False):
        """src/bsdf.rs on the device for the rows of `queries` (n x 16 words: material index as uint32, then float32 normal, tangent, wo,
        wi, u, v and a spare word) against the uploaded scene -> n x 8 uint32 words (f, wi_out, pr, flags).  `lambert`: through the kernel
        specialised as k_shade's Lambert variants are (Lambert-only scenes)."""
        queries = np.ascontiguousarray(queries)
        assert queries.ndim == 2 and queries.shape[1] == BSDF_QUERY_WORDS and queries.dtype.itemsize == 4
        out = np.zeros((len(queries), BSDF_RESULT_WORDS), dtype=np.uint32)
        self._check(self._L.pbrs_bsdf_eval(self._h, BSDF_OPS[op], 1 if lambert else 0, len(queries), queries.ctypes.data, out.ctypes.data),
                    "pbrs_bsdf_eval")
        return out
