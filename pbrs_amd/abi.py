"""ctypes mirrors of the C ABI (include/pbrs_gpu.h, include/pbrs_host.h): the structures with their constructors, the name tables
of their planes, and the helpers that turn an option of the driver (api.py) into one of them.  Nothing here loads a library."""
import ctypes as C
import itertools
import math

import numpy as np


class Node(C.Structure):
    _fields_ = [("min", C.c_float * 3), ("a", C.c_uint32), ("max", C.c_float * 3), ("b", C.c_uint32)]


class SceneDesc(C.Structure):
    _fields_ = [("n_tlas_nodes", C.c_uint32), ("tlas_nodes", C.c_void_p), ("tlas_height", C.c_uint32),
                ("n_instances", C.c_uint32), ("instances", C.c_void_p),
                ("n_shapes", C.c_uint32), ("shapes", C.c_void_p),
                ("n_meshes", C.c_uint32), ("meshes", C.c_void_p),
                ("n_blas_nodes", C.c_uint32), ("blas_nodes", C.c_void_p),
                ("n_triangles", C.c_uint32), ("tri_verts", C.c_void_p), ("tri_shade", C.c_void_p),
                ("n_materials", C.c_uint32), ("materials", C.c_void_p),
                ("n_bxdfs", C.c_uint32), ("bxdfs", C.c_void_p),
                ("n_area_lights", C.c_uint32), ("area_lights", C.c_void_p),
                ("n_delta_lights", C.c_uint32), ("delta_lights", C.c_void_p),
                ("env_constant", C.c_float * 3), ("env_kind", C.c_uint32),
                ("n_textures", C.c_uint32), ("textures", C.c_void_p),
                ("n_tex_floats", C.c_uint32), ("tex_floats", C.c_void_p),
                ("n_tex_words", C.c_uint32), ("tex_words", C.c_void_p),
                ("env_texture", C.c_uint32), ("env_scale", C.c_float * 3),
                ("n_fourier_tables", C.c_uint32), ("fourier_tables", C.c_void_p)]


class Camera(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("width", C.c_uint32), ("c", C.c_float * 3), ("height", C.c_uint32),
                ("a", C.c_float * 3), ("pad0", C.c_float), ("b", C.c_float * 3), ("pad1", C.c_float)]


class Stats(C.Structure):
    _fields_ = ([(n, C.c_uint64) for n in (
        "samples", "closest_rays", "shadow_rays", "shade_events", "tlas_nodes", "blas_nodes", "instances", "instance_hits",
        "triangles", "tri_shading", "spheres", "quads", "cuboids", "disks", "shadow_tlas_nodes", "shadow_blas_nodes",
        "shadow_instances", "shadow_triangles", "shadow_prims", "invalid_samples")] +
                [(n, C.c_float) for n in ("ms_raygen", "ms_extend", "ms_shade", "ms_shadow", "ms_accumulate", "ms_total")] +
                [(n, C.c_uint32) for n in ("launches_extend", "launches_shadow", "launches_shade", "passes", "kernel_features_extend", "kernel_features_shadow")] +
                [("paths_at_bounce", C.c_uint64 * 16), ("shadow_rays_at_bounce", C.c_uint64 * 16)])

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n.endswith("_at_bounce") else getattr(self, n)) for n, _ in self._fields_}


class RenderParams(C.Structure):
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("strata_x", C.c_uint32),
                ("strata_y", C.c_uint32), ("max_depth", C.c_uint32), ("samples_per_pass", C.c_uint32), ("seed", C.c_uint64),
                ("collect_counters", C.c_uint32), ("time_stages", C.c_uint32),
                ("band_rows", C.c_uint32), ("band_count", C.c_uint32), ("band_index", C.c_uint32), ("integrator", C.c_uint32)]


class AovBuffers(C.Structure):
    """pbrs_aov_buffers: one pointer per first-hit AOV, NULL = not wanted (include/pbrs_gpu.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("albedo", "normal", "coverage", "depth", "instance", "material", "prim")]


# name -> (channels, dtype) of each AOV, in the order of pbrs_aov_buffers
AOVS = {"albedo": (3, np.float32), "normal": (3, np.float32), "coverage": (1, np.float32), "depth": (1, np.float32),
        "instance": (1, np.uint32), "material": (1, np.uint32), "prim": (1, np.uint32)}
AOV_NAMES = ("albedo", "normal", "depth", "instance", "material", "prim", "coverage")


VARIANCE = "variance"  # the variance AOV (pbrs_render_tile_aovs_var): (h, w) f32, a pointer of its own beside pbrs_aov_buffers


def _aov_names(aovs):
    names = tuple(aovs)
    unknown = [n for n in names if n not in AOVS and n != VARIANCE]
    if unknown:
        raise ValueError(f"unknown AOV name(s) {unknown}; known: {sorted(AOVS) + [VARIANCE]}")
    return names


class PixelFilter(C.Structure):
    """pbrs_pixel_filter (include/pbrs_gpu.h): kind, radius (x, y), a, b.  The constructors carry pbrt-v3's defaults."""
    BOX, TRIANGLE, GAUSSIAN, MITCHELL, LANCZOS = range(5)
    _fields_ = [("kind", C.c_uint32), ("radius", C.c_float * 2), ("a", C.c_float), ("b", C.c_float), ("pad", C.c_uint32)]

    @classmethod
    def make(cls, kind, rx, ry=None, a=0.0, b=0.0):
        f = cls()
        f.kind, f.radius[0], f.radius[1], f.a, f.b = kind, rx, rx if ry is None else ry, a, b
        return f

    @classmethod
    def box(cls, rx=0.5, ry=None):
        return cls.make(cls.BOX, rx, ry)

    @classmethod
    def triangle(cls, rx=2.0, ry=None):
        return cls.make(cls.TRIANGLE, rx, ry)

    @classmethod
    def gaussian(cls, rx=2.0, ry=None, alpha=2.0):
        return cls.make(cls.GAUSSIAN, rx, ry, alpha)

    @classmethod
    def mitchell(cls, rx=2.0, ry=None, B=1.0 / 3.0, C=1.0 / 3.0):
        return cls.make(cls.MITCHELL, rx, ry, B, C)

    @classmethod
    def lanczos(cls, rx=4.0, ry=None, tau=3.0):
        return cls.make(cls.LANCZOS, rx, ry, tau)

    def as_tuple(self):
        return (int(self.kind), float(self.radius[0]), float(self.radius[1]), float(self.a), float(self.b))

    def __repr__(self):
        names = ("box", "triangle", "gaussian", "mitchell", "lanczos")
        k = names[self.kind] if self.kind < len(names) else self.kind
        return f"PixelFilter({k}, radius=({self.radius[0]}, {self.radius[1]}), a={self.a}, b={self.b})"


class _DenoiseParamsMixin:
    """What DenoiseParams and DenoiseVarParams share: the flag bits, the defaults that follow the guides, as_dict."""
    DEMODULATE, ID_STOP = 1, 2
    MAX_ITERATIONS = 6

    @classmethod
    def _make(cls, w, h, iterations, sigmas, albedo_floor, demodulate, id_stop):
        p = cls()
        p.w, p.h, p.iterations = w, h, iterations
        p.flags = (cls.DEMODULATE if demodulate else 0) | (cls.ID_STOP if id_stop else 0)
        for (n, _), v in zip(cls._fields_[4:7], sigmas):
            setattr(p, n, v)
        p.albedo_floor = albedo_floor
        return p

    @classmethod
    def for_guides(cls, w, h, albedo=False, instance=False, **params):
        """The defaults for the guides at hand: demodulate when there is an albedo, stop at instance edges when there are ids."""
        params.setdefault("demodulate", bool(albedo))
        params.setdefault("id_stop", bool(instance))
        return cls.make(w, h, **params)

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DenoiseParams(_DenoiseParamsMixin, C.Structure):
    """pbrs_denoise_params (include/pbrs_gpu.h): image size, iterations, flags, the three sigmas and the albedo floor.  `make` carries
    the defaults ("Denoiser": chosen from the measured error ratios)."""
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("iterations", C.c_uint32), ("flags", C.c_uint32), ("sigma_color", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("albedo_floor", C.c_float)]

    @classmethod
    def make(cls, w, h, iterations=5, sigma_color=16.0, sigma_normal=0.3, sigma_depth=0.2, albedo_floor=1e-3, demodulate=False,
             id_stop=False):
        return cls._make(w, h, iterations, (sigma_color, sigma_normal, sigma_depth), albedo_floor, demodulate, id_stop)


class DenoiseGuides(C.Structure):
    """pbrs_denoise_guides: the AOV layouts, NULL = that stop is off."""
    _fields_ = [(n, C.c_void_p) for n in ("albedo", "normal", "depth", "instance")]


class DenoiseVarParams(_DenoiseParamsMixin, C.Structure):
    """pbrs_denoise_var_params (include/pbrs_gpu.h): DenoiseParams with sigma_luminance, a count of standard deviations (SVGF's 4),
    in the place of sigma_color."""
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("iterations", C.c_uint32), ("flags", C.c_uint32), ("sigma_luminance", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("albedo_floor", C.c_float)]

    @classmethod
    def make(cls, w, h, iterations=5, sigma_luminance=4.0, sigma_normal=0.3, sigma_depth=0.2, albedo_floor=1e-3, demodulate=False,
             id_stop=False):
        return cls._make(w, h, iterations, (sigma_luminance, sigma_normal, sigma_depth), albedo_floor, demodulate, id_stop)


class DenoiseVarGuides(C.Structure):
    """pbrs_denoise_var_guides: the four guides of DenoiseGuides and the variance, which is required."""
    _fields_ = [(n, C.c_void_p) for n in ("albedo", "normal", "depth", "instance", "variance")]


class MatteParams(C.Structure):
    """pbrs_matte_params (include/pbrs_gpu.h): what a hit is keyed by and how many (id, count) entries a pixel keeps."""
    INSTANCE, MATERIAL = 0, 1
    KEYS = {"instance": INSTANCE, "material": MATERIAL}
    MAX_SLOTS = 8
    MAX_SELECT = 4096
    _fields_ = [("key", C.c_uint32), ("slots", C.c_uint32)]

    @classmethod
    def make(cls, key="instance", slots=6):
        if key not in cls.KEYS:
            raise ValueError(f"unknown matte key {key!r}; known: {sorted(cls.KEYS)}")
        p = cls()
        p.key, p.slots = cls.KEYS[key], slots
        return p


class MatteBuffers(C.Structure):
    """pbrs_matte_buffers: ids and coverage, (h, w, slots) u32 / f32, ranked per pixel; residual (h, w) f32, NULL = not wanted."""
    _fields_ = [(n, C.c_void_p) for n in ("ids", "coverage", "residual")]


MATTE_LAYERS = ("ids", "coverage", "residual")


class PassBuffers(C.Structure):
    """pbrs_pass_buffers: direct and indirect light, (h, w, 3) f32, and the variance of each one's pixel mean, (h, w) f32; NULL = not
    wanted (include/pbrs_gpu.h, "light passes")."""
    _fields_ = [(n, C.c_void_p) for n in ("direct", "indirect", "direct_variance", "indirect_variance")]


# name -> channels of each light pass, in the order of pbrs_pass_buffers
PASSES = ("direct", "indirect", "direct_variance", "indirect_variance")
PASS_CHANNELS = {"direct": 3, "indirect": 3, "direct_variance": 1, "indirect_variance": 1}


def _pass_names(passes):
    names = tuple(passes)
    unknown = [n for n in names if n not in PASS_CHANNELS]
    if unknown:
        raise ValueError(f"unknown light pass(es) {unknown}; known: {list(PASSES)}")
    return names


class TemporalParams(C.Structure):
    """pbrs_temporal_params (include/pbrs_gpu.h, "temporal accumulation"): image size, flags, where the history length saturates, the
    two reprojection tolerances and the length from which the variance comes from the temporal moments."""
    ID_TEST = 1
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("flags", C.c_uint32), ("max_history", C.c_float), ("depth_tolerance", C.c_float),
                ("normal_tolerance", C.c_float), ("min_temporal", C.c_float), ("pad", C.c_uint32)]

    @classmethod
    def make(cls, w, h, max_history=32.0, depth_tolerance=0.05, normal_tolerance=0.3, min_temporal=4.0, id_test=False):
        p = cls()
        p.w, p.h, p.flags = w, h, cls.ID_TEST if id_test else 0
        p.max_history, p.depth_tolerance, p.normal_tolerance, p.min_temporal = max_history, depth_tolerance, normal_tolerance, min_temporal
        return p

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class TemporalFrame(C.Structure):
    """pbrs_temporal_frame: this frame's image, its variance AOV and its guides; rgb and depth are required."""
    _fields_ = [(n, C.c_void_p) for n in ("rgb", "variance", "depth", "normal", "instance")]


class TemporalGuides(C.Structure):
    """pbrs_temporal_guides: the previous frame's depth, normal and instance."""
    _fields_ = [(n, C.c_void_p) for n in ("depth", "normal", "instance")]


class TemporalHistory(C.Structure):
    """pbrs_temporal_history: accumulated colour (h, w, 3), luminance moments (h, w, 2) and history length (h, w), all f32."""
    _fields_ = [(n, C.c_void_p) for n in ("rgb", "moments", "length")]


class InstanceMotion(C.Structure):
    """pbrs_instance_motion (include/pbrs_gpu.h, "moving instances and motion vectors"): where a point of one instance was one frame
    ago (m, rows of an affine map), what that does to a normal (n) and IDENTITY = the record is not applied.  96 bytes."""
    IDENTITY = 1
    _fields_ = [("m", (C.c_float * 4) * 3), ("n", (C.c_float * 3) * 3), ("flags", C.c_uint32), ("pad", C.c_uint32 * 2)]


class HistoryClipParams(C.Structure):
    """pbrs_history_clip_params (include/pbrs_gpu.h, "history clipping"): the radius of the window whose colour box the reprojected
    history is clipped to, the box's half width in standard deviations, and the most history a clipped pixel keeps (+inf: all of it)."""
    MAX_RADIUS = 3
    _fields_ = [("radius", C.c_uint32), ("gamma", C.c_float), ("clip_history", C.c_float), ("flags", C.c_uint32)]

    @classmethod
    def make(cls, radius=1, gamma=1.0, clip_history=None):
        p = cls()
        p.radius, p.gamma, p.clip_history = radius, gamma, float("inf") if clip_history is None else clip_history
        return p

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def _history_clip(clip):
    """temporal_accumulate's `clip` -> a HistoryClipParams or None: None or False is the call without a clip, True the defaults, a dict
    HistoryClipParams.make's keywords (an unknown one fails here)."""
    if clip is None or clip is False:
        return None
    if isinstance(clip, HistoryClipParams):
        return clip
    if clip is True:
        return HistoryClipParams.make()
    if isinstance(clip, dict):
        return HistoryClipParams.make(**clip)
    raise ValueError("clip is None, True, a dict of HistoryClipParams.make's keywords or a HistoryClipParams")


class SpatialVarianceParams(C.Structure):
    """pbrs_spatial_variance_params (include/pbrs_gpu.h, "spatial variance estimate for short histories"): image size, the window's
    radius, flags, the two guide sigmas of the denoisers and the history length below which a pixel's variance is estimated."""
    ID_STOP, ONLY_UNKNOWN = 1, 2
    MAX_RADIUS = 3
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("radius", C.c_uint32), ("flags", C.c_uint32), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("min_temporal", C.c_float), ("pad", C.c_uint32)]

    @classmethod
    def make(cls, w, h, radius=3, sigma_normal=0.3, sigma_depth=0.2, min_temporal=4.0, id_stop=False, only_unknown=False):
        p = cls()
        p.w, p.h, p.radius = w, h, radius
        p.flags = (cls.ID_STOP if id_stop else 0) | (cls.ONLY_UNKNOWN if only_unknown else 0)
        p.sigma_normal, p.sigma_depth, p.min_temporal = sigma_normal, sigma_depth, min_temporal
        return p

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DisplayParams(C.Structure):
    """pbrs_display_params (include/pbrs_gpu.h, "display transform"): image size, tone curve, transfer function, quantiser, flags, the
    exposure, and what the auto exposure reads (key, exposure limits, adapt, the ranks kept); white is the Reinhard curve's."""
    CURVES = {"none": 0, "reinhard": 1, "aces": 2}
    ENCODES = {"sqrt": 0, "srgb": 1}
    QUANTIZERS = {"trunc": 0, "round": 1, "dither": 2}
    AUTO_EXPOSURE = 1
    BINS = 512
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("curve", C.c_uint32), ("encode", C.c_uint32), ("quantize", C.c_uint32),
                ("flags", C.c_uint32), ("exposure", C.c_float), ("key", C.c_float), ("white", C.c_float), ("min_exposure", C.c_float),
                ("max_exposure", C.c_float), ("adapt", C.c_float), ("low_q16", C.c_uint32), ("high_q16", C.c_uint32), ("pad", C.c_uint32 * 2)]

    @classmethod
    def make(cls, w, h, curve="aces", encode="srgb", quantize="round", auto=False, exposure=1.0, key=0.18, white=None, min_exposure=2.0 ** -20,
             max_exposure=2.0 ** 20, adapt=1.0, low_q16=6554, high_q16=62259):
        """The defaults are pbrs_display_params_default's; curve, encode and quantize by name (or by their number); white None = +inf."""
        p = cls()
        p.w, p.h = w, h
        p.curve = cls.CURVES[curve] if isinstance(curve, str) else curve
        p.encode = cls.ENCODES[encode] if isinstance(encode, str) else encode
        p.quantize = cls.QUANTIZERS[quantize] if isinstance(quantize, str) else quantize
        p.flags = cls.AUTO_EXPOSURE if auto else 0
        p.exposure, p.key, p.white = exposure, key, float("inf") if white is None else white
        p.min_exposure, p.max_exposure, p.adapt = min_exposure, max_exposure, adapt
        p.low_q16, p.high_q16 = low_q16, high_q16
        return p

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad"}


class UpsampleParams(C.Structure):
    """pbrs_upsample_params (include/pbrs_gpu.h, "guided upsampling"): the full size, the factor per axis, the tent's radius in low
    pixels, flags, the two guide sigmas of the denoisers, the albedo floor and the guided weight below which a pixel takes the plain
    tent."""
    DEMODULATE, ID_STOP = 1, 2
    FACTORS, RADII = (2, 3, 4), (1, 2)
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("factor", C.c_uint32), ("radius", C.c_uint32), ("flags", C.c_uint32),
                ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("albedo_floor", C.c_float), ("min_weight", C.c_float),
                ("pad", C.c_uint32 * 3)]

    @classmethod
    def make(cls, w, h, factor=2, radius=1, sigma_normal=0.3, sigma_depth=0.2, albedo_floor=1e-3, min_weight=1e-3, demodulate=False,
             id_stop=False):
        """The defaults are pbrs_upsample_params_default's."""
        p = cls()
        p.w, p.h, p.factor, p.radius = w, h, factor, radius
        p.flags = (cls.DEMODULATE if demodulate else 0) | (cls.ID_STOP if id_stop else 0)
        p.sigma_normal, p.sigma_depth, p.albedo_floor, p.min_weight = sigma_normal, sigma_depth, albedo_floor, min_weight
        return p

    @classmethod
    def for_guides(cls, w, h, factor, albedo=False, instance=False, **params):
        """make() with the image demodulated when there is an albedo pair and taps stopped at id edges when there is an instance pair,
        unless `params` says otherwise."""
        params.setdefault("demodulate", bool(albedo))
        params.setdefault("id_stop", bool(instance))
        return cls.make(w, h, factor, **params)

    @property
    def low_size(self):
        return (self.w + self.factor - 1) // self.factor, (self.h + self.factor - 1) // self.factor

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad"}


def scaled_camera(camera, factor):
    """`camera` for a film of 1 / factor of the resolution per axis -> a new Camera: width and height rounded up, the pixel steps a and b
    multiplied in f32 by (float)factor, c and center kept.  A low pixel then sees exactly its factor x factor full pixels for factor 2
    and 4; for factor 3 the products round, and that is the definition."""
    factor = int(factor)
    if factor < 1:
        raise ValueError("the factor is a positive integer")
    cam = Camera.from_buffer_copy(camera)
    cam.width, cam.height = (camera.width + factor - 1) // factor, (camera.height + factor - 1) // factor
    f = np.float32(factor)
    for k in range(3):
        cam.a[k] = np.float32(camera.a[k]) * f
        cam.b[k] = np.float32(camera.b[k]) * f
    return cam


def _upscale_params(upscale, guides):
    """render_temporal's / render_animation's `upscale` -> (factor, UpsampleParams.for_guides' keywords), or None: None is the sequence
    at full resolution, an int the factor, a dict UpsampleParams.make's keywords plus "factor" (2 unless given).  Demodulation follows
    the albedo guide and the id stop the instance guide unless the dict says otherwise.  An unknown keyword fails here."""
    if upscale is None or upscale is False:
        return None
    if isinstance(upscale, dict):
        up = dict(upscale)
        factor = int(up.pop("factor", 2))
    elif isinstance(upscale, (int, np.integer)) and not isinstance(upscale, bool):
        up, factor = {}, int(upscale)
    else:
        raise ValueError("upscale is None, a factor or a dict of UpsampleParams.make's keywords plus \"factor\"")
    if factor not in UpsampleParams.FACTORS:
        raise ValueError(f"the upscale factor is one of {UpsampleParams.FACTORS}, not {factor}")
    UpsampleParams.for_guides(1, 1, factor, "albedo" in guides, "instance" in guides, **up)
    return factor, up


class DisplayIO(C.Structure):
    """pbrs_display_io: the previous exposure (one float), where this call's goes, where the 512 histogram counts go; each may be NULL."""
    _fields_ = [(n, C.c_void_p) for n in ("exposure_in", "exposure_out", "histogram_out")]


def _display_params(display):
    """render_temporal's / render_animation's `display` -> DisplayParams.make's keywords, or None: None or False is the sequence
    without a display transform, True the defaults with the auto exposure, a dict the keywords (auto=True unless it says otherwise).  An
    unknown keyword fails here."""
    if display is None or display is False:
        return None
    if display is not True and not isinstance(display, dict):
        raise ValueError("display is None, True or a dict of DisplayParams.make's keywords")
    dp = {} if display is True else dict(display)
    dp.setdefault("auto", True)
    DisplayParams.make(1, 1, **dp)
    return dp


class CompareParams(C.Structure):
    """pbrs_compare_params (include/pbrs_gpu.h, "image comparison"): image size, the transform both images go through, flags, the floor
    of the relative error and SSIM's peak."""
    TRANSFORMS = {"linear": 0, "reinhard": 1}
    SSIM = 1
    TILE = 16
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("transform", C.c_uint32), ("flags", C.c_uint32), ("rel_epsilon", C.c_float),
                ("peak", C.c_float), ("pad", C.c_uint32 * 2)]

    @classmethod
    def make(cls, w, h, transform="reinhard", ssim=True, rel_epsilon=1e-2, peak=1.0):
        """The defaults are pbrsx_compare_params_default's; transform by name (or by its number)."""
        p = cls()
        p.w, p.h = w, h
        p.transform = cls.TRANSFORMS[transform] if isinstance(transform, str) else transform
        p.flags = cls.SSIM if ssim else 0
        p.rel_epsilon, p.peak = rel_epsilon, peak
        return p

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad"}


class CompareMaps(C.Structure):
    """pbrs_compare_maps: where the per-pixel squared error and the per-pixel SSIM go ((h, w) f32 each); each may be NULL."""
    _fields_ = [(n, C.c_void_p) for n in ("error_out", "ssim_out")]


class CompareResult(C.Structure):
    """pbrs_compare_result: the means over the valid pixels, the largest difference, and the counts."""
    _fields_ = [("mse", C.c_double), ("rel_mse", C.c_double), ("mae", C.c_double), ("ssim", C.c_double), ("max_abs", C.c_double),
                ("n_valid", C.c_uint32), ("n_invalid", C.c_uint32), ("n_ssim", C.c_uint32), ("pad", C.c_uint32 * 3)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad"}

    def psnr(self, peak=1.0):
        """10 log10(peak^2 / mse) in dB: +inf for identical images, NaN where there was no valid pixel."""
        if not self.mse > 0.0:
            return float("inf") if self.mse == 0.0 else float("nan")
        return 10.0 * math.log10(peak * peak / self.mse)


def _reference_frames(reference):
    """render_temporal's / render_animation's `reference` -> an iterator of one image per frame, or None: a single (h, w, 3) array
    stands for every frame, anything else is iterated.  A single array of another rank or channel count fails here."""
    if reference is None:
        return None
    if isinstance(reference, np.ndarray):
        if reference.ndim != 3 or reference.shape[2] != 3:
            raise ValueError(f"the reference is (h, w, 3), not {reference.shape}")
        return itertools.repeat(reference)
    return iter(reference)


def _reference_frame(frames, i, w, h):
    """Frame i's reference out of _reference_frames' iterator, as a contiguous (h, w, 3) f32 array."""
    try:
        ref = np.ascontiguousarray(next(frames), dtype=np.float32)
    except StopIteration:
        raise ValueError(f"the reference ends before frame {i}") from None
    if ref.shape != (h, w, 3):
        raise ValueError(f"frame {i}'s reference is ({h}, {w}, 3), not {ref.shape}")
    return ref


class DespeckleParams(C.Structure):
    """pbrs_despeckle_params (include/pbrs_gpu.h, "despeckle"): image size, the window's radius, the order statistic of the neighbours'
    luminances, the factor on it and the additive floor of the limit."""
    CLAMPED, REPAIRED = 1, 2  # mask_out's bits
    TILE = 16
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("radius", C.c_uint32), ("rank", C.c_uint32), ("gain", C.c_float), ("floor", C.c_float),
                ("flags", C.c_uint32), ("pad", C.c_uint32)]

    @classmethod
    def make(cls, w, h, radius=1, rank=2, gain=2.0, floor=0.0):
        """The defaults are pbrsi_despeckle_params_default's."""
        p = cls()
        p.w, p.h = w, h
        p.radius, p.rank, p.gain, p.floor = radius, rank, gain, floor
        return p

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad"}


DESPECKLE_PLANES = ("rgb_in", "rgb_out", "variance_in", "variance_out", "mask_out", "removed_out")


class DespeckleIO(C.Structure):
    """pbrs_despeckle_io: the image in and out ((h, w, 3) f32), the variance pair ((h, w) f32, both or neither), the mask ((h, w) u32) and
    the removed energy ((h, w, 3) f32); the last four may be NULL."""
    _fields_ = [(n, C.c_void_p) for n in DESPECKLE_PLANES]


class DespeckleResult(C.Structure):
    """pbrs_despeckle_result: how many pixels were clamped and how many repaired."""
    _fields_ = [("n_clamped", C.c_uint32), ("n_repaired", C.c_uint32), ("pad", C.c_uint32 * 2)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad"}


def _despeckle_params(despeckle):
    """render_temporal's / render_animation's `despeckle` -> DespeckleParams.make's keywords, or None: None or False is the sequence
    without the step, True the defaults, a dict the keywords.  An unknown keyword fails here."""
    if despeckle is None or despeckle is False:
        return None
    if despeckle is not True and not isinstance(despeckle, dict):
        raise ValueError("despeckle is None, True or a dict of DespeckleParams.make's keywords")
    dp = {} if despeckle is True else dict(despeckle)
    DespeckleParams.make(1, 1, **dp)
    return dp


class BloomParams(C.Structure):
    """pbrs_bloom_params (include/pbrs_gpu.h, "bloom"): image size, the pyramid's levels, the bright pass's threshold and soft knee, the
    strength of the composite and how much of each coarser level reaches the finer one."""
    MIX = 1  # flags: out = rgb + strength * (B - rgb)
    MAX_LEVELS = 8
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("levels", C.c_uint32), ("flags", C.c_uint32), ("threshold", C.c_float), ("knee", C.c_float),
                ("strength", C.c_float), ("spread", C.c_float)]

    @classmethod
    def make(cls, w, h, levels=6, threshold=1.0, knee=0.5, strength=0.05, spread=0.6, mix=False):
        """The defaults are pbrsb_bloom_params_default's."""
        p = cls()
        p.w, p.h = w, h
        p.levels, p.flags = levels, cls.MIX if mix else 0
        p.threshold, p.knee, p.strength, p.spread = threshold, knee, strength, spread
        return p

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def _bloom_params(bloom):
    """render_temporal's / render_animation's `bloom` -> BloomParams.make's keywords, or None: None or False is the sequence without the
    step, True the defaults, a dict the keywords.  An unknown keyword fails here."""
    if bloom is None or bloom is False:
        return None
    if bloom is not True and not isinstance(bloom, dict):
        raise ValueError("bloom is None, True or a dict of BloomParams.make's keywords")
    bp = {} if bloom is True else dict(bloom)
    BloomParams.make(1, 1, **bp)
    return bp


class DofParams(C.Structure):
    """pbrs_dof_params (include/pbrs_gpu.h, "depth of field"): image size, the largest blur radius (also the gather's reach), the depth
    AOV's value that is sharp and the blur radius in pixels of a point at infinity."""
    MAX_RADIUS = 16
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("max_radius", C.c_uint32), ("flags", C.c_uint32), ("focus", C.c_float), ("scale", C.c_float),
                ("reserved", C.c_uint32 * 2)]

    @classmethod
    def make(cls, w, h, max_radius=8, focus=1.0, scale=0.0):
        """The defaults are pbrsf_dof_params_default's; api.lens(camera, focus_distance, lens_radius) gives focus and scale."""
        p = cls()
        p.w, p.h = w, h
        p.max_radius, p.focus, p.scale = max_radius, focus, scale
        return p

    def as_dict(self):
        return {"w": self.w, "h": self.h, "max_radius": self.max_radius, "flags": self.flags, "focus": self.focus, "scale": self.scale}


def lens(camera, focus_distance, lens_radius):
    """A thin lens in front of the pinhole `camera` (a Camera) -> {"focus": ..., "scale": ...}, DofParams.make's keywords: the plane at
    `focus_distance` along the view axis (world units) is sharp, and `lens_radius` is the aperture's radius (world units).  The depth
    AOV is the ray parameter t of the direction c + a x + b y, whose component along the view axis n = normalize(cross(a, b)) is
    D = |dot(c, n)| for every pixel: focus = focus_distance / D.  A point at depth z spreads over a circle of the world radius
    lens_radius |z - F| / z on the plane of focus, where one pixel step is |a| focus: scale = lens_radius / (|a| focus).  Computed in
    f64 and rounded once.  With `upscale`, pass the full-size camera."""
    a, b, c = (np.array(list(v), dtype=np.float64) for v in (camera.a, camera.b, camera.c))
    n = np.cross(a, b)
    norm = float(np.sqrt(n @ n))
    if not (norm > 0.0 and np.isfinite(norm)):
        raise ValueError("the camera's a and b do not span an image plane")
    D = abs(float(c @ (n / norm)))
    if not (D > 0.0 and focus_distance > 0.0 and lens_radius >= 0.0 and np.isfinite(focus_distance) and np.isfinite(lens_radius)):
        raise ValueError("lens takes a camera that looks along its axis, a focus_distance > 0 and a lens_radius >= 0")
    focus = float(focus_distance) / D
    scale = float(lens_radius) / (float(np.sqrt(a @ a)) * focus)
    return {"focus": float(np.float32(focus)), "scale": float(np.float32(scale))}


def _dof_params(dof):
    """render_temporal's / render_animation's `dof` -> a function frame index -> DofParams.make's keywords, or None: None or False is
    the sequence without the step, a dict the keywords of every frame, a list or tuple of dicts one per frame (a focus pull; a sequence
    longer than the list fails at the frame that has none).  An unknown keyword fails here."""
    if dof is None or dof is False:
        return None
    per_frame = isinstance(dof, (list, tuple))
    if not (isinstance(dof, dict) or (per_frame and len(dof) and all(isinstance(d, dict) for d in dof))):
        raise ValueError("dof is None, a dict of DofParams.make's keywords or a list of such dicts, one per frame")
    frames = [dict(d) for d in (dof if per_frame else [dof])]
    for d in frames:
        DofParams.make(1, 1, **d)

    def of_frame(i):
        if not per_frame:
            return frames[0]
        if i >= len(frames):
            raise ValueError(f"dof holds {len(frames)} frames' keywords: none for frame {i}")
        return frames[i]
    return of_frame


class MotionBlurParams(C.Structure):
    """pbrs_motion_blur_params (include/pbrs_gpu.h, "motion blur"): image size, the longest half-exposure vector in pixels (also the
    gather's reach), the taps along the line, the jitter flag, the open fraction of the frame interval and the relative depth
    difference over which a tap goes from level to behind."""
    MAX_RADIUS, MAX_TAPS, JITTER = 16, 64, 1
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("max_radius", C.c_uint32), ("taps", C.c_uint32), ("flags", C.c_uint32), ("shutter", C.c_float),
                ("z_rel", C.c_float), ("reserved", C.c_uint32)]

    @classmethod
    def make(cls, w, h, max_radius=16, taps=16, jitter=False, shutter=0.5, z_rel=0.05):
        """The defaults are pbrsm_motion_blur_params_default's."""
        p = cls()
        p.w, p.h = w, h
        p.max_radius, p.taps, p.flags, p.shutter, p.z_rel = max_radius, taps, cls.JITTER if jitter else 0, shutter, z_rel
        return p

    def as_dict(self):
        return {"w": self.w, "h": self.h, "max_radius": self.max_radius, "taps": self.taps, "flags": self.flags, "shutter": self.shutter, "z_rel": self.z_rel}


def _motion_blur_params(motion_blur):
    """render_temporal's / render_animation's `motion_blur` -> a function frame index -> MotionBlurParams.make's keywords, or None: None
    or False is the sequence without the step, True the defaults, a dict the keywords of every frame, a list or tuple of dicts one per
    frame (a sequence longer than the list fails at the frame that has none).  An unknown keyword fails here."""
    if motion_blur is None or motion_blur is False:
        return None
    if motion_blur is True:
        motion_blur = {}
    per_frame = isinstance(motion_blur, (list, tuple))
    if not (isinstance(motion_blur, dict) or (per_frame and len(motion_blur) and all(isinstance(d, dict) for d in motion_blur))):
        raise ValueError("motion_blur is None, True, a dict of MotionBlurParams.make's keywords or a list of such dicts, one per frame")
    frames = [dict(d) for d in (motion_blur if per_frame else [motion_blur])]
    for d in frames:
        MotionBlurParams.make(1, 1, **d)

    def of_frame(i):
        if not per_frame:
            return frames[0]
        if i >= len(frames):
            raise ValueError(f"motion_blur holds {len(frames)} frames' keywords: none for frame {i}")
        return frames[i]
    return of_frame


class SpatialVarianceGuides(C.Structure):
    """pbrs_spatial_variance_guides: depth, normal and instance of the frame; each may be NULL."""
    _fields_ = [(n, C.c_void_p) for n in ("depth", "normal", "instance")]


# name -> (channels, dtype) of the planes of each struct above
TEMPORAL_FRAME = {"rgb": (3, np.float32), "variance": (1, np.float32), "depth": (1, np.float32), "normal": (3, np.float32),
                  "instance": (1, np.uint32)}
TEMPORAL_GUIDES = {n: TEMPORAL_FRAME[n] for n in ("depth", "normal", "instance")}
TEMPORAL_HISTORY = {"rgb": (3, np.float32), "moments": (2, np.float32), "length": (1, np.float32)}
SPATIAL_VARIANCE_PLANES = {"moments": (2, np.float32), "length": (1, np.float32), "variance": (1, np.float32)}


def _temporal_struct(cls, layout, ptrs, what):
    """The ctypes struct `cls` from {name: pointer} (None entries: NULL)."""
    s = cls()
    for n, ptr in dict(ptrs).items():
        if n not in layout:
            raise ValueError(f"unknown {what} plane {n!r}; known: {list(layout)}")
        setattr(s, n, ptr)
    return s


def _matte_select(select):
    """The selected ids as pbrs_matte_mask wants them: u32, strictly ascending (sorted and deduplicated here)."""
    sel = np.unique(np.asarray(select, dtype=np.int64).reshape(-1))
    if sel.size and (sel[0] < 0 or sel[-1] > 0xFFFFFFFF):
        raise ValueError("a selected id is not a u32")
    return np.ascontiguousarray(sel, dtype=np.uint32)


DENOISE_GUIDES = {"albedo": (3, np.float32), "normal": (3, np.float32), "depth": (1, np.float32), "instance": (1, np.uint32)}

HIT_DTYPE = np.dtype([("t", np.float32), ("inst", np.uint32), ("prim", np.uint32), ("b1", np.float32), ("b2", np.float32)])
NUMERIC_FNS = {"sin": 0, "cos": 1, "tan": 2, "atan": 3, "atan2": 4, "acos": 5, "exp": 6, "ln": 7, "hypot": 8, "div": 9,
               "sqrt": 10, "asin": 11, "powi": 12, "fract": 13, "floor": 14, "box_quotient": 15, "trunc": 16, "f32_to_i32": 17, "ldexp": 18, "max": 19,
               "min": 20, "signum": 21, "weak_recip": 22, "sincos64_sin_hi": 23, "sincos64_sin_lo": 24, "sincos64_cos_hi": 25,
               "sincos64_cos_lo": 26, "rng_u32": 27, "rng_f32": 28}
# include/pbrs_numeric_probe.h: ids from 16 on return raw 32-bit words (view the result as uint32 where it is no f32)
NUMERIC_K_FNS = {"mul_add": 0, "clamp": 1, "slab_filter": 2, "rng_init_lo": 3, "rng_init_hi": 4, "rng_stream_u32": 5, "rng_stream_f32": 6}
# include/pbrs_gpu.h: PBRS_BSDF_EVAL .. _SAMPLE_SPECULAR; a query is 16 words, a result 8
BSDF_OPS = {"eval": 0, "pdf": 1, "sample": 2, "sample_specular": 3}
BSDF_QUERY_WORDS, BSDF_RESULT_WORDS = 16, 8


def _motion_args(motion):
    """(pointer, record count) of a motion table: a ctypes array of InstanceMotion, or None."""
    if motion is None:
        return None, 0
    if not isinstance(motion, C.Array) or motion._type_ is not InstanceMotion:
        raise ValueError("a motion table is a ctypes array of InstanceMotion (api.instance_motion)")
    return C.addressof(motion), len(motion)


INTEGRATORS = {"path": 0, "direct": 1, "materials": 2, "normals": 3}  # PBRS_INTEGRATOR_*
