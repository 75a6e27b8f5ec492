#!/usr/bin/env python3
"""Renders a pbrt-v3 scene file on the GPU and writes an EXR (or PNG):  tools/render_pbrt.py scene.pbrt out.exr [msaa] [depth] [path|direct|materials|normals] [--aovs] [--pixel-filter] [--denoise [--denoise-iterations N] [--denoise-sigma c,n,d]] [--denoise-var [--denoise-sigma-luminance X]] [--matte instance|material [--matte-slots N] [--matte-select i,j,...]] [--passes] [--denoise-passes] [--frames N [--orbit DEG] [--temporal] [--spatial-variance] [--spin ID[,ID...] --spin-deg DEG] [--motion-vectors]] [--display none|reinhard|aces [--encode sqrt|srgb] [--auto-exposure] [--exposure X]] [--compare-strata N] [--despeckle [--despeckle-gain X] [--despeckle-rank K] [--despeckle-radius R]]

--aovs: also writes the first-hit AOVs of the same samples (include/pbrs_gpu.h, pbrs_aov_buffers) beside the image, for a denoiser:
<out>.albedo.exr, <out>.normal.exr and <out>.depth.exr (depth in all three channels; +inf where no sample hits).
--pixel-filter: reconstructs the image with the file's `Filter` (include/pbrs_gpu.h, pbrs_render_tile_filtered) instead of the plain
per-pixel mean; the AOVs stay per-pixel means (a separate render of the same samples).
--denoise: also writes <out>.denoised.<ext>, the image through the edge-avoiding a-trous denoiser (include/pbrs_gpu.h, pbrs_denoise)
guided by the albedo, normal, depth and instance AOVs of the same samples; --denoise-iterations (default 5) and --denoise-sigma
(colour, normal, depth) override Context.denoise's defaults.
--denoise-var: also writes <out>.denoised_var.<ext>, the image through the variance-guided denoiser (include/pbrs_gpu.h,
pbrs_denoise_var) with the variance AOV of the same samples: no sigma depends on the units of the scene.  --denoise-sigma-luminance
(default 4, in standard deviations) overrides Context.denoise_var's default; --denoise-iterations and the normal and depth sigmas of
--denoise-sigma apply to it too.
--matte instance|material: also writes <out>.matte.npz, the id matte of the same samples (include/pbrs_gpu.h, pbrs_render_tile_matte):
`ids` (h, w, slots) u32, `coverage` (h, w, slots) f32, `residual` (h, w) f32 — per pixel the ids ranked by the share of the pixel each
covers (an .npz because the EXR writer holds RGB f32 only and cannot hold ids).  --matte-slots (default 6, at most 8) is the number of
ids kept per pixel.  --matte-select i,j,...: also writes <out>.mask.png, the anti-aliased mask of those ids (pbrs_matte_mask).
--passes: also writes <out>.direct.exr and <out>.indirect.exr, the light of the same samples that reaches the camera after one path
vertex and after more (include/pbrs_gpu.h, pbrs_render_tile_passes; the path integrator only).
--denoise-passes: also writes <out>.denoised_passes.<ext>: direct and indirect light each through the variance-guided denoiser with its
own variance, summed again (pbrs_combine_passes); --denoise-var's parameters apply.
--frames N: a sequence of N frames instead of one image, frame k with the seed 1 + k and the camera turned by k * DEG degrees (--orbit,
default 0) about the file's look-at point around its up vector; one image per frame, <out>.0000.<ext>, <out>.0001.<ext>, ...  (the path
integrator; the other options above do not apply).  With --temporal every frame is accumulated over the frames before it and filtered
(include/pbrs_gpu.h, pbrs_temporal_accumulate; Context.render_temporal): the frame's image is then the accumulated and filtered one,
and <out>.NNNN.accumulated.<ext> and <out>.NNNN.noisy.<ext> are written beside it; --denoise-var's parameters apply.
--spin ID[,ID...] --spin-deg DEG (with --frames and --temporal): the named instances (ids as the instance AOV counts them; mesh instances)
turn by DEG degrees per frame about the vertical axis through the centre of their world box; every frame's scene is uploaded and the
accumulation follows the instances through a motion table (Context.render_animation; include/pbrs_gpu.h, pbrs_temporal_accumulate_motion).
--motion-vectors (with --temporal): also writes <out>.NNNN.motion.exr per frame, the screen-space motion vectors (pbrs_motion_vectors):
x and y in R and G (where the pixel's surface point was one frame ago minus where it is, in pixels), the previous depth in B.
--spatial-variance (with --temporal): pixels whose history is shorter than the accumulation's min_temporal (the first frames, and
disocclusions later) are filtered with a variance estimated over their neighbourhood instead of an unknown one (include/pbrs_gpu.h,
pbrs_spatial_variance; render_temporal's spatial=True).
--history-clip GAMMA [--history-clip-radius R] (with --temporal): the reprojected history is clipped to mean +- GAMMA * sigma of the
frame's colours over the (2 R + 1)^2 window around the pixel (R 1 .. 3, default 1) before the blend, so that shadows of moving instances
and lights that change do not lag (include/pbrs_gpu.h, pbrs_temporal_accumulate_clip; render_temporal's clip=).
--display CURVE: also writes <out>.display.png, the image through the display transform on the GPU (include/pbrs_gpu.h, pbrs_display): the
exposure (--exposure X, default 1; with --auto-exposure the trimmed log-average luminance is mapped to 0.18 and X is a compensation on
top), the tone curve, the transfer function (--encode, default srgb) and rounding to 8 bits; the file holds the GPU's bytes.  With
--frames N --temporal every frame's filtered image goes through it on the frame's stream (render_temporal's display=) and
<out>.NNNN.display.png is written; the auto exposure then eases from frame to frame.
--upscale F [--upscale-radius R]: the frame traced and filtered at 1 / F of the resolution per axis (F 2 .. 4) and rebuilt at full size by
guided upsampling (include/pbrs_gpu.h, pbrs_upsample; R 1 .. 2, default 1: the tent's half-width in low pixels) with full-size guides of one
sample per pixel: also writes <out>.upscaled.<ext> and <out>.upscaled_low.<ext> (Context.render_upscaled; --denoise-var's parameters apply
to the low-resolution filter).  With --frames N --temporal the sequence itself runs at low resolution (render_temporal's upscale=) and
<out>.NNNN.<ext> is the full-size image.  --msaa counts samples per traced, low-resolution pixel.
--compare-strata N (one image, not --frames): also renders a reference at N x N strata (seed 4242) and prints, as one JSON line, what the
library's comparison (include/pbrs_gpu.h, pbrsx_compare; Context.compare's defaults) says of the produced image against it: mse, rel_mse,
mae, ssim, max_abs, psnr_db and the counts, under "image", and likewise under "upscaled", "denoised" and "denoised_var" where those are
produced.
--despeckle [--despeckle-gain X] [--despeckle-rank K] [--despeckle-radius R]: fireflies clamped to X (>= 1, default 2) times the K-th
brightest (1 .. 4, default 2) of the neighbours within R pixels (1 .. 2, default 1) and non-finite pixels rebuilt from their neighbours
(include/pbrs_gpu.h, pbrsi_despeckle; the flag itself takes no value): also writes <out>.despeckled.<ext> and prints how many pixels were clamped and
repaired and the mean energy removed; with --denoise-var also <out>.despeckled_denoised_var.<ext>, the filter behind the step on the
despeckled image and variance.  With --frames N --temporal every frame is despeckled between its render and the accumulation
(render_temporal's despeckle=).  --compare-strata scores "despeckled" and "despeckled_denoised_var" as well.
--bloom [--bloom-threshold T] [--bloom-strength S] [--bloom-levels N] [--bloom-mix]: glare on linear radiance (include/pbrs_gpu.h,
pbrsb_bloom; the flag itself takes no value): the part of the image above the luminance T (default 1; 0 = the whole image) goes down a
pyramid of N levels (1 .. 8, default 6), comes back up and is added to the image S times (default 0.05), or mixed into it
(--bloom-mix: out = rgb + S (B - rgb), for T = 0 and S <= 1): also writes <out>.bloom.<ext>, and --display then shows the bloomed image.
With --frames N --temporal every frame's first image is bloomed behind the filter (render_temporal's bloom=), <out>.NNNN.bloom.<ext>.
--dof-focus D --dof-lens-radius A [--dof-max-radius R]: depth of field as an image operation (include/pbrs_gpu.h, pbrsf_dof): a thin lens
of the aperture radius A (world units) focused on the plane at the distance D along the view axis (world units; api.lens turns both into
the call's focus and scale), the circles clamped to R pixels (1 .. 16, default 8), from the depth AOV of the same samples: also writes
<out>.dof.<ext>; --bloom and --display then act on the defocused image.  --dof-focus-pixel X Y in the place of --dof-focus focuses on
what pixel (X, Y) shows (one image only).  With --frames N --temporal every frame's first image is defocused behind the filter and the
upsample (render_temporal's dof=), <out>.NNNN.dof.<ext>.
--motion-blur [--shutter S] [--motion-blur-taps N] [--motion-blur-radius R] [--motion-blur-jitter] (with --frames N --temporal; the flag
itself takes no value): a shutter as an image operation (include/pbrs_gpu.h, pbrsm_motion_blur; render_temporal's motion_blur=): every
frame from the second on is smeared along its motion vectors against the frame before (the camera's orbit, and with --spin the
instances'), open for the fraction S of the frame interval (0 .. 1, default 0.5), N taps along the line (2 .. 64, default 16), the
vectors clamped to R pixels (1 .. 16, default 16), behind the depth of field and in front of the bloom: also writes
<out>.NNNN.motion_blur.<ext>; --bloom and --display then act on the blurred image."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pbrs_amd

temporal = "--temporal" in sys.argv
motion_vectors = "--motion-vectors" in sys.argv
spatial_variance = "--spatial-variance" in sys.argv
history_clip = None  # HistoryClipParams.make's keywords
display = None  # DisplayParams.make's keywords
upscale = None  # UpsampleParams.make's keywords plus "factor"
auto_exposure = "--auto-exposure" in sys.argv
spin, spin_deg = [], 0.0
aovs = "--aovs" in sys.argv
filtered = "--pixel-filter" in sys.argv
denoise = "--denoise" in sys.argv
denoise_var = "--denoise-var" in sys.argv
passes = "--passes" in sys.argv
denoise_passes = "--denoise-passes" in sys.argv
denoise_params, denoise_var_params = {}, {}
matte_key, matte_slots, matte_select = None, 6, None
frames, orbit = 0, 0.0
compare_strata = 0
despeckle = None  # DespeckleParams.make's keywords
if "--despeckle" in sys.argv:  # takes no value: a number behind it would be indistinguishable from msaa and depth
    sys.argv.remove("--despeckle")
    despeckle = {}
bloom = None  # BloomParams.make's keywords
if "--bloom" in sys.argv:  # takes no value, like --despeckle
    sys.argv.remove("--bloom")
    bloom = {}
if "--bloom-mix" in sys.argv:
    sys.argv.remove("--bloom-mix")
    if bloom is None:
        sys.exit("--bloom-mix goes with --bloom")
    bloom["mix"] = True
motion_blur = None  # MotionBlurParams.make's keywords
if "--motion-blur" in sys.argv:  # takes no value, like --despeckle
    sys.argv.remove("--motion-blur")
    motion_blur = {}
if "--motion-blur-jitter" in sys.argv:
    sys.argv.remove("--motion-blur-jitter")
    if motion_blur is None:
        sys.exit("--motion-blur-jitter goes with --motion-blur")
    motion_blur["jitter"] = True
dof = None  # --dof-*: {"focus": D or None, "lens_radius": A, "max_radius": R, "focus_pixel": (X, Y) or None}
if "--dof-focus-pixel" in sys.argv:  # takes two values
    k = sys.argv.index("--dof-focus-pixel")
    dof = {"focus_pixel": (int(sys.argv[k + 1]), int(sys.argv[k + 2]))}
    del sys.argv[k:k + 3]
for flag in ("--shutter", "--motion-blur-taps", "--motion-blur-radius", "--dof-focus", "--dof-lens-radius", "--dof-max-radius", "--bloom-threshold", "--bloom-strength", "--bloom-levels", "--despeckle-gain", "--despeckle-rank", "--despeckle-radius", "--compare-strata", "--frames", "--orbit", "--spin", "--spin-deg", "--history-clip", "--history-clip-radius", "--display", "--encode", "--exposure", "--upscale", "--upscale-radius", "--denoise-iterations", "--denoise-sigma", "--denoise-sigma-luminance", "--matte", "--matte-slots", "--matte-select"):
    if flag in sys.argv:
        k = sys.argv.index(flag)
        value = sys.argv[k + 1]
        del sys.argv[k:k + 2]
        if flag == "--frames":
            frames = int(value)
        elif flag == "--compare-strata":
            compare_strata = int(value)
        elif flag in ("--despeckle-gain", "--despeckle-rank", "--despeckle-radius"):
            if despeckle is None:
                sys.exit("--despeckle-gain, --despeckle-rank and --despeckle-radius go with --despeckle")
            despeckle[flag[len("--despeckle-"):]] = float(value) if flag == "--despeckle-gain" else int(value)
        elif flag in ("--bloom-threshold", "--bloom-strength", "--bloom-levels"):
            if bloom is None:
                sys.exit("--bloom-threshold, --bloom-strength and --bloom-levels go with --bloom")
            bloom[flag[len("--bloom-"):]] = int(value) if flag == "--bloom-levels" else float(value)
        elif flag in ("--shutter", "--motion-blur-taps", "--motion-blur-radius"):
            if motion_blur is None:
                sys.exit("--shutter, --motion-blur-taps and --motion-blur-radius go with --motion-blur")
            motion_blur[{"--shutter": "shutter", "--motion-blur-taps": "taps", "--motion-blur-radius": "max_radius"}[flag]] = float(value) if flag == "--shutter" else int(value)
        elif flag in ("--dof-focus", "--dof-lens-radius", "--dof-max-radius"):
            dof = dict(dof or {}, **{flag[len("--dof-"):].replace("-", "_"): int(value) if flag == "--dof-max-radius" else float(value)})
        elif flag == "--orbit":
            orbit = float(value)
        elif flag == "--spin":
            spin = [int(v) for v in value.split(",") if v]
        elif flag == "--spin-deg":
            spin_deg = float(value)
        elif flag == "--history-clip":
            history_clip = dict(history_clip or {}, gamma=float(value))
        elif flag == "--history-clip-radius":
            history_clip = dict(history_clip or {}, radius=int(value))
        elif flag == "--display":
            display = dict(display or {}, curve=value)
        elif flag == "--encode":
            display = dict(display or {}, encode=value)
        elif flag == "--exposure":
            display = dict(display or {}, exposure=float(value))
        elif flag == "--upscale":
            upscale = dict(upscale or {}, factor=int(value))
        elif flag == "--upscale-radius":
            upscale = dict(upscale or {}, radius=int(value))
        elif flag == "--denoise-iterations":
            denoise_params["iterations"] = denoise_var_params["iterations"] = int(value)
        elif flag == "--matte":
            matte_key = value
        elif flag == "--matte-slots":
            matte_slots = int(value)
        elif flag == "--matte-select":
            matte_select = [int(v) for v in value.split(",") if v]
        elif flag == "--denoise-sigma-luminance":
            denoise_var_params["sigma_luminance"] = float(value)
        else:
            denoise_params.update(zip(("sigma_color", "sigma_normal", "sigma_depth"), (float(v) for v in value.split(","))))
            denoise_var_params.update({k: v for k, v in denoise_params.items() if k in ("sigma_normal", "sigma_depth")})
sys.argv = [a for a in sys.argv if a not in ("--aovs", "--pixel-filter", "--denoise", "--denoise-var", "--passes", "--denoise-passes", "--temporal", "--motion-vectors", "--spatial-variance", "--auto-exposure")]
if upscale is not None and (upscale.get("factor") not in pbrs_amd.UpsampleParams.FACTORS or upscale.get("radius", 1) not in pbrs_amd.UpsampleParams.RADII):
    sys.exit("--upscale 2|3|4 [--upscale-radius 1|2]")
if display is not None or auto_exposure:
    if "curve" not in (display or {}):
        sys.exit("--encode, --exposure and --auto-exposure go with --display none|reinhard|aces")
    if display["curve"] not in pbrs_amd.DisplayParams.CURVES or display.get("encode", "srgb") not in pbrs_amd.DisplayParams.ENCODES:
        sys.exit("--display none|reinhard|aces [--encode sqrt|srgb]")
    display["auto"] = auto_exposure
if dof is not None and ("lens_radius" not in dof or ("focus" in dof) == ("focus_pixel" in dof)):
    sys.exit("--dof-lens-radius A goes with --dof-focus D or --dof-focus-pixel X Y [--dof-max-radius R]")
if motion_blur is not None and not (frames and temporal):
    sys.exit("--motion-blur goes with --frames N --temporal: it smears a frame along its motion against the frame before")
scene, out = sys.argv[1], sys.argv[2]
msaa = int(sys.argv[3]) if len(sys.argv) > 3 else 4
depth = int(sys.argv[4]) if len(sys.argv) > 4 else 5  # src/main.rs:205
integrator = sys.argv[5] if len(sys.argv) > 5 else "path"
class _Spec:
    """A scene spec under HostScene's eyes."""

    def __init__(self, spec):
        self.spec = spec

    def build(self):
        return self.spec


def _mat(a):
    return np.array(list(a), dtype=np.float64).reshape(4, 4).T  # (column-major in the spec)


def spun_scenes(spec, ids, deg, cams):
    """Frame k's (HostScene, Camera, seed): the file's scene with the instances `ids` turned by k * deg degrees about the vertical axis
    through the centre of their world box (the instance transforms of the spec are rewritten in place for every frame)."""
    from pbrs_amd.spec import SHAPE_MESH as MESH
    start, pivots = {}, {}
    for i in ids:
        if not 0 <= i < spec.n_instances or spec.shapes[spec.instances[i].shape].kind != MESH:
            sys.exit(f"--spin: instance {i} is not a mesh instance of this scene")
        inst = spec.instances[i]
        shape = spec.shapes[inst.shape]
        mesh = spec.meshes[shape.mesh]
        v = np.ctypeslib.as_array(mesh.positions, shape=(mesh.n_vertices, 3)).astype(np.float64)
        start[i] = (_mat(inst.forward), _mat(inst.inverse))
        world = (start[i][0] @ np.hstack([v, np.ones((len(v), 1))]).T).T[:, :3]
        pivots[i] = 0.5 * (world.min(axis=0) + world.max(axis=0))
    for k, cam in enumerate(cams):
        t = np.radians(deg * k)
        for i in ids:
            def about(angle, c=pivots[i]):
                R = np.array([[np.cos(angle), 0.0, np.sin(angle)], [0.0, 1.0, 0.0], [-np.sin(angle), 0.0, np.cos(angle)]])
                M = np.eye(4)
                M[:3, :3], M[:3, 3] = R, c - R @ c
                return M
            fwd, inv = about(t) @ start[i][0], start[i][1] @ about(-t)
            spec.instances[i].forward[:] = [float(x) for x in fwd.T.reshape(-1)]
            spec.instances[i].inverse[:] = [float(x) for x in inv.T.reshape(-1)]
        yield pbrs_amd.HostScene(_Spec(spec)), cam, 1 + k


ls = pbrs_amd.load_pbrt(scene)
ctx = pbrs_amd.Context(0)
hs = pbrs_amd.HostScene(ls)
ctx.upload(hs)
if compare_strata and (frames or compare_strata < 1):
    sys.exit("--compare-strata N (N >= 1) goes with one image, not with --frames")
if frames:
    spec = ls.build().camera
    cams = [pbrs_amd.api.orbited(hs.camera, list(spec.target), list(spec.up), orbit * k) for k in range(frames)]
    stem, ext = (out[:-4], out[-4:]) if out.lower().endswith((".exr", ".png")) else (out, ".exr")
    if (spin or motion_vectors) and not temporal:
        sys.exit("--spin and --motion-vectors go with --frames N --temporal")
    if spatial_variance and not temporal:
        sys.exit("--spatial-variance goes with --frames N --temporal")
    if history_clip is not None and (not temporal or "gamma" not in history_clip):
        sys.exit("--history-clip GAMMA goes with --frames N --temporal, --history-clip-radius with --history-clip")
    if display is not None and not temporal:
        sys.exit("with --frames N, --display goes with --temporal")
    if upscale is not None and not temporal:
        sys.exit("with --frames N, --upscale goes with --temporal")
    if despeckle is not None and not temporal:
        sys.exit("with --frames N, --despeckle goes with --temporal")
    if bloom is not None and not temporal:
        sys.exit("with --frames N, --bloom goes with --temporal")
    if dof is not None and (not temporal or "focus_pixel" in dof):
        sys.exit("with --frames N, --dof-focus goes with --temporal; --dof-focus-pixel goes with one image")
    extra = {} if despeckle is None else {"despeckle": despeckle}  # (a keyword of the sequences only when asked for)
    if dof is not None:
        extra["dof"] = dict(pbrs_amd.lens(hs.camera, dof["focus"], dof["lens_radius"]), max_radius=dof.get("max_radius", 8))
    if motion_blur is not None:
        extra["motion_blur"] = motion_blur
    if bloom is not None:
        extra["bloom"] = bloom
    spatial = True if spatial_variance else None
    if spin or motion_vectors:
        sequence = ctx.render_animation(spun_scenes(ls.build(), spin, spin_deg, cams), msaa, msaa, depth, motion_vectors="prev_depth" if motion_vectors else False,
                                        spatial=spatial, clip=history_clip, display=display, upscale=upscale, **extra, **denoise_var_params)
    elif temporal:
        sequence = ctx.render_temporal(cams, msaa, msaa, depth, range(1, frames + 1), spatial=spatial, clip=history_clip, display=display,
                                       upscale=upscale, **extra, **denoise_var_params)
    else:
        sequence = ((ctx.render_aovs(msaa, msaa, depth, 1 + k, aovs=(), camera=cam)[0],) for k, cam in enumerate(cams))
    for k, images in enumerate(sequence):
        pbrs_amd.write_image(f"{stem}.{k:04d}{ext}", images[0])
        if temporal:
            pbrs_amd.write_image(f"{stem}.{k:04d}.accumulated{ext}", images[1])
            pbrs_amd.write_image(f"{stem}.{k:04d}.noisy{ext}", images[2])
        if dof is not None:
            pbrs_amd.write_image(f"{stem}.{k:04d}.dof{ext}", images[3]["dof"])
        if motion_blur is not None:
            pbrs_amd.write_image(f"{stem}.{k:04d}.motion_blur{ext}", images[3]["motion_blur"])
        if bloom is not None:
            pbrs_amd.write_image(f"{stem}.{k:04d}.bloom{ext}", images[3]["bloom"])
        if display is not None:
            pbrs_amd.write_image_u8(f"{stem}.{k:04d}.display.png", images[3]["display"])
        if motion_vectors:
            pbrs_amd.write_image(f"{stem}.{k:04d}.motion.exr", images[4])
    print(f"{frames} frames of {hs.width}x{hs.height} at {msaa * msaa} spp, {orbit} degrees per frame"
          f"{', accumulated and filtered' if temporal else ''} -> {stem}.0000{ext} ..")
    sys.exit(0)
if integrator in ("materials", "normals"):  # --visualize-materials / --visualize-normals (src/main.rs:180-185): one ray per pixel
    msaa = 1
guides = ("albedo", "normal", "depth") + (("instance",) if denoise or denoise_var or denoise_passes else ())
want = guides + (("variance",) if denoise_var else ())
want_buf = aovs or denoise or denoise_var or denoise_passes
want_layers = pbrs_amd.api.PASSES if denoise_passes else ("direct", "indirect") if passes else ()
if filtered:
    pf = ls.pixel_filter()
    img, st = ctx.render_filtered(pf, msaa, msaa, depth, 1, integrator=integrator, timing=True)
    print(f"pixel filter: {pf}")
    if want_buf:
        _, buf, _ = ctx.render_aovs(msaa, msaa, depth, 1, aovs=want, integrator=integrator)
    if matte_key:  # like the AOVs: per-pixel, from a separate render of the same samples
        matte = ctx.render_matte(msaa, msaa, depth, 1, key=matte_key, slots=matte_slots, integrator=integrator)[1]
elif matte_key:
    img, matte, buf, st = ctx.render_matte(msaa, msaa, depth, 1, key=matte_key, slots=matte_slots, aovs=want if want_buf else (),
                                           integrator=integrator, timing=True)
elif want_layers:
    img, layers, buf, st = ctx.render_passes(msaa, msaa, depth, 1, passes=want_layers, aovs=want if want_buf else (), integrator=integrator, timing=True)
elif want_buf:
    img, buf, st = ctx.render_aovs(msaa, msaa, depth, 1, aovs=want, integrator=integrator, timing=True)
else:
    img, st = ctx.render(msaa, msaa, depth, 1, integrator=integrator, timing=True)
if want_layers and (filtered or matte_key):  # like the AOVs beside a filtered image: from a separate render of the same samples
    layers = ctx.render_passes(msaa, msaa, depth, 1, passes=want_layers, integrator=integrator)[1]
pbrs_amd.write_image(out, img)
scored = {"image": img}  # what --compare-strata scores
stem, ext = (out[:-4], out[-4:]) if out.lower().endswith((".exr", ".png")) else (out, ".exr")
glare = img  # what --display shows
if dof is not None:
    z = buf["depth"] if want_buf else ctx.render_aovs(msaa, msaa, depth, 1, aovs=("depth",), integrator=integrator)[1]["depth"]  # the same samples' first hits
    if "focus_pixel" in dof:  # the focus in the AOV's units; the scale follows it: lens() at any distance gives focus * scale
        x, y = dof["focus_pixel"]
        if not (0 <= x < z.shape[1] and 0 <= y < z.shape[0] and np.isfinite(z[y, x]) and z[y, x] > 0):
            sys.exit(f"--dof-focus-pixel {x} {y}: nothing to focus on there")
        unit = pbrs_amd.lens(hs.camera, 1.0, dof["lens_radius"])
        thin = {"focus": float(z[y, x]), "scale": unit["focus"] * unit["scale"] / float(z[y, x])}
    else:
        thin = pbrs_amd.lens(hs.camera, dof["focus"], dof["lens_radius"])
    thin["max_radius"] = dof.get("max_radius", 8)
    glare = ctx.dof(img, z, **thin)
    pbrs_amd.write_image(f"{stem}.dof{ext}", glare)
    print(f"-> {stem}.dof{ext} ({pbrs_amd.DofParams.make(img.shape[1], img.shape[0], **thin).as_dict()})")
if bloom is not None:
    glare = ctx.bloom(glare, **bloom)
    pbrs_amd.write_image(f"{stem}.bloom{ext}", glare)
    print(f"-> {stem}.bloom{ext} ({pbrs_amd.BloomParams.make(img.shape[1], img.shape[0], **bloom).as_dict()})")
if display is not None:
    shown, e = ctx.display(glare, return_exposure=True, **display)
    pbrs_amd.write_image_u8(f"{stem}.display.png", shown)
    print(f"-> {stem}.display.png ({display['curve']}, {display.get('encode', 'srgb')}, exposure {float(e) * display.get('exposure', 1.0):.4g})")
if upscale is not None:
    up = {k: v for k, v in upscale.items() if k != "factor"}
    full, low, _ = ctx.render_upscaled(msaa, msaa, depth, 1, factor=upscale["factor"], upsample=up, **denoise_var_params)
    pbrs_amd.write_image(f"{stem}.upscaled{ext}", full)
    scored["upscaled"] = full
    pbrs_amd.write_image(f"{stem}.upscaled_low{ext}", low)
    print(f"-> {stem}.upscaled{ext} ({low.shape[1]}x{low.shape[0]} traced and filtered, factor {upscale['factor']}, radius {upscale.get('radius', 1)})")
if denoise:
    scored["denoised"] = ctx.denoise(img, **{n: buf[n] for n in guides}, **denoise_params)
    pbrs_amd.write_image(f"{stem}.denoised{ext}", scored["denoised"])
    print(f"-> {stem}.denoised{ext}")
if denoise_var:
    scored["denoised_var"] = ctx.denoise_var(img, buf["variance"], **{n: buf[n] for n in guides}, **denoise_var_params)
    pbrs_amd.write_image(f"{stem}.denoised_var{ext}", scored["denoised_var"])
    print(f"-> {stem}.denoised_var{ext}")
if despeckle is not None:
    variance = buf["variance"] if denoise_var else None
    clean = ctx.despeckle(img, variance, removed=True, **despeckle)
    scored["despeckled"] = clean[0]
    pbrs_amd.write_image(f"{stem}.despeckled{ext}", clean[0])
    print(f"-> {stem}.despeckled{ext} ({clean[-1].n_clamped} pixels clamped, {clean[-1].n_repaired} repaired, mean energy removed {float(clean[-2].mean()):.4g})")
    if denoise_var:
        scored["despeckled_denoised_var"] = ctx.denoise_var(clean[0], clean[1], **{n: buf[n] for n in guides}, **denoise_var_params)
        pbrs_amd.write_image(f"{stem}.despeckled_denoised_var{ext}", scored["despeckled_denoised_var"])
        print(f"-> {stem}.despeckled_denoised_var{ext}")
if passes:
    for name in ("direct", "indirect"):
        pbrs_amd.write_image(f"{stem}.{name}.exr", layers[name])
        print(f"-> {stem}.{name}.exr")
if denoise_passes:
    clean = [ctx.denoise_var(layers[n], layers[n + "_variance"], **{g: buf[g] for g in guides}, **denoise_var_params) for n in ("direct", "indirect")]
    pbrs_amd.write_image(f"{stem}.denoised_passes{ext}", ctx.combine_passes(*clean))
    print(f"-> {stem}.denoised_passes{ext}")
if aovs:
    for name in ("albedo", "normal", "depth"):
        a = buf[name] if buf[name].ndim == 3 else np.repeat(buf[name][:, :, None], 3, axis=2)
        pbrs_amd.write_image(f"{stem}.{name}.exr", a)
        print(f"-> {stem}.{name}.exr")
if matte_key:
    np.savez(f"{stem}.matte.npz", **matte)
    print(f"-> {stem}.matte.npz ({matte_key} ids, {matte_slots} per pixel; {int((matte['residual'] > 0).sum())} pixels hold more)")
    if matte_select is not None:
        m = ctx.matte_mask(matte["ids"], matte["coverage"], matte_select)
        pbrs_amd.write_image(f"{stem}.mask.png", np.repeat(m[:, :, None], 3, axis=2))
        print(f"-> {stem}.mask.png")
print(f"{img.shape[1]}x{img.shape[0]} at {msaa * msaa} spp in {st['ms_total']:.1f} ms -> {out}")
if compare_strata:
    import json
    reference = ctx.render(compare_strata, compare_strata, depth, 4242, integrator=integrator)[0]
    metrics = {"reference_strata": compare_strata}
    for name, image in scored.items():
        r = ctx.compare(image, reference)
        metrics[name] = dict(r.as_dict(), psnr_db=r.psnr())
    print(json.dumps({"compare": metrics}))
