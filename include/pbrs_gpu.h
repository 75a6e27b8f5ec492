/* pbrs_gpu.h — C ABI of the MI355X wavefront path tracer (libpbrs_gpu.so).
 *
 * What it replaces.  The reference has no FFI or plugin interface; its only seam on this path is
 * the integrator function pointer `fn(&Scene, ray::Ray, i32) -> Color` chosen at
 * src/main.rs:160-163 and called once per camera sample from the row loop at src/main.rs:192-213,
 * which rayon runs over rows at :219-224.  A per-ray seam cannot feed a GPU, so this ABI lifts it to
 * a per-tile batch seam that replaces src/main.rs:192-231 as a whole:
 *     (scene, camera, strata, depth) -> row-major RGB f32
 * with the same semantics (stratified jitter :197-201, `shoot_ray` :203, sequential f32 sum over
 * samples :205, `scale_down_by` :208).  Each entry point below cites the reference lines it stands
 * for.  INTEGRATION.md shows the Rust `extern "C"` block a maintainer would add.
 *
 * Conventions: POD structs, little-endian, plain pointers + counts, no ownership transfer
 * (`pbrs_upload_scene` copies; the caller keeps its buffers).  Never unwinds or aborts: every call
 * returns 0 or a negative PBRS_E_* and `pbrs_last_error` explains.  The reference's error model is
 * panic: where an `assert!` of the reference would fire, the device carries on with the
 * arithmetic result, as the oracle does.  What comes of it is visible in the output and counted:
 * `pbrs_stats.invalid_samples` is the number of camera samples whose radiance is not finite (a NaN or
 * an infinity in any channel) — always filled, equal to the oracle's count on the same scene and
 * seeds (tests/test_gpu_fuzz.py).  The assert sites themselves are counted by the oracle only
 * (`oracle_stats.panics`, test infrastructure): the parity tests assert that count to be zero on the
 * BASELINE scenes.
 * Threading: one `pbrs_ctx` per GPU (several on one GPU work too, e.g. one per scene); different contexts may be
 * driven concurrently from different host threads/processes (tests/test_gpu_contexts.py: two threads, two contexts,
 * disjoint bands of one frame); a single context is not re-entrant.  Nothing process-wide depends on the scene a
 * context holds (the kernels' dynamic-LDS limit is raised once per device, to the cap, in `pbrs_create`).
 * Stream ordering: a context runs on its own NON-BLOCKING stream.  Work the caller queues on the legacy default stream
 * (or on any other stream) is NOT ordered against a render: the output of `pbrs_render_tile_device` is valid only after
 * `pbrs_collect_stats`, after the caller has synchronised the context's stream, or — with `pbrs_set_stream` — in the
 * caller's own stream's order.  `pbrs_render_tile` (host output) synchronises before it returns.
 * Environment: the library reads no environment variable (developer builds with -DPBRS_DEV_OVERRIDES aside).
 *
 * The flattened scene (`pbrs_scene_desc`) is produced by the host side of the boundary — in the
 * reference's own language that is scene/ + tlas/ + shape/ (Rust); here pbrs_amd/csrc/host
 * (C++, include/pbrs_host.h) — by running `tlas::build_bvh` (tlas/src/bvh.rs:116-152) and
 * `recursive_build` (shape/src/blas.rs:333-420) and linearising the trees.
 */
#ifndef PBRS_GPU_H
#define PBRS_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBRS_OK 0
#define PBRS_E_INVALID (-1)   /* bad argument / inconsistent scene description */
#define PBRS_E_DEVICE (-2)    /* HIP runtime error (message in pbrs_last_error) */
#define PBRS_E_NO_SCENE (-3)  /* render called before pbrs_upload_scene */
#define PBRS_E_LIMIT (-4)     /* traversal stack deeper than the LDS budget, tile too large, ... */

#define PBRS_LEAF_FLAG 0x80000000u
#define PBRS_TLAS_LEAF_KIND_SHIFT 8 /* TLAS leaves also carry the instance's shape kind in bits 8..10 of b */

/* A BVH node, 32 B, pre-order: the left child of node i is node i+1.
 *   inner: a = index of the right child, b = split axis (BLAS; 0 for TLAS)
 *   leaf : b = PBRS_LEAF_FLAG | count;  a = first triangle (BLAS, count <= n) or instance (TLAS, count = 1)
 * bbox as in geometry/src/bvh.rs:11-14.  TLAS: tlas/src/bvh.rs:11-18.  BLAS: shape/src/blas.rs:10-18. */
typedef struct pbrs_node {
    float min[3];
    uint32_t a;
    float max[3];
    uint32_t b;
} pbrs_node;

/* tlas/src/instance.rs:12-16.  Rows of the two affine Mat4 of geometry/src/transform.rs:16-19:
 * row r = (cols[0][r], cols[1][r], cols[2][r], cols[3][r]); the fourth row is (0,0,0,1). */
typedef struct pbrs_instance {
    float inv[3][4];
    float fwd[3][4];
    uint32_t shape_kind;  /* enum pbrs_shape_kind (pbrs_scene_spec.h) */
    uint32_t shape_index; /* analytic: index into shapes[]; mesh: index into meshes[] */
    uint32_t material;
    uint32_t flags; /* PBRS_INSTANCE_* */
    /* mesh instances: copies of meshes[shape_index].root / .flags so that entering the BLAS costs one record;
     * PBRS_SHAPE_TRIANGLE instances: blas_root = index of the triangle's own record in tri_verts[] */
    uint32_t blas_root;
    uint32_t mesh_flags;
    uint32_t pad[2];
} pbrs_instance;
/* inv and fwd are bit-exactly the identity: for a ray whose components are all finite and non-zero
 * `inverse * ray` (tlas/src/instance.rs:51) returns the ray's own bits, so the product can be skipped. */
#define PBRS_INSTANCE_IDENTITY 1u

/* Analytic shape parameters, 12 floats (shape/src/simple.rs:10-196), laid out as in pbrs_shape_spec.p;
 * cuboid min/max already ordered (Cuboid::from_points), disk normal already unit (Disk::new). */
typedef struct pbrs_shape {
    float p[12];
} pbrs_shape;

typedef struct pbrs_mesh {
    uint32_t root;       /* index of the BLAS root in blas_nodes[] */
    uint32_t n_nodes;
    uint32_t first_tri;  /* first triangle of this mesh in tri_verts[] / tri_shade[] */
    uint32_t n_tris;
    uint32_t height;     /* IsoBvhNode::height(), shape/src/blas.rs:21-26 */
    uint32_t flags;      /* PBRS_MESH_* */
    uint32_t pad[2];
} pbrs_mesh;
/* Every triangle of the mesh has three bit-identical vertex normals AND passes the tangent check of
 * shape/src/blas.rs:193-200 (which then depends on the triangle only, not on the hit or the ray), so the
 * traversal need not evaluate the shading frame of candidate hits. */
#define PBRS_MESH_FLAT_SHADING_OK 1u
/* Every triangle of the mesh passes the same tangent check for ANY hit on it, by a bound instead of an identity: the
 * rejected quantity |dpdu . n| is the rounding residue of a Gram-Schmidt step and stays below 12 eps / sin(theta),
 * theta = angle(dpdu_raw, n); the host proves sin(theta) >= 0.044 for every normal the interpolation can produce
 * (host/flatten.cpp, `smooth_shading_bound`), i.e. |dpdu . n| < 2e-5 against the 1e-3 threshold. */
#define PBRS_MESH_SMOOTH_SHADING_OK 2u
#define PBRS_MESH_SHADING_OK_MASK 3u

/* One triangle's geometry in BLAS leaf order, Q11 swap applied: `let (i,k,j) = index_triple`
 * (shape/src/blas.rs:162) => p0 = positions[i], p1 = positions[j], p2 = positions[k].
 * n = `(p0 - p1).cross(p2 - p1).try_hat()` (shape/src/simple.rs:436), which depends on the triangle only:
 * evaluated once by the host with the reference's operand order; all-NaN when try_hat returns None. */
typedef struct pbrs_tri_verts {
    float p0[3];
    float nx;
    float p1[3];
    float ny;
    float p2[3];
    float nz;
} pbrs_tri_verts;

/* Shading attributes of the same triangle, same vertex order (shape/src/blas.rs:170-185). */
typedef struct pbrs_tri_shade {
    float n0[3], n1[3], n2[3];
    float uv0[2], uv1[2], uv2[2];
    uint32_t orig; /* index of the triangle in the input index buffer */
} pbrs_tri_shade;

/* geometry/src/bxdf.rs:263-269 flattened: `bxdfs_at` is constant per material when its textures are Solid; a lobe whose
 * colour comes from another texture names it in `tex` and the colour is evaluated per hit (material/src/lib.rs). */
enum pbrs_bxdf_kind { PBRS_BXDF_SPECULAR = 0, PBRS_BXDF_DIFFUSE = 1, PBRS_BXDF_MICROFACET = 2, PBRS_BXDF_FOURIER = 3 };
enum pbrs_intrusion { PBRS_REFLECTION = 0, PBRS_TRANSMISSION = 1, PBRS_HYBRID = 2 };        /* bxdf.rs:35-40  */
enum pbrs_fresnel_kind { PBRS_FRESNEL_NOP = 0, PBRS_FRESNEL_DIELECTRIC = 1, PBRS_FRESNEL_CONDUCTOR = 2 }; /* :284-289 */
typedef struct pbrs_bxdf {
    uint32_t kind;
    uint32_t intrusion;   /* Specular; Fourier: index into pbrs_scene_desc::fourier_tables */
    uint32_t fresnel;     /* Specular, Microfacet */
    uint32_t oren_nayar;  /* Diffuse: 0 Lambertian, 1 Oren-Nayar */
    float albedo[3];
    float alpha_x;        /* Beckmann (microfacet.rs:11); already through roughness_to_alpha */
    float eta[3];         /* dielectric: eta_front, eta_back, -; conductor: eta_t rgb (eta_i = 1) */
    float alpha_y;
    float k[3];           /* conductor k rgb; Oren-Nayar: coeff_a, coeff_b, - */
    uint32_t tex;         /* 0: `albedo` is the colour; else (texture index + 1) | PBRS_BXDF_TEX_DROP_IF_BLACK */
} pbrs_bxdf;
/* Uber pushes a textured lobe only when the texture's value at the hit is not black (material/src/lib.rs:326-362) */
#define PBRS_BXDF_TEX_DROP_IF_BLACK 0x80000000u

#define PBRS_MAX_BXDFS 5 /* Uber, material/src/lib.rs:317-365 */
typedef struct pbrs_material {
    float emission[3]; /* Material::emission, material/src/lib.rs:24-26, :294-296 */
    uint32_t n_bxdfs;
    uint32_t first_bxdf;
    uint32_t flags; /* PBRS_MATERIAL_TEXTURED: some lobe has tex != 0 */
    uint32_t vis_class; /* palette entry of material_visualizer for `Material::summary()`, src/directlighting.rs:247-259 */
    /* 1 + index of a pbrs_bxdf record (outside the material's lobe list) whose albedo / tex hold the colour that
     * `Material::scatter` returns where it is a constant of the material — Lambertian albedo (possibly a texture), Mirror
     * albedo, Plastic diffuse, Dielectric transmit (material/src/lib.rs:163-177, :224-228, :427-432, :246-264) — for
     * normal_visualizer; 0 = not provided (PBRS_INTEGRATOR_NORMALS is then refused) */
    uint32_t vis_bxdf;
} pbrs_material;
#define PBRS_MATERIAL_TEXTURED 1u

/* texture/src/lib.rs:35-223 (Solid is folded into the lobes).  PERLIN: rand_vec = tex_floats[data .. data + 768),
 * perm_x|y|z = tex_words[perm .. perm + 768); IMAGE: texels = tex_floats[data .. data + 3 * width * height). */
typedef struct pbrs_texture {
    uint32_t kind; /* enum pbrs_texture_kind (pbrs_scene_spec.h) */
    float odd[3];
    float even[3];
    float freq;
    uint32_t width, height;
    uint32_t data; /* offset into tex_floats */
    uint32_t perm; /* offset into tex_words */
} pbrs_texture;

/* FourierTable (geometry/src/fourier.rs:99-151) after `build`: every array lives in the texture pools.  tex_floats: mu
 * [n_mu], cdf [n_mu^2], a0 [n_mu^2] (the order-0 cache), a [n_coeffs], recip [m_max] (recip[i] = 1 / i); tex_words:
 * a_offset [n_mu^2], m_lookup [n_mu^2] (i32 bit patterns, validated non-negative and in range by the host). */
typedef struct pbrs_fourier_table {
    uint32_t n_mu, n_channels, m_max;
    uint32_t mu, cdf, a0, a, recip; /* offsets into tex_floats */
    uint32_t a_offset, m_lookup;    /* offsets into tex_words  */
    uint32_t n_coeffs;
    uint32_t pad;
} pbrs_fourier_table;

/* light/src/lib.rs:107-111 + light/src/sample_shape.rs:38-43 (world-space shape, area precomputed). */
typedef struct pbrs_area_light {
    float emit[3];
    uint32_t shape_kind;
    float p[9];
    float area;
    float pad[2];
} pbrs_area_light;

/* light/src/lib.rs:29-39 */
typedef struct pbrs_delta_light {
    uint32_t kind;
    float v[3];
    float color[3];
    float world_radius;
} pbrs_delta_light;

typedef struct pbrs_scene_desc {
    uint32_t n_tlas_nodes;
    const pbrs_node* tlas_nodes;
    uint32_t tlas_height; /* BvhNode::height(), tlas/src/bvh.rs:56-61 */
    uint32_t n_instances;
    const pbrs_instance* instances;
    uint32_t n_shapes;
    const pbrs_shape* shapes;
    uint32_t n_meshes;
    const pbrs_mesh* meshes;
    uint32_t n_blas_nodes;
    const pbrs_node* blas_nodes;
    uint32_t n_triangles;
    const pbrs_tri_verts* tri_verts;
    const pbrs_tri_shade* tri_shade;
    uint32_t n_materials;
    const pbrs_material* materials;
    uint32_t n_bxdfs;
    const pbrs_bxdf* bxdfs;
    uint32_t n_area_lights;
    const pbrs_area_light* area_lights;
    uint32_t n_delta_lights;
    const pbrs_delta_light* delta_lights;
    float env_constant[3]; /* EnvLight::Constant, scene/src/lib.rs:12-16 */
    uint32_t env_kind;     /* enum pbrs_env_kind (pbrs_scene_spec.h) */
    uint32_t n_textures;
    const pbrs_texture* textures;
    uint32_t n_tex_floats;
    const float* tex_floats;
    uint32_t n_tex_words;
    const uint32_t* tex_words;
    uint32_t env_texture;  /* PBRS_ENV_IMAGE: index into textures[] */
    float env_scale[3];
    uint32_t n_fourier_tables;
    const pbrs_fourier_table* fourier_tables;
} pbrs_scene_desc;

/* geometry/src/camera.rs:9-17 with the three `orientation * {c,a,b}` products of shoot_ray (:68-70)
 * hoisted: they do not depend on the pixel. */
typedef struct pbrs_camera {
    float center[3];
    uint32_t width;
    float c[3]; /* orientation * c */
    uint32_t height;
    float a[3]; /* orientation * a */
    float pad0;
    float b[3]; /* orientation * b */
    float pad1;
} pbrs_camera;

/* Work counters in the units of SURVEY.md §8(d); filled only when `collect_counters` is set
 * (an instrumented kernel variant runs; the timed variant carries no counters). */
typedef struct pbrs_stats {
    uint64_t samples;       /* camera samples rendered                                  */
    uint64_t closest_rays;  /* BvhNode::intersect equivalents (tlas/src/bvh.rs:77)       */
    uint64_t shadow_rays;   /* BvhNode::occludes equivalents  (tlas/src/bvh.rs:105)      */
    uint64_t shade_events;  /* path vertices shaded                                      */
    uint64_t tlas_nodes, blas_nodes, instances, instance_hits, triangles, tri_shading;
    uint64_t spheres, quads, cuboids, disks;
    uint64_t shadow_tlas_nodes, shadow_blas_nodes, shadow_instances, shadow_triangles, shadow_prims;
    uint64_t invalid_samples; /* camera samples whose radiance has a NaN or infinite component (always filled) */
    /* HIP-event time per stage, summed over launches, in ms, on the context's stream */
    float ms_raygen, ms_extend, ms_shade, ms_shadow, ms_accumulate, ms_total;
    uint32_t launches_extend, launches_shadow, launches_shade, passes;
    /* Which instantiation of the traversal kernels the render's passes launched (always filled): bit 0 analytic shapes, 1 per-candidate
     * shading check, 2 scanned TLAS, 3 several node steps per round (deep BLAS), 4 walks over four-wide nodes, 5 full further node
     * steps (a scene with coordinates outside the guarded range of the division-free box test), 6 scene arrays staged in LDS, 7 an unscanned TLAS staged in LDS,
     * 8 (k_extend) the TLAS extent follows the reference's ray.t_max to the letter, rises included (a ParallelQuad next to a mesh);
     * 0x80000000: the instrumented variant (collect_counters). */
    uint32_t kernel_features_extend, kernel_features_shadow;
    /* Queue sizes per bounce, summed over the passes of the render (filled with the work counters): paths_at_bounce[b] = rays
     * `scene.tlas.intersect` sees at `for bounces in 0..depth` iteration b (src/pathintegrator.rs:14-16), i.e. k_extend's queue;
     * shadow_rays_at_bounce[b] = `scene.tlas.occludes` calls of that iteration's light estimate (k_shadow's queue).
     * Bounces beyond PBRS_STATS_MAX_BOUNCES - 1 are added to the last entry. */
    uint64_t paths_at_bounce[16];
    uint64_t shadow_rays_at_bounce[16];
} pbrs_stats;
#define PBRS_STATS_MAX_BOUNCES 16

typedef struct pbrs_ctx pbrs_ctx;

/* One context per device.  Stands for the per-thread state of the rayon row loop (src/main.rs:219-224). */
int pbrs_create(int device_ordinal, pbrs_ctx** out);
void pbrs_destroy(pbrs_ctx*);
const char* pbrs_last_error(const pbrs_ctx*);
/* Run the pipeline on an existing HIP stream (e.g. torch's current stream); NULL = the context's own, which is
 * created hipStreamNonBlocking: see "Stream ordering" above. */
int pbrs_set_stream(pbrs_ctx*, void* hip_stream);

/* A render of several passes hands every pass's late bounces (near-empty launches that end with the latency of their longest walks) to a
 * second, high-priority stream of the context, where they run beside the next pass's first bounces; the passes' samples still reach the
 * pixel sums in pass order (src/main.rs:205), so the image does not depend on it.  On by default; 0 keeps every pass on the context's
 * stream — what a host wants when it reads the per-stage milliseconds of pbrs_stats as exclusive times (with the overlap a stage's
 * event brackets include the time its kernels share the chip with the other stream's). */
int pbrs_set_pass_overlap(pbrs_ctx*, int enabled);

/* Entry nodes of the camera rays.  The rays of a pixel share their origin and differ by less than a pixel in direction; in a scene whose
 * deepest mesh qualifies (a BLAS of at least twelve levels with every child box inside its parent's, under an instance that is the identity
 * or a pure translation, coordinates inside the guarded range of the division-free box test) a pre-pass of one lane per pixel finds, once
 * per render, up to eight nodes of that BLAS under which every leaf a ray of the pixel can reach must lie, and the first bounce's
 * closest-hit walks enter the mesh there instead of at its root.  The walks visit the same leaves in the same order with the same
 * extents: the image does not depend on it, bit for bit.  On by default; 0 walks every ray from the root.  An instrumented render
 * (collect_counters) never uses the table: its node counts are the reference's. */
int pbrse_set_entry_nodes(pbrs_ctx*, int enabled);
/* What the pre-pass of the last render queued on the context found (all zero where it did not run: the feature off, a scene without a
 * qualifying mesh, an instrumented render, a pass without a bounce).  Waits for that render. */
typedef struct pbrs_entry_info {
    uint32_t pixels_with_entries; /* pixels whose rays enter the mesh at the pixel's entries              */
    uint32_t pixels_empty;        /* ... whose rays cannot reach the mesh at all: an empty list           */
    uint32_t pixels_from_root;    /* ... without a table: a direction component that is zero or changes   */
                                  /* sign inside the pixel, a ray outside the guarded range, no stack rows */
    uint32_t entries;             /* entries written, over the pixels with entries                         */
} pbrs_entry_info;
int pbrse_last_entry_info(pbrs_ctx*, pbrs_entry_info* out);
/* (The two functions' prefix is pbrse_; the struct carries pbrs_.) */

/* Copies the flattened scene into HBM.  Stands for building `Scene` (scene/src/lib.rs:36-63). */
int pbrs_upload_scene(pbrs_ctx*, const pbrs_scene_desc*);

typedef struct pbrs_render_params {
    uint32_t x0, y0, w, h;         /* tile, in pixels of the camera film                           */
    uint32_t strata_x, strata_y;   /* spp = strata_x * strata_y; the reference has both = msaa    */
    uint32_t max_depth;            /* `for bounces in 0..depth`, src/pathintegrator.rs:14          */
    uint32_t samples_per_pass;     /* sample indices traced concurrently per pixel (0 = auto)      */
    uint64_t seed;                 /* RNG contract, include/pbrs_numeric.h                          */
    uint32_t collect_counters;     /* run the instrumented kernels and fill the work counters      */
    uint32_t time_stages;          /* bracket every launch with HIP events and fill ms_*           */
    /* Interleaved row bands, the multi-GPU partition of the rayon row loop (src/main.rs:219-224):
     * with band_count > 1 the tile's h rows are the rows of bands band_index, band_index+band_count, ...
     * (band_rows rows each) counted from y0, packed:  film_row = y0 + ((r / band_rows) * band_count
     * + band_index) * band_rows + r % band_rows.  band_count <= 1 means a plain rectangular tile. */
    uint32_t band_rows, band_count, band_index;
    uint32_t integrator;           /* PBRS_INTEGRATOR_*: which `fn(&Scene, Ray, i32) -> Color` of src/main.rs:160-163 */
} pbrs_render_params;
/* src/pathintegrator.rs:9-74 */
#define PBRS_INTEGRATOR_PATH 0u
/* direct_lighting_integrator, src/directlighting.rs:14-47: emission, or the one-light estimate plus one level of perfect
 * specular reflection/refraction (src/bsdf.rs:104-113) followed by direct_lighting_debug_integrator (:49-56).  max_depth
 * only gates it (`depth <= 0` returns black); the chain is at most two rays long. */
#define PBRS_INTEGRATOR_DIRECT 1u
/* material_visualizer, src/directlighting.rs:234-271 (`--visualize-materials`, src/main.rs:166-187): one un-jittered ray per
 * pixel (`shoot_ray(row, col, (0.0, 0.0))`), a palette colour per kind of material at the first hit, a grey checker of
 * the ray direction where nothing is hit.  strata must be 1 x 1; max_depth is ignored (the reference passes 0). */
#define PBRS_INTEGRATOR_MATERIALS 2u
/* normal_visualizer, src/directlighting.rs:273-289 (`--visualize-normals`): one un-jittered ray per pixel,
 * (albedo of `mtl.scatter(-ray.dir, &hit)` + hit.normal) * 0.5, the environment where nothing is hit.  `scatter` is
 * `todo!()` for Glossy, Uber, Substrate and Fourier: their albedo counts as black.  Dielectric::scatter draws one random
 * number: the pixel's RNG stream supplies it (first draw after the two of the unused jitter).  strata must be 1 x 1. */
#define PBRS_INTEGRATOR_NORMALS 3u

/* Renders a tile; replaces src/main.rs:192-231 for the rows/cols of the tile.  `rgb_out` is
 * w*h*3 floats, row-major.  _host writes to caller-owned host memory (one D2H copy at the end);
 * _device leaves the result in caller-owned device memory and does not synchronise the stream. */
int pbrs_render_tile(pbrs_ctx*, const pbrs_camera*, const pbrs_render_params*, float* rgb_out_host, pbrs_stats* stats_out);
int pbrs_render_tile_device(pbrs_ctx*, const pbrs_camera*, const pbrs_render_params*, float* rgb_out_device, pbrs_stats* stats_out);
/* After a _device render with time_stages/collect_counters: waits for the stream and fills the stats. */
int pbrs_collect_stats(pbrs_ctx*, pbrs_stats* stats_out);

/* First-hit AOVs beside the image: per-pixel buffers of the render's own camera samples (the same jittered rays, all
 * strata_x * strata_y sample indices, the tile / band packing of rgb_out).  For sample s of a pixel the first hit is the
 * hit record of `scene.tlas.intersect` on its camera ray (bounce 0).  Every pointer may be NULL (not wanted); spp =
 * strata_x * strata_y, sums are sequential f32 sums in sample-index order from +0, scaled like the radiance (`* (1.0f / spp)`):
 *   albedo    3 x f32 row-major RGB: (sum_s a_s) * (1 / spp).  a_s = the colours of the lobes the hit's material pushes at that
 *             hit summed in lobe order from +0 (a textured lobe: its texture at the hit's (u, v, pos); Uber drops a lobe whose
 *             texture is black there; a Fourier lobe counts as (1, 1, 1)), each channel then clamped, fminf(fmaxf(x, 0), 1).
 *             A miss and an emitter without lobes give 0.
 *   normal    3 x f32: (sum_s n_s) * (1 / spp), n_s = the world-space shading normal of the hit (the normal PBRS_INTEGRATOR_NORMALS
 *             shows), not renormalised; 0 for a miss.
 *   coverage  f32: (float)n_hit * (1 / spp), n_hit = samples that hit something.
 *   depth     f32: t of the nearest hit among the pixel's samples (smallest t; a tie keeps the lowest sample index), +inf if none.
 *             t is the ray parameter of the reference: camera directions are not unit length (geometry/src/camera.rs:65-77),
 *             so t is not a distance.
 *   instance  u32: that hit's instance, an index into pbrs_scene_desc::instances; 0xffffffff if no sample hits.
 *   material  u32: instances[instance].material; 0xffffffff if no sample hits.
 *   prim      u32: that hit's primitive, numbered as pbrs_hit_record::prim; 0xffffffff if no sample hits.
 * Pointers are host memory for pbrs_render_tile_aovs, device memory for pbrs_render_tile_aovs_device. */
typedef struct pbrs_aov_buffers {
    float* albedo;
    float* normal;
    float* coverage;
    float* depth;
    uint32_t* instance;
    uint32_t* material;
    uint32_t* prim;
} pbrs_aov_buffers;
/* pbrs_render_tile / pbrs_render_tile_device that also fill the requested AOVs (the image is the same, bit for bit).  Any
 * integrator; the visualisers trace their one cast even at max_depth 0, PBRS_INTEGRATOR_PATH / _DIRECT with max_depth == 0
 * trace no camera ray and return PBRS_E_INVALID when a buffer is requested.  `aovs` NULL or all-NULL: exactly the plain call.
 * The AOV kernels' time counts in pbrs_stats::ms_total only.  The context keeps 40 B of AOV state per pixel (and, for the host
 * variant, 44 B per pixel of staging); _device is asynchronous like pbrs_render_tile_device: valid after pbrs_collect_stats. */
int pbrs_render_tile_aovs(pbrs_ctx*, const pbrs_camera*, const pbrs_render_params*, float* rgb_out_host, const pbrs_aov_buffers* aovs_host,
                          pbrs_stats* stats_out);
int pbrs_render_tile_aovs_device(pbrs_ctx*, const pbrs_camera*, const pbrs_render_params*, float* rgb_out_device,
                                 const pbrs_aov_buffers* aovs_device, pbrs_stats* stats_out);

/* Filtered film: the image reconstructed with the scene's pixel filter (pbrt-v3's `Filter`, math/src/filter.rs) instead of
 * the plain per-pixel mean of src/main.rs:205-208, which pbrs_render_tile[_device] keep.  The reference parses the filter and
 * never applies it; the support and normalisation below are pbrt-v3's Film::AddSample / WriteImage.  All arithmetic is f32
 * without fused multiply-add, in the order written; pn_* is include/pbrs_numeric.h, the factors are include/pbrs_filter.h.
 *   Sample i of film pixel (col, row) sits at xs = (float)col + pn_fract(jx), ys = (float)row + pn_fract(jy): k_raygen's
 *   jitter, the same draws.  For output pixel (px, py): ox = xs - ((float)px + 0.5f), oy = ys - ((float)py + 0.5f).
 *   Support: the sample counts iff pn_abs(ox) <= rx && pn_abs(oy) <= ry (inclusive); outside it is skipped, inside it is
 *   added even with weight 0.  Weight w = fx(ox) * fy(oy), each factor with its own axis's radius r:
 *     BOX       1.0f                                                                   (pbrt-v3 default radius 0.5)
 *     TRIANGLE  pn_max(r - pn_abs(o), 0.0f)                                            (2)
 *     GAUSSIAN  pn_max(pn_exp((-alpha * o) * o) - pn_exp((-alpha * r) * r), 0.0f)     (2, alpha 2) — pbrt-v3's form: filter.rs:40-41
 *               misses the first term's .exp() (every weight 0 there; the reference never calls it)
 *     MITCHELL  x = pn_abs(2.0f * (o / r)), RN(1/6) * poly(x): filter.rs:72-90's coefficients, each computed in f32 from B, C in
 *               the written order, the x > 1.0f branch or the other, Horner as float.rs:106-110 (fold from 0)   (2, B = C = 1/3)
 *     LANCZOS   sinc(pn_abs(o) / tau) * sinc(pn_abs(o)), sinc(x) = pn_abs(x) < 1e-5f ? 1.0f : pn_sin(PN_PI * x) / (PN_PI * x)  (4, tau 3)
 *   Per output pixel, from S = (+0, +0, +0), W = +0: for sample index i = 0 .. spp-1, for dy = -hy .. hy, for dx = -hx .. hx
 *   (h = floor(r + 0.5) per axis), neighbour q = (px + dx, py + dy) inside the camera film (samples exist only there), each
 *   sample of q inside the support: S.c = S.c + w * L.c per channel, then W = W + w.  Result: W == 0 gives 0, else
 *   v = S.c * (1.0f / W), then v < 0 ? +0 : v (pbrt-v3's clamp of negative lobes; a NaN stays NaN, as in the plain image).
 *   The sample index is the outer loop, so the result does not depend on the passes; a tile traces its pixels plus hx columns
 *   and hy rows of halo (clipped to the film) and writes its own pixels, so a filtered tile is the same crop of the filtered
 *   full frame, bit for bit.
 * pbrs_stats: samples = samples traced, halo included; invalid_samples = the tile's own pixels only (the plain render's count);
 * the filter stage's time counts in ms_accumulate.  The filter's weights use the render's own camera samples only (AOVs stay
 * per-pixel means: pbrs_render_tile_aovs).
 * Refused with PBRS_E_INVALID (the context stays usable): a NULL filter, band_count > 1, the visualiser integrators, an unknown
 * kind, a radius that is not finite or not > 0, a non-finite parameter of the kind; a radius above PBRS_FILTER_MAX_RADIUS in
 * either axis is PBRS_E_LIMIT. */
enum pbrs_filter_kind { PBRS_FILTER_BOX = 0, PBRS_FILTER_TRIANGLE = 1, PBRS_FILTER_GAUSSIAN = 2, PBRS_FILTER_MITCHELL = 3, PBRS_FILTER_LANCZOS = 4 };
#define PBRS_FILTER_MAX_RADIUS 4.0f
typedef struct pbrs_pixel_filter {
    uint32_t kind;     /* enum pbrs_filter_kind */
    float radius[2];   /* pbrt-v3 "xwidth", "ywidth" (they are radii) */
    float a, b;        /* GAUSSIAN: alpha, -; MITCHELL: B, C; LANCZOS: tau, -; else unused */
    uint32_t pad;
} pbrs_pixel_filter;   /* 24 B */
/* pbrs_render_tile / pbrs_render_tile_device through the filter above; _device is asynchronous like pbrs_render_tile_device. */
int pbrs_render_tile_filtered(pbrs_ctx*, const pbrs_camera*, const pbrs_render_params*, const pbrs_pixel_filter*, float* rgb_out_host,
                              pbrs_stats* stats_out);
int pbrs_render_tile_filtered_device(pbrs_ctx*, const pbrs_camera*, const pbrs_render_params*, const pbrs_pixel_filter*,
                                     float* rgb_out_device, pbrs_stats* stats_out);

/* Denoiser: the edge-avoiding a-trous wavelet filter of Dammertz, Sewtz, Hanika and Lensch (HPG 2010) over a finished image, guided by
 * the first-hit AOVs above.  An image operation: it needs a context (device, stream) and no uploaded scene.  All arithmetic is f32
 * without fused multiply-add, in the order written; pn_* is include/pbrs_numeric.h; p, q are pixels of the w x h image, c = r, g, b.
 *   Demodulation.  With PBRS_DENOISE_DEMODULATE: d.c = albedo(p).c > albedo_floor ? albedo(p).c : 1.0f (a miss, an emitter, a black
 *     lobe and a NaN albedo give 1) and c_0(p).c = rgb(p).c / d.c.  Without the flag c_0 = rgb and d = 1.
 *   Iteration k = 0 .. iterations-1, tap spacing s = 1 << k, gives c_{k+1} from c_k.  For pixel p, from S = (+0, +0, +0), W = +0:
 *     for dy = -2 .. 2 (outer), for dx = -2 .. 2 (inner): q = p + s * (dx, dy).  q outside the image is skipped; q with a channel of
 *     c_k(q) that is not finite (pn_isfinite) is skipped.  Otherwise
 *       spline   hw = K[|dx|] * K[|dy|], K = {0.375f, 0.25f, 0.0625f} (the B3 spline; every product is exact in f32)
 *       colour   e.c = c_k(q).c - c_k(p).c, d2 = (e.r * e.r + e.g * e.g) + e.b * e.b, wc = pn_exp(-d2 * ic_k) with
 *                sc_k = sigma_color * pn_exp2i(-k), ic_k = 1.0f / (sc_k * sc_k): the colour sigma halves every iteration
 *       normal   guides.normal != NULL: the same d2 on normal(q) - normal(p), wn = pn_exp(-d2 * (1.0f / (sigma_normal * sigma_normal)));
 *                NULL: wn = 1.0f
 *       depth    guides.depth != NULL, zp = depth(p), zq = depth(q) (+inf where no sample hit): both infinite (pn_isinf): wd = 1.0f;
 *                exactly one infinite: wd = +0; otherwise r = ((zq - zp) / zp) / (float)s and
 *                wd = pn_exp(-(r * r) * (1.0f / (sigma_depth * sigma_depth))) — a relative slope per pixel of tap distance, so a
 *                slanted plane does not stop the filter at large s.  NULL: wd = 1.0f
 *       wgt = ((hw * wc) * wn) * wd; with PBRS_DENOISE_ID_STOP, instance(q) != instance(p) makes wgt = +0 whatever the stops gave.
 *     A tap whose wgt is NaN (wgt != wgt: a non-finite guide value, or zp == 0) is skipped.  Otherwise S.c = S.c + wgt * c_k(q).c per
 *     channel, then W = W + wgt.  The centre tap weighs 0.140625f, so W > 0 whenever the guides at p are finite.
 *     c_{k+1}(p).c = S.c * (1.0f / W).  If W == 0 (only a non-finite guide at p itself does that), or if a channel of c_k(p) is
 *     not finite, c_{k+1}(p) = c_k(p): the pixel passes through, a NaN stays visible as in the plain image and, by the tap rule,
 *     contaminates no neighbour.
 *   Result.  out(p).c = c_N(p).c * d.c with PBRS_DENOISE_DEMODULATE, c_N(p).c without.
 * A result pixel depends on 2 * (2^iterations - 1) pixels of surround per side, so the calls take whole images, not tiles.
 * Guides are the layouts pbrs_aov_buffers writes (albedo, normal: 3 x f32 per pixel; depth: f32; instance: u32); any pointer may be
 * NULL: that stop is off.  Pointers are host memory for pbrs_denoise (which synchronises before it returns), device memory for
 * pbrs_denoise_device, which runs on the context's stream (pbrs_set_stream honoured) and does not wait on the device: queued after
 * pbrs_render_tile_aovs_device on the same context it needs no synchronisation in between, and its output is valid when that
 * render's would be (pbrs_collect_stats, or the stream's order).  rgb_out may equal rgb_in.
 * Memory: the first call allocates 52 B of scratch per pixel (two ping-pong colour planes {c.rgb, finite flag} and a guide plane
 * {normal.xyz, depth} of 16 B each, the instance ids 4 B; pbrs_denoise another 44 B per pixel of staging), a larger image grows it,
 * pbrs_destroy frees it; a context that never denoises allocates nothing.
 * Refused with PBRS_E_INVALID (the context stays usable): NULL params, rgb_in, rgb_out or guides; w or h 0; iterations 0 or above
 * PBRS_DENOISE_MAX_ITERATIONS; a sigma that is not finite or not > 0; an albedo_floor that is not finite or < 0; unknown flag bits;
 * PBRS_DENOISE_DEMODULATE without guides.albedo; PBRS_DENOISE_ID_STOP without guides.instance.  w * h above 2^28: PBRS_E_LIMIT. */
#define PBRS_DENOISE_MAX_ITERATIONS 6
#define PBRS_DENOISE_DEMODULATE 1u /* filter rgb / albedo, multiply back afterwards */
#define PBRS_DENOISE_ID_STOP 2u    /* a tap on another instance id has weight 0      */
typedef struct pbrs_denoise_params {
    uint32_t w, h;       /* image size; every buffer is w*h pixels, row-major */
    uint32_t iterations; /* 1 .. PBRS_DENOISE_MAX_ITERATIONS: iteration k uses tap spacing 1 << k */
    uint32_t flags;      /* PBRS_DENOISE_* */
    float sigma_color, sigma_normal, sigma_depth; /* finite and > 0 */
    float albedo_floor;                           /* finite and >= 0 */
} pbrs_denoise_params;                            /* 32 B */
typedef struct pbrs_denoise_guides {
    const float* albedo;
    const float* normal;
    const float* depth;
    const uint32_t* instance;
} pbrs_denoise_guides;
int pbrs_denoise(pbrs_ctx*, const pbrs_denoise_params*, const float* rgb_in_host, const pbrs_denoise_guides* guides_host, float* rgb_out_host);
int pbrs_denoise_device(pbrs_ctx*, const pbrs_denoise_params*, const float* rgb_in_device, const pbrs_denoise_guides* guides_device,
                        float* rgb_out_device);

/* ---- parity-harness entry points (the reference's own functions, batched) -------------------------- */
typedef struct pbrs_hit_record {
    float t;
    uint32_t inst; /* 0xffffffff = miss */
    uint32_t prim;
    float b1, b2;
} pbrs_hit_record;
/* `scene.tlas.intersect(&mut ray)` (tlas/src/bvh.rs:77-103) / `scene.tlas.occludes(&ray)` (:105-113)
 * for n caller-supplied rays (host pointers; origins/dirs are n*3 floats). Either output may be NULL. */
int pbrs_intersect_rays(pbrs_ctx*, uint32_t n, const float* origins, const float* dirs, const float* tmax,
                        pbrs_hit_record* hits_out, uint8_t* occluded_out);
/* Which walks the context's last pbrs_intersect_rays call went through: every query takes the walk its stage runs in the pipeline
 * for the uploaded scene (occlusion: the four-wide any-hit walk of k_shadow where the TLAS is scanned and the BLASes are deep
 * enough, with its hand-off of rays outside the guarded range to the binary walk; closest hit: the binary walk).  slow_*: rays the
 * wide walk handed to the binary walk (0 when the stage runs the binary walk anyway). */
typedef struct pbrs_intersect_info {
    uint32_t wide_any, wide_closest;
    uint32_t slow_any, slow_closest;
} pbrs_intersect_info;
int pbrs_last_intersect_info(const pbrs_ctx*, pbrs_intersect_info* out);
/* Camera rays of one sample index for a tile (src/main.rs:197-203, geometry/src/camera.rs:65-77). */
int pbrs_camera_rays(pbrs_ctx*, const pbrs_camera*, const pbrs_render_params*, uint32_t sample_index, float* origins_out,
                     float* dirs_out);
/* include/pbrs_numeric.h evaluated on the device (fn ids as oracle_numeric_eval). */
int pbrs_numeric_eval(pbrs_ctx*, uint32_t fn, uint32_t n, const float* x, const float* y, float* out);
/* Its functions of more than two operands (include/pbrs_numeric_probe.h: pn_probe_eval_k): `ops` is an n x k matrix of 32-bit
 * words, row-major, k <= 16; out[i] is the result word of row i. */
int pbrs_numeric_eval_k(pbrs_ctx*, uint32_t fn, uint32_t n, uint32_t k, const uint32_t* ops, uint32_t* out);
/* src/bsdf.rs evaluated on the device for n queries against a material of the uploaded scene, through the code k_shade runs
 * (device/bsdf.h): the frame of bsdf_new_frame over the query's normal and tangent, the material's lobes, then one of
 *   PBRS_BSDF_EVAL             f = BSDF::eval(wo, wi)
 *   PBRS_BSDF_PDF              pr = BSDF::pdf(wo, wi)
 *   PBRS_BSDF_SAMPLE           (f, wi_out, pr) = BSDF::sample(wo, u, v)
 *   PBRS_BSDF_SAMPLE_SPECULAR  BSDF::sample_specular(wo): flag bit 1 and (f, wi_out, pr) where the material has a Specular lobe
 * A query is 16 words: material index (u32), then f32 normal[3], tangent[3], wo[3], wi[3] (world space), u, v, and a spare word
 * that is ignored.  PBRS_BSDF_SAMPLE asks for 0 <= u < 1: BSDF::sample picks lobe `(u * n) as usize`.  A result is 8 words:
 * f32 f[3], wi_out[3], pr, then a u32 of flags (PBRS_BSDF_IS_MASS: pr is a mass; PBRS_BSDF_FOUND); what an op does not return is 0.
 * `lambert` != 0 runs the kernel specialised as k_shade's PBRS_SHADE_LAMBERT variants are, and is accepted only for a scene whose
 * every lobe is an untextured Lambertian DiffuseReflect (the scenes those variants render).  Scenes with a Fourier material run
 * the lobe in its generic form (no LDS series column).
 * Refused with PBRS_E_INVALID (the context stays usable): no scene uploaded; NULL queries or results; an unknown op; a material index
 * out of range; a material with PBRS_MATERIAL_TEXTURED (its lobes depend on the hit's uv and position, which a query does not
 * carry); `lambert` on another scene; for PBRS_BSDF_SAMPLE a u that is not in [0, 1), NaN included.  n == 0 returns PBRS_OK and
 * touches nothing. */
#define PBRS_BSDF_EVAL 0u
#define PBRS_BSDF_PDF 1u
#define PBRS_BSDF_SAMPLE 2u
#define PBRS_BSDF_SAMPLE_SPECULAR 3u
#define PBRS_BSDF_QUERY_WORDS 16u
#define PBRS_BSDF_RESULT_WORDS 8u
#define PBRS_BSDF_IS_MASS 1u
#define PBRS_BSDF_FOUND 2u
int pbrs_bsdf_eval(pbrs_ctx*, uint32_t op, uint32_t lambert, uint32_t n, const uint32_t* queries, uint32_t* results);
/* Per-sample radiance of one sample index for a tile (before the sum over samples), for bisecting. */
int pbrs_render_sample_radiance(pbrs_ctx*, const pbrs_camera*, const pbrs_render_params*, uint32_t sample_index, float* rgb_out_host);

/* ---- the variance AOV and the variance-guided denoiser ----------------------------------------------- */
/* In both: f32 without fused multiply-add, in the order written; pn_* is include/pbrs_numeric.h;
 * lum(c) = (0.21267127f * c.r + 0.71515972f * c.g) + 0.07216883f * c.b.
 *
 * Variance AOV.  pbrs_render_tile_aovs[_device] plus `variance`: w*h f32, the tile / band packing of rgb_out; NULL = exactly
 * pbrs_render_tile_aovs[_device].  The image and the seven AOVs are the bits of that call.  For a pixel, L_i the radiance of its
 * sample index i (what pbrs_render_sample_radiance exports):
 *   from m1 = +0, m2 = +0, n = 0; for i = 0 .. spp-1 in order: y = lum(L_i); if pn_isfinite(y): m1 = m1 + y, m2 = m2 + y * y, n = n + 1
 *   n < 2: variance = +inf ("unknown": the denoiser's luminance stop stays open)
 *   else:  mean = m1 * (1.0f / (float)n); v = m2 * (1.0f / (float)n) - mean * mean; v = v < 0 ? +0 : v;
 *          variance = v * (1.0f / (float)(n - 1))
 * — the variance of the pixel's mean luminance.  The one-pass form cancels for a nearly constant pixel; that is part of the definition
 * (the clamp catches the negative results).  The sample index is the only loop, so the result does not depend on the passes.
 * Refused like pbrs_render_tile_aovs (a requested variance counts as a requested buffer).  The context keeps 12 B of moment state per
 * pixel (m1, m2, n; the host variant 4 B per pixel of staging), allocated by the first call that asks for the variance; the kernel that
 * folds a pass runs beside k_accumulate and its time counts in pbrs_stats::ms_accumulate. */
int pbrs_render_tile_aovs_var(pbrs_ctx*, const pbrs_camera*, const pbrs_render_params*, float* rgb_out_host, const pbrs_aov_buffers* aovs_host,
                              float* variance_host, pbrs_stats* stats_out);
int pbrs_render_tile_aovs_var_device(pbrs_ctx*, const pbrs_camera*, const pbrs_render_params*, float* rgb_out_device,
                                     const pbrs_aov_buffers* aovs_device, float* variance_device, pbrs_stats* stats_out);

/* Variance-guided denoiser: pbrs_denoise with the colour stop replaced by the luminance stop of SVGF's spatial filter (Schied et al.,
 * HPG 2017): luminance differences are measured in units of the pixel's own standard deviation, and the variance is filtered along
 * with the colour, so the stop tightens by itself from one iteration to the next and no sigma depends on the units of the scene.
 * Everything pbrs_denoise's text says holds unless restated here; v_k(p) is the variance carried beside c_k(p), in [+0, +inf] with
 * +inf = "unknown".
 *   Pack.  d and c_0 as pbrs_denoise.  vin = variance(p), +inf if it is NaN or < 0.  With PBRS_DENOISE_DEMODULATE: ld = lum(d),
 *     v_0(p) = vin / (ld * ld), +inf if that is NaN (0 / 0, inf / inf); without the flag v_0 = vin.
 *   Rule for every k: where a channel of c_k(p) is not finite, v_k(p) = +inf; a v_k that comes out NaN is +inf.
 *   Iteration k = 0 .. iterations-1, tap spacing s = 1 << k.  For pixel p:
 *     Prefiltered variance, always at spacing 1: from A = +0, B = +0, for dy = -1 .. 1 (outer), dx = -1 .. 1 (inner), n = p + (dx, dy)
 *       inside the image with pn_isfinite(v_k(n)): A = A + G * v_k(n), then B = B + G, G = 0.25f (dx = dy = 0), 0.125f (one of them 0),
 *       0.0625f.  vbar = B == 0 ? +inf : A * (1.0f / B); sd = sigma_luminance * pn_sqrt(vbar).
 *     Taps: the 25 taps, their order, the skip rules, hw, wn, wd and the id stop of pbrs_denoise; instead of wc,
 *       dl = pn_abs(lum(c_k(q)) - lum(c_k(p))) and
 *       pn_isinf(sd): wl = 1.0f;  else sd == 0: wl = dl == 0 ? 1.0f : +0 (a pixel known exactly, such as an emitter seen directly, is
 *       not blurred);  else wl = pn_exp(-(dl / sd)).
 *       wgt = ((hw * wl) * wn) * wd, then the id stop and the NaN rule as before.
 *     Fold: S.c = S.c + wgt * c_k(q).c per channel, W = W + wgt, then ww = wgt * wgt and, unless ww == 0 (a closed tap must not turn an
 *       unknown neighbour into 0 * inf), V = V + ww * v_k(q), from V = +0.  An infinite v_k(q) behind an open tap makes V infinite:
 *       "unknown" spreads, and the next iteration's stop at p stays open.
 *     Result: iw = 1.0f / W; c_{k+1}(p).c = S.c * iw; v_{k+1}(p) = V * (iw * iw).  The pass-through cases of pbrs_denoise (W == 0, a
 *       non-finite channel of c_k(p)) keep v as well: v_{k+1}(p) = v_k(p).
 *     No sigma halves per iteration: the variance shrinks instead (v_{k+1} <= the largest v_k under the taps).
 *   Result.  out as pbrs_denoise.  variance_out (NULL = not wanted; may equal guides.variance): v_N(p) * (ld * ld) with
 *     PBRS_DENOISE_DEMODULATE, v_N(p) without.
 * Scale invariance.  For an integer j, denoising (rgb * 2^j, variance * 4^j) gives out * 2^j and variance_out * 4^j bit for bit, as
 * long as no product or sum above that depends on the scale (rgb / d, lum, G * v, sd, wgt * c, ww * v, S * iw, V * (iw * iw), c * d, ...)
 * overflows or is a nonzero value below the smallest normal f32 at either scale: every weight is a function of quotients dl / sd and of
 * the guides, which do not move.  (A stop that is nearly closed, wgt around 1e-38, puts wgt * c among the denormals, where the claim
 * ends.)
 * Memory: the first call allocates 52 B of scratch per pixel of its own (two ping-pong planes {c.rgb, v}, a guide plane {normal.xyz,
 * depth}, the ids; pbrs_denoise_var another 52 B per pixel of staging), grown and freed like pbrs_denoise's; a context that never calls it
 * allocates nothing.  Host / device pointers, the stream and the ordering after pbrs_render_tile_aovs_var_device: as pbrs_denoise[_device].
 * Refused with PBRS_E_INVALID (the context stays usable): what pbrs_denoise refuses (sigma_luminance in place of sigma_color), and a NULL
 * guides.variance.  w * h above 2^28: PBRS_E_LIMIT. */
typedef struct pbrs_denoise_var_params {
    uint32_t w, h;       /* image size; every buffer is w*h pixels, row-major */
    uint32_t iterations; /* 1 .. PBRS_DENOISE_MAX_ITERATIONS */
    uint32_t flags;      /* PBRS_DENOISE_DEMODULATE, PBRS_DENOISE_ID_STOP */
    float sigma_luminance, sigma_normal, sigma_depth; /* finite and > 0; sigma_luminance counts standard deviations (SVGF: 4) */
    float albedo_floor;                               /* finite and >= 0 */
} pbrs_denoise_var_params;                            /* 32 B */
typedef struct pbrs_denoise_var_guides {
    const float* albedo;
    const float* normal;
    const float* depth;
    const uint32_t* instance;
    const float* variance; /* required: f32 per pixel, as pbrs_render_tile_aovs_var writes it */
} pbrs_denoise_var_guides;
int pbrs_denoise_var(pbrs_ctx*, const pbrs_denoise_var_params*, const float* rgb_in_host, const pbrs_denoise_var_guides* guides_host,
                     float* rgb_out_host, float* variance_out_host);
int pbrs_denoise_var_device(pbrs_ctx*, const pbrs_denoise_var_params*, const float* rgb_in_device, const pbrs_denoise_var_guides* guides_device,
                            float* rgb_out_device, float* variance_out_device);

/* ---- id mattes ---------------------------------------------------------------------------------------- */
/* Per pixel the few ids that cover it and how much of the pixel each covers, from the render's own camera samples, so that a matte for
 * any set of objects can be pulled afterwards with the image's own anti-aliasing (Friedman and Jones, "Fully automatic ID mattes with
 * support for motion blur and transparency", SIGGRAPH 2015 posters: Cryptomatte).  The ids are the indices the AOVs use; names for them
 * (a manifest, hashed names) are not part of this interface.
 *
 * The key of a hit is its instance, an index into pbrs_scene_desc::instances (PBRS_MATTE_INSTANCE), or instances[instance].material
 * (PBRS_MATTE_MATERIAL).  The first hit of sample s of a pixel is the one the first-hit AOVs use (pbrs_aov_buffers): the hit record of
 * `scene.tlas.intersect` on its camera ray (bounce 0); spp = strata_x * strata_y.
 *   Per pixel a table of `slots` entries (id, count), all empty, and overflow = 0.  For sample index s = 0 .. spp-1 in order: a miss does
 *   nothing; a hit with key `id`: if an entry holds `id`, its count + 1; else if an entry is empty, the first empty one becomes (id, 1);
 *   else overflow + 1.  First come, first kept: nothing is ever evicted, so overflow == 0 means the table is exact, and the sample
 *   index is the only loop, so the result does not depend on the passes.
 *   Ranks: the used entries sorted by count, descending; equal counts: the lower id first.  Output, the tile / band packing of rgb_out:
 *     ids       u32, w * h * slots, pixel-major ([pixel][rank]); an unused rank: 0xffffffff
 *     coverage  f32, the same shape: (float)count * (1.0f / spp), the expression of the coverage AOV; an unused rank: +0
 *     residual  f32, w * h: (float)overflow * (1.0f / spp); may be NULL (not wanted)
 *   In integers, for every pixel: the sum of the counts + overflow == n_hit of the coverage AOV.
 * pbrs_render_tile_matte[_device]: pbrs_render_tile_aovs_var[_device] (`aovs` and `variance` may be NULL) that also fills the matte; a
 * NULL `matte` is exactly that call (`params` is then not read), and the image, the seven AOVs and the variance are the bits of that
 * call.  Pointers are host memory for pbrs_render_tile_matte, device memory for pbrs_render_tile_matte_device, which is asynchronous like
 * pbrs_render_tile_device: valid after pbrs_collect_stats.  Any integrator.  The matte kernels' time counts in pbrs_stats::ms_total
 * only.  The context keeps 8 * slots + 4 B of matte state per pixel (and, for the host variant, as many bytes of staging), allocated by
 * the first call that asks for a matte.  Not offered through the filtered film.
 * Refused with PBRS_E_INVALID (the context stays usable), beside what pbrs_render_tile_aovs_var refuses: PBRS_INTEGRATOR_PATH / _DIRECT
 * with max_depth == 0 (no camera ray is traced); NULL params beside a matte; slots 0 or above PBRS_MATTE_MAX_SLOTS; an unknown key; NULL
 * ids or coverage. */
#define PBRS_MATTE_INSTANCE 0u
#define PBRS_MATTE_MATERIAL 1u
#define PBRS_MATTE_MAX_SLOTS 8u
typedef struct pbrs_matte_params {
    uint32_t key;   /* PBRS_MATTE_INSTANCE or PBRS_MATTE_MATERIAL */
    uint32_t slots; /* 1 .. PBRS_MATTE_MAX_SLOTS: entries kept (and ranks written) per pixel */
} pbrs_matte_params; /* 8 B */
typedef struct pbrs_matte_buffers {
    uint32_t* ids;   /* w * h * slots */
    float* coverage; /* w * h * slots */
    float* residual; /* w * h; may be NULL */
} pbrs_matte_buffers;
int pbrs_render_tile_matte(pbrs_ctx*, const pbrs_camera*, const pbrs_render_params*, float* rgb_out_host, const pbrs_aov_buffers* aovs_host,
                           float* variance_host, const pbrs_matte_params* params, const pbrs_matte_buffers* matte_host, pbrs_stats* stats_out);
int pbrs_render_tile_matte_device(pbrs_ctx*, const pbrs_camera*, const pbrs_render_params*, float* rgb_out_device,
                                  const pbrs_aov_buffers* aovs_device, float* variance_device, const pbrs_matte_params* params,
                                  const pbrs_matte_buffers* matte_device, pbrs_stats* stats_out);

/* The mask of a set of ids, pulled from the layers above.  An image operation like pbrs_denoise: it needs a context (device, stream)
 * and no uploaded scene.  `ids` and `coverage` are w * h * slots as pbrs_render_tile_matte writes them; `select` is n_select ids in
 * strictly ascending order (NULL allowed when n_select == 0).  For every pixel, from m = +0, for rank r = 0 .. slots-1 in order: where
 * ids[r] is one of the selected ids, m = m + coverage[r].  mask_out: f32, w * h.
 * ids, coverage and mask_out are host memory for pbrs_matte_mask (which synchronises before it returns), device memory for
 * pbrs_matte_mask_device, which runs on the context's stream (pbrs_set_stream honoured): queued after pbrs_render_tile_matte_device on
 * the same context it needs no synchronisation in between, and its output is valid when that render's would be.  `select` is host
 * memory in both (a parameter, like the structs: the call checks and copies it before it returns).
 * Memory: the first call allocates PBRS_MATTE_MAX_SELECT * 4 B for the selection; pbrs_matte_mask another 8 * slots + 4 B per pixel of
 * staging, shared with pbrs_render_tile_matte's.
 * Refused with PBRS_E_INVALID (the context stays usable): NULL ids, coverage or mask_out; w or h 0; slots 0 or above
 * PBRS_MATTE_MAX_SLOTS; n_select above PBRS_MATTE_MAX_SELECT (the selection is staged in LDS: 16 KB); NULL select with n_select > 0; a
 * selection that is not strictly ascending.  w * h above 2^28: PBRS_E_LIMIT. */
#define PBRS_MATTE_MAX_SELECT 4096u
int pbrs_matte_mask(pbrs_ctx*, uint32_t w, uint32_t h, uint32_t slots, const uint32_t* ids_host, const float* coverage_host,
                    const uint32_t* select, uint32_t n_select, float* mask_out_host);
int pbrs_matte_mask_device(pbrs_ctx*, uint32_t w, uint32_t h, uint32_t slots, const uint32_t* ids_device, const float* coverage_device,
                           const uint32_t* select, uint32_t n_select, float* mask_out_device);

/* ---- light passes -------------------------------------------------------------------------------------- */
/* Direct and indirect light beside the image, each with the variance of its pixel mean, from the render's own camera samples: what a
 * compositor takes as separate layers, and what lets the variance-guided denoiser filter the two apart (SVGF filters direct and indirect
 * illumination separately: direct light is nearly converged at a few samples per pixel, the noise sits in the indirect light).  All
 * arithmetic is f32 without fused multiply-add, in the order written; lum is the variance AOV's.
 *
 * For camera sample i of a pixel, rendered with PBRS_INTEGRATOR_PATH at max_depth >= 1:
 *   L_i  its radiance (what pbrs_render_sample_radiance exports).
 *   D_i  its radiance after the first path vertex: the emission of the surface hit, or the environment a primary miss sees, plus the
 *        light estimate at the first hit (`radiance` after the first iteration of src/pathintegrator.rs:14-71).  Neither the random
 *        draws nor Russian roulette depend on `depth`, so D_i is L_i of the same sample rendered at max_depth = 1, bit for bit.
 *   I_i  = L_i - D_i, per component.  A path that ends at its first vertex gives +0; non-finite values propagate as written
 *        (inf - inf is NaN).  Emission picked up behind a specular bounce belongs to I_i.
 * Outputs, the tile / band packing of rgb_out, spp = strata_x * strata_y; every pointer may be NULL (not wanted):
 *   direct             3 x f32 row-major RGB: (sum_i D_i, i ascending, from +0) * (1.0f / spp)
 *   indirect           3 x f32: the same over I_i
 *   direct_variance    f32: the variance AOV's recipe with lum(D_i) in the place of lum(L_i), its skip of non-finite luminances and its
 *                      +inf below two finite samples included
 *   indirect_variance  f32: the same with lum(I_i)
 * The sample index is the only loop, so no output depends on the passes.  direct + indirect equals the image only to rounding, not
 * bit for bit: the image sums L_i, the layers sum D_i and L_i - D_i, and each of those sums and differences rounds on its own.
 * pbrs_render_tile_passes[_device]: pbrs_render_tile_matte[_device] (`aovs`, `variance`, `matte` may be NULL) that also fills the light
 * passes; `passes` NULL or all-NULL is exactly that call, and the image, the AOVs, the variance and the matte are the bits of that call
 * whatever is asked for here.  Pointers are host memory for pbrs_render_tile_passes, device memory for pbrs_render_tile_passes_device,
 * which is asynchronous like pbrs_render_tile_device: valid after pbrs_collect_stats.  Row bands are supported.  While passes are
 * wanted every path of a pass carries 16 B more state (D_i beside L_i; the samples per pass chosen for samples_per_pass = 0 account for
 * it) and the context keeps 48 B of state per pixel (the host variant 32 B per pixel of staging), allocated by the first call that asks
 * for a pass; a render that asks for none allocates none of it, launches the kernels it launched before and takes passes of the same
 * size.  Two kernels per pass (one copies D_i behind bounce 0, one folds the pass beside k_accumulate: its time counts in
 * pbrs_stats::ms_accumulate; the copy's in ms_total only).  Not offered through the filtered film.
 * Refused with PBRS_E_INVALID (the context stays usable), beside what pbrs_render_tile_matte refuses, when a pass is wanted: any integrator
 * but PBRS_INTEGRATOR_PATH (the direct integrator has depth semantics of its own and keeps 1 / mass beside its radiance; the visualisers
 * bypass the film); max_depth == 0. */
typedef struct pbrs_pass_buffers {
    float* direct;            /* w * h * 3 */
    float* indirect;          /* w * h * 3 */
    float* direct_variance;   /* w * h */
    float* indirect_variance; /* w * h */
} pbrs_pass_buffers;          /* NULL = not wanted */
int pbrs_render_tile_passes(pbrs_ctx*, const pbrs_camera*, const pbrs_render_params*, float* rgb_out_host, const pbrs_aov_buffers* aovs_host,
                            float* variance_host, const pbrs_matte_params* matte_params, const pbrs_matte_buffers* matte_host,
                            const pbrs_pass_buffers* passes_host, pbrs_stats* stats_out);
int pbrs_render_tile_passes_device(pbrs_ctx*, const pbrs_camera*, const pbrs_render_params*, float* rgb_out_device,
                                   const pbrs_aov_buffers* aovs_device, float* variance_device, const pbrs_matte_params* matte_params,
                                   const pbrs_matte_buffers* matte_device, const pbrs_pass_buffers* passes_device, pbrs_stats* stats_out);

/* Puts the two layers back together: rgb_out = direct + indirect per component, w * h * 3 f32 each.  An image operation like
 * pbrs_denoise: it needs a context (device, stream) and no uploaded scene.  rgb_out may be either input.  Host memory for
 * pbrs_combine_passes (which synchronises before it returns; it stages through the host render's pass staging), device memory for
 * pbrs_combine_passes_device, which runs on the context's stream (pbrs_set_stream honoured) and does not wait: queued after
 * pbrs_render_tile_passes_device or pbrs_denoise_var_device on the same context it needs no synchronisation in between.
 * Refused with PBRS_E_INVALID: a NULL pointer, w or h 0.  w * h above 2^28: PBRS_E_LIMIT. */
int pbrs_combine_passes(pbrs_ctx*, uint32_t w, uint32_t h, const float* direct_host, const float* indirect_host, float* rgb_out_host);
int pbrs_combine_passes_device(pbrs_ctx*, uint32_t w, uint32_t h, const float* direct_device, const float* indirect_device,
                               float* rgb_out_device);

/* ---- temporal accumulation ------------------------------------------------------------------------------ */
/* The temporal half of SVGF (Schied et al., HPG 2017): the previous frame's accumulated colour, luminance moments and history length
 * are reprojected to this frame through the two cameras and the depth AOV, tested against the previous frame's guides, and blended
 * with this frame's image; the variance of the accumulated pixel comes from the moments once the history is long enough.  Only the
 * camera moves (instances have no motion here; pbrs_temporal_accumulate_motion below carries a surface point through its instance's
 * own motion), and a miss pixel (depth +inf) gets no history.  An image operation like pbrs_denoise:
 * it needs a context (device, stream) and no uploaded scene.  All arithmetic is f32 without fused multiply-add, in the order written;
 * pn_* is include/pbrs_numeric.h; lum is the variance AOV's; dot(p, q) = (p.x * q.x + p.y * q.y) + p.z * q.z;
 * cross(p, q) = (p.y * q.z - p.z * q.y, p.z * q.x - p.x * q.z, p.x * q.y - p.y * q.x); d2 is pbrs_denoise's squared distance.
 * center, c, a, b are `cam`'s, the primed ones `cam_prev`'s.  For pixel p = (px, py), cur = rgb(p), y = lum(cur):
 *   A. Non-finite pixel.  A channel of cur is not finite (pn_isfinite): rgb_out = cur, moments_out = (+0, +0), length_out = +0,
 *      variance_out = +inf.  The NaN stays visible in this frame; length 0 carries nothing into the next one (rule B skips it).
 *   B. Reprojection, with history_in != NULL and z = depth(p) finite and > 0.
 *      x = (float)px + 0.5f, yc = (float)py + 0.5f; dir = (c + a * x) + b * yc per component (the camera ray through the pixel's
 *      centre); P = center + dir * z (the depth AOV is the ray parameter of that direction, not normalised: the surface point).
 *      e = P - center'; nu = cross(b', c'), nv = cross(c', a'), nw = cross(a', b'), D = dot(a', nu) (Cramer's rule for
 *      e = wq * (c' + a' * xq + b' * yq)).  wq = dot(e, nw) / D: the depth the previous frame would have recorded; rejected unless
 *      pn_isfinite(wq) && wq > 0.  xq = (dot(e, nu) / D) / wq, yq = (dot(e, nv) / D) / wq; fx = xq - 0.5f, fy = yq - 0.5f; rejected
 *      unless fx > -1.0f && fx < (float)w && fy > -1.0f && fy < (float)h (a NaN rejects; the casts below stay in range).
 *      ix = pn_f32_to_i32(pn_floor(fx)), tx = fx - pn_floor(fx); iy, ty likewise.  Taps j = 0, 1 (outer), i = 0, 1 (inner):
 *      q = (ix + i, iy + j), bw = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty).  A tap counts only if q is inside the image, bw > 0,
 *      length_in(q) > 0 (a NaN fails), every channel of rgb_in(q) and both moments are finite, zq = depth'(q) is finite and
 *      pn_abs(zq - wq) <= depth_tolerance * wq, with both normals given d2(normal'(q) - normal(p)) <= normal_tolerance *
 *      normal_tolerance, and with PBRS_TEMPORAL_ID_TEST instance'(q) == instance(p).  For each counted tap, from +0:
 *      S.c = S.c + bw * rgb_in(q).c, A1 = A1 + bw * m1(q), A2 = A2 + bw * m2(q), N = N + bw * length_in(q), W = W + bw.
 *      W == 0 or a rejected pixel: no history.  Otherwise iw = 1.0f / W, H = S * iw, h1 = A1 * iw, h2 = A2 * iw, n = N * iw.
 *   C. Blend.  No history: rgb_out = cur, moments_out = (y, y * y), length_out = 1.0f.  With history:
 *      n1 = pn_min(n + 1.0f, max_history), al = 1.0f / n1; rgb_out.c = H.c + al * (cur.c - H.c); m1 = h1 + al * (y - h1),
 *      m2 = h2 + al * (y * y - h2); length_out = n1: the running mean up to max_history frames, an exponential average after that.
 *   D. Variance of the accumulated pixel's luminance.  length_out >= min_temporal: v = m2 - m1 * m1; v = v < 0 ? +0 : v; a NaN becomes
 *      +inf; variance_out = v * (1.0f / length_out).  Otherwise vin = +inf where frame.variance is NULL, NaN or < 0, else variance(p),
 *      and variance_out = vin * (1.0f / length_out); +inf keeps its meaning of "unknown", as in pbrs_denoise_var.
 * Scale rule.  For an integer j, inputs times 2^j (rgb, rgb_in, m1; m2 and the variance times 4^j) give rgb_out times 2^j, the moments
 * times (2^j, 4^j), variance_out times 4^j and the same lengths, bit for bit, with pbrs_denoise_var's proviso: no product or sum that
 * depends on the scale overflows or is a nonzero value below the smallest normal f32 at either scale.
 * Layouts: frame and prev as pbrs_aov_buffers writes them (rgb, normal: 3 x f32 per pixel; variance, depth: f32; instance: u32); a history
 * is rgb 3, moments 2 (m1, m2), length 1 f32 per pixel.  history_in == NULL is the first frame of a sequence; cam_prev and prev may then
 * be NULL and are not read.  variance_out may be NULL.  The caller keeps this frame's depth, normal and instance as the next call's
 * `prev`.  Pointers inside the structs are host memory for pbrs_temporal_accumulate (which stages 108 B per pixel on first use and
 * synchronises before it returns), device memory for pbrs_temporal_accumulate_device, which needs no scratch, runs on the context's
 * stream (pbrs_set_stream honoured) and does not wait: queued behind pbrs_render_tile_passes_device and ahead of
 * pbrs_denoise_var_device on the same context it needs no synchronisation in between.  A context that never calls it allocates nothing.
 * Refused with PBRS_E_INVALID (the context stays usable): NULL params, cam, frame, frame->rgb, frame->depth, history_out or one of its
 * planes; history_in with a NULL plane or with cam_prev, prev or prev->depth NULL; a normal or an instance given for only one of the two
 * frames; PBRS_TEMPORAL_ID_TEST without frame->instance; unknown flag bits; w or h 0; a camera whose size is not w x h; max_history not
 * finite or < 1; a tolerance not finite or not > 0; min_temporal not finite or < 2; a plane of history_out equal to the matching plane of
 * history_in (the kernel gathers: it cannot run in place).  w * h above 2^28: PBRS_E_LIMIT. */
#define PBRS_TEMPORAL_ID_TEST 1u
typedef struct pbrs_temporal_params {
    uint32_t w, h;           /* whole images; both cameras must have width == w, height == h */
    uint32_t flags;          /* PBRS_TEMPORAL_ID_TEST */
    float max_history;       /* finite, >= 1: the history length saturates here (SVGF's alpha 0.2 is 5) */
    float depth_tolerance;   /* finite, > 0: relative */
    float normal_tolerance;  /* finite, > 0 */
    float min_temporal;      /* finite, >= 2: from this length on the variance comes from the temporal moments (SVGF: 4) */
    uint32_t pad;
} pbrs_temporal_params;      /* 32 B */
typedef struct pbrs_temporal_frame { /* this frame, layouts of pbrs_aov_buffers */
    const float* rgb;         /* required: the image or one light-pass layer */
    const float* variance;    /* nullable: the variance AOV of rgb */
    const float* depth;       /* required */
    const float* normal;      /* nullable */
    const uint32_t* instance; /* nullable; required with PBRS_TEMPORAL_ID_TEST */
} pbrs_temporal_frame;
typedef struct pbrs_temporal_guides { /* the previous frame's */
    const float* depth;
    const float* normal;
    const uint32_t* instance;
} pbrs_temporal_guides;
typedef struct pbrs_temporal_history {
    float* rgb;     /* w * h * 3 */
    float* moments; /* w * h * 2 */
    float* length;  /* w * h */
} pbrs_temporal_history;
int pbrs_temporal_accumulate(pbrs_ctx*, const pbrs_temporal_params*, const pbrs_camera* cam, const pbrs_camera* cam_prev,
                             const pbrs_temporal_frame* frame_host, const pbrs_temporal_guides* prev_host,
                             const pbrs_temporal_history* history_in_host, const pbrs_temporal_history* history_out_host, float* variance_out_host);
int pbrs_temporal_accumulate_device(pbrs_ctx*, const pbrs_temporal_params*, const pbrs_camera* cam, const pbrs_camera* cam_prev,
                                    const pbrs_temporal_frame* frame_device, const pbrs_temporal_guides* prev_device,
                                    const pbrs_temporal_history* history_in_device, const pbrs_temporal_history* history_out_device,
                                    float* variance_out_device);

/* ---- moving instances and motion vectors ---------------------------------------------------------------- */
/* Temporal accumulation that follows moving instances.  A sequence in which an object moves is rendered by uploading a new scene per
 * frame; instance ids are stable (`instance` indexes pbrs_scene_desc::instances, which keeps the scene spec's order), so a table with one
 * record per instance says where each surface point was one frame ago.  The caller computes the records (for rigid or affine motion
 * m = fwd_prev * inv_cur, n = the inverse transpose of m's linear part).
 * The rule is rule B of pbrs_temporal_accumulate with these lines changed, the same f32 arithmetic without fused multiply-add:
 *   After P = center + dir * z let i = instance(p).
 *   If motion != NULL && i < n_motion && !(motion[i].flags & PBRS_MOTION_IDENTITY), with m, n of motion[i] and nrm = normal(p):
 *     Pm.r = ((m[r][0] * P.x + m[r][1] * P.y) + m[r][2] * P.z) + m[r][3]      r = 0, 1, 2
 *     nm.r = (n[r][0] * nrm.x + n[r][1] * nrm.y) + n[r][2] * nrm.z            (only with both normals given)
 *   Otherwise Pm = P and nm = normal(p), their own bits.
 *   Then e = Pm - center', and the normal test reads d2(normal'(q) - nm) <= normal_tolerance * normal_tolerance.
 * An id at or above n_motion (the miss id 0xFFFFFFFF included) is a static instance: a table shorter than the scene is legal.  A
 * non-finite record needs no rule of its own: wq is not finite and the pixel has no history.  The id test, where asked for, still compares
 * instance'(q) with instance(p).  The scale rule holds unchanged (the records are not scaled).  Lights that move, and shadows or
 * reflections of a moving instance on other surfaces, are not followed: the history of such a pixel is stale until the depth, normal or
 * id test refuses it, as in SVGF, unless the call clips it to this frame's colours ("history clipping" below).
 * pbrs_temporal_accumulate_motion[_device] are pbrs_temporal_accumulate[_device] plus the table; motion == NULL with n_motion == 0 is
 * exactly that call (which forwards here), bit for bit.  The table is HOST memory in both variants and is read before the call returns:
 * the library copies it on the context's stream into a buffer of the context that grows on first need, so the device variant stays
 * asynchronous and the copy is ordered against the kernels of earlier calls (two calls with different tables need no wait in between).
 * Refused beside what pbrs_temporal_accumulate refuses: motion != NULL without frame->instance (with or without the id test) or with
 * n_motion == 0, motion == NULL with n_motion != 0: PBRS_E_INVALID; n_motion above 2^24: PBRS_E_LIMIT. */
#define PBRS_MOTION_IDENTITY 1u
typedef struct pbrs_instance_motion {
    float m[3][4];   /* a world point of THIS frame -> where the same material point was in the PREVIOUS frame's world */
    float n[3][3];   /* a normal of this frame -> the previous frame's (the caller's inverse transpose; not renormalised) */
    uint32_t flags;  /* PBRS_MOTION_IDENTITY: the record is not applied (P and the normal keep their own bits) */
    uint32_t pad[2];
} pbrs_instance_motion;  /* 96 B */
int pbrs_temporal_accumulate_motion(pbrs_ctx*, const pbrs_temporal_params*, const pbrs_camera* cam, const pbrs_camera* cam_prev,
                                    const pbrs_temporal_frame* frame_host, const pbrs_temporal_guides* prev_host,
                                    const pbrs_temporal_history* history_in_host, const pbrs_temporal_history* history_out_host,
                                    float* variance_out_host, const pbrs_instance_motion* motion, uint32_t n_motion);
int pbrs_temporal_accumulate_motion_device(pbrs_ctx*, const pbrs_temporal_params*, const pbrs_camera* cam, const pbrs_camera* cam_prev,
                                           const pbrs_temporal_frame* frame_device, const pbrs_temporal_guides* prev_device,
                                           const pbrs_temporal_history* history_in_device, const pbrs_temporal_history* history_out_device,
                                           float* variance_out_device, const pbrs_instance_motion* motion, uint32_t n_motion);

/* The screen-space motion vector AOV: the same reprojection written out per pixel, what a compositor's vector blur and an external
 * temporal denoiser take as their flow.  Rule B up to (wq, xq, yq) with the motion rule above (z = depth(p), i = instance(p)), then
 *   motion_out(p) = (xq - x, yq - yc)   where the point was minus where it is, in pixels; 2 x f32 per pixel
 *   prev_depth_out(p) = wq              the depth the previous frame would have recorded
 * without rejection by the film's bounds (a point that was off-screen still has a vector).  Where z is not finite or not > 0, or wq is
 * not finite or not > 0: motion_out(p) = (+0, +0) and prev_depth_out(p) = +inf.  prev_depth_out may be NULL; instance may be NULL only
 * when motion is NULL (it is then not read).  An image operation like pbrs_denoise: no uploaded scene is needed.  depth, instance and
 * the outputs are host memory for pbrs_motion_vectors (which stages 20 B per pixel on first use and synchronises before it returns),
 * device memory for pbrs_motion_vectors_device, which runs on the context's stream and does not wait; the table is host memory in both.
 * Refused with PBRS_E_INVALID (the context stays usable): NULL cam, cam_prev, depth or motion_out; w or h 0; a camera whose size is not
 * w x h; motion != NULL without instance or with n_motion == 0; motion == NULL with n_motion != 0.  w * h above 2^28 or n_motion above
 * 2^24: PBRS_E_LIMIT. */
int pbrs_motion_vectors(pbrs_ctx*, uint32_t w, uint32_t h, const pbrs_camera* cam, const pbrs_camera* cam_prev, const float* depth_host,
                        const uint32_t* instance_host, const pbrs_instance_motion* motion, uint32_t n_motion, float* motion_out_host,
                        float* prev_depth_out_host);
int pbrs_motion_vectors_device(pbrs_ctx*, uint32_t w, uint32_t h, const pbrs_camera* cam, const pbrs_camera* cam_prev,
                               const float* depth_device, const uint32_t* instance_device, const pbrs_instance_motion* motion,
                               uint32_t n_motion, float* motion_out_device, float* prev_depth_out_device);

/* ---- history clipping ------------------------------------------------------------------------------------ */
/* Temporal accumulation that clips the reprojected history to this frame's colours.  The surface under a moving shadow or under a light
 * that is switched does not move: its depth, normal and id never refuse the history, and the old lighting stays until the running mean
 * forgets it, max_history frames later.  Neighbourhood clipping bounds that: before the blend the history colour is clamped to
 * mean +- gamma * sigma of this frame's colours over the (2 * radius + 1)^2 window around the pixel, per channel.
 * The rule sits between rules B and C of pbrs_temporal_accumulate (with the motion step of pbrs_temporal_accumulate_motion) and applies
 * only to a pixel that has a history (W != 0).  The same f32 arithmetic without fused multiply-add, in the order written; rgb is
 * frame->rgb, H, h1, h2, n are rule B's:
 *   Box.  From s1 = s2 = (+0, +0, +0), cnt = +0, for dy = -radius .. radius (outer), for dx = -radius .. radius (inner), q = p + (dx, dy):
 *     q outside the image is skipped; q is skipped if a channel of rgb(q) is not finite (pn_isfinite).  Otherwise, per channel c,
 *     s1.c = s1.c + rgb(q).c, s2.c = s2.c + rgb(q).c * rgb(q).c, and cnt = cnt + 1.0f.  (p itself always counts: rule A has taken a
 *     non-finite p.)  ic = 1.0f / cnt; mu.c = s1.c * ic; v.c = s2.c * ic - mu.c * mu.c; v.c = v.c < 0 ? +0 : v.c; sd.c = pn_sqrt(v.c);
 *     lo.c = mu.c - gamma * sd.c; hi.c = mu.c + gamma * sd.c.
 *   Clip.  Hc.c = lo.c <= hi.c ? pn_min(pn_max(H.c, lo.c), hi.c) : H.c: a NaN bound (an overflowed sum) clips nothing in that channel.
 *   Moments and length.  If Hc.c == H.c for every c, then h1, h2 and n keep their bits.  Otherwise vh = h2 - h1 * h1;
 *     vh = vh < 0 ? +0 : vh; a NaN vh becomes +0; h1 = lum(Hc); h2 = vh + h1 * h1; n = pn_min(n, clip_history): the mean moves and the
 *     spread stays, and a shortened length sends the pixel back to the frame's variance, or to pbrs_spatial_variance, through rule D's
 *     min_temporal.
 *   Rule C then runs with Hc in the place of H; rule D is unchanged.
 * A window that holds p alone gives sd = 0 and Hc = cur.  The box is of the noisy frame, so gamma trades the lag that is left against the
 * noise the clip lets through: a history within gamma * sigma of the window's mean passes untouched.
 * Scale rule.  As pbrs_temporal_accumulate's, under the same proviso: every box quantity scales with the colours (s1, mu, sd, lo, hi by
 * 2^j; s2, v by 4^j; pn_sqrt of a value times 4^j is the root times 2^j), and cnt does not.
 * pbrs_temporal_accumulate_clip[_device] are pbrs_temporal_accumulate_motion[_device] plus `clip`; clip == NULL is exactly that call
 * (it forwards there), bit for bit.  The first frame of a sequence (history_in == NULL) has nothing to clip: `clip` is checked and not
 * used.  Memory, stream and staging are the motion call's: the device variant allocates nothing, runs on the context's stream and does
 * not wait.
 * Refused with PBRS_E_INVALID beside what pbrs_temporal_accumulate_motion refuses: radius 0 or above PBRS_CLIP_MAX_RADIUS; gamma not
 * finite or not > 0; clip_history NaN or < 1 (+inf is allowed: the length is never shortened); unknown flag bits; with clip != NULL,
 * history_out->rgb == frame->rgb (the kernel gathers a halo of frame->rgb: what the unclipped call tolerates is a race here). */
#define PBRS_CLIP_MAX_RADIUS 3u
typedef struct pbrs_history_clip_params {
    uint32_t radius;     /* 1 .. PBRS_CLIP_MAX_RADIUS: the window is (2 * radius + 1)^2 */
    float gamma;         /* finite, > 0: the box is mean +- gamma * sigma */
    float clip_history;  /* >= 1, +inf allowed: a clipped pixel's history length is at most this */
    uint32_t flags;      /* none defined: must be 0 */
} pbrs_history_clip_params; /* 16 B */
int pbrs_temporal_accumulate_clip(pbrs_ctx*, const pbrs_temporal_params*, const pbrs_camera* cam, const pbrs_camera* cam_prev,
                                  const pbrs_temporal_frame* frame_host, const pbrs_temporal_guides* prev_host,
                                  const pbrs_temporal_history* history_in_host, const pbrs_temporal_history* history_out_host,
                                  float* variance_out_host, const pbrs_instance_motion* motion, uint32_t n_motion,
                                  const pbrs_history_clip_params* clip);
int pbrs_temporal_accumulate_clip_device(pbrs_ctx*, const pbrs_temporal_params*, const pbrs_camera* cam, const pbrs_camera* cam_prev,
                                         const pbrs_temporal_frame* frame_device, const pbrs_temporal_guides* prev_device,
                                         const pbrs_temporal_history* history_in_device, const pbrs_temporal_history* history_out_device,
                                         float* variance_out_device, const pbrs_instance_motion* motion, uint32_t n_motion,
                                         const pbrs_history_clip_params* clip);

/* ---- spatial variance estimate for short histories -------------------------------------------------------- */
/* The piece of SVGF (Schied et al., HPG 2017) that joins its temporal and its spatial half.  Rule D of pbrs_temporal_accumulate takes the
 * variance from the temporal moments only from min_temporal frames on; before that it falls back on the frame's own variance AOV, which
 * at a few samples is +inf ("unknown") or very noisy, and pbrs_denoise_var then filters those pixels with its luminance stop open: every
 * pixel of the first frames of a sequence, and every pixel that is disoccluded later.  For exactly those pixels this call replaces the
 * variance by a guide-weighted estimate of the luminance moments over the (2 * radius + 1)^2 neighbourhood.  An image operation like
 * pbrs_denoise: it needs a context (device, stream) and no uploaded scene.  All arithmetic is f32 without fused multiply-add, in the order
 * written; pn_* is include/pbrs_numeric.h.  m1(q), m2(q) are the two words of `moments` at q (the layout of pbrs_temporal_history),
 * n = length(p).
 *   Pass-through.  variance_out(p) = variance_in(p), bit for bit, when
 *     p is not short: short means n > 0 && n < min_temporal (a NaN length is not short); or
 *     PBRS_SPATIAL_ONLY_UNKNOWN is set and variance_in(p) is known: neither NaN, nor < 0, nor +inf; or
 *     the sum W below comes out 0 (only a non-finite guide at p itself, or depth(p) == 0, or no valid pixel under the window does that).
 *   Estimate.  From M1 = +0, M2 = +0, W = +0, for dy = -radius .. radius (outer), for dx = -radius .. radius (inner), q = p + (dx, dy):
 *     q outside the image is skipped; q is skipped unless length(q) > 0 (a NaN fails) and m1(q), m2(q) are finite (pn_isfinite).
 *     wgt = (1.0f * wn) * wd, with wn and wd exactly pbrs_denoise's normal and depth stops at s = 1 (the both-infinite and the
 *     exactly-one-infinite depth cases included); a NULL guide gives 1.0f.  With PBRS_SPATIAL_ID_STOP, instance(q) != instance(p) makes
 *     wgt = +0.  A tap whose wgt is NaN is skipped.  Otherwise M1 = M1 + wgt * m1(q), M2 = M2 + wgt * m2(q), W = W + wgt.
 *     iw = 1.0f / W; a = M1 * iw; b = M2 * iw; v = b - a * a; v = v < 0 ? +0 : v; a NaN v becomes +inf;
 *     variance_out(p) = v * (1.0f / n).
 * What it estimates.  There is no luminance stop and no spline: a box window over the surface the guides delimit.  v is the variance of one
 * frame's pixel luminance, divided by the history length like rule D.  On flat noise it has 1 - 1 / taps of the true variance (the
 * window's own mean is subtracted), and it counts texture under the window as variance, so it errs toward more blur, never toward less.
 * Like the variance AOV's, the one-pass form cancels for a nearly constant neighbourhood (b and a * a round separately); the clamp catches
 * the negative results, and a constant neighbourhood gives +0 or a value within rounding of it.
 * Scale rule.  For an integer j, moments times (2^j, 4^j) and variance_in times 4^j give variance_out times 4^j bit for bit, with
 * pbrs_denoise_var's proviso (no product or sum that depends on the scale overflows or is a nonzero value below the smallest normal f32 at
 * either scale): every weight depends on the guides only.
 * In place.  variance_out may equal variance_in: a pixel reads only its own variance_in.  It may not alias the moments or the length
 * (the same pointer is refused).
 * Pointers are host memory for pbrs_spatial_variance, which stages what it copies (up to 36 B per pixel) on first use and synchronises
 * before it returns; device memory for pbrs_spatial_variance_device, which needs no scratch, runs on the context's stream (pbrs_set_stream
 * honoured) and does not wait: queued between pbrs_temporal_accumulate[_motion]_device and pbrs_denoise_var_device on the same context it
 * needs no synchronisation.  A context that never calls it allocates nothing.  `guides` may be NULL (every stop off), and so may each of
 * its pointers.
 * Refused with PBRS_E_INVALID (the context stays usable): NULL params, moments, length, variance_in or variance_out; w or h 0; radius 0 or
 * above PBRS_SPATIAL_MAX_RADIUS; a sigma that is not finite or not > 0; min_temporal not finite or < 1; unknown flag bits;
 * PBRS_SPATIAL_ID_STOP without guides->instance; variance_out equal to moments or length.  w * h above 2^28: PBRS_E_LIMIT. */
#define PBRS_SPATIAL_ID_STOP 1u      /* a tap on another instance id has weight 0 */
#define PBRS_SPATIAL_ONLY_UNKNOWN 2u /* a short pixel whose variance_in is known keeps it */
#define PBRS_SPATIAL_MAX_RADIUS 3u
typedef struct pbrs_spatial_variance_params {
    uint32_t w, h;        /* image size; every plane is w*h pixels, row-major */
    uint32_t radius;      /* 1 .. PBRS_SPATIAL_MAX_RADIUS: the window is (2 * radius + 1)^2 (SVGF: 3) */
    uint32_t flags;       /* PBRS_SPATIAL_* */
    float sigma_normal, sigma_depth; /* finite and > 0: pbrs_denoise's */
    float min_temporal;   /* finite, >= 1: the temporal accumulation's; shorter histories are estimated */
    uint32_t pad;
} pbrs_spatial_variance_params; /* 32 B */
typedef struct pbrs_spatial_variance_guides { /* layouts of pbrs_aov_buffers; any pointer may be NULL: that stop is off */
    const float* depth;
    const float* normal;
    const uint32_t* instance;
} pbrs_spatial_variance_guides;
int pbrs_spatial_variance(pbrs_ctx*, const pbrs_spatial_variance_params*, const float* moments_host, const float* length_host,
                          const pbrs_spatial_variance_guides* guides_host, const float* variance_in_host, float* variance_out_host);
int pbrs_spatial_variance_device(pbrs_ctx*, const pbrs_spatial_variance_params*, const float* moments_device, const float* length_device,
                                 const pbrs_spatial_variance_guides* guides_device, const float* variance_in_device,
                                 float* variance_out_device);

/* ---- display transform ----------------------------------------------------------------------------------------- */
/* The last step of the image pipeline on the device: an f32 radiance plane (a render, an accumulated or a filtered image) becomes 8-bit
 * RGBA, 4 B per pixel ready to show, through an exposure, a tone curve, a transfer function and a quantiser.  The exposure is given, or
 * follows the image (PBRS_DISPLAY_AUTO_EXPOSURE): the trimmed log-average luminance of the frame, read from a 512-bin histogram, is mapped
 * to `key`, and a sequence eases from one frame's exposure to the next.  An image operation like pbrs_denoise: it needs a context (device,
 * stream) and no uploaded scene.
 * Nothing below depends on the order in which pixels arrive, and there is no float reduction: the histogram and its resolve are integer
 * arithmetic, the per-pixel part is f32 without fused multiply-add, in the order written.  pn_* is include/pbrs_numeric.h;
 * lum(c) = (0.21267127f * c.r + 0.71515972f * c.g) + 0.07216883f * c.b.  rgb is w * h pixels, row-major, 3 floats each; rgba8_out is
 * w * h words, row-major.
 *   Histogram.  Runs when PBRS_DISPLAY_AUTO_EXPOSURE is set or io->histogram_out is given.  Y = lum(rgb(p)) of the input as given,
 *     u = pn_bits(Y).  A pixel is counted iff 0x2F800000 <= u < 0x7F800000: Y is finite and >= 2^-32 (zeros, negatives, NaN, +-inf and
 *     smaller values are not).  Its bin is min((u - 0x2F800000) >> 20, 511): eight bins per octave from 2^-32 on, taken from the exponent
 *     and three mantissa bits, without a logarithm; bin 511, [2^31.875, 2^32), also holds everything above.  Counts n_b are u32 and only
 *     ever added as integers.  histogram_out receives the PBRS_DISPLAY_BINS counts.
 *   Resolve (PBRS_DISPLAY_AUTO_EXPOSURE).  Integers, 64-bit where needed, until the last step.  N = sum of n_b.
 *     lo = (N * low_q16) >> 16, hi = (N * high_q16) >> 16; if hi == lo then lo = 0, hi = N.  K = hi - lo.  With c_b the exclusive prefix
 *     sum of n (the rank of the bin's first pixel), k_b = the size of [c_b, c_b + n_b) intersected with [lo, hi): the pixels of the bin
 *     whose rank is kept.  S = sum of k_b * (2 * b + 1).  Q = (S << 8) / K (integer division): the mean log2 luminance of the kept
 *     pixels plus 32, in 1/4096 octave, every pixel counted at the middle of its bin.
 *     Lavg = pn_ldexp(pn_exp((float)(Q & 4095) * (0.6931472f * 0.000244140625f)), (int)(Q >> 12) - 32).
 *     a = pn_clamp(key / Lavg, min_exposure, max_exposure).  With io->exposure_in whose value prev is finite and > 0:
 *     e = prev + (a - prev) * adapt; otherwise e = a.  With N == 0 (nothing counted): e = prev if it is finite and > 0, else 1.0f.
 *     Without PBRS_DISPLAY_AUTO_EXPOSURE: e = 1.0f, and exposure_in is not read.
 *     exposure_out receives e.  scale = e * exposure.
 *   Per pixel at (x, y) and per channel c of rgb(p):
 *     v = c * scale; v = v > 0 ? v : +0 (NaN, negatives and -0 become +0); v = pn_min(v, 65504.0f).
 *     Curve.  PBRS_CURVE_NONE: t = v.  PBRS_CURVE_REINHARD: t = (v * (1.0f + v * iw2)) / (1.0f + v) with iw2 = 1.0f / (white * white),
 *       which is +0 for white = +inf (plain Reinhard).  PBRS_CURVE_ACES (Narkowicz' fit):
 *       t = (v * (2.51f * v + 0.03f)) / (v * (2.43f * v + 0.59f) + 0.14f).  Then t = t < 1.0f ? t : 1.0f.
 *     Encode.  PBRS_ENCODE_SQRT: g = sqrtf(t), correctly rounded (the reference's gamma_encode).  PBRS_ENCODE_SRGB: t <= 0.0031308f gives
 *       g = 12.92f * t; t >= 1.0f gives g = 1.0f; otherwise g = 1.055f * pn_exp(pn_ln(t) * (1.0f / 2.4f)) - 0.055f.  (The formula gives
 *       0.99999994 at t = 1, which truncation would turn into 254: hence the middle case.)
 *     Quantise.  q = g * 255.0f + d; byte = q >= 255.0f ? 255 : (uint32_t)q.  PBRS_QUANT_TRUNC: d = 0 (the reference's to_u8).
 *       PBRS_QUANT_ROUND: d = 0.5f.  PBRS_QUANT_DITHER: d = ((float)M[y & 3][x & 3] + 0.5f) * 0.0625f with the 4 x 4 Bayer matrix
 *       M = {{0, 8, 2, 10}, {12, 4, 14, 6}, {3, 11, 1, 9}, {15, 7, 13, 5}}.
 *     rgba8_out(p) = r | g << 8 | b << 16 | 255u << 24.
 * Scale rule.  With PBRS_DISPLAY_AUTO_EXPOSURE, no exposure_in, the clamp inactive (min_exposure < key / Lavg < max_exposure at both
 * scales) and no counted pixel's luminance leaving [2^-32, 2^32) at either scale (nor a product that depends on the scale overflowing
 * or falling below the smallest normal f32), the image times 2^j gives the same bytes bit for bit: every bin moves by exactly 8 * j, Q by
 * 4096 * j, Lavg by 2^j and e by 2^-j.  The resolve is integer so that this holds.
 * With the reference's settings (exposure 1, PBRS_CURVE_NONE, PBRS_ENCODE_SQRT, PBRS_QUANT_TRUNC, no flag) the bytes are those
 * pbrs_host_write_png writes (include/pbrs_host.h).
 * Pointers are host memory for pbrs_display, which stages the image and the result (12 + 4 B per pixel) on first use and synchronises
 * before it returns; device memory for pbrs_display_device (the io struct itself is host memory, its pointers device memory), which runs
 * on the context's stream (pbrs_set_stream honoured) and does not wait.  The applied exposure travels in a device word: a sequence that
 * hands one frame's exposure_out to the next frame's exposure_in needs no synchronisation between frames.  `io` may be NULL, and so may
 * each of its pointers; exposure_out may be exposure_in.  A context that never calls this allocates nothing; one that does holds one small
 * scratch (the histogram and the exposure word, about 2 KiB), zeroed on the stream before each call that fills it.  The vector path of the
 * per-pixel kernel needs rgb and rgba8_out 16-byte aligned; other pointers take a scalar path with the same bytes.
 * Refused with PBRS_E_INVALID (the context stays usable): NULL params, rgb or rgba8_out; w or h 0; an unknown curve, encode or quantize
 * value; unknown flag bits; exposure or key not finite or <= 0; white NaN or <= 0; min_exposure or max_exposure not finite or <= 0, or
 * min_exposure > max_exposure; adapt outside (0, 1]; low_q16 >= high_q16 or high_q16 > 65536; rgba8_out equal to rgb.  key, min_exposure,
 * max_exposure, adapt, low_q16 and high_q16 are checked only with PBRS_DISPLAY_AUTO_EXPOSURE.  w * h above 2^28: PBRS_E_LIMIT. */
#define PBRS_DISPLAY_BINS 512u
#define PBRS_CURVE_NONE 0u
#define PBRS_CURVE_REINHARD 1u
#define PBRS_CURVE_ACES 2u
#define PBRS_ENCODE_SQRT 0u /* the reference's gamma_encode */
#define PBRS_ENCODE_SRGB 1u
#define PBRS_QUANT_TRUNC 0u /* the reference's to_u8 */
#define PBRS_QUANT_ROUND 1u
#define PBRS_QUANT_DITHER 2u
#define PBRS_DISPLAY_AUTO_EXPOSURE 1u
typedef struct pbrs_display_params {
    uint32_t w, h;                    /* image size */
    uint32_t curve, encode, quantize; /* PBRS_CURVE_*, PBRS_ENCODE_*, PBRS_QUANT_* */
    uint32_t flags;                   /* PBRS_DISPLAY_* */
    float exposure;                   /* finite, > 0: multiplies the image (with AUTO_EXPOSURE: a compensation on top) */
    float key;                        /* AUTO_EXPOSURE: the value the trimmed log-average luminance is mapped to (0.18) */
    float white;                      /* REINHARD: the value mapped to 1; > 0, +inf allowed (plain Reinhard) */
    float min_exposure, max_exposure; /* AUTO_EXPOSURE: finite, 0 < min <= max */
    float adapt;                      /* AUTO_EXPOSURE with exposure_in: in (0, 1]; 1 = jump to the new exposure */
    uint32_t low_q16, high_q16;       /* AUTO_EXPOSURE: ranks kept, in 1/65536 of the counted pixels; low < high <= 65536 */
    uint32_t pad[2];
} pbrs_display_params; /* 64 B */
typedef struct pbrs_display_io { /* each pointer may be NULL */
    const float* exposure_in;  /* one float: the previous frame's exposure_out */
    float* exposure_out;       /* one float: e */
    uint32_t* histogram_out;   /* PBRS_DISPLAY_BINS words */
} pbrs_display_io;
/* ACES, sRGB, rounding, no flag, exposure 1, key 0.18, white +inf, exposure limits 2^-20 and 2^20, adapt 1, ranks 6554 .. 62259 (the
 * darkest 10 % and the brightest 5 % are trimmed); `out` NULL does nothing.  Host code: needs no context. */
void pbrs_display_params_default(uint32_t w, uint32_t h, pbrs_display_params* out);
int pbrs_display(pbrs_ctx*, const pbrs_display_params*, const float* rgb_host, const pbrs_display_io* io_host, uint32_t* rgba8_out_host);
int pbrs_display_device(pbrs_ctx*, const pbrs_display_params*, const float* rgb_device, const pbrs_display_io* io_device,
                        uint32_t* rgba8_out_device);

/* ---- guided upsampling ------------------------------------------------------------------------------------------ */
/* Joint bilateral upsampling (Kopf, Cohen, Lischinski and Uyttendaele, SIGGRAPH 2007): an image traced and filtered at 1 / factor of the
 * resolution per axis is rebuilt at full size with weights taken from first-hit guides rendered at full size, which cost one cast per
 * pixel.  With albedo demodulation the texture detail comes back from the full-size albedo.  An image operation like pbrs_denoise: it
 * needs a context (device, stream) and no uploaded scene.  All arithmetic is f32 without fused multiply-add, in the order written; pn_* is
 * include/pbrs_numeric.h; c = r, g, b.
 *   Sizes.  w x h is the full size, factor f in {2, 3, 4} applies to both axes, the low size is wl = (w + f - 1) / f, hl = (h + f - 1) / f.
 *     rgb_lo and the planes of guides_lo are wl x hl, out, weight_out and the planes of guides_hi are w x h, all row-major.  Low pixel
 *     Q = (X, Y) lies under the full pixels fX .. fX + f - 1, fY .. fY + f - 1.
 *   Demodulation.  With PBRS_UPSAMPLE_DEMODULATE: d(.).c = albedo.c > albedo_floor ? albedo.c : 1.0f, exactly pbrs_denoise's, d_lo(Q)
 *     from guides_lo->albedo and d_hi(p) from guides_hi->albedo; c(Q).c = rgb_lo(Q).c / d_lo(Q).c.  Without the flag c = rgb_lo, d = 1.
 *   Footprint of full pixel p = (x, y).  X0 = floor_div(2x + 1 - f, 2f) in integer arithmetic (floor toward -inf), Y0 likewise.  The taps
 *     are Y = Y0 - R + 1 .. Y0 + R (outer, ascending), X = X0 - R + 1 .. X0 + R (inner, ascending), R = radius in {1, 2}.  With
 *     D = 2 * f * R: nx = |2f * X + f - (2x + 1)|, ny likewise (integers: twice the distance of the centres in full pixels).  A tap outside
 *     the low image is skipped; a tap with nx >= D or ny >= D is skipped.  Otherwise
 *       hw = ((float)(D - nx) / (float)D) * ((float)(D - ny) / (float)D),
 *     a tent of half-width R low pixels around p's centre (R = 1: the bilinear footprint).  A tap with a channel of c(Q) that is not
 *     finite (pn_isfinite) is skipped.
 *   Sums.  From T = (+0, +0, +0), V = +0, S = (+0, +0, +0), W = +0, per counted tap:
 *     T.c = T.c + hw * c(Q).c per channel, then V = V + hw: the unguided sums.
 *     wn, wd are exactly pbrs_denoise's normal and depth stops between the low guide at Q and the full guide at p: the normal stop on
 *     normal_lo(Q) - normal_hi(p); the depth stop with zp = depth_hi(p), zq = depth_lo(Q) and s = factor (r = ((zq - zp) / zp) /
 *     (float)factor), the both-infinite case (1.0f) and the exactly-one-infinite case (+0) included.  A guide counts when both guides_lo
 *     and guides_hi give it; a pair of NULLs gives 1.0f.
 *     g = (hw * wn) * wd; with PBRS_UPSAMPLE_ID_STOP, instance_lo(Q) != instance_hi(p) makes g = +0 whatever the stops gave.
 *     A tap whose g is NaN is left out of the guided sums only.  Otherwise S.c = S.c + g * c(Q).c per channel, then W = W + g.
 *   Result.  W > min_weight: r.c = S.c * (1.0f / W).  Else V > 0: r.c = T.c * (1.0f / V), the plain tent: it covers a full-size feature the
 *     low image does not hold, and a non-finite guide at p.  Else r = c(N), N = (x / f, y / f): a non-finite value stays visible, as
 *     everywhere in this library, and by the tap rule contaminates no pixel that has another tap.
 *     out(p).c = r.c * d_hi(p).c.  weight_out(p) = W where that plane is given (NULL: not wanted).
 * Scale rule.  The weights depend on the guides alone: rgb_lo times 2^j gives out times 2^j bit for bit, with pbrs_denoise_var's proviso
 * (no product or sum that depends on the scale overflows or is a nonzero value below the smallest normal f32 at either scale).
 * The albedo and the instance planes are read only with their flag.  Pointers are host memory for pbrs_upsample, which stages what it
 * copies on first use (up to 11 words per low pixel and 12 per full pixel) and synchronises before it returns; device memory for
 * pbrs_upsample_device (the two guide structs themselves are host memory), which needs no scratch, runs on the context's stream
 * (pbrs_set_stream honoured) and does not wait: queued behind pbrs_denoise_var_device and the guide render on the same context it needs
 * no synchronisation.  A context that never calls it allocates nothing.
 * Refused with PBRS_E_INVALID (the context stays usable): NULL params, rgb_lo, guides_lo, guides_hi or out; w or h 0; factor outside
 * 2 .. 4; radius outside 1 .. 2; a sigma that is not finite or not > 0; an albedo_floor or a min_weight that is not finite or < 0; unknown
 * flag bits; a guide given by only one of guides_lo and guides_hi; PBRS_UPSAMPLE_DEMODULATE without the albedo pair;
 * PBRS_UPSAMPLE_ID_STOP without the instance pair; out equal to rgb_lo or to a guide plane; weight_out equal to out, to rgb_lo or to a
 * guide plane.  w * h above 2^28: PBRS_E_LIMIT. */
#define PBRS_UPSAMPLE_DEMODULATE 1u /* rebuild rgb / albedo, multiply by the full-size albedo afterwards */
#define PBRS_UPSAMPLE_ID_STOP 2u    /* a tap on another instance id has weight 0 */
#define PBRS_UPSAMPLE_MIN_FACTOR 2u
#define PBRS_UPSAMPLE_MAX_FACTOR 4u
#define PBRS_UPSAMPLE_MAX_RADIUS 2u
typedef struct pbrs_upsample_params {
    uint32_t w, h;                   /* the full size */
    uint32_t factor;                 /* 2 .. 4 */
    uint32_t radius;                 /* 1 .. 2: the tent's half-width in low pixels */
    uint32_t flags;                  /* PBRS_UPSAMPLE_* */
    float sigma_normal, sigma_depth; /* finite and > 0: pbrs_denoise's */
    float albedo_floor;              /* finite and >= 0 */
    float min_weight;                /* finite and >= 0: a guided sum W at or below it falls back on the plain tent */
    uint32_t pad[3];
} pbrs_upsample_params; /* 48 B */
/* radius 1, no flag, sigma_normal 0.3, sigma_depth 0.2, albedo_floor 1e-3 (the denoiser's), min_weight 1e-3; `out` NULL does
 * nothing.  Host code: needs no context. */
void pbrs_upsample_params_default(uint32_t w, uint32_t h, uint32_t factor, pbrs_upsample_params* out);
int pbrs_upsample(pbrs_ctx*, const pbrs_upsample_params*, const float* rgb_lo_host, const pbrs_denoise_guides* guides_lo_host,
                  const pbrs_denoise_guides* guides_hi_host, float* out_host, float* weight_out_host);
int pbrs_upsample_device(pbrs_ctx*, const pbrs_upsample_params*, const float* rgb_lo_device, const pbrs_denoise_guides* guides_lo_device,
                         const pbrs_denoise_guides* guides_hi_device, float* out_device, float* weight_out_device);

/* ---- image comparison -------------------------------------------------------------------------------------------- */
/* What a step of the image chain buys: an image `a` under test is compared with a reference `b` on the device — mean squared error,
 * relative squared error, mean absolute error, the largest difference, the structural similarity index (SSIM; Wang, Bovik, Sheikh and
 * Simoncelli 2004) and, where asked for, per-pixel maps of the error and of the SSIM.  a and b are w * h pixels, row-major, 3 floats
 * each; the maps are w * h floats.  An image operation like pbrs_denoise: it needs a context (device, stream) and no uploaded scene.
 * Per-pixel image arithmetic is f32 without fused multiply-add, in the order written; error terms and sums are f64 without fused
 * multiply-add; pn_* is include/pbrs_numeric.h.  Every sum has one stated order, so the result does not depend on the launch shape or on
 * the order in which blocks finish, and a CPU model of this text gives the same 64 bytes.
 *   Validity.  A pixel p is valid when all six values a(p).c, b(p).c, c = r, g, b, pass pn_isfinite.  n_valid and n_invalid count the two
 *     kinds.  An invalid pixel contributes +0.0 to every sum and weight 0 to every window.
 *   Transform.  PBRS_COMPARE_LINEAR: t(x) = x.  PBRS_COMPARE_REINHARD: x' = x < 0 ? +0 : x, t(x) = x' / (1.0f + x'), a correctly rounded
 *     division and no libm: negative radiance counts as black, the rest lands in [0, 1).
 *   Terms.  At a valid pixel A.c = (double)t(a(p).c), B.c = (double)t(b(p).c), D.c = A.c - B.c, eps = (double)rel_epsilon:
 *       se(p) = (D.r * D.r + D.g * D.g) + D.b * D.b
 *       ae(p) = (|D.r| + |D.g|) + |D.b|
 *       re(p) = (D.r * D.r / (B.r * B.r + eps) + D.g * D.g / (B.g * B.g + eps)) + D.b * D.b / (B.b * B.b + eps)
 *   Order of every sum T(v) of a per-pixel f64 value v.  The image is cut into PBRS_COMPARE_TILE x PBRS_COMPARE_TILE tiles from pixel
 *     (0, 0).  The 256 entries of a tile are taken row-major, positions outside the image (and invalid pixels) as +0.0, and reduced by the
 *     adjacent-pair tree: v'[j] = v[2j] + v[2j + 1], until one value is left.  The tile sums, row-major over tiles and padded with +0.0
 *     to the next power of two, are reduced by the same tree.  (Adding +0.0 to a sum that is not -0.0 is exact: an implementation
 *     need not materialise padding beyond a value's first partner.)  PBRS_COMPARE_TILE is part of the contract because it fixes this order.
 *   Result.  mse = T(se) / (double)(3 * n_valid), mae = T(ae) / (double)(3 * n_valid), rel_mse = T(re) / (double)(3 * n_valid); with
 *     n_valid == 0 the three are what 0.0 / 0.0 gives (NaN).  max_abs is the largest |D.c| over valid pixels and channels, +0.0 when there
 *     are none.  The pads are written as 0.
 *   SSIM (only with PBRS_COMPARE_SSIM), on luminance through an 11 x 11 Gaussian window, sigma 1.5.
 *     lum(c) = (0.21267127f * c.r + 0.71515972f * c.g) + 0.07216883f * c.b, the variance AOV's.  Fields: x(p) = lum(t(a(p))),
 *     y(p) = lum(t(b(p))), both +0 at invalid pixels; m(p) = 1.0f at valid pixels, +0 elsewhere.  Six fields are filtered: m, x, y, x * x,
 *     y * y, x * y (the products are f32, formed per pixel before the filter).
 *     g[k] = PBRS_COMPARE_G0 .. PBRS_COMPARE_G5 below: the f32 nearest to exp(-k * k / 4.5), k = 0 .. 5.  Not normalised: W does that.
 *     The filter is separable, first along the row, then along the column of the row pass' result.  Each pass starts from A = +0 and
 *     does A = A + g[|k|] * v(q) for k = -5 .. 5 ascending, q the position k further along the axis; a tap outside the image is skipped.
 *     The six window sums of p are W, Sx, Sy, Sxx, Syy, Sxy.  At a valid pixel (W >= 1 there):
 *       iw = 1.0f / W;  mx = Sx * iw;  my = Sy * iw;
 *       sxx = Sxx * iw - mx * mx;  syy = Syy * iw - my * my;  sxy = Sxy * iw - mx * my;
 *       C1 = (0.01f * peak) * (0.01f * peak);  C2 = (0.03f * peak) * (0.03f * peak);
 *       ssim(p) = ((2.0f * (mx * my) + C1) * (2.0f * sxy + C2)) / (((mx * mx + my * my) + C1) * ((sxx + syy) + C2))
 *     The variances are not clamped at 0: that keeps ssim(a, a) == 1.0f exactly and the formula symmetric in a and b.  A valid pixel
 *     whose ssim(p) is not finite (pn_isfinite) is left out; that can only happen on linear values far above peak, where the one-pass
 *     variances cancel.  n_ssim counts the pixels that are kept, and ssim = T((double)ssim(p)) / (double)n_ssim over them (0.0 / 0.0
 *     with none).  Without the flag ssim is written as 0.0 and n_ssim as 0.
 *   Maps (maps NULL, or a pointer of it NULL: not wanted).  error_out(p) = (float)se(p).  ssim_out(p) = ssim(p): the computed value,
 *     finite or not, at valid pixels.  Both hold the quiet NaN 0x7fc00000 at invalid pixels.
 * Scale rule.  With PBRS_COMPARE_LINEAR, a and b times 2^j give mse and se times 4^j and mae and max_abs times 2^j, bit for bit, while
 * nothing overflows or goes subnormal.
 * SSIM is meant for display-referred values in [0, peak]; with PBRS_COMPARE_REINHARD peak = 1 is exact.  PSNR is left to the caller:
 * 10 * log10(peak^2 / mse).
 * Pointers are host memory for pbrsx_compare, which stages the two images, the maps and the record on first use (32 B per pixel) and
 * synchronises before it returns; device memory for pbrsx_compare_device (the maps struct itself is host memory, its pointers and
 * result_device device memory), which runs on the context's stream (pbrs_set_stream honoured), writes the 64-byte record from its last
 * kernel and does not wait: a sequence scores its frames without leaving the stream.  Its only scratch is the per-tile partial sums
 * (80 B per tile), allocated on first use; a context that never calls it allocates nothing.  a == b is allowed.
 * Refused with PBRS_E_INVALID (the context stays usable): NULL params, a, b or result; w or h 0; an unknown transform; unknown flag bits;
 * rel_epsilon or peak not finite or not > 0; ssim_out without PBRS_COMPARE_SSIM; a map equal to a, to b or to the other map.  w * h
 * above 2^28: PBRS_E_LIMIT. */
#define PBRS_COMPARE_TILE 16u
#define PBRS_COMPARE_LINEAR 0u
#define PBRS_COMPARE_REINHARD 1u
#define PBRS_COMPARE_SSIM 1u
#define PBRS_COMPARE_G0 0x1p+0f
#define PBRS_COMPARE_G1 0x1.99fa4p-1f
#define PBRS_COMPARE_G2 0x1.a4fa9ep-2f
#define PBRS_COMPARE_G3 0x1.152aaap-3f
#define PBRS_COMPARE_G4 0x1.d40464p-6f
#define PBRS_COMPARE_G5 0x1.fab6c2p-9f
typedef struct pbrs_compare_params {
    uint32_t w, h;      /* image size */
    uint32_t transform; /* PBRS_COMPARE_LINEAR, PBRS_COMPARE_REINHARD */
    uint32_t flags;     /* PBRS_COMPARE_SSIM */
    float rel_epsilon;  /* finite, > 0: the relative error's floor under B * B */
    float peak;         /* finite, > 0: SSIM's dynamic range L */
    uint32_t pad[2];
} pbrs_compare_params; /* 32 B */
typedef struct pbrs_compare_maps { /* each pointer may be NULL */
    float* error_out; /* w * h f32: se(p) */
    float* ssim_out;  /* w * h f32: ssim(p); needs PBRS_COMPARE_SSIM */
} pbrs_compare_maps;
typedef struct pbrs_compare_result {
    double mse, rel_mse, mae, ssim, max_abs;
    uint32_t n_valid, n_invalid, n_ssim;
    uint32_t pad[3]; /* 0 */
} pbrs_compare_result; /* 64 B */
/* (The three functions' prefix is pbrsx_; the structs and constants above carry pbrs_.)
 * Filler: PBRS_COMPARE_REINHARD, PBRS_COMPARE_SSIM, rel_epsilon 1e-2, peak 1; `out` NULL does nothing.  Host code: needs no context. */
void pbrsx_compare_params_default(uint32_t w, uint32_t h, pbrs_compare_params* out);
int pbrsx_compare(pbrs_ctx*, const pbrs_compare_params*, const float* a_host, const float* b_host, const pbrs_compare_maps* maps_host,
                 pbrs_compare_result* result_host);
int pbrsx_compare_device(pbrs_ctx*, const pbrs_compare_params*, const float* a_device, const float* b_device,
                        const pbrs_compare_maps* maps_device, pbrs_compare_result* result_device);

/* ---- despeckle --------------------------------------------------------------------------------------------------- */
/* Fireflies and non-finite pixels, the artefact of a path tracer at a few samples per pixel, taken out of an image before the steps
 * that would spread them (the a-trous filters) or keep them (the temporal accumulation): a pixel that is brighter than `gain` times
 * the rank-th brightest of its neighbours is scaled down to that limit, and a pixel that is not finite is rebuilt from its neighbours.
 * An image operation like pbrs_denoise: it needs a context (device, stream) and no uploaded scene.  rgb_in and rgb_out are w * h pixels,
 * row-major, 3 floats each; the variance planes (the variance AOV: of the pixel's luminance, +inf = "unknown"), mask_out (u32) and
 * removed_out (3 floats per pixel) follow the same order.  The filter is biased: it removes energy, and removed_out says how much.
 * All arithmetic is f32 without fused multiply-add, in the order written; divisions are correctly rounded; pn_* is
 * include/pbrs_numeric.h.  No sum here depends on the launch shape or on arrival order: a CPU model of this text gives the same bytes.
 *   1. Luminance.  lum(c) = (0.21267127f * c.r + 0.71515972f * c.g) + 0.07216883f * c.b, the variance AOV's.
 *   2. Good pixels.  A pixel q is good when c(q).r, c(q).g, c(q).b and lum(c(q)) all pass pn_isfinite: a finite colour whose luminance
 *      overflows is not good.  (These weights sum to less than 1, so no finite f32 colour has such a luminance today: 3e38 in every
 *      channel is a good, very bright pixel.  The clause keeps "good" meaning "has a usable luminance" whatever the weights.)
 *   3. Window.  G(p) is the set of good pixels q != p inside the image with |dx| <= radius and |dy| <= radius; n = |G(p)|.
 *   4. Repair, only where p is not good.  With n == 0: c' = (+0, +0, +0).  Otherwise per channel a sum that starts from +0 and adds
 *      c(q).ch over G(p) in row-major order (dy outer, dx inner, ascending), then / (float)n.  If that c' is not good (the sum
 *      overflowed), c' = (+0, +0, +0).  Where p is good, c' = c(p).
 *   5. Limit, only with n > 0.  S is the k-th largest of { lum(c(q)) : q in G(p) }, counted with multiplicity, k = min(rank, n).
 *      limit = gain * S + floor; a limit that is < 0, or -0, is replaced by +0 (S may be negative where channels are).
 *   6. Clamp.  With n > 0 and l' = lum(c') > limit:  s = limit / l',  out.ch = c'.ch * s  (p is "clamped"; l' > limit >= 0, so s is in
 *      [0, 1)).  Otherwise out = c': a good pixel that is not clamped keeps its bits.
 *   7. Variance (when the pair is given).  A repaired pixel (p not good): +inf.  A clamped good pixel whose variance v passes
 *      pn_isfinite: (v * s) * s.  Every other pixel: the input word, a NaN's payload included.
 *   8. mask_out(p) = PBRS_DESPECKLE_CLAMPED where p is clamped | PBRS_DESPECKLE_REPAIRED where p is not good.
 *   9. removed_out(p).ch = c'.ch - out.ch at clamped pixels, +0 elsewhere.
 *  10. n_clamped and n_repaired count the pixels with each bit over the image; the result's pads are written as 0.
 * Scale rule.  With floor == 0, an input times 2^j gives an output and a removed_out times 2^j, a variance times 4^j and the same mask and
 * counts, bit for bit, while nothing overflows or goes subnormal.
 * Pass-through rule.  An image of good pixels none of which exceeds its limit comes back bit for bit; with gain >= 1 every constant
 * image does (S is then the pixel's own luminance).
 * rank stops at 4 because the kernel holds the four largest taps in four registers.  With radius 1 and rank 2 a single bright pixel is
 * clamped and two bright neighbours are too, each seeing the other as the largest and the background as the second.
 * Pointers of pbrs_despeckle_io (the struct itself is host memory) and `result` are host memory for pbrsi_despeckle, which stages its
 * planes on first use (44 B per pixel) and synchronises before it returns; device memory for pbrsi_despeckle_device, which runs on the
 * context's stream (pbrs_set_stream honoured) and does not wait.  `result` may be NULL; where it is given, the blocks store their two
 * integer counts in a scratch of 16 KiB, which the first such call of a context allocates, and a last kernel sums them and writes the
 * 16-byte record: no atomics, and a context that never asks for the record allocates nothing.
 * Refused with PBRS_E_INVALID (the context stays usable): NULL params, io, rgb_in or rgb_out; w or h 0; radius outside 1 .. 2; rank
 * outside 1 .. 4; gain not finite or < 1; floor not finite or < 0; flag bits (none is defined); one variance pointer without the
 * other; rgb_out == rgb_in (neighbours are read); any output plane (rgb_out, variance_out, mask_out, removed_out) equal to another
 * plane of the call, except variance_out == variance_in, which is allowed because the variance is pixel-local.  w * h above 2^28:
 * PBRS_E_LIMIT. */
#define PBRS_DESPECKLE_TILE 16u
#define PBRS_DESPECKLE_MAX_RADIUS 2u
#define PBRS_DESPECKLE_MAX_RANK 4u
#define PBRS_DESPECKLE_CLAMPED 1u
#define PBRS_DESPECKLE_REPAIRED 2u
typedef struct pbrs_despeckle_params {
    uint32_t w, h;   /* image size */
    uint32_t radius; /* 1 .. PBRS_DESPECKLE_MAX_RADIUS: the window is (2 radius + 1)^2 pixels less the centre */
    uint32_t rank;   /* 1 .. PBRS_DESPECKLE_MAX_RANK: the order statistic of the neighbours' luminances, 1 = the largest */
    float gain;      /* finite, >= 1: the factor on that statistic */
    float floor;     /* finite, >= 0: the additive floor of the limit */
    uint32_t flags;  /* none defined: 0 */
    uint32_t pad;
} pbrs_despeckle_params; /* 32 B */
typedef struct pbrs_despeckle_io {
    const float* rgb_in;      /* w * h * 3 f32 */
    float* rgb_out;           /* w * h * 3 f32 */
    const float* variance_in; /* w * h f32, or NULL: both variance pointers or neither */
    float* variance_out;      /* w * h f32, or NULL; may be variance_in */
    uint32_t* mask_out;       /* w * h u32, or NULL */
    float* removed_out;       /* w * h * 3 f32, or NULL */
} pbrs_despeckle_io;
typedef struct pbrs_despeckle_result {
    uint32_t n_clamped, n_repaired;
    uint32_t pad[2]; /* 0 */
} pbrs_despeckle_result; /* 16 B */
/* (The three functions' prefix is pbrsi_; the structs and constants above carry pbrs_.)
 * Filler: radius 1, rank 2, gain 2, floor 0, flags 0; `out` NULL does nothing.  Host code: needs no context. */
void pbrsi_despeckle_params_default(uint32_t w, uint32_t h, pbrs_despeckle_params* out);
int pbrsi_despeckle(pbrs_ctx*, const pbrs_despeckle_params*, const pbrs_despeckle_io* io_host, pbrs_despeckle_result* result_host);
int pbrsi_despeckle_device(pbrs_ctx*, const pbrs_despeckle_params*, const pbrs_despeckle_io* io_device, pbrs_despeckle_result* result_device);

/* ---- bloom ------------------------------------------------------------------------------------------------------- */
/* Glare, the step between the filter and the display transform: part of a bright pixel's energy is spread over its surround, on linear
 * radiance, before the tone curve clamps it to white.  The bright part of the image goes down a pyramid of half-size levels, comes back
 * up with each coarser level mixed into the finer one, and is added to (or mixed into) the image.  An image operation like
 * pbrs_denoise: it needs a context (device, stream) and no uploaded scene.  rgb and rgb_out are w * h pixels, row-major, 3 floats each.
 * All arithmetic is f32 without fused multiply-add, in the order written; divisions are correctly rounded; pn_* is
 * include/pbrs_numeric.h; lum(c) = (0.21267127f * c.r + 0.71515972f * c.g) + 0.07216883f * c.b, the variance AOV's.  No sum here
 * depends on the launch shape or on arrival order: a CPU model of this text gives the same bytes.
 *   1. Level sizes.  w_0 = (w + 1) / 2, h_0 = (h + 1) / 2; w_{l+1} = (w_l + 1) / 2 and likewise h (integer divisions).  The effective level
 *      count N is `levels`, cut at the first level that is 1 x 1: that level is the last one.
 *   2. Bright pass, applied to a pixel of rgb as the first downsample reads it.  A pixel with a channel that does not pass pn_isfinite
 *      gives (+0, +0, +0).  Otherwise, per channel, c = c > 0 ? c : +0; then Y = lum(c), t = threshold, k = threshold * knee:
 *      Y <= t - k gives f = +0; otherwise Y >= t + k gives f = (Y - t) / Y; otherwise s = (Y - t) + k and
 *      f = ((s * s) * (1.0f / (4.0f * k))) / Y.  bright.c = c.c * f.  With threshold 0, f is exactly 1 for every Y > 0.
 *   3. Downsample: rgb to level 0 through the bright pass, then level l to level l + 1.  Destination (X, Y) sums the source at
 *      (2X + dx, 2Y + dy) for dy = -1 .. 2 (outer) and dx = -1 .. 2 (inner), coordinates clamped to the source's edge, with the weight
 *      K[dx + 1] * K[dy + 1], K = {0.125f, 0.375f, 0.375f, 0.125f} (every product is exact).  Per channel acc = acc + weight * c, in
 *      that order, from +0.  There is no division.  This gives d_l.
 *   4. Upsample and merge, from the coarsest level down: u_{N-1} = d_{N-1}; for l = N-2 .. 0,
 *      u_l(p).c = d_l(p).c + spread * (up(u_{l+1})(p).c - d_l(p).c).  up(v)(x, y) reads v at X0 = x >> 1 and
 *      X1 = X0 + ((x & 1) ? 1 : -1) clamped to v's edge, with the weights 0.75f and 0.25f, and y likewise; the four products wx * wy
 *      are exact, and acc = acc + (wx * wy) * v(X, Y).c over (X0, Y0), (X1, Y0), (X0, Y1), (X1, Y1), from +0.
 *   5. Composite, at full size: B(p) = up(u_0)(p).  Without PBRS_BLOOM_MIX out.c = rgb.c + strength * B.c; with it
 *      out.c = rgb.c + strength * (B.c - rgb.c), the energy-conserving glare (use it with threshold 0; strength is then <= 1).  A
 *      pixel of rgb with a channel that does not pass pn_isfinite passes through with its bits; it has entered the pyramid as +0, so
 *      no neighbour becomes non-finite by it.  strength == 0 returns rgb's bits: a copy, or nothing where rgb_out == rgb.
 * Scale rule.  With rgb and threshold both times 2^j the output is 2^j times the output, bit for bit, while nothing that depends on
 * the scale overflows or becomes a nonzero value below the smallest normal f32.
 * Fixed point.  A constant image of the finite value v > 0 in every channel is its own bloom under PBRS_BLOOM_MIX with threshold 0
 * wherever 0.375f * v and every partial sum of steps 3 and 4 are exact.  The partial sums are multiples k / 64 of v, k <= 64 (seven
 * bits), so a v with at most 17 significant bits, away from the ends of the exponent range, qualifies (0.75f is one).  Every level is
 * then v, B is v, and v + strength * (v - v) is v.
 * Pointers are host memory for pbrsb_bloom, which stages the image on first use (12 B per pixel; the result lands in the staged
 * input's place) and synchronises before it returns; device memory for pbrsb_bloom_device, which runs on the context's stream
 * (pbrs_set_stream honoured) and does not wait.  rgb_out may equal rgb: the one kernel that writes out(p) reads rgb only at p, after
 * the pyramid has been built.  The first call allocates the pyramid, one chain of levels of 16 B per level pixel (r, g, b and a pad):
 * the levels hold a third of the image's pixels (a little more where a size is odd), 5.4 B per image pixel.  A larger image grows it,
 * pbrs_destroy frees it, and a context that never calls this (or only with strength 0) allocates nothing.
 * Refused with PBRS_E_INVALID (the context stays usable): NULL params, rgb or rgb_out; w or h 0; levels 0 or above
 * PBRS_BLOOM_MAX_LEVELS; unknown flag bits; threshold not finite or < 0; knee not finite or outside [0, 1]; strength not finite or
 * < 0; spread not finite or outside [0, 1]; PBRS_BLOOM_MIX with strength > 1.  w * h above 2^28: PBRS_E_LIMIT. */
#define PBRS_BLOOM_MAX_LEVELS 8u
#define PBRS_BLOOM_MIX 1u
typedef struct pbrs_bloom_params {
    uint32_t w, h;   /* image size */
    uint32_t levels; /* 1 .. PBRS_BLOOM_MAX_LEVELS */
    uint32_t flags;  /* PBRS_BLOOM_MIX */
    float threshold; /* finite, >= 0: luminance above which a pixel blooms; 0 = the whole image */
    float knee;      /* finite, in [0, 1]: soft knee as a fraction of threshold */
    float strength;  /* finite, >= 0 (<= 1 with PBRS_BLOOM_MIX) */
    float spread;    /* finite, in [0, 1]: how much of each coarser level reaches the finer one */
} pbrs_bloom_params; /* 32 B */
/* (The three functions' prefix is pbrsb_; the struct and the constants above carry pbrs_.)
 * Filler: levels 6, flags 0, threshold 1, knee 0.5, strength 0.05, spread 0.6 (choices, not measurements); `out` NULL does nothing.
 * Host code: needs no context. */
void pbrsb_bloom_params_default(uint32_t w, uint32_t h, pbrs_bloom_params* out);
int pbrsb_bloom(pbrs_ctx*, const pbrs_bloom_params*, const float* rgb_host, float* rgb_out_host);
int pbrsb_bloom_device(pbrs_ctx*, const pbrs_bloom_params*, const float* rgb_device, float* rgb_out_device);

/* ---- depth of field ---------------------------------------------------------------------------------------------- */
/* A thin-lens blur as an image operation: the camera of this library is a pinhole, and this call defocuses its image afterwards from the
 * depth AOV.  That depth (pbrs_aov_buffers.depth) is the ray parameter t of the unnormalised direction c + a x + b y; a and b span the
 * image plane, so t is the planar depth along the view axis in units of one constant, and the thin-lens circle of confusion depends on
 * depth only through |z - F| / z, a ratio that t gives exactly.  Each pixel gets a blur radius from its depth (step 1); the image is
 * rebuilt from its neighbours' circles in one gather (step 2), under two occlusion rules: a near, blurred object spreads over what is
 * behind it, and a sharp object keeps its edge against a blurred background.  An image operation like pbrs_denoise: it needs a context
 * (device, stream) and no uploaded scene.  rgb and rgb_out are w * h pixels, row-major, 3 floats each; depth is w * h floats as
 * pbrs_aov_buffers writes it, +inf where nothing was hit.  All arithmetic is f32 without fused multiply-add, in the order written;
 * divisions and square roots are correctly rounded; pn_* is include/pbrs_numeric.h.  No sum here depends on the launch shape or on
 * arrival order: a CPU model of this text gives the same bytes.  R = max_radius, F = focus, K = scale.
 *   0. K == 0 comes before everything else: rgb_out gets rgb's bits (a copy) and coc_out, where given, +0.  So 0 * inf never forms.
 *   1. Circle of confusion r(p) from z = depth(p).  !(z > 0) (zero, negative, NaN: the depth is unknown) gives r = +0.  Otherwise
 *      q = 1.0f where z is +inf and q = pn_abs(z - F) / z elsewhere; r = K * q; r = r < (float)R ? r : (float)R.
 *   2. Gather.  A pixel p of rgb with a channel that does not pass pn_isfinite passes through with its bits.  Otherwise start from
 *      acc = (+0, +0, +0), W = +0, n = 0, and for dy = -R .. R (outer) and dx = -R .. R (inner), q = p + (dx, dy):
 *        q outside the image: left out.  rgb(q) has a channel that does not pass pn_isfinite: left out.
 *        dist = sqrt((float)(dx * dx + dy * dy)).
 *        e = depth(q) < depth(p) ? r(q) : (r(q) < r(p) ? r(q) : r(p)).  A tap in front spreads by its own circle; a tap at or
 *            behind p never spreads further than p's own circle.  An unordered comparison is false.
 *        cov = (e - dist) + 0.5f; cov <= 0: left out; then cov = cov < 1.0f ? cov : 1.0f.
 *        rr = e > 0.5f ? e : 0.5f; wgt = cov / (rr * rr).
 *        acc.c = acc.c + wgt * rgb(q).c per channel; W = W + wgt; n = n + 1.
 *      The centre always counts: dist = 0, e = r(p) >= 0, cov >= 0.5.  n == 1 gives rgb(p)'s bits; otherwise out.c = acc.c / W.
 *      A tap that is left out is not added at all, so an implementation may shorten its loops wherever it can prove cov <= 0, and
 *      nothing changes.
 *   3. coc_out, optional (NULL: not wanted), w * h floats: r(p), with the sign bit set where depth(p) < F (an unordered comparison is
 *      false): the near field is negative, and a depth of zero or below gives -0.
 * Rules.  (a) With rgb times 2^j the output is 2^j times the output, bit for bit, while nothing overflows or becomes a nonzero value
 * below the smallest normal f32.  (b) With depth and focus both times 2^j, likewise, the output and coc_out keep their bits.  (c) Where
 * every r is <= 0.5 the output is rgb, bit for bit.  (d) A pixel with r = 0 takes nothing from any pixel at or behind its own depth.
 * What a gather cannot know is the background hidden behind a blurred foreground: where a near object is spread thin, what shows through
 * it is the neighbouring visible background, not what a lens would see past the object's edge.  The bokeh is a disk.
 * Pointers are host memory for pbrsf_dof, which stages the planes on first use (32 B per pixel) and synchronises before it returns;
 * device memory for pbrsf_dof_device, which runs on the context's stream (pbrs_set_stream honoured) and does not wait: one launch, no
 * scratch, no allocation.  rgb_out must not be rgb: a gather reads its neighbours.  Any other overlap is the caller's error.
 * Refused, in this order, with PBRS_E_INVALID (the context stays usable): NULL params, rgb, depth or rgb_out; rgb_out == rgb; w or h 0;
 * max_radius 0 or above PBRS_DOF_MAX_RADIUS; non-zero flags or reserved words; focus not finite or <= 0; scale not finite or < 0.
 * Then w * h above 2^28: PBRS_E_LIMIT. */
#define PBRS_DOF_MAX_RADIUS 16u
typedef struct pbrs_dof_params {
    uint32_t w, h;        /* image size */
    uint32_t max_radius;  /* 1 .. PBRS_DOF_MAX_RADIUS: pixels; also the loop's reach */
    uint32_t flags;       /* 0 */
    float focus;          /* finite, > 0: the depth AOV's value that is sharp */
    float scale;          /* finite, >= 0: blur radius in pixels of a point at infinity */
    uint32_t reserved[2]; /* 0 */
} pbrs_dof_params;        /* 32 B */
/* (The three functions' prefix is pbrsf_; the struct and the constant above carry pbrs_.)
 * Filler: max_radius 8, flags 0, focus 1, scale 0 (a copy until the caller sets a lens), reserved 0; `out` NULL does nothing.
 * Host code: needs no context. */
void pbrsf_dof_params_default(uint32_t w, uint32_t h, pbrs_dof_params* out);
int pbrsf_dof(pbrs_ctx*, const pbrs_dof_params*, const float* rgb_host, const float* depth_host, float* rgb_out_host, float* coc_out_host);
int pbrsf_dof_device(pbrs_ctx*, const pbrs_dof_params*, const float* rgb_device, const float* depth_device, float* rgb_out_device, float* coc_out_device);

/* ---- motion blur ------------------------------------------------------------------------------------------------- */
/* A shutter as an image operation: every frame of a sequence is an instantaneous exposure, and this call smears it afterwards along
 * the motion vector AOV (pbrs_motion_vectors above: per pixel, where the surface point was one frame ago minus where it is, in pixels,
 * through the camera's motion and each instance's).  It is not a plain directional blur: a fast object smears over a static background,
 * a static object in front keeps its edge against a moving background, and a moving object's thinning edge lets the background show
 * through.  That takes the depth, every pixel's own speed and a dominant velocity per neighbourhood (McGuire et al. 2012, "A
 * reconstruction filter for plausible motion blur"; Jimenez 2014, "Next generation post processing in Call of Duty: Advanced
 * Warfare").  An image operation like pbrsf_dof: it needs a context (device, stream) and no uploaded scene.  rgb and rgb_out are w * h
 * pixels, row-major, 3 floats each; depth is w * h floats as pbrs_aov_buffers writes it, +inf where nothing was hit; motion is w * h
 * pixels of 2 floats, exactly what pbrs_motion_vectors writes.  All arithmetic is f32 without fused multiply-add, in the order written;
 * divisions and square roots are correctly rounded; pn_* is include/pbrs_numeric.h.  No sum here depends on the launch shape or on
 * arrival order: a CPU model of this text gives the same bytes.  R = max_radius, S = taps.
 *   0. shutter == 0 comes before everything else: rgb_out gets rgb's bits (a copy) and velocity_out, where given, +0.
 *   1. Velocity, the half-exposure vector: the exposure is centred on the frame, so a point is seen from -v to +v.  k = shutter * 0.5f;
 *      v(p) = (motion(p).x * k, motion(p).y * k).  A component of motion(p) that does not pass pn_isfinite gives v = (+0, +0).
 *      ll = v.x * v.x + v.y * v.y; len = sqrt(ll).  If len > (float)R: s = (float)R / len; v = (v.x * s, v.y * s); ll and len are
 *      computed again from that v; and len = len < (float)R ? len : (float)R.
 *   2. The dominant velocity of a tile.  Tiles are 16 x 16 pixels, anchored at (0, 0): part of the contract.  vn(tile) is v(q) of the
 *      pixel q with the largest ll over the tile grown by R pixels on every side and cut at the image; among equal ll the lowest
 *      row-major index y * w + x wins.  (ll, index) is a total order (ll is never NaN), so the maximum is the same in any reduction
 *      shape.  Every pixel whose smear can reach a pixel of the tile has len <= R and lies in that window, which is why R ends at the
 *      tile's size.  If len(q) <= 0.5 for that q, every pixel of the tile gets its rgb bits.
 *   3. Gather, for a pixel p of any other tile.  A p with a channel that does not pass pn_isfinite passes through with its bits.
 *      zeff(p) = depth(p) > 0 ? depth(p) : +inf (zero, negative, NaN: unknown, taken as far).  j = 0, or with PBRS_MOTION_BLUR_JITTER
 *      j = ((float)M[y & 3][x & 3] + 0.5f) / 16.0f - 0.5f with the display transform's 4 x 4 Bayer matrix M.  Start from
 *      acc = (+0, +0, +0), W = +0, n = 0, and for i = 0 .. S - 1:
 *        t = (((float)i + 0.5f) + j) / (float)S * 2.0f - 1.0f.
 *        dx = (int)pn_floor(vn.x * t + 0.5f), dy = (int)pn_floor(vn.y * t + 0.5f), q = p + (dx, dy); |dx|, |dy| <= R.
 *        (dx, dy) == (0, 0): left out.  q outside the image: left out.  rgb(q) has a channel that does not pass pn_isfinite: left out.
 *        dist = sqrt((float)(dx * dx + dy * dy)).
 *        f = 1.0f where zeff(q) <= zeff(p); otherwise a = 1.0f - (zeff(q) - zeff(p)) / (z_rel * zeff(p)); f = a > 0 ? a : +0.  An
 *            unordered comparison is false.  A q in front of p or level with it gives 1; f falls to 0 as q goes behind p by the
 *            fraction z_rel of p's depth.
 *        cyl(d, l) = c = (l - d) + 0.5f; c = c > 0 ? c : +0; c = c < 1.0f ? c : 1.0f: a line of the length l with a one-pixel soft end.
 *        wgt = f * cyl(dist, len(q)) + (1.0f - f) * cyl(dist, len(p)).  A tap in front spreads by its own speed; a tap behind shows
 *            only as far as p itself is smeared thin.
 *        wgt <= 0: left out.  Otherwise acc.c = acc.c + wgt * rgb(q).c per channel; W = W + wgt; n = n + 1.
 *      n == 0 gives rgb(p)'s bits; otherwise out.c = (acc.c + ((float)S - W) * rgb(p).c) / (float)S.  The slices of the exposure that
 *      no tap claims show the pixel itself: coverage is the share of the line's taps, not a ratio of heuristic weights.
 *   4. velocity_out, optional (NULL: not wanted), w * h pixels of 2 floats: v(p) of step 1.
 * Rules.  (a) With rgb times 2^j the output is 2^j times the output, bit for bit, while nothing overflows or becomes a nonzero value
 * below the smallest normal f32.  (b) With depth times 2^j, likewise, nothing changes.  (c) Where every len is <= 0.5 the output is rgb,
 * bit for bit.  (d) A pixel with v = 0 takes nothing from a pixel behind it (f == 0): its weight is cyl(dist, 0) with dist >= 1.
 * (e) A tap that is left out is not added at all, so an implementation may cut its loops wherever it can prove wgt <= 0, and nothing
 * changes.
 * What the method cannot know: the background hidden behind a moving object is taken from its visible neighbours; the motion within
 * the exposure is taken as linear and centred on the frame; shadows and reflections of movers have no vectors (the limit the temporal
 * section states), so they stay sharp.
 * Pointers are host memory for pbrsm_motion_blur, which stages the planes on first use (44 B per pixel) and synchronises before it
 * returns; device memory for pbrsm_motion_blur_device, which runs on the context's stream (pbrs_set_stream honoured) and does not wait:
 * one launch, no scratch, no allocation.  rgb_out must not be rgb: a gather reads its neighbours.  Any other overlap is the caller's
 * error.
 * Refused, in this order, with PBRS_E_INVALID (the context stays usable): NULL params, rgb, depth, motion or rgb_out; rgb_out == rgb;
 * w or h 0; max_radius 0 or above PBRS_MOTION_BLUR_MAX_RADIUS; taps below 2 or above PBRS_MOTION_BLUR_MAX_TAPS; flag bits other than
 * PBRS_MOTION_BLUR_JITTER; a non-zero reserved word; shutter not finite or outside 0 .. 1; z_rel not finite or <= 0.  Then w * h above
 * 2^28: PBRS_E_LIMIT. */
#define PBRS_MOTION_BLUR_MAX_RADIUS 16u
#define PBRS_MOTION_BLUR_MAX_TAPS 64u
#define PBRS_MOTION_BLUR_JITTER 1u /* flags: each pixel shifts its taps by a 4 x 4 ordered offset, banding becomes a fine pattern */
typedef struct pbrs_motion_blur_params {
    uint32_t w, h;       /* image size */
    uint32_t max_radius; /* 1 .. PBRS_MOTION_BLUR_MAX_RADIUS: pixels, the longest half-exposure vector */
    uint32_t taps;       /* 2 .. PBRS_MOTION_BLUR_MAX_TAPS: samples along the line from -vn to +vn */
    uint32_t flags;      /* 0 or PBRS_MOTION_BLUR_JITTER */
    float shutter;       /* finite, 0 .. 1: the open fraction of the frame interval, centred on the frame */
    float z_rel;         /* finite, > 0: the relative depth difference over which a tap goes from level to behind */
    uint32_t reserved;   /* 0 */
} pbrs_motion_blur_params; /* 32 B */
/* (The three functions' prefix is pbrsm_; the struct and the constants above carry pbrs_.)
 * Filler: max_radius 16, taps 16, flags 0, shutter 0.5 (a 180 degree shutter), z_rel 0.05, reserved 0: choices, not measurements;
 * `out` NULL does nothing.  Host code: needs no context. */
void pbrsm_motion_blur_params_default(uint32_t w, uint32_t h, pbrs_motion_blur_params* out);
int pbrsm_motion_blur(pbrs_ctx*, const pbrs_motion_blur_params*, const float* rgb_host, const float* depth_host, const float* motion_host,
                      float* rgb_out_host, float* velocity_out_host);
int pbrsm_motion_blur_device(pbrs_ctx*, const pbrs_motion_blur_params*, const float* rgb_device, const float* depth_device,
                             const float* motion_device, float* rgb_out_device, float* velocity_out_device);

#ifdef __cplusplus
}
#endif
#endif
