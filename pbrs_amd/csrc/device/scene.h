// device/scene.h — what the host prepares at upload and the kernels read: the scene view every kernel takes (DevScene), the four-wide
// node, and the constants both sides agree on (feature bits, thresholds, k_shade's selector bits, the block size).
//
// No device code and no dmath.h: host/scene_prepare.cpp and host/kernel_choice.cpp are plain C++ and include this header as it is;
// shapes.h, wide.h and kernels.h include it for the kernels.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../../include/pbrs_gpu.h"

constexpr uint32_t kBlock = 256;
constexpr size_t kLdsBytesPerCU = 160 * 1024;

struct pbrs_wnode;  // below
struct DevScene {
    // Every BVH node of the scene in one array with absolute links: the TLAS at 0 (root = node 0), its leaves again at
    // flat_off when the TLAS is small (below), then the BLASes; a mesh instance's blas_root is an index into it.
    const pbrs_node* nodes;
    const pbrs_instance* inst;
    const pbrs_shape* shapes;
    const pbrs_mesh* meshes;
    const pbrs_tri_verts* tv;
    const pbrs_tri_shade* ts;
    const pbrs_material* mats;
    const pbrs_bxdf* bxdfs;
    const pbrs_area_light* alights;
    const pbrs_delta_light* dlights;
    uint32_t n_area, n_delta;
    float env[3];
    uint32_t has_env;
    uint32_t fast_slab;  // node coordinates are inside the range the division-free box test is exact for (traverse.h)
    uint32_t exact_extent;  // a ParallelQuad instance (hits outside its own box, D1) next to a mesh (hits beyond the extent it was given): the closest-hit walks take PBRS_FEAT_EXTENT
    // Small TLAS (PBRS_FLAT_TLAS_MIN..MAX instances): its leaves alone, in pre-order = the order the tree walk reaches them.
    // A box inside a box that a ray misses is missed too (each slab bound is a correctly rounded, hence monotonic,
    // function of the box coordinate), so testing the leaf boxes in this order — each against the t_max of its turn —
    // processes exactly the leaves, in exactly the order, of the reference's recursion (tlas/src/bvh.rs:84-88) without
    // visiting the inner nodes.  The wave runs those tests for its new rays together (traverse.h, FlatScan).  Only for
    // rays on the division-free box test (no NaN quotients); other rays walk the tree.  n_flat = 0 outside the range
    // (kernels without PBRS_FEAT_FLAT_TLAS do not contain the scan).
    uint32_t flat_off, n_flat;
    uint32_t features;   // PBRS_FEAT_*: what the traversal kernels must be able to do for this scene
    uint32_t refill_below;  // a wave of a traversal kernel takes new rays when fewer of its lanes than this are walking
    uint32_t refill_below_shadow;  // ... of k_shadow (any-hit walks end at the first occluder: later, larger refills)
    // The mesh instance whose BLAS the camera rays enter at per-pixel entry nodes (device/entry_nodes.h; prepare_scene), or
    // PBRS_ENTRY_NONE.  (Like n_wnodes below, this word fills what was padding: the layout of every other member stays.)
    uint32_t entry_inst;
    // texture/src/lib.rs (device/textures.h) and the environment light (scene/src/lib.rs:105-117)
    const pbrs_texture* textures;
    const float* tex_floats;
    const uint32_t* tex_words;
    uint32_t env_kind, env_texture;
    float env_scale[3];
    const pbrs_fourier_table* fourier;  // geometry/src/fourier.rs tables (device/fourier.h); their arrays are in the texture pools
    // Shading classes: materials with the same lobe signature (kinds, Fresnel forms, textured or not) share one; the device
    // copy of an instance carries its material's class in pad[0].  More than one class with lobes: the bounce queues are
    // ordered by class before k_shade (kernels.h, k_class_sort).
    uint32_t n_classes;
    // Four-wide nodes over every BLAS (device/wide.h; a mesh instance's wide root is in the device copy of its record, pad[1])
    // and the entries a lane's stack may hold in the kernels that walk them (beyond that a ray goes to the binary-walk kernels)
    const pbrs_wnode* wnodes;
    uint32_t wide_cap;
    // Scenes of a few KB (a Cornell box: 8 KB): what the walks read — every node, triangle-vertex record, instance record and analytic
    // shape — is copied into each block's LDS behind its stack rows at kernel start (PBRS_FEAT_LDS_SCENE kernels; kernels.h,
    // stage_scene): element counts, and the word offset of the copy in the block's dynamic LDS (a multiple of 4).  0 nodes: not staged.
    uint32_t lds_off_words, lds_nodes, lds_tris, lds_inst, lds_shapes;
    // PBRS_FEAT_LDS_TOP kernels: only the first lds_nodes nodes (the TLAS) are staged, and read through this pointer (nullptr in the uploaded
    // scene; the kernel points it at its block's copy): nodes[i] for i < lds_nodes comes from the LDS, every other node from DevScene::nodes
    const pbrs_node* nodes_top;
    // element counts of the arrays k_shade may stage in LDS (kernels.h, stage_shade_scene); n_area / n_delta above
    uint32_t n_inst, n_shapes, n_tris, n_mats, n_bxdfs;
    // tri_leaf: one word per triangle record of `tv`, the index in `nodes` of the BLAS leaf that holds it.  A packed leaf reference
    // (PBRS_WREF_PACKED) names its triangles, not its node; the any-hit walk finds the node — the leaf's box — through this table, and only
    // once a triangle of the leaf has passed (traverse.h, AnyWalkW::verify_leaf).  The table lies in the wide nodes' allocation, right behind
    // the n_wnodes wide nodes (device/wide.h, tri_leaf); 0 without wide nodes.  (This word fills what was the structure's padding: a kernel
    // that takes the scene and does not read the table keeps its argument layout.)
    uint32_t n_wnodes;
};

// Scene features the traversal kernels are specialised on (prepare_scene derives them from the arrays check_scene has checked).
// Code a scene cannot reach still costs registers and issue slots on every wave, so each combination is its own
// instantiation: a mesh-only scene whose meshes all carry a PBRS_MESH_*_SHADING_OK flag runs the leanest one.
// pbrs_instance::flags bit set by prepare_scene on the device copy (not part of the ABI): the 3x3 part of `inv` is
// bit-exactly the identity, i.e. the instance is only translated (traverse.h, enter_instance)
#define PBRS_INSTANCE_TRANSLATION 0x100u
#define PBRS_FEAT_ANALYTIC 1u       // some instance is an analytic shape (sphere, disk, quad, cuboid, triangle)
#define PBRS_FEAT_SHADING_CHECK 2u  // some mesh needs the tangent check of blas.rs:193-200 evaluated per candidate hit
#define PBRS_FEAT_FLAT_TLAS 4u      // the leaf copies at DevScene::flat_off are built: rays on the division-free box test scan the TLAS leaves
#define PBRS_FEAT_ALL 7u
#define PBRS_FEAT_EXTENT 256u        // closest-hit walk only (one k_extend each way, host/kernel_choice.h kExtentFeatures): the TLAS extent is the reference's ray.t_max to the letter, rises included
                                    // (traverse.h, ClosestWalk::EXT): scenes with a ParallelQuad next to a mesh (prepare_scene)
#define PBRS_FEAT_LONG_WALKS 8u     // kernels only (not a property of the walks): several node steps per loop round (kernels.h)
#define PBRS_FEAT_WIDE 16u          // kernels only: the walks over four-wide nodes (device/wide.h); needs PBRS_FEAT_FLAT_TLAS
#define PBRS_FEAT_LDS_TOP 128u      // kernels only: the head of DevScene::nodes — a TLAS too large to scan — is copied into the block's LDS (scenes whose arrays do not fit as a whole)
#define PBRS_FEAT_LDS_SCENE 64u     // kernels only: the arrays the walks read are copied into the block's LDS at kernel start (scenes of a few KB; kernels.h)
#define PBRS_FEAT_FULL_STEPS 32u    // kernels only (with PBRS_FEAT_LONG_WALKS): a round's further node steps are full steps (kernels.h): scenes outside the guarded range of the division-free box test
// The light a shadow ray was aimed at, as one word (0: none).  prepare_scene links an area light to the analytic instance that IS the
// light (same shape, identity matrices); pbrs_upload_scene writes the two halves, as bit patterns, into pad[0] (instance + 1) and pad[1]
// (flat leaf + 1) of the uploaded copy of the light record; k_shade puts them together in sr[2][j].w of a lone ray whose own test of that
// instance is false, and k_shadow passes the instance's TLAS leaf over (traverse.h, AnyWalk::skip).
#define PBRS_SKIP_INST_MASK 0x00ffffffu  // instance + 1 (a scene with more instances sets no links)
#define PBRS_SKIP_FLAT_SHIFT 24          // above it: index + 1 of the instance's leaf among the leaf copies at DevScene::flat_off; 0 without them
#define PBRS_FLAT_TLAS_MIN 2u
// Largest TLAS the wave scans instead of walking (tools/tlas_probe.py, C5's scene family at 960x540, ms per 64 spp, walk vs
// scan): closest hit 4.84 / 4.74 at 20 instances, 5.10 / 5.28 at 24, 5.66 / 6.15 at 30 — the scan only filters there and every
// surviving leaf is still visited; any hit 3.33 / 2.38 at 20, 3.58 / 2.53 at 24, 3.97 / 2.86 at 30 — there the scan is the test.
// The candidate mask is one word: <= 32.
#ifndef PBRS_FLAT_TLAS_MAX
#define PBRS_FLAT_TLAS_MAX 20u         // k_extend
#endif
#ifndef PBRS_FLAT_TLAS_MAX_ANYHIT
#define PBRS_FLAT_TLAS_MAX_ANYHIT 32u  // k_shadow
#endif

// The four-wide node of device/wide.h (which says what the walks over it compute, and why that is the reference's result).
// 128 bytes = one L2 line.  Planes as structure-of-arrays over the four slots so that a lane reads the planes its ray meets
// first / last on each axis as one 16-byte vector each (the choice follows the sign of the direction: a per-lane byte offset).
struct pbrs_wnode {
    float lo[3][4];     // [axis][slot]: min planes   (bytes   0 ..  47)
    float hi[3][4];     // [axis][slot]: max planes   (bytes  48 ..  95)
    uint32_t child[4];  // PBRS_WREF_LEAF | index of the reference's leaf node in DevScene::nodes, or, as uploaded, PBRS_WREF_LEAF | PBRS_WREF_PACKED |
                        // count - 1 | first triangle (below); else index of a wide node; PBRS_WREF_NONE
                        // in a slot not in use (its box is inverted — lo = 2^60, hi = -2^60 — and fails the filter for every ray of the
                        // guarded range, without an overflow).  Slots 0 and 2 are always in use and carry the three split axes above
                        // the index (PBRS_WREF_AXIS_SHIFT): child[0] bits 27-28 X's, bits 29-30 its left child's; child[2] bits 27-28 its
                        // right child's — a node step reads seven vectors, not eight (a load whose lanes name different lines costs
                        // the L1 a cycle per lane whatever its width: C4 k_shadow 151 accesses per ray)
    uint32_t pad[4];
};
#ifndef PBRS_WIDE_STACK_MAX
#define PBRS_WIDE_STACK_MAX 16  // LDS stack entries per lane of the wide-walk kernels (C4's terrain: 12 at most over a frame's rays)
#endif
#ifndef PBRS_WIDE_MIN_LEVELS
#define PBRS_WIDE_MIN_LEVELS 4u  // scenes whose deepest BLAS has fewer wide levels keep the binary-walk kernels
#endif
#define PBRS_WREF_LEAF 0x80000000u
#define PBRS_WREF_NONE 0xffffffffu
#define PBRS_WREF_INDEX 0x07ffffffu  // a leaf's index in DevScene::nodes (below 2^27: the node array is addressed with 32-bit byte offsets); a wide
#define PBRS_WREF_AXIS_SHIFT 27      // node's index loses the bits above it in `index * sizeof(pbrs_wnode)` (below 2^25 for the same reason)
// A leaf reference that carries its triangles (host/scene_prepare.cpp, pack_wide_leaves): inside the 27 index bits, bit 26 set, bits 24-25
// the triangle count - 1, bits 0-23 the first triangle's index in DevScene::tv.  For a leaf of one to four triangles that start below 2^24
// (a terrain of 2^24 triangles packs whole); a leaf of more (coincident centroids), an empty leaf and a leaf further up the triangle array
// keep the node form, which never has bit 26 set: prepare_scene builds wide nodes only where every node index is below 2^26.
#define PBRS_WREF_PACKED 0x04000000u
#define PBRS_WREF_TRI_BITS 24
#define PBRS_WREF_TRI 0x00ffffffu
#define PBRS_WREF_COUNT_SHIFT 24
#define PBRS_WREF_COUNT_MAX 4u
static_assert((PBRS_WREF_PACKED & PBRS_WREF_INDEX) == PBRS_WREF_PACKED && PBRS_WREF_PACKED < (1u << PBRS_WREF_AXIS_SHIFT), "the packed flag lies inside the index bits, below the axes");
static_assert(PBRS_WREF_TRI == (1u << PBRS_WREF_TRI_BITS) - 1u && PBRS_WREF_COUNT_SHIFT == PBRS_WREF_TRI_BITS, "first triangle: the low bits, the count above them");
static_assert(((PBRS_WREF_COUNT_MAX - 1u) << PBRS_WREF_COUNT_SHIFT) < PBRS_WREF_PACKED && (PBRS_WREF_PACKED >> PBRS_WREF_COUNT_SHIFT) == PBRS_WREF_COUNT_MAX,
              "two bits of count - 1 between the triangle index and the flag");
static_assert((PBRS_WREF_PACKED | ((PBRS_WREF_COUNT_MAX - 1u) << PBRS_WREF_COUNT_SHIFT) | PBRS_WREF_TRI) == PBRS_WREF_INDEX, "flag, count and triangle fill the 27 bits exactly");
static_assert(PBRS_WREF_TRI_BITS >= 24, "a mesh of 2^24 triangles (indices 0 .. 2^24 - 1) packs");
static_assert((PBRS_WREF_LEAF | PBRS_WREF_INDEX | (15u << PBRS_WREF_AXIS_SHIFT)) == 0xffffffffu && PBRS_WREF_LEAF == (1u << 31), "leaf bit, four axis bits, 27 index bits");
#define PBRS_WIDE_UNUSED_PLANE 1152921504606846976.0f /* 2^60 */
// slots 0, 1: the children of X's left child (or that child itself in slot 0, where it is a leaf); slots 2, 3: of its right child

// A wave takes new rays when fewer than DevScene::refill_below of its lanes are walking (prepare_scene): short walks
// (a small TLAS scanned by the wave, BLASes of a few nodes) favour late, large refills — the shared scan of the new rays
// fills its windows and the step kernels run on fuller waves less often; long walks (C4's 18-level BLAS) favour early ones.
#ifndef PBRS_REFILL_BELOW_SHORT
#define PBRS_REFILL_BELOW_SHORT 20u  // C2 extend 9.23 / 8.92 / 9.04 ms per 16 spp at 40 / 24 / 16
#endif
#ifndef PBRS_REFILL_BELOW_LONG
#define PBRS_REFILL_BELOW_LONG 48u   // C4 extend 25.9 / 24.5 / 23.8 ms per 16 spp at 24 / 40 / 48; per frame 398.5 / 392.4 / 418.3 / 452.5 ms at 40 / 48 / 56 / 60 (round 4)
#endif
#ifndef PBRS_REFILL_BELOW_LONG_SHADOW
#define PBRS_REFILL_BELOW_LONG_SHADOW 40u  // C4 shadow 205.3 / 209.9 / 231.5 ms per frame at 40 / 48 / 56 (profiles/r04j_ab_refill_thresholds_c4.log)
#endif
#define PBRS_LONG_WALK_HEIGHT 12u    // a mesh whose BLAS is at least this high makes the scene's walks "long"

// k_shade's SPEC (kernels.h): what the scene's materials and lights allow the stage to leave out (derived at upload, prepare_scene):
//   PBRS_SHADE_LAMBERT        every lobe is an untextured Lambertian DiffuseReflect, at most one per material
//   PBRS_SHADE_LIGHT_SPHERE / _TRIANGLE   every area light has that shape
// Code a scene cannot reach still costs the loads that decide not to take it (a lobe's kind, a light's shape kind), the
// registers of its longest path and the instructions around it: C2 (Lambert + triangle lights) shades in 87.7 instead of
// 110.5 ms per frame, C4 (Lambert + sphere lights: 96 VGPRs, five waves per SIMD) in 116.7 instead of 150.6.
#define PBRS_SHADE_LAMBERT 1u
#define PBRS_SHADE_LIGHT_SPHERE 2u
#define PBRS_SHADE_LIGHT_TRIANGLE 4u
//   PBRS_SHADE_FOURIER        the other way round: some material is a Fourier BSDF (device/fourier.h), whose code only the
//                             kernels with this bit contain (its f64 series sums and Newton loops are long and register-hungry)
#define PBRS_SHADE_FOURIER 8u
//   PBRS_SHADE_FOURIER_ONLY   (with PBRS_SHADE_FOURIER) every vertex the launch meets is on a Fourier material, whose one lobe is the
//                             Fourier BSDF: the launch over that class of a class-major queue (host/kernel_choice.cpp)
#define PBRS_SHADE_FOURIER_ONLY 16u
//   PBRS_SHADE_LDS_RECORDS    the scene's instance records, analytic shapes, materials, lobes and lights are copied into the block's LDS
//   PBRS_SHADE_LDS_TRIS       ... and its triangle vertex and shading records (scenes of a few KB)
// at kernel start (stage_shade_scene): a vertex's ~25 record fetches — the instance's two matrices, the triangle's seven vectors, material,
// lobe and light — are gathers that cost the CU's texture path a cycle or two per lane each (k_shade's texture data unit was 0.93-0.95
// busy on C2 / C3) and the LDS a third of that, at a third of the latency (tools/microbench/gather_lds_coop.hip).  Chosen per scene by what fits
// (prepare_scene): C2 / C3 both, C4 (a million triangles, six instances) the records.
#define PBRS_SHADE_LDS_RECORDS 32u
#define PBRS_SHADE_LDS_TRIS 64u
// Shading classes a scene may have (DevScene::n_classes; kernels.h, class sort)
#define PBRS_MAX_CLASSES 16u

// What the pass driver (host/pass_plan.h) and the kernels agree on: the sizes behind a pass's grids, counters and sort tables.
// The traversal kernels are persistent: at most this many blocks, each lane keeps pulling rays (kernels.h).
#define PBRS_PERSISTENT_BLOCKS 1536
// Their work fetch (kernels.h, WaveWork): the queue is cut into this many segments, each with its own head word
#ifndef PBRS_WORK_HEADS
#define PBRS_WORK_HEADS 8u
#endif
#define PBRS_WORK_HEAD_STRIDE 32u  // u32 words between head words
// Queue positions per tile of the class sort (kernels.h, k_class_sort): one block per tile
#define PBRS_SORT_TILE 16384u
// k_extend's `split` argument (kernels.h; k_aov's and k_matte's `qsplit`), 0 where the queue is not split:
#define PBRS_QSPLIT_ON 1u   // the queue is split into kept and dropped paths
#define PBRS_QSPLIT_ENV 2u  // ... at the first bounce, where a miss sees the environment
