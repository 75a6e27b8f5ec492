// host/scene_prepare.h — what pbrs_upload_scene does to a pbrs_scene_desc before anything touches the device: plain C++, no HIP
// header, so that tests/scene_prepare_check.cpp runs it on a CPU under AddressSanitizer.
//
//   check_scene    every index the kernels dereference is in range, and the scene is within the limits of the device code
//   prepare_scene  of a checked scene: the node array the walks read (TLAS, leaf copies, BLASes with absolute links), the split
//                  planes of its inner BLAS nodes, the device copies of the instance records, the four-wide nodes, the DevScene scalars and the SceneFacts of choose_kernels
// Neither copies the triangle, material, texture or light arrays: those go to the device straight from the descriptor.
#pragma once
#include <cstdint>
#include <vector>

#include "../device/scene.h"
#include "kernel_choice.h"

namespace pbrs {

// The levels of the scene's trees, from the trees themselves (the heights in the description are not trusted), and the depth of the
// per-lane traversal stack they ask for.  check_scene needs them for its limit and hands them on to prepare_scene: one pass over the nodes.
struct SceneLevels {
    uint32_t tlas = 0;          // levels of the TLAS (a lone leaf: 1)
    uint32_t max_blas = 0;      // ... of the deepest BLAS a walk can enter
    uint32_t stack = 0;         // entries of a lane's traversal stack
    bool exact_extent = false;  // a ParallelQuad next to a mesh: DevScene::exact_extent
};
struct SceneCheck {
    int code = PBRS_OK;             // PBRS_OK, or the code pbrs_upload_scene returns
    const char* message = nullptr;  // ... and its pbrs_last_error
    SceneLevels levels;             // of an accepted scene
};
SceneCheck check_scene(const pbrs_scene_desc& d);

struct PreparedScene {
    DevScene S{};  // every scalar but the lds_* of the kernel choice (pbrs_upload_scene); the pointers are null
    std::vector<pbrs_node> nodes;    // DevScene::nodes
    std::vector<uint32_t> node_planes;  // per node of `nodes`: the split planes of an inner BLAS node, packed for its b word (device/split_planes.h); 0 for leaves and the TLAS
    std::vector<pbrs_instance> inst; // DevScene::inst: pad[0] the shading class, pad[1] the wide root, blas_root and flags as the walks read them
    std::vector<pbrs_wnode> wide;    // DevScene::wnodes; empty where the scene keeps the binary walks (S.wnodes stays null)
    std::vector<uint32_t> tri_leaf;  // DevScene::tri_leaf: per triangle record, the BLAS leaf of `nodes` that holds it; built with the wide nodes, empty without them
    std::vector<uint32_t> light_link;  // per area light: the analytic instance that is the light, as a PBRS_SKIP_* word (device/scene.h); 0: none
    uint32_t wide_levels = 0;        // wide nodes on the longest way down a BLAS (0: no wide nodes)
    SceneFacts facts;
    uint32_t stack_depth = 0;      // entries of a lane's traversal stack
    // The instance with the entry table (DevScene::entry_inst, device/entry_nodes.h), if any: the levels of its BLAS, and the stack rows
    // a lane has left when it enters it (the stack less the TLAS entries that may wait below the instance)
    uint32_t entry_height = 0, entry_rows = 0;
    bool has_vis_records = false;  // every material names its pbrs_material::vis_bxdf record (normal_visualizer)
    uint64_t walk_bytes = 0;       // what the walks read: nodes, wide nodes, tri_leaf, triangle vertices, instance records (pbrs_ctx::overlap_from)
};
// `d` has passed check_scene, which returned `levels`.  Of `dev`, refill_below alone is read (DevScene::refill_below).
PreparedScene prepare_scene(const pbrs_scene_desc& d, const SceneLevels& levels, const DevOverrides& dev);
// What pbrs_upload_scene does to `P.wide` before it uploads it: the references to leaves of one to four triangles take the form that names
// the triangles themselves (device/scene.h, PBRS_WREF_PACKED).  Returns how many it rewrote.
uint32_t pack_wide_leaves(PreparedScene& P);
// ... and to its copy of the description's area lights before it uploads that: `P.light_link` into the records' padding words.
void write_light_links(const PreparedScene& P, std::vector<pbrs_area_light>& lights);

}  // namespace pbrs
