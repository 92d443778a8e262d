// entry_checks.h -- what the node-update, visibility, material-alpha, scene-edit, query and frame entry points refuse of their arguments before they
// touch the device, each rule once (entry_checks.cpp).  No HIP type: tests/test_entry_checks.py compiles it with g++.  Like
// vertex_anim.h: VKRT_OK, or a vkrt code with the whole message of vkrt_last_error in err; the functions take plain facts -- counts,
// pointers, the structs of include/vkrt.h -- and never a scene.  A call that is accepted leaves err alone and allocates nothing.  The
// entry points keep their own NULL-scene refusals and chain these in the order include/vkrt.h lists them.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>
#include "../../include/vkrt.h"

namespace vkrt {

// ---- node updates
// [first, first + count) in 64 bits against the scene's nodes; who = NULL: the message carries no caller (vkrt_scene_update_nodes)
int check_node_range(const char* who, uint32_t first, uint32_t count, size_t nodeCount, std::string& err);
// vkrt_scene_update_nodes: an update moves node `node`, it does not change its geometry
int check_prim_mesh_kept(uint32_t node, int32_t given, int32_t kept, std::string& err);
// vkrt_scene_update_node_transforms, of the descriptor alone: NULL, struct_size, memory, first != 0 with node_indices
int check_node_update_desc(const vkrt_node_update* u, std::string& err);
// behind the NULL-scene refusal: the dense range, NULL matrices, then device arrays misaligned or -- host memory, read here -- an index
// outside the scene and a matrix value that is not finite, with its entry and node
int check_node_update_range(const vkrt_node_update& u, size_t nodeCount, std::string& err);

// ---- instance visibility and material alpha: the setters' arrays (NULL with count > 0, then entry by entry), then -- behind the
// NULL-scene refusal -- the range, which the getters share
int check_visibility_values(const char* who, uint32_t count, const vkrt_instance_visibility* vis, std::string& err);
int check_alpha_values(const char* who, uint32_t count, const vkrt_material_alpha* alpha, std::string& err);
int check_material_range(const char* who, uint32_t first, uint32_t count, uint32_t materialCount, std::string& err);

// ---- editing a live scene (vkrt_scene_update_lights / _materials / _texture), each in the order include/vkrt.h lists
// of the descriptor alone: NULL, struct_size, memory
int check_light_update_desc(const vkrt_light_update* u, std::string& err);
// behind the NULL-scene refusal: the range, NULL lights with count > 0, a misaligned device array
int check_light_update_range(const vkrt_light_update& u, uint32_t lightCount, std::string& err);
// the array (NULL with count > 0); then, when the scene is known and has textures (textureCount > 0), the rule of validate_scene: no
// texture index >= textureCount.  The range behind the NULL-scene refusal is check_material_range's
int check_material_update_values(const char* who, uint32_t count, const GltfPBRMaterial* materials, uint32_t textureCount, std::string& err);
int check_texture_update_desc(const vkrt_texture_update* u, std::string& err);
// behind the NULL-scene refusal: the index; then, with the size of that texture, the size, NULL rgba8, a misaligned device array
int check_texture_index(const char* who, uint32_t texture, uint32_t textureCount, std::string& err);
int check_texture_update_image(const vkrt_texture_update& u, uint32_t width, uint32_t height, std::string& err);

// ---- queries
// the options of vkrt_intersect_ex / vkrt_occluded_ex / vkrt_intersect_multi (include/vkrt.h)
int check_query_opts(const vkrt_query_opts* q, const char* who, std::string& err);
// the options of vkrt_closest_point: those of vkrt_intersect_ex (NULL = the defaults), and no ray flag -- a point has no facing and no
// any-hit stage.  q = the options the call runs with
int check_point_opts(const vkrt_query_opts* opts, const char* who, vkrt_query_opts& q, std::string& err);
int check_max_hits(uint32_t maxHits, std::string& err);  // vkrt_intersect_multi: 1..VKRT_MULTIHIT_MAX
// The arrays of a query call, behind its NULL-scene refusal (n > 0): one that is NULL, then one that is misaligned.  alignText: the
// call's list of alignments as its message shows it.
struct QueryArray
{
  const void* p;
  unsigned align;  // bytes, a power of two
  bool mayBeNull;
};
int check_query_arrays(const char* who, uint32_t n, std::initializer_list<QueryArray> arrays, const char* alignText, std::string& err);

// ---- frames.  (vkrt_shard_rows, the third rule of a shard, is include/vkrt.h's own and defined beside these.)
int check_shard(const vkrt_shard* shard, std::string& err);
int shard_tiles(const vkrt_shard* shard, uint32_t& tileCount, std::string& err);  // 8x8 tiles that cover a shard's rows
int check_frame_count(uint32_t nFrames, int32_t firstFrame, std::string& err);    // vkrt_pathtrace_frames: 1..65536, and the last frame's number fits
int check_lights_count(const char* what, int32_t lightsCount, uint32_t lightCount, std::string& err);  // what: the argument as the message names it
// what = "samples/depth" (vkrt_pathtrace*), or "depth" with samples = 0 (vkrt_hybrid_trace*, which reads no sample count)
int check_samples_depth(const char* what, int32_t samples, int32_t depth, std::string& err);

}  // namespace vkrt
