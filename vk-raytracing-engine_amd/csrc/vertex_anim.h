// vertex_anim.h -- what vkrt_scene_update_vertices, vkrt_scene_add_skin / _skin_vertices and vkrt_scene_add_morph / _morph_vertices
// refuse before they touch the device, each rule once (vertex_anim.cpp).  No HIP type: tests/test_vertex_anim.py compiles it with g++.
// Like scene_pack.h: VKRT_OK, or a vkrt code with the whole message of vkrt_last_error in err.  A call that is accepted leaves err
// alone and allocates nothing.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include "../../include/vkrt.h"

namespace vkrt {

struct VertexRange
{
  uint32_t first = 0, count = 0;
};

// The disjoint vertex ranges of a scene's skins or morphs, numbered as they were added.  A view: the ranges live in the scene's own
// records, `stride` bytes apart, so no call copies them.
struct RangeSet
{
  const VertexRange* ranges = nullptr;
  size_t size = 0, stride = sizeof(VertexRange);
  const VertexRange& operator[](size_t j) const { return *(const VertexRange*)((const char*)ranges + j * stride); }
  // the member that overlaps [first, first + count), or -1 (the members are disjoint: a range inside one touches no other)
  int overlapping(uint32_t first, uint32_t count) const;
  // whether [first, first + count) lies wholly inside member j
  bool contains(size_t j, uint32_t first, uint32_t count) const;
};

// the rules every call shares
int check_memory(const char* who, uint32_t memory, std::string& err);  // VKRT_MEMORY_HOST or VKRT_MEMORY_DEVICE
int check_vertex_range(const char* who, uint32_t first, uint32_t count, size_t vertexCount, std::string& err);  // first + count in 64 bits
size_t first_non_finite(const float* a, size_t n);  // index of the first float that is not finite, or n

// Per entry point, in the order include/vkrt.h lists the refusals: what can be said of the arguments alone (check_*_desc, and
// check_memory for the two posing calls), then -- behind the caller's NULL out_* and NULL scene refusals -- what needs the scene.
int check_update_desc(const vkrt_vertex_update* u, std::string& err);
int check_update_range(const vkrt_vertex_update& u, size_t vertexCount, std::string& err);  // outside the scene, a non-finite host position

int check_skin_desc(const vkrt_skin_desc* k, std::string& err);
// outside the scene, empty, over a skin, over a morph ("add skins before morphs")
int check_skin_range(const vkrt_skin_desc& k, size_t vertexCount, const RangeSet& skins, const RangeSet& morphs, std::string& err);
// the skin's number, then (jointCount known) the matrices: NULL, misaligned device memory, a non-finite host value
int check_skin_index(uint32_t skin, size_t skinCount, std::string& err);
int check_joint_matrices(const float* jointMatrices, uint32_t memory, uint32_t jointCount, std::string& err);

int check_morph_desc(const vkrt_morph_desc* m, std::string& err);
// outside the scene, empty, over a morph, across a skin's boundary; inSkin = the skin the range lies inside, or -1
int check_morph_range(const vkrt_morph_desc& m, size_t vertexCount, const RangeSet& skins, const RangeSet& morphs, int& inSkin, std::string& err);
int check_morph_index(uint32_t morph, size_t morphCount, std::string& err);
int check_morph_weights(const float* weights, uint32_t memory, uint32_t targetCount, std::string& err);

}  // namespace vkrt
