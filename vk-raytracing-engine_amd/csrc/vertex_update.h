// vertex_update.h -- deforming meshes of a live scene (vertex_update.hip): the device side of vkrt_scene_update_vertices.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace vkrt {

// New attributes for vertices [first, first + count) of the scene's shared vertex arrays.  The four sources are device memory, SoA like
// vkrt_scene_desc's arrays (vec3 / vec3 / vec4 / vec2 per vertex, element 0 = vertex `first`); nullptr = the attribute keeps its value.
struct VertexUpdate
{
  uint32_t first = 0, count = 0;
  const float* positions = nullptr;
  const float* normals = nullptr;
  const float* tangents = nullptr;
  const float* texcoords0 = nullptr;
};

// Enqueued on `stream`, no allocation, no host synchronisation: writes positions[3 v ..] (DevScene::positions) and the changed parts of
// the three float4 of vertexPN[v] (DevScene::vertexPN), bit for bit what vkrt_scene_create packs from the same arrays.  The caller has
// checked the range against the scene's vertex count.
hipError_t launch_vertex_update(float* positions, float4* vertexPN, const VertexUpdate& u, hipStream_t stream);

}  // namespace vkrt
