// skin.h -- linear-blend skinning of a live scene's vertices (skin.hip): the device side of vkrt_scene_add_skin and
// vkrt_scene_skin_vertices.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "vertex_anim.h"
#include "vertex_record.h"

namespace vkrt {

// One skin's device arrays, carved out of one allocation (skin_carve): per vertex of [first, first + count) the bind pose captured by
// vkrt_scene_add_skin (vertex_record.h Pose, 40 B) and the influences (16 B of weights, 8 B of joint indices).  Every array starts
// 16-byte aligned.
struct SkinArrays : VertexRange
{
  Pose bind;
  float4* weights = nullptr;  // WEIGHTS_0
  uint2* joints = nullptr;    // JOINTS_0: four u16, (j0 | j1 << 16, j2 | j3 << 16)
};

// bytes of one skin's allocation, and the arrays inside it
size_t skin_bytes(uint32_t count);
void skin_carve(void* mem, uint32_t first, uint32_t count, SkinArrays& out);

// Vertices [first, first + count) as the scene's arrays hold them at this point of `stream`, into `pose` (a skin's bind pose, a morph's
// base shape): a device copy out of `positions` (DevScene::positions) and `vertexPN` (DevScene::vertexPN).
hipError_t launch_pose_capture(const float* positions, const float4* vertexPN, uint32_t first, uint32_t count, Pose pose, hipStream_t stream);

// One launch of k_skin on `stream`, no allocation, no host synchronisation: the bind pose blended through `jointMatrices` (device,
// 16-byte aligned, [joint_count][16] column-major, rows 0..2 read) into positions[3 v ..] and the position, normal and tangent words of
// vertexPN[v]; the uv words are not touched.  The arithmetic is the one include/vkrt.h states.  Every joint index of the skin was
// checked against joint_count by vkrt_scene_add_skin, so the gather stays inside the palette.
hipError_t launch_skin(float* positions, float4* vertexPN, const SkinArrays& k, const float4* jointMatrices, hipStream_t stream);

}  // namespace vkrt
