// morph.h -- morph targets (blend shapes) of a live scene's vertices (morph.hip): the device side of vkrt_scene_add_morph and
// vkrt_scene_morph_vertices.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "vertex_anim.h"
#include "vertex_record.h"

namespace vkrt {

// One morph's device arrays, carved out of one allocation (morph_carve): per vertex of [first, first + count) the base shape captured
// by vkrt_scene_add_morph (vertex_record.h Pose, 40 B, like a skin's bind pose) and, per attribute that has them, the deltas: vec3 at
// dword alignment, target-major ([targetCount][count][3] floats), so that the loads of one wave for one target are one contiguous
// span.  A delta pointer is NULL where the morph has no deltas for that attribute.
struct MorphArrays : VertexRange
{
  uint32_t targetCount = 0;
  Pose base;
  float* dPos = nullptr;
  float* dNrm = nullptr;
  float* dTan = nullptr;
};

// bytes of one morph's allocation, and the arrays inside it (hasPos / hasNrm / hasTan: which delta arrays it holds)
size_t morph_bytes(uint32_t count, uint32_t targetCount, bool hasPos, bool hasNrm, bool hasTan);
void morph_carve(void* mem, uint32_t first, uint32_t count, uint32_t targetCount, bool hasPos, bool hasNrm, bool hasTan, MorphArrays& out);

// One launch of k_morph on `stream`, no allocation, no host synchronisation: the captured base plus the weighted deltas (`weights`:
// device, 4-byte aligned, [targetCount]; a weight of exactly zero skips its target), by the arithmetic include/vkrt.h states.
// launch_morph_live writes positions[3 v ..] and the position, normal and tangent words of vertexPN[v], never the uv words;
// launch_morph_bind writes element i of `bind`, a skin's bind pose at the morph's first vertex (Pose::at), and nothing else.
hipError_t launch_morph_live(float* positions, float4* vertexPN, const MorphArrays& m, const float* weights, hipStream_t stream);
hipError_t launch_morph_bind(Pose bind, const MorphArrays& m, const float* weights, hipStream_t stream);

}  // namespace vkrt
