// skin.hip -- linear-blend skinning inside the library: the device side of vkrt_scene_add_skin / vkrt_scene_skin_vertices
// (include/vkrt.h).
//
// A skinned glTF mesh carries JOINTS_0 / WEIGHTS_0 per vertex and is posed every frame from a palette of joint matrices.  The scene's
// vertices live in DevScene::positions (vec3) and DevScene::vertexPN (three float4 per vertex: position + normal.x | normal.yz + uv |
// tangent); k_skin writes both straight from the bind pose that k_skin_capture copied out of them when the skin was added, so no
// caller-side blend, no SoA arrays in between and no second pass (k_vertex_update) are needed.  vkrt_accel_refit then follows.
//
// One lane per vertex, pure streaming: 40 B of bind pose + 8 B of joints + 16 B of weights read, the four gathered joint matrices
// (three rows of four columns each, read as the caller's column-major float4 columns: the palette is a few KiB and stays in cache),
// 12 + 40 B written.  The record side is 16-byte aligned: quad 0 and the tangent go out as four-dword stores, normal.yz as a two-dword
// store that leaves the uv words beside it alone, the vec3 position as a three-dword store at dword alignment.
//
// Arithmetic (binary32, source order, no contraction: the Makefile's -ffp-contract=off): see include/vkrt.h.
#include <hip/hip_runtime.h>

#include "device_scene.h"
#include "skin.h"

namespace vkrt {

namespace {

constexpr unsigned kBlock = 256;

__global__ __launch_bounds__(kBlock) void k_skin_capture(uint32_t first, uint32_t count, const float* __restrict__ positions,
                                                         const float4* __restrict__ vertexPN, float4* __restrict__ posePN,
                                                         float2* __restrict__ poseNyz, float4* __restrict__ poseTan)
{
  const Pose pose = {posePN, poseTan, poseNyz};  // (as three arguments in this order: the registers come out as they always did)
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= count)
    return;
  const size_t v = (size_t)first + i;
  const f3 p = *(const f3u*)(positions + 3 * v);
  const float4* rec = vertexPN + VKRT_VERTEX_QUADS * v;
  const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2];
  pose_store(pose, i, PoseVertex{p, {q0.w, q1.x, q1.y}, {q2.x, q2.y, q2.z}, q2.w});
}

// M * (x, y, z) over the blended 3x3: (M[r][0] * x + M[r][1] * y) + M[r][2] * z per row
__device__ __forceinline__ f3 mul3(f3 c0, f3 c1, f3 c2, f3 a) { return (c0 * a.x + c1 * a.y) + c2 * a.z; }

__global__ __launch_bounds__(kBlock) void k_skin(uint32_t first, uint32_t count, Pose bind, const uint2* __restrict__ joints,
                                                 const float4* __restrict__ weights, const float4* __restrict__ palette, float* __restrict__ positions,
                                                 float4* __restrict__ vertexPN)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= count)
    return;
  const uint2 jj = joints[i];
  const float4 w = weights[i];
  const PoseVertex b = pose_load(bind, i);
  const float4* J0 = palette + 4u * (jj.x & 0xffffu);
  const float4* J1 = palette + 4u * (jj.x >> 16);
  const float4* J2 = palette + 4u * (jj.y & 0xffffu);
  const float4* J3 = palette + 4u * (jj.y >> 16);
  // column c of the blended matrix, rows 0..2: ((w0 * J0 + w1 * J1) + w2 * J2) + w3 * J3
  f3 col[4];
#pragma unroll
  for(int c = 0; c < 4; c++)
  {
    const float4 a0 = J0[c], a1 = J1[c], a2 = J2[c], a3 = J3[c];
    const f3 e0 = {a0.x, a0.y, a0.z}, e1 = {a1.x, a1.y, a1.z}, e2 = {a2.x, a2.y, a2.z}, e3 = {a3.x, a3.y, a3.z};
    col[c] = ((e0 * w.x + e1 * w.y) + e2 * w.z) + e3 * w.w;
  }
  const f3 p = mul3(col[0], col[1], col[2], b.p) + col[3];
  const f3 n = normalizeGuarded(mul3(col[0], col[1], col[2], b.n));
  const f3 t = normalizeGuarded(mul3(col[0], col[1], col[2], b.t));
  live_store(positions, vertexPN, (size_t)first + i, PoseVertex{p, n, t, b.tw});
}

}  // namespace

size_t skin_bytes(uint32_t count) { return 3 * (size_t)count * 16 + 2 * align16((size_t)count * 8); }

void skin_carve(void* mem, uint32_t first, uint32_t count, SkinArrays& out)
{
  out.first = first;
  out.count = count;
  out.weights = (float4*)pose_carve((char*)mem, count, out.bind);
  out.joints = (uint2*)(out.weights + count);
}

hipError_t launch_pose_capture(const float* positions, const float4* vertexPN, uint32_t first, uint32_t count, Pose pose, hipStream_t stream)
{
  if(count == 0)
    return hipSuccess;
  hipLaunchKernelGGL(k_skin_capture, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, first, count, positions, vertexPN, pose.pn,
                     pose.nyz, pose.tan);
  return hipGetLastError();
}

hipError_t launch_skin(float* positions, float4* vertexPN, const SkinArrays& k, const float4* jointMatrices, hipStream_t stream)
{
  if(k.count == 0)
    return hipSuccess;
  hipLaunchKernelGGL(k_skin, dim3((k.count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, k.first, k.count, k.bind, k.joints, k.weights,
                     jointMatrices, positions, vertexPN);
  return hipGetLastError();
}

}  // namespace vkrt
