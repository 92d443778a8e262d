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

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f3 __attribute__((ext_vector_type(3)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f3u __attribute__((ext_vector_type(3), aligned(4)));  // the scene's own vec3 positions

static_assert(VKRT_VERTEX_QUADS == 3, "the skin kernels read and write the three float4 of a vertex record");

constexpr unsigned kBlock = 256;

__global__ __launch_bounds__(kBlock) void k_skin_capture(uint32_t first, uint32_t count, const float* __restrict__ positions,
                                                         const float4* __restrict__ vertexPN, float4* __restrict__ bindPN,
                                                         float2* __restrict__ bindNyz, float4* __restrict__ bindTan)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= count)
    return;
  const size_t v = (size_t)first + i;
  const f3 p = *(const f3u*)(positions + 3 * v);
  const float4* rec = vertexPN + VKRT_VERTEX_QUADS * v;
  const float4 q0 = rec[0], q1 = rec[1];
  bindPN[i] = make_float4(p.x, p.y, p.z, q0.w);
  bindNyz[i] = make_float2(q1.x, q1.y);
  bindTan[i] = rec[2];
}

// M * (x, y, z) over the blended 3x3: (M[r][0] * x + M[r][1] * y) + M[r][2] * z per row
__device__ __forceinline__ f3 mul3(f3 c0, f3 c1, f3 c2, f3 a) { return (c0 * a.x + c1 * a.y) + c2 * a.z; }

// device_math.h normalize3, guarded: a zero or overflowing length leaves the vector as it is
__device__ __forceinline__ f3 normalizeGuarded(f3 a)
{
  const float d = (a.x * a.x + a.y * a.y) + a.z * a.z;
  if(d > 0.0f && d < __builtin_inff())
  {
    const float inv = 1.0f / sqrtf(d);
    return a * inv;
  }
  return a;
}

__global__ __launch_bounds__(kBlock) void k_skin(uint32_t first, uint32_t count, const float4* __restrict__ bindPN, const float2* __restrict__ bindNyz,
                                                 const float4* __restrict__ bindTan, const uint2* __restrict__ joints, const float4* __restrict__ weights,
                                                 const float4* __restrict__ palette, float* __restrict__ positions, float4* __restrict__ vertexPN)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= count)
    return;
  const uint2 jj = joints[i];
  const float4 w = weights[i];
  const float4 b0 = bindPN[i];
  const float2 b1 = bindNyz[i];
  const float4 b2 = bindTan[i];
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
  const f3 p = mul3(col[0], col[1], col[2], f3{b0.x, b0.y, b0.z}) + col[3];
  const f3 n = normalizeGuarded(mul3(col[0], col[1], col[2], f3{b0.w, b1.x, b1.y}));
  const f3 t = normalizeGuarded(mul3(col[0], col[1], col[2], f3{b2.x, b2.y, b2.z}));
  const size_t v = (size_t)first + i;
  float* rec = (float*)(vertexPN + VKRT_VERTEX_QUADS * v);  // 48 B, 16-byte aligned
  *(f3u*)(positions + 3 * v) = p;
  *(f4*)rec = f4{p.x, p.y, p.z, n.x};        // quad 0 = position.xyz, normal.x
  *(f2*)(rec + 4) = f2{n.y, n.z};            // quad 1 = normal.yz, uv (kept)
  *(f4*)(rec + 8) = f4{t.x, t.y, t.z, b2.w};  // quad 2 = tangent, its handedness as given
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

}  // namespace

size_t skin_bytes(uint32_t count) { return 3 * (size_t)count * 16 + 2 * align16((size_t)count * 8); }

void skin_carve(void* mem, uint32_t first, uint32_t count, SkinArrays& out)
{
  char* at = (char*)mem;
  out.first = first;
  out.count = count;
  out.bindPN = (float4*)at;   at += (size_t)count * 16;
  out.bindTan = (float4*)at;  at += (size_t)count * 16;
  out.weights = (float4*)at;  at += (size_t)count * 16;
  out.bindNyz = (float2*)at;  at += align16((size_t)count * 8);
  out.joints = (uint2*)at;
}

hipError_t launch_skin_capture(const float* positions, const float4* vertexPN, const SkinArrays& k, hipStream_t stream)
{
  if(k.count == 0)
    return hipSuccess;
  hipLaunchKernelGGL(k_skin_capture, dim3((k.count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, k.first, k.count, positions, vertexPN, k.bindPN,
                     k.bindNyz, k.bindTan);
  return hipGetLastError();
}

hipError_t launch_skin(float* positions, float4* vertexPN, const SkinArrays& k, const float4* jointMatrices, hipStream_t stream)
{
  if(k.count == 0)
    return hipSuccess;
  hipLaunchKernelGGL(k_skin, dim3((k.count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, k.first, k.count, k.bindPN, k.bindNyz, k.bindTan, k.joints,
                     k.weights, jointMatrices, positions, vertexPN);
  return hipGetLastError();
}

}  // namespace vkrt
