// vertex_update.hip -- deforming meshes of a live scene: the device side of vkrt_scene_update_vertices (include/vkrt.h).
//
// The Vulkan interface that vkrt_accel_build stands in for updates a bottom-level acceleration structure in place from a new vertex
// buffer (VK_BUILD_ACCELERATION_STRUCTURE_MODE_UPDATE_KHR), usually one a compute shader has just written.  Here the vertices live in two
// device arrays that every later stage reads: DevScene::positions (vec3, read by the builders' k_flatten and by the refit's k_rf_tris)
// and DevScene::vertexPN (three float4 per vertex: position + normal.x | normal.yz + uv | tangent, read by the hit shading, the hybrid
// mode and the G-buffer).  k_vertex_update copies the caller's SoA arrays into both; vkrt_accel_refit then re-derives records and boxes.
//
// One lane per vertex, pure streaming: 12 + 12 + 16 + 8 B read and 12 + 48 B written per vertex when everything is given.  The record
// side is 16-byte aligned, so every attribute combination is written with the widest store that touches no kept word (no
// read-modify-write: a kept attribute is never loaded).  The caller's vec3 arrays are only 4-byte aligned (12-byte stride): they are
// read as three-dword vectors (global_load_dwordx3), and tangents and texture coordinates as four- and two-dword vectors: gfx950 takes
// multi-dword global accesses at dword alignment, so one code path serves every pointer the caller may pass.
#include <hip/hip_runtime.h>

#include "vertex_record.h"
#include "vertex_update.h"

namespace vkrt {

namespace {

// vertex_record.h's vectors at the alignment of a float, like its f3u: the caller's arrays
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

__global__ __launch_bounds__(256) void k_vertex_update(uint32_t first, uint32_t count, const float* __restrict__ pos, const float* __restrict__ nrm,
                                                       const float* __restrict__ tan, const float* __restrict__ uv, float* __restrict__ positions, float4* __restrict__ vertexPN)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= count)
    return;
  const size_t v = (size_t)first + i;
  float* rec = (float*)(vertexPN + VKRT_VERTEX_QUADS * v);  // 48 B, 16-byte aligned
  f3 p = {0.f, 0.f, 0.f}, n = {0.f, 0.f, 0.f};
  if(pos)
    p = *(const f3u*)(pos + 3 * (size_t)i);
  if(nrm)
    n = *(const f3u*)(nrm + 3 * (size_t)i);
  if(pos)
    *(f3u*)(positions + 3 * v) = p;
  // quad 0 = position.xyz, normal.x; quad 1 = normal.yz, uv
  if(pos && nrm)
    *(f4*)rec = f4{p.x, p.y, p.z, n.x};
  else if(pos)
    *(f3*)rec = p;
  else if(nrm)
    rec[3] = n.x;
  f2 t = {0.f, 0.f};
  if(uv)
    t = *(const f2u*)(uv + 2 * (size_t)i);
  if(nrm && uv)
    *(f4*)(rec + 4) = f4{n.y, n.z, t.x, t.y};
  else if(nrm)
    *(f2*)(rec + 4) = f2{n.y, n.z};
  else if(uv)
    *(f2*)(rec + 6) = t;
  // quad 2 = tangent
  if(tan)
    *(f4*)(rec + 8) = *(const f4u*)(tan + 4 * (size_t)i);
}

}  // namespace

hipError_t launch_vertex_update(float* positions, float4* vertexPN, const VertexUpdate& u, hipStream_t stream)
{
  if(u.count == 0 || (!u.positions && !u.normals && !u.tangents && !u.texcoords0))
    return hipSuccess;
  const unsigned B = 256;
  hipLaunchKernelGGL(k_vertex_update, dim3((u.count + B - 1) / B), dim3(B), 0, stream, u.first, u.count, u.positions, u.normals, u.tangents,
                     u.texcoords0, positions, vertexPN);
  return hipGetLastError();
}

}  // namespace vkrt
