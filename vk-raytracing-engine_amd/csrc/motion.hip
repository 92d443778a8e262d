// motion.hip -- where the surface point of a hit record is now and where it was at the scene's last vkrt_scene_motion_mark
// (vkrt_hit_motion, include/vkrt.h): the world positions a temporal filter reprojects moving and deforming geometry with (NRD's IN_MV,
// as positions).  Needs no tree: a record (instance, primitive, u, v) is resolved and validated as k_hit_surface does it (surface.hip),
// through the primitive-mesh table of DevSurfaceScene.
// The point is formed in the operation order of k_gbuffer's wPos (hybrid.hip, the vert_shader.vert loop): every corner to world space
// first, then ((0 + P0 bw0) + P1 bw1) + P2 bw2 -- not raytrace.rchit's order (interpolate, then transform).  For a record of
// vkrt_gbuffer_raycast_hits the current point is then the G-buffer's position in every bit, and for a scene that did not move the
// previous point is the current one in every bit (a still frame's reprojection stays exactly on the pixel).
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_scene.h"
#include "kernels.h"
#include "query_common.h"
#include "shade.h"

namespace {

// rows of the object -> world matrix of one instance record: the first three of its six 16-byte quads
VKRT_DEV void motionLoadO2w(const DevInstance* __restrict__ instances, uint32_t inst, DevInstance& in)
{
  const float4* q = (const float4*)(instances + inst);
  const float4 q0 = q[0], q1 = q[1], q2 = q[2];
  in.o2w[0] = q0.x; in.o2w[1] = q0.y; in.o2w[2] = q0.z; in.o2w[3] = q0.w; in.o2w[4] = q1.x; in.o2w[5] = q1.y; in.o2w[6] = q1.z; in.o2w[7] = q1.w;
  in.o2w[8] = q2.x; in.o2w[9] = q2.y; in.o2w[10] = q2.z; in.o2w[11] = q2.w;
}

VKRT_DEV float4 motionPoint(const DevInstance& in, f3 p0, f3 p1, f3 p2, const float bw[3])
{
  f3 w = mk3(0.0f);
  w = w + xformPoint(in, p0) * bw[0];
  w = w + xformPoint(in, p1) * bw[1];
  w = w + xformPoint(in, p2) * bw[2];
  return make_float4(w.x, w.y, w.z, 1.0f);
}

}  // namespace

// One lane per record of [first, end).  hits: 2 float4 per record (vkrt_hit); cur / prev: one float4 per record, either may be NULL.
__global__ __launch_bounds__(64) void k_hit_motion(const DevMotionScene sc, const float4* __restrict__ hits, uint64_t first, uint64_t end,
                                                   float4* __restrict__ cur, float4* __restrict__ prev)
{
  const uint64_t i = first + (uint64_t)blockIdx.x * 64u + threadIdx.x;
  if(i >= end)
    return;
  const float4 h0 = hits[2 * i], h1 = hits[2 * i + 1];
  const float u = h0.y, v = h0.z;
  const int inst = __float_as_int(h0.w), prim = __float_as_int(h1.x);
  float4 oc = make_float4(0.0f, 0.0f, 0.0f, 0.0f), op = oc;
  // the range checks of k_hit_surface, each before the load that depends on it
  bool ok = inst >= 0 && (uint32_t)inst < sc.instanceCount && isfinite(u) && isfinite(v);
  uint4 pm = make_uint4(0u, 0u, 0u, 0u);
  if(ok)
  {
    pm = sc.primMeshes[sc.instances[inst].primMesh];  // (firstIndex, vertexOffset, triangles, material); an update keeps a node's primMesh
    ok = prim >= 0 && (uint32_t)prim < pm.z;
  }
  if(ok)
  {
    const uint32_t* idx = sc.indices + ((size_t)pm.x + 3u * (size_t)(uint32_t)prim);
    const uint32_t i0 = idx[0] + pm.y, i1 = idx[1] + pm.y, i2 = idx[2] + pm.y;
    const float bw[3] = {1.0f - u - v, u, v};
    DevInstance in;
    if(cur)
    {
      const float4 a0 = sc.vertexPN[VKRT_VERTEX_QUADS * (size_t)i0], a1 = sc.vertexPN[VKRT_VERTEX_QUADS * (size_t)i1],
                   a2 = sc.vertexPN[VKRT_VERTEX_QUADS * (size_t)i2];
      motionLoadO2w(sc.instances, (uint32_t)inst, in);
      oc = motionPoint(in, mk3(a0.x, a0.y, a0.z), mk3(a1.x, a1.y, a1.z), mk3(a2.x, a2.y, a2.z), bw);
    }
    if(prev)
    {
      const float* __restrict__ P = sc.prevPositions;
      const f3 p0 = mk3(P[3 * (size_t)i0], P[3 * (size_t)i0 + 1], P[3 * (size_t)i0 + 2]);
      const f3 p1 = mk3(P[3 * (size_t)i1], P[3 * (size_t)i1 + 1], P[3 * (size_t)i1 + 2]);
      const f3 p2 = mk3(P[3 * (size_t)i2], P[3 * (size_t)i2 + 1], P[3 * (size_t)i2 + 2]);
      motionLoadO2w(sc.prevInstances, (uint32_t)inst, in);
      op = motionPoint(in, p0, p1, p2, bw);
    }
  }
  if(cur)
    cur[i] = oc;
  if(prev)
    prev[i] = op;
}

hipError_t vkrt_launch_hit_motion(const DevMotionScene& sc, const float4* hits, uint32_t n, float4* cur, float4* prev, hipStream_t stream)
{
  return query_launch_chunks(n, [&](uint64_t first, uint64_t end, dim3 grid) {
    hipLaunchKernelGGL(k_hit_motion, grid, dim3(64), 0, stream, sc, hits, first, end, cur, prev);
  });
}
