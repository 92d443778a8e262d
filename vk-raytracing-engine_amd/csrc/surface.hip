// surface.hip -- shading inputs at the hits of ray queries (vkrt_hit_surface, include/vkrt.h): raytrace.rchit:34-113 on caller records
// (instance, primitive, u, v) instead of the path tracer's record streams.  Needs no tree: a record is resolved the way rchit:34-50
// does it, instance -> primitive-mesh -> three indices, through a primitive-mesh table of the kernel's own (DevSurfaceScene).
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_scene.h"
#include "kernels.h"
#include "shade.h"

// rchit:68-79 + the geometric normal: what VKRT_SURFACE_GEOMETRY returns, in the operation order of closestHitFront (shade.h), whose
// loads these are (in the MATERIAL instantiation the compiler merges the two sets)
struct SurfaceGeom
{
  f3 worldPos, worldNrm, worldTag, worldBin, geomNrm;
  float tu, tv;
};

VKRT_DEV void surfaceGeometry(const DevScene& sc, const uint32_t instId, const uint32_t i0, const uint32_t i1, const uint32_t i2, const float u, const float v,
                              SurfaceGeom& g)
{
  const f3 b = mk3(1.0f - u - v, u, v);  // rchit:68 (texcoordAt forms the same b)
  const BufView vPN = bufView(sc.vertexPN), vInst = bufView(sc.instances);
  const float4 a0 = bufLoad4(vPN, VKRT_VERTEX_BYTES * i0), b0 = bufLoad4(vPN, VKRT_VERTEX_BYTES * i0 + 16u), tq0 = bufLoad4(vPN, VKRT_VERTEX_BYTES * i0 + 32u);
  const float4 a1 = bufLoad4(vPN, VKRT_VERTEX_BYTES * i1), b1 = bufLoad4(vPN, VKRT_VERTEX_BYTES * i1 + 16u), tq1 = bufLoad4(vPN, VKRT_VERTEX_BYTES * i1 + 32u);
  const float4 a2 = bufLoad4(vPN, VKRT_VERTEX_BYTES * i2), b2 = bufLoad4(vPN, VKRT_VERTEX_BYTES * i2 + 16u), tq2 = bufLoad4(vPN, VKRT_VERTEX_BYTES * i2 + 32u);
  DevInstance in;
  {
    const uint32_t io = 96u * instId;
    const float4 q0 = bufLoad4(vInst, io), q1 = bufLoad4(vInst, io + 16u), q2 = bufLoad4(vInst, io + 32u), q3 = bufLoad4(vInst, io + 48u), q4 = bufLoad4(vInst, io + 64u),
                 q5 = bufLoad4(vInst, io + 80u);
    in.o2w[0] = q0.x; in.o2w[1] = q0.y; in.o2w[2] = q0.z; in.o2w[3] = q0.w; in.o2w[4] = q1.x; in.o2w[5] = q1.y; in.o2w[6] = q1.z; in.o2w[7] = q1.w;
    in.o2w[8] = q2.x; in.o2w[9] = q2.y; in.o2w[10] = q2.z; in.o2w[11] = q2.w;
    in.w2o[0] = q3.x; in.w2o[1] = q3.y; in.w2o[2] = q3.z; in.w2o[3] = q3.w; in.w2o[4] = q4.x; in.w2o[5] = q4.y; in.w2o[6] = q4.z; in.w2o[7] = q4.w;
    in.w2o[8] = q5.x; in.primMesh = __float_as_int(q5.y); in.vis = 0u; in.pad = 0;
  }
  texcoordAt(b0, b1, b2, u, v, g.tu, g.tv);
  const f3 p0 = mk3(a0.x, a0.y, a0.z), p1 = mk3(a1.x, a1.y, a1.z), p2 = mk3(a2.x, a2.y, a2.z);
  const f3 pos = p0 * b.x + p1 * b.y + p2 * b.z;
  g.worldPos = xformPoint(in, pos);
  const f3 nrm = normalize3(mk3(a0.w, b0.x, b0.y) * b.x + mk3(a1.w, b1.x, b1.y) * b.y + mk3(a2.w, b2.x, b2.y) * b.z);
  g.worldNrm = normalize3(xformNormal(in, nrm));
  const f3 tag = normalize3(mk3(tq0.x, tq0.y, tq0.z) * b.x + mk3(tq1.x, tq1.y, tq1.z) * b.y + mk3(tq2.x, tq2.y, tq2.z) * b.z);
  f3 worldTag = normalize3(xformNormal(in, tag));
  worldTag = normalize3(worldTag - dot3(worldTag, g.worldNrm) * g.worldNrm);
  g.worldTag = worldTag;
  g.worldBin = tq0.w * cross3(g.worldNrm, worldTag);
  // the counter-clockwise front face of the object-space triangle, carried to world space like a vertex normal (inverse transpose)
  g.geomNrm = normalize3(xformNormal(in, cross3(p1 - p0, p2 - p0)));
}

// One lane per record.  hits: 2 float4 per record (vkrt_hit); out: 8 float4 per record (vkrt_surface).  A record that is not a hit of
// this scene (the range checks below, each before the load that depends on it) gives zeros with material = -1, valid = 0.
template <bool MATERIAL>
__global__ __launch_bounds__(256) void k_hit_surface(const DevSurfaceScene sc, const float4* __restrict__ hits, uint64_t n, float4* __restrict__ out)
{
  __shared__ float lutLds[MATERIAL ? 512 : 1];
  ShadeStats st;
  st.hits = st.diffuse = st.taps = 0u;
  st.lut = MATERIAL ? ldsTexelLut(sc, lutLds) : nullptr;
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if(i >= n)
    return;
  const float4 h0 = hits[2 * i], h1 = hits[2 * i + 1];
  const float u = h0.y, v = h0.z;
  const int inst = __float_as_int(h0.w), prim = __float_as_int(h1.x);
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float4 o0 = zero, o1 = zero, o2 = zero, o3 = zero, o4 = zero, o5 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1)), o6 = zero, o7 = zero;
  bool ok = inst >= 0 && (uint32_t)inst < sc.instanceCount && isfinite(u) && isfinite(v);
  uint4 pm = make_uint4(0u, 0u, 0u, 0u);
  if(ok)
  {
    pm = sc.primMeshes[sc.instances[inst].primMesh];  // (firstIndex, vertexOffset, triangles, max(0, materialIndex)); primMesh checked at upload
    ok = prim >= 0 && (uint32_t)prim < pm.z;
  }
  if(ok)
  {
    const uint32_t* idx = sc.indices + ((size_t)pm.x + 3u * (size_t)(uint32_t)prim);  // rchit:41-50
    const uint4 ts = make_uint4(idx[0] + pm.y, idx[1] + pm.y, idx[2] + pm.y, pm.w);
    SurfaceGeom g;
    surfaceGeometry(sc, (uint32_t)inst, ts.x, ts.y, ts.z, u, v, g);
    f3 shadingN = g.worldNrm, tangent = g.worldTag, binormal = g.worldBin;
    if(MATERIAL)
    {
      RayHit hit;
      hit.t = 0.0f; hit.u = u; hit.v = v; hit.slot = -1;
      Payload prd;
      prd.depth = 0u;  // the emission is evaluated (rchit:83)
      prd.isSpecular = false;
      HitMid mid;
      closestHitFront(sc, hit, (uint32_t)inst, ts, mk3(0.0f, 0.0f, 1.0f), prd, st, mid);
      shadingN = mid.N; tangent = mid.tangent; binormal = mid.binormal;
      o2.w = materialAlpha<false>(sc, ts.w, g.tu, g.tv, st.lut);  // texel.h: the value the walks' alpha test compares
      o3.w = mid.metalU;
      o4.w = mid.roughU;
      o6.x = mid.baseColor.x; o6.y = mid.baseColor.y; o6.z = mid.baseColor.z;
      o7.x = mid.emittance.x; o7.y = mid.emittance.y; o7.z = mid.emittance.z;
    }
    o0 = make_float4(g.worldPos.x, g.worldPos.y, g.worldPos.z, g.tu);
    o1 = make_float4(g.geomNrm.x, g.geomNrm.y, g.geomNrm.z, g.tv);
    o2.x = g.worldNrm.x; o2.y = g.worldNrm.y; o2.z = g.worldNrm.z;
    o3.x = shadingN.x; o3.y = shadingN.y; o3.z = shadingN.z;
    o4.x = tangent.x; o4.y = tangent.y; o4.z = tangent.z;
    o5 = make_float4(binormal.x, binormal.y, binormal.z, __int_as_float((int)ts.w));
    o6.w = __int_as_float(1);
  }
  float4* o = out + 8 * i;
  o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3; o[4] = o4; o[5] = o5; o[6] = o6; o[7] = o7;
}

// n records; material: VKRT_SURFACE_GEOMETRY | VKRT_SURFACE_MATERIAL, else the geometry alone (no texel is read)
hipError_t vkrt_launch_hit_surface(const DevSurfaceScene& sc, const float4* hits, uint32_t n, bool material, float4* out, hipStream_t stream)
{
  const dim3 g((unsigned)(((uint64_t)n + 255u) / 256u)), b(256);
  if(material)
    hipLaunchKernelGGL(k_hit_surface<true>, g, b, 0, stream, sc, hits, (uint64_t)n, out);
  else
    hipLaunchKernelGGL(k_hit_surface<false>, g, b, 0, stream, sc, hits, (uint64_t)n, out);
  return hipGetLastError();
}
