// query.hip -- batched ray queries on caller rays (vkrt_intersect / vkrt_occluded, include/vkrt.h): the traversal kernel of the
// wavefront pipeline (wf_traverse.hip) reading vkrt_ray records and writing vkrt_hit records instead of path-record streams.
// Built with the flags of wf_traverse.hip (csrc/Makefile) for the same reasons: the walks are the same code.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_scene.h"
#include "kernels.h"
#include "traverse.h"
#include "traverse_wide.h"
#include "traverse_share.h"
#include "wf_streams.h"  // wfLoad
#include "wide_node.h"

// A ray the walks never see: tmin < 0, tmin >= tmax (NaN bounds included), a zero direction, a NaN or infinite origin or direction component
VKRT_DEV bool queryRayValid(float4 r0, float4 r1)
{
  const bool finite = isfinite(r0.x) && isfinite(r0.y) && isfinite(r0.z) && isfinite(r1.x) && isfinite(r1.y) && isfinite(r1.z);
  const bool nonzero = r1.x != 0.0f || r1.y != 0.0f || r1.z != 0.0f;
  return finite && nonzero && r0.w >= 0.0f && r0.w < r1.w;
}

// One thread per ray, one wave per workgroup.  rays: 2 float4 per ray (origin, tmin) (direction, tmax); hits: 2 float4 per ray
// (t, u, v, instance) (primitive, prim_mesh, triangle, material) as int bits; occ: one int per ray (ANYHIT).  Rays [first, n).
// TM & VKRT_TM_FILTER: the walks read the query fields of sc (traverse.h query_rejects); a cull mask of 0 admits nothing, so every
// ray is a miss without a walk.
template <bool ANYHIT, bool WIDE, int TM>
__global__ __launch_bounds__(64)
__attribute__((amdgpu_waves_per_eu(TM != 0 && WIDE ? 5 : 1)))
void k_query(const DevQueryScene sc, const float4* __restrict__ rays, uint64_t first, uint64_t n, uint32_t seed, float4* __restrict__ hits,
             int* __restrict__ occ)
{
  extern __shared__ int lds_stack[];
  __shared__ int shareLds[VKRT_SHARE_LDS_WORDS];
  const uint64_t i = first + (uint64_t)blockIdx.x * 64u + threadIdx.x;
  const bool inRange = i < n;
  float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
  if(inRange)
  {
    r0 = wfLoad(rays + 2 * i);
    r1 = wfLoad(rays + 2 * i + 1);
  }
  const bool valid = inRange && queryRayValid(r0, r1) && (!(TM & VKRT_TM_FILTER) || sc.cullMask != 0u);
  const unsigned long long validMask = __ballot(valid);
  RayHit hit;
  hit.t = r1.w; hit.u = 0.0f; hit.v = 0.0f; hit.slot = -1;
  TravCount tc;
  if(validMask != 0ull)  // (wave-uniform: a wave of rejected rays walks nothing)
  {
    const f3 o = valid ? mk3(r0.x, r0.y, r0.z) : mk3(0.0f, 0.0f, 0.0f);
    const f3 d = valid ? mk3(r1.x, r1.y, r1.z) : mk3(1.0f, 0.0f, 0.0f);
    const float tmax = valid ? r1.w : 0.0f;
    // The shared walk hands (origin, direction, tmax) of a ray to the lanes that adopt part of it, but every lane tests against its
    // own tmin: it serves waves whose rays share one tmin (a batch with one scalar bound), the others walk lane by lane.
    const float tmin0 = __shfl(r0.w, __ffsll((long long)validMask) - 1);
    const bool share = WIDE && sc.shareMinIdle != 0u && sc.triThreshold != 0u && __ballot(valid && r0.w != tmin0) == 0ull;
    if(share)
    {
      // the whole wave walks together: lanes without a valid ray have none of their own but help
      uint2* stk = ((uint2*)lds_stack) + threadIdx.x;
      traverse_wide8_share<false, ANYHIT, TM>(sc, valid, o, d, tmin0, tmax, stk, shareRes(shareLds), hit, tc, seed);
    }
    else if(valid)
      traverse_any<false, WIDE, TM>(sc, o, d, r0.w, tmax, ANYHIT, lds_stack, (int)threadIdx.x, 64, hit, tc, seed);
  }
  if(!inRange)
    return;
  const bool found = valid && hit.slot >= 0;
  if(ANYHIT)
  {
    occ[i] = found ? 1 : 0;
    return;
  }
  if(found)
  {
    const float4 c = sc.tris[(size_t)hit.slot * VKRT_TRI_QUADS + 2];  // (e2.z, gid | non-opaque flag, instance, primitive)
    const int inst = __float_as_int(c.z);
    hits[2 * i] = make_float4(hit.t, hit.u, hit.v, __int_as_float(inst));
    hits[2 * i + 1] = make_float4(c.w, __int_as_float(sc.instances[inst].primMesh), __int_as_float(__float_as_int(c.y) & 0x7fffffff),
                                  __uint_as_float(sc.triShade[hit.slot].w));
  }
  else
  {
    hits[2 * i] = make_float4(r1.w, 0.0f, 0.0f, __int_as_float(-1));
    hits[2 * i + 1] = make_float4(__int_as_float(-1), __int_as_float(-1), __int_as_float(-1), __int_as_float(-1));
  }
}

// n rays from `rays`; hits != NULL: closest hit, else occluded flags into occ.  Grids of at most 2^24 workgroups (2^30 rays) per launch.
// VKRT_RAY_OPAQUE on a scene built with the dissolve stage: the records carry its flag in their id words, so the walk masks it
// (VKRT_TM_MASKID) and ignores nothing.
hipError_t vkrt_launch_query(const DevQueryScene& sc, const float4* rays, uint64_t n, uint32_t seed, bool filter, bool opaque, float4* hits, int* occ,
                             hipStream_t stream)
{
  const size_t lds = (size_t)sc.stackCap * 64 * sizeof(int);
  const bool wide = sc.layout == 1u, anyHit = hits == nullptr;
  const int tm = (sc.watertight ? VKRT_TM_WATERTIGHT : 0) | (sc.dissolve ? (opaque ? VKRT_TM_MASKID : VKRT_TM_DISSOLVE) : 0) |
                 (filter ? VKRT_TM_FILTER : 0);
  const uint64_t chunk = 1ull << 30;
  for(uint64_t first = 0; first < n; first += chunk)
  {
    const uint64_t end = n - first < chunk ? n : first + chunk;
    const dim3 g((unsigned)((end - first + 63) / 64)), b(64);
#define VKRT_Q(A, W, TM) hipLaunchKernelGGL((k_query<A, W, TM>), g, b, lds, stream, sc, rays, first, end, seed, hits, occ)
#define VKRT_Q_MODES(A, W)                              \
  do {                                                  \
    switch(tm)                                          \
    {                                                   \
      case 0: VKRT_Q(A, W, 0); break;                   \
      case 1: VKRT_Q(A, W, 1); break;                   \
      case 2: VKRT_Q(A, W, 2); break;                   \
      case 3: VKRT_Q(A, W, 3); break;                   \
      case 4: VKRT_Q(A, W, 4); break;                   \
      case 5: VKRT_Q(A, W, 5); break;                   \
      case 8: VKRT_Q(A, W, 8); break;                   \
      case 9: VKRT_Q(A, W, 9); break;                   \
      case 10: VKRT_Q(A, W, 10); break;                 \
      case 11: VKRT_Q(A, W, 11); break;                 \
      case 12: VKRT_Q(A, W, 12); break;                 \
      default: VKRT_Q(A, W, 13); break;                 \
    }                                                   \
  } while(0)
    if(anyHit) { if(wide) VKRT_Q_MODES(true, true); else VKRT_Q_MODES(true, false); }
    else { if(wide) VKRT_Q_MODES(false, true); else VKRT_Q_MODES(false, false); }
#undef VKRT_Q_MODES
#undef VKRT_Q
    const hipError_t e = hipGetLastError();
    if(e != hipSuccess)
      return e;
  }
  return hipSuccess;
}

// One pass of the node-mask table over every node of a wide8 tree (layout: wide_node.h): byte s of node k = OR of the instance masks of
// the triangle records of leaf slot s, or of all eight bytes of the child node of internal slot s.  Reads its children's bytes of the
// previous pass (or of this one: either is a subset of the final value, and the last pass a node needs finds its children exact).
// Every index is checked against the arrays it reads, so that a node entry outside the tree cannot read out of bounds.
__global__ __launch_bounds__(256) void k_node_masks(const float4* __restrict__ nodes, const float4* __restrict__ tris, uint32_t triCount,
                                                    const DevInstance* __restrict__ inst, uint32_t instCount, uint32_t nodeCount, uint2* masks)
{
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if(k >= nodeCount)
    return;
  const float4 q0 = nodes[(size_t)k * VKRT_WNODE_QUADS], q1 = nodes[(size_t)k * VKRT_WNODE_QUADS + 1];
  const unsigned imask = __float_as_uint(q0.w) >> 24, childBase = __float_as_uint(q1.x), triBase = __float_as_uint(q1.y);
  unsigned out[2] = {0u, 0u};
  for(unsigned s = 0; s < 8u; s++)
  {
    const unsigned meta = (__float_as_uint(s < 4u ? q1.z : q1.w) >> (8u * (s & 3u))) & 0xffu;
    unsigned m = 0u;
    if((imask >> s) & 1u)
    {
      const unsigned c = childBase + (unsigned)__popc(imask & ((1u << s) - 1u));
      if(c < nodeCount)
      {
        const uint2 cm = masks[c];
        const unsigned x = cm.x | cm.y;
        m = (x | (x >> 8) | (x >> 16) | (x >> 24)) & 0xffu;
      }
    }
    else if(meta != 0u)
    {
      const unsigned firstSlot = triBase + (meta & 31u), cnt = (unsigned)__popc(meta >> 5);
      for(unsigned j = 0; j < cnt; j++)
      {
        const unsigned slot = firstSlot + j;
        if(slot >= triCount)
          break;
        const unsigned id = (unsigned)__float_as_int(tris[(size_t)slot * VKRT_TRI_QUADS + 2].z);
        if(id < instCount)
          m |= inst[id].vis & 0xffu;
      }
    }
    out[s >> 2] |= m << (8u * (s & 3u));
  }
  masks[k] = make_uint2(out[0], out[1]);
}

hipError_t vkrt_launch_node_masks(const DevScene& sc, uint32_t nodeCount, uint32_t instCount, uint32_t sweeps, uint2* masks, hipStream_t stream)
{
  if(nodeCount == 0u)
    return hipSuccess;
  for(uint32_t p = 0; p < sweeps; p++)
    hipLaunchKernelGGL(k_node_masks, dim3((nodeCount + 255u) / 256u), dim3(256), 0, stream, sc.nodes, sc.tris, sc.triCount, sc.instances, instCount,
                       nodeCount, masks);
  return hipGetLastError();
}
