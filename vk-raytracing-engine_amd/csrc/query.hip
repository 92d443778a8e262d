// query.hip -- batched ray queries on caller rays (vkrt_intersect / vkrt_occluded, include/vkrt.h): the traversal kernel of the
// wavefront pipeline (wf_traverse.hip) reading vkrt_ray records and writing vkrt_hit records instead of path-record streams.
// Built with the flags of wf_traverse.hip (csrc/Makefile) for the same reasons: the walks are the same code.
// What it shares with multihit.hip and closest.hip -- the invalid-ray rule, the records, the mode dispatch, the launch loop: query_common.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include "device_math.h"
#include "device_scene.h"
#include "kernels.h"
#include "query_common.h"
#include "traverse.h"
#include "traverse_wide.h"
#include "traverse_share.h"
#include "wf_streams.h"  // wfLoad
#include "wide_node.h"

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
    query_write_hit(sc, hits + 2 * i, hit.t, hit.u, hit.v, hit.slot, __float_as_int(sc.tris[(size_t)hit.slot * VKRT_TRI_QUADS + 2].y) & 0x7fffffff);
  else
    query_write_miss(hits + 2 * i, r1.w);
}

// n rays from `rays`; hits != NULL: closest hit, else occluded flags into occ.
hipError_t vkrt_launch_query(const DevQueryScene& sc, const float4* rays, uint64_t n, uint32_t seed, bool filter, bool opaque, bool alpha, float4* hits,
                             int* occ, hipStream_t stream)
{
  const size_t lds = (size_t)sc.stackCap * 64 * sizeof(int);
  const bool wide = sc.layout == 1u, anyHit = hits == nullptr;
  const int tm = query_tri_mode(sc, filter, opaque, alpha);
  return query_launch_chunks(n, [&](uint64_t first, uint64_t end, dim3 g) {
#define VKRT_Q(A, W, TM) hipLaunchKernelGGL((k_query<A, W, TM>), g, dim3(64), lds, stream, sc, rays, first, end, seed, hits, occ)
#define VKRT_Q_TM(TM)                                                          \
  do {                                                                         \
    if(anyHit) { if(wide) VKRT_Q(true, true, TM); else VKRT_Q(true, false, TM); } \
    else { if(wide) VKRT_Q(false, true, TM); else VKRT_Q(false, false, TM); }  \
  } while(0)
    VKRT_QUERY_TM_SWITCH(tm, VKRT_Q_TM);
#undef VKRT_Q_TM
#undef VKRT_Q
  });
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

// 256 (mode, cutoff) pairs per launch: 2 KiB of the 4 KiB of kernel arguments
#define VKRT_ALPHA_PER_LAUNCH 256u
struct MaterialAlphaBatch
{
  uint32_t first, count;
  uint2 rec[VKRT_ALPHA_PER_LAUNCH];
};
__global__ __launch_bounds__(VKRT_ALPHA_PER_LAUNCH) void k_material_alpha(const MaterialAlphaBatch b, DevMaterial* table)
{
  if(threadIdx.x < b.count)
  {
    DevMaterial& m = table[b.first + threadIdx.x];
    m.alphaMode = b.rec[threadIdx.x].x;
    m.alphaCutoff = __uint_as_float(b.rec[threadIdx.x].y);
  }
}

hipError_t vkrt_launch_material_alpha(DevMaterial* table, uint32_t first, uint32_t count, const uint2* src, hipStream_t stream)
{
  for(uint32_t done = 0; done < count; done += VKRT_ALPHA_PER_LAUNCH)
  {
    MaterialAlphaBatch b;
    b.first = first + done;
    b.count = count - done < VKRT_ALPHA_PER_LAUNCH ? count - done : VKRT_ALPHA_PER_LAUNCH;
    memcpy(b.rec, src + done, (size_t)b.count * sizeof(uint2));
    hipLaunchKernelGGL(k_material_alpha, dim3(1), dim3(VKRT_ALPHA_PER_LAUNCH), 0, stream, b, table);
  }
  return hipGetLastError();
}
