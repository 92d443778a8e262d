// query_common.h -- what the query kernels share (query.hip, multihit.hip, closest.hip, motion.hip; hybrid.hip takes the record writers
// for k_gbuffer's per-pixel hit records, nothing else includes it): the rule for a ray
// the walks never see, the vkrt_hit and miss record writers, the per-lane BVH2 walk, and on the host side the triangle mode of a ray
// query, its dispatch and the chunked launch loop.
// Deliberately NOT here: the wide8 lane loops (traverse_wide8_multi is the twin of w8_iterate on the hot path, cp_walk_wide8 has a group
// encoding of its own) and the closest-hit candidate rule inside traverse.h / traverse_wide.h, which the wavefront kernels share.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_scene.h"
#include "traverse.h"  // VKRT_TM_*

// A ray the walks never see: tmin < 0, tmin >= tmax (NaN bounds included), a zero direction, a NaN or infinite origin or direction component
VKRT_DEV bool queryRayValid(float4 r0, float4 r1)
{
  const bool finite = isfinite(r0.x) && isfinite(r0.y) && isfinite(r0.z) && isfinite(r1.x) && isfinite(r1.y) && isfinite(r1.z);
  const bool nonzero = r1.x != 0.0f || r1.y != 0.0f || r1.z != 0.0f;
  return finite && nonzero && r0.w >= 0.0f && r0.w < r1.w;
}

// The vkrt_hit of triangle record `slot` into out[0..1]: (t, u, v, instance) (primitive, prim_mesh, triangle, material) as int bits.
// gid: the record's flattened triangle id without the non-opaque flag.
VKRT_DEV void query_write_hit(const DevScene& sc, float4* __restrict__ out, float t, float u, float v, int slot, int gid)
{
  const float4 c = sc.tris[(size_t)slot * VKRT_TRI_QUADS + 2];  // (e2.z, gid | non-opaque flag, instance, primitive)
  const int inst = __float_as_int(c.z);
  out[0] = make_float4(t, u, v, __int_as_float(inst));
  out[1] = make_float4(c.w, __int_as_float(sc.instances[inst].primMesh), __int_as_float(gid), __uint_as_float(sc.triShade[slot].w));
}

// The miss record: t = the query's bound (tmax, radius), every id -1
VKRT_DEV void query_write_miss(float4* __restrict__ out, float bound)
{
  out[0] = make_float4(bound, 0.0f, 0.0f, __int_as_float(-1));
  out[1] = make_float4(__int_as_float(-1), __int_as_float(-1), __int_as_float(-1), __int_as_float(-1));
}

// BVH2, lane by lane: the loop of traverse.h (front to back, per-lane stack column in LDS, word k of the column at stk[k * stride]).
// nodeTest(q0, q1, q2, h0, h1, k0, k1): which of the node's two children are admitted (h0, h1) and their keys, the smaller the nearer;
// both admitted: the nearer is walked first, the other parked.  leaf(slot): once per triangle record of a leaf that is reached.
// steps: the caller's step budget; running out of it, or of stack, is a fault (VKRT_TRAV_FAULT).
template <class NodeTest, class Leaf>
VKRT_DEV void bvh2_lane_walk(const DevScene& sc, int* stk, int stride, unsigned& steps, NodeTest nodeTest, Leaf leaf)
{
  const float4* __restrict__ nodes = sc.nodes;
  const int cap = (int)sc.stackCap;
  int cur = sc.rootRef;
  int sp = 0;
  const auto pop = [&]() {
    if(sp == 0)
      cur = VKRT_TRAV_DONE;
    else
    {
      sp--;
      cur = stk[sp * stride];
    }
  };
  while(cur != VKRT_TRAV_DONE)
  {
    while(cur >= 0)
    {
      if(--steps == 0u)
      {
        VKRT_TRAV_FAULT(sc);
        return;
      }
      const float4 q0 = nodes[cur * VKRT_NODE_QUADS + 0];
      const float4 q1 = nodes[cur * VKRT_NODE_QUADS + 1];
      const float4 q2 = nodes[cur * VKRT_NODE_QUADS + 2];
      const float4 q3 = nodes[cur * VKRT_NODE_QUADS + 3];
      bool h0, h1;
      float k0, k1;
      nodeTest(q0, q1, q2, h0, h1, k0, k1);
      const int c0 = __float_as_int(q3.x), c1 = __float_as_int(q3.y);
      if(h0 && h1)
      {
        const bool swap = k1 < k0;
        const int nearC = swap ? c1 : c0, farC = swap ? c0 : c1;
        if(sp < cap)
        {
          stk[sp * stride] = farC;
          sp++;
        }
        else
          VKRT_TRAV_FAULT(sc);
        cur = nearC;
      }
      else if(h0)
        cur = c0;
      else if(h1)
        cur = c1;
      else
        pop();
    }
    if(cur != VKRT_TRAV_DONE)
    {
      if(--steps == 0u)
      {
        VKRT_TRAV_FAULT(sc);
        return;
      }
      const unsigned code = ~(unsigned)cur;
      const unsigned first = code >> 3, cnt = (code & 7u) + 1u;
      for(unsigned k = 0; k < cnt; k++)
        leaf(first + k);
      pop();
    }
  }
}

// The triangle mode of a ray query.  VKRT_RAY_OPAQUE on a scene built with the dissolve stage: the records carry its flag in their id
// words, so the walk masks it (VKRT_TM_MASKID) and ignores nothing.  alpha: the scene has a VKRT_ALPHA_MASK material right now; unless
// the call is opaque the walk then carries the alpha-test stage, always together with the filter (whose defaults reject nothing), which
// keeps the stage to four more modes instead of eight.
inline int query_tri_mode(const DevScene& sc, bool filter, bool opaque, bool alpha)
{
  const bool stage = alpha && !opaque;
  return (sc.watertight ? VKRT_TM_WATERTIGHT : 0) | (sc.dissolve ? (opaque ? VKRT_TM_MASKID : VKRT_TM_DISSOLVE) : 0) |
         (filter || stage ? VKRT_TM_FILTER : 0) | (stage ? VKRT_TM_ALPHA : 0);
}

// X(TM) for the triangle mode tm, a compile-time constant there: the sixteen values query_tri_mode can give
#define VKRT_QUERY_TM_SWITCH(tm, X) \
  switch(tm)                        \
  {                                 \
    case 0: X(0); break;            \
    case 1: X(1); break;            \
    case 2: X(2); break;            \
    case 3: X(3); break;            \
    case 4: X(4); break;            \
    case 5: X(5); break;            \
    case 8: X(8); break;            \
    case 9: X(9); break;            \
    case 10: X(10); break;          \
    case 11: X(11); break;          \
    case 12: X(12); break;          \
    case 13: X(13); break;          \
    case 24: X(24); break;          \
    case 25: X(25); break;          \
    case 26: X(26); break;          \
    default: X(27); break; /* case 27 */ \
  }

// n items, one thread each, one wave per workgroup, in launches of at most 2^24 workgroups (2^30 items): launch(first, end, grid) starts
// the kernel on items [first, end).  The first launch error ends the loop.
template <class Launch>
inline hipError_t query_launch_chunks(uint64_t n, Launch launch)
{
  const uint64_t chunk = 1ull << 30;
  for(uint64_t first = 0; first < n; first += chunk)
  {
    const uint64_t end = n - first < chunk ? n : first + chunk;
    launch(first, end, dim3((unsigned)((end - first + 63) / 64)));
    const hipError_t e = hipGetLastError();
    if(e != hipSuccess)
      return e;
  }
  return hipSuccess;
}
