// multihit.hip -- vkrt_intersect_multi (include/vkrt.h): the first K candidates of every caller ray in the order (t, triangle id), the
// any-hit stage a caller without callbacks can have.  The walks are those of k_query (query.hip) taken lane by lane -- the BVH2 loop of
// traverse.h and the immediate 8-wide loop of traverse_wide.h, with the same box tests, triangle tests and candidate filters -- but the
// triangle step keeps a sorted per-lane list in LDS instead of one best hit, and the bound the box tests prune with is tmax until the
// list is full and the t of its last entry from then on.  The box tests admit tn <= bound, so a candidate with the t of the last entry
// and a smaller id is still reached.  Separate functions: the existing walks compile to what they were.
// Built with the flags of query.hip (csrc/Makefile): the same walks.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_scene.h"
#include "kernels.h"
#include "traverse.h"
#include "traverse_wide.h"
#include "wf_streams.h"  // wfLoad
#include "wide_node.h"

// A ray the walks never see (query.hip queryRayValid: the same rule)
VKRT_DEV bool multiRayValid(float4 r0, float4 r1)
{
  const bool finite = isfinite(r0.x) && isfinite(r0.y) && isfinite(r0.z) && isfinite(r1.x) && isfinite(r1.y) && isfinite(r1.z);
  const bool nonzero = r1.x != 0.0f || r1.y != 0.0f || r1.z != 0.0f;
  return finite && nonzero && r0.w >= 0.0f && r0.w < r1.w;
}

// The list of one lane: up to K entries (t, gid, slot, u, v) sorted by (t, gid), in five planes of K x 64 words behind the wave's stack
// columns; word j of plane f of lane l sits at (f * K + j) * 64 + l, so the 64 lanes of an access fall into 64 consecutive words (no
// bank conflict).  (boundT, boundGid) is the key a candidate has to be smaller than: (tmax, -1) while the list has room -- which is
// t < tmax, the closest-hit walks' start -- and the key of entry K - 1 once it is full.
struct MultiList
{
  int* p;  // this lane's word of plane 0, entry 0
  int K, cnt;
  float boundT;
  int boundGid;

  VKRT_DEV int& word(int f, int j) const { return p[(f * K + j) * 64]; }
  VKRT_DEV void begin(int* lanePtr, int k, float tmax)
  {
    p = lanePtr; K = k; cnt = 0; boundT = tmax; boundGid = -1;
  }
  VKRT_DEV bool admits(float t, int gid) const { return t < boundT || (t == boundT && gid < boundGid); }
  // an admitted candidate: sorted insertion; a key already in the list is a second reference to the same triangle record (pre-splitting:
  // same record, same ray, same (t, u, v)) and is dropped
  VKRT_DEV void insert(float t, int gid, int slot, float u, float v)
  {
    int j = cnt;
    while(j > 0)
    {
      const float tj = __int_as_float(word(0, j - 1));
      const int gj = word(1, j - 1);
      if(tj < t || (tj == t && gj <= gid))
      {
        if(tj == t && gj == gid)
          return;
        break;
      }
      j--;
    }
    const int last = cnt < K ? cnt : K - 1;  // where the entry pushed up furthest lands (a full list drops its last entry)
    for(int k = last; k > j; k--)
    {
#pragma unroll
      for(int f = 0; f < 5; f++)
        word(f, k) = word(f, k - 1);
    }
    word(0, j) = __float_as_int(t);
    word(1, j) = gid;
    word(2, j) = slot;
    word(3, j) = __float_as_int(u);
    word(4, j) = __float_as_int(v);
    cnt = last + 1;
    if(cnt == K)
    {
      boundT = __int_as_float(word(0, K - 1));
      boundGid = word(1, K - 1);
    }
  }
};

// one triangle record against the ray: the candidate rule of the closest-hit walks with the list's bound in the place of the best hit
template <int TM, class TR>
VKRT_DEV void multi_test_triangle(const DevScene& sc, const TR& tr, f3 o, f3 d, float tmin, unsigned s, const float4* __restrict__ tris, MultiList& L,
                                  uint32_t raySeed)
{
  const float4* __restrict__ tp = tris + (size_t)s * VKRT_TRI_QUADS;
  const float4 a = tp[0];
  const float4 b = tp[1];
  const float4 c = tp[2];
  float t, u, v;
  bool ccw;
  if(tr.hit(o, d, a, b, c, t, u, v, ccw) && t > tmin)
  {
    const int gid = tri_gid<TM>(c.y);
    if(L.admits(t, gid) && !query_rejects<TM>(sc, c, ccw) && !anyhit_ignores<TM>(sc, s, c.y, raySeed))
      L.insert(t, gid, (int)s, u, v);
  }
}

// BVH2: the loop of traverse.h (front to back, per-lane stack column in LDS)
template <int TM>
VKRT_DEV void traverse_multi(const DevScene& sc, f3 o, f3 d, float tmin, int* stk, int stride, MultiList& L, uint32_t raySeed)
{
  const f3 id = mk3(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
  TriRay<(TM & VKRT_TM_WATERTIGHT) != 0> tr;
  tr.set(d);
  const float4* __restrict__ nodes = sc.nodes;
  const float4* __restrict__ tris = sc.tris;
  const int cap = (int)sc.stackCap;
  int cur = sc.rootRef;
  int sp = 0;
  unsigned steps = sc.stepLimit;
  while(cur != VKRT_TRAV_DONE)
  {
    while(cur >= 0)
    {
      if(--steps == 0u)
      {
        VKRT_TRAV_FAULT(sc);
        cur = VKRT_TRAV_DONE;
        break;
      }
      const float4 q0 = nodes[cur * VKRT_NODE_QUADS + 0];
      const float4 q1 = nodes[cur * VKRT_NODE_QUADS + 1];
      const float4 q2 = nodes[cur * VKRT_NODE_QUADS + 2];
      const float4 q3 = nodes[cur * VKRT_NODE_QUADS + 3];
      float tn0, tn1;
      const bool h0 = box_test(o, id, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, tmin, L.boundT, tn0);
      const bool h1 = box_test(o, id, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, tmin, L.boundT, tn1);
      const int c0 = __float_as_int(q3.x), c1 = __float_as_int(q3.y);
      if(h0 && h1)
      {
        const bool swap = tn1 < tn0;
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
      {
        if(sp == 0)
          cur = VKRT_TRAV_DONE;
        else
        {
          sp--;
          cur = stk[sp * stride];
        }
      }
    }
    if(cur != VKRT_TRAV_DONE)
    {
      if(--steps == 0u)
      {
        VKRT_TRAV_FAULT(sc);
        break;
      }
      const unsigned code = ~(unsigned)cur;
      const unsigned first = code >> 3, cnt = (code & 7u) + 1u;
      for(unsigned k = 0; k < cnt; k++)
        multi_test_triangle<TM>(sc, tr, o, d, tmin, first + k, tris, L, raySeed);
      if(sp == 0)
        cur = VKRT_TRAV_DONE;
      else
      {
        sp--;
        cur = stk[sp * stride];
      }
    }
  }
}

// wide8: the immediate loop of traverse_wide.h (w8_begin / w8_iterate): nearest pending child of the group, its eight children
// against the list's bound, the triangles the ray's boxes touched, then pop
template <int TM>
VKRT_DEV void traverse_wide8_multi(const DevScene& sc, f3 o, f3 d, float tmin, uint2* stk, int stride, MultiList& L, uint32_t raySeed)
{
  TriRay<(TM & VKRT_TM_WATERTIGHT) != 0> tr;
  tr.set(d);
  const float4* __restrict__ nodes = sc.nodes;
  const float4* __restrict__ tris = sc.tris;
  const int cap = (int)(sc.stackCap >> 1);
  const f3 id = mk3(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
  const bool px = !(id.x < 0.0f), py = !(id.y < 0.0f), pz = !(id.z < 0.0f);
  const unsigned octinv = (px ? 1u : 0u) | (py ? 2u : 0u) | (pz ? 4u : 0u);
  uint2 G = make_uint2(0u, sc.rootRef == VKRT_TRAV_DONE ? 0u : 0x80000000u);
  int sp = 0;
  unsigned steps = sc.stepLimit;
  TravCount tc;
  while(G.y & 0xff000000u)
  {
    const unsigned bitIdx = 31u - (unsigned)__clz((int)G.y);
    const unsigned slot = (bitIdx - 24u) ^ octinv;
    const unsigned child = G.x + (unsigned)__popc(G.y & 0xffu & ((1u << slot) - 1u));
    G.y &= ~(1u << bitIdx);
    if(G.y & 0xff000000u)
    {
      if(sp < cap)
      {
        stk[sp * stride] = G;
        sp++;
      }
      else
        VKRT_TRAV_FAULT(sc);
    }
    if(--steps == 0u)
    {
      VKRT_TRAV_FAULT(sc);
      return;
    }
    uint2 T;
    w8_test_children<false, (TM & VKRT_TM_FILTER) != 0>(nodes, child, o, id, octinv * 0x01010101u, px, py, pz, tmin, L.boundT, G, T, tc,
                                                        query_node_masks<TM>(sc), query_cull_mask<TM>(sc));
    while(T.y != 0u)
    {
      const unsigned i = (unsigned)__ffs((int)T.y) - 1u;
      T.y &= T.y - 1u;
      if(--steps == 0u)
      {
        VKRT_TRAV_FAULT(sc);
        return;
      }
      multi_test_triangle<TM>(sc, tr, o, d, tmin, T.x + i, tris, L, raySeed);
    }
    if((G.y & 0xff000000u) == 0u)
    {
      if(sp == 0)
        return;
      sp--;
      G = stk[sp * stride];
    }
  }
}

// One thread per ray, one wave per workgroup.  rays: 2 float4 per ray as in k_query; hits: maxHits records of 2 float4 per ray, ray-major;
// counts: one int per ray or NULL.  Rays [first, n).  Dynamic LDS: the stack columns (sc.stackCap x 64 words), then the lists (5 x maxHits
// x 64 words).  Records behind a ray's count are the miss record of k_query.
template <bool WIDE, int TM>
__global__ __launch_bounds__(64)
void k_query_multi(const DevQueryScene sc, const float4* __restrict__ rays, uint64_t first, uint64_t n, uint32_t seed, int maxHits,
                   float4* __restrict__ hits, int* __restrict__ counts)
{
  extern __shared__ int lds_multi[];
  const uint64_t i = first + (uint64_t)blockIdx.x * 64u + threadIdx.x;
  if(i >= n)
    return;  // (no barrier and no cross-lane operation below: the walks are lane by lane)
  const float4 r0 = wfLoad(rays + 2 * i), r1 = wfLoad(rays + 2 * i + 1);
  const bool valid = multiRayValid(r0, r1) && (!(TM & VKRT_TM_FILTER) || sc.cullMask != 0u);
  MultiList L;
  L.begin(lds_multi + (size_t)sc.stackCap * 64 + threadIdx.x, maxHits, r1.w);
  if(valid)
  {
    const f3 o = mk3(r0.x, r0.y, r0.z), d = mk3(r1.x, r1.y, r1.z);
    if(WIDE)
      traverse_wide8_multi<TM>(sc, o, d, r0.w, ((uint2*)lds_multi) + threadIdx.x, 64, L, seed);
    else
      traverse_multi<TM>(sc, o, d, r0.w, lds_multi + threadIdx.x, 64, L, seed);
  }
  float4* __restrict__ out = hits + 2 * (i * (uint64_t)maxHits);
  for(int j = 0; j < maxHits; j++)
  {
    if(j < L.cnt)
    {
      const int slot = L.word(2, j);
      const float4 c = sc.tris[(size_t)slot * VKRT_TRI_QUADS + 2];  // (e2.z, gid | non-opaque flag, instance, primitive)
      const int inst = __float_as_int(c.z);
      out[2 * j] = make_float4(__int_as_float(L.word(0, j)), __int_as_float(L.word(3, j)), __int_as_float(L.word(4, j)), __int_as_float(inst));
      out[2 * j + 1] = make_float4(c.w, __int_as_float(sc.instances[inst].primMesh), __int_as_float(L.word(1, j)),
                                   __uint_as_float(sc.triShade[slot].w));
    }
    else
    {
      out[2 * j] = make_float4(r1.w, 0.0f, 0.0f, __int_as_float(-1));
      out[2 * j + 1] = make_float4(__int_as_float(-1), __int_as_float(-1), __int_as_float(-1), __int_as_float(-1));
    }
  }
  if(counts)
    counts[i] = L.cnt;
}

static size_t multiLdsBytes(const DevQueryScene& sc, uint32_t maxHits) { return ((size_t)sc.stackCap + 5u * (size_t)maxHits) * 64 * sizeof(int); }

// n rays from `rays`, maxHits (1..VKRT_MULTIHIT_MAX, checked by the caller) records each into hits, counts may be NULL.  Mode dispatch and
// chunking as vkrt_launch_query: grids of at most 2^24 workgroups (2^30 rays) per launch.
hipError_t vkrt_launch_query_multi(const DevQueryScene& sc, const float4* rays, uint64_t n, uint32_t seed, bool filter, bool opaque, uint32_t maxHits,
                                   float4* hits, int* counts, hipStream_t stream)
{
  const size_t lds = multiLdsBytes(sc, maxHits);
  const bool wide = sc.layout == 1u;
  const int tm = (sc.watertight ? VKRT_TM_WATERTIGHT : 0) | (sc.dissolve ? (opaque ? VKRT_TM_MASKID : VKRT_TM_DISSOLVE) : 0) |
                 (filter ? VKRT_TM_FILTER : 0);
  const uint64_t chunk = 1ull << 30;
  for(uint64_t first = 0; first < n; first += chunk)
  {
    const uint64_t end = n - first < chunk ? n : first + chunk;
    const dim3 g((unsigned)((end - first + 63) / 64)), b(64);
#define VKRT_QM(W, TM) hipLaunchKernelGGL((k_query_multi<W, TM>), g, b, lds, stream, sc, rays, first, end, seed, (int)maxHits, hits, counts)
#define VKRT_QM_MODES(W)                             \
  do {                                               \
    switch(tm)                                       \
    {                                                \
      case 0: VKRT_QM(W, 0); break;                  \
      case 1: VKRT_QM(W, 1); break;                  \
      case 2: VKRT_QM(W, 2); break;                  \
      case 3: VKRT_QM(W, 3); break;                  \
      case 4: VKRT_QM(W, 4); break;                  \
      case 5: VKRT_QM(W, 5); break;                  \
      case 8: VKRT_QM(W, 8); break;                  \
      case 9: VKRT_QM(W, 9); break;                  \
      case 10: VKRT_QM(W, 10); break;                \
      case 11: VKRT_QM(W, 11); break;                \
      case 12: VKRT_QM(W, 12); break;                \
      default: VKRT_QM(W, 13); break;                \
    }                                                \
  } while(0)
    if(wide) VKRT_QM_MODES(true); else VKRT_QM_MODES(false);
#undef VKRT_QM_MODES
#undef VKRT_QM
    const hipError_t e = hipGetLastError();
    if(e != hipSuccess)
      return e;
  }
  return hipSuccess;
}
