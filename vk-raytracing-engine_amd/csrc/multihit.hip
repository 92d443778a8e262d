// multihit.hip -- vkrt_intersect_multi (include/vkrt.h): the first K candidates of every caller ray in the order (t, triangle id), the
// any-hit stage a caller without callbacks can have.  The walks are those of k_query (query.hip) taken lane by lane -- the BVH2 loop of
// traverse.h (query_common.h bvh2_lane_walk) and the immediate 8-wide loop of traverse_wide.h, with the same box tests, triangle tests
// and candidate filters; the invalid-ray rule, the records and the launch loop are those of query_common.h -- but the
// triangle step keeps a sorted per-lane list in LDS instead of one best hit, and the bound the box tests prune with is tmax until the
// list is full and the t of its last entry from then on.  The box tests admit tn <= bound, so a candidate with the t of the last entry
// and a smaller id is still reached.  Separate functions: the existing walks compile to what they were.
// Built with the flags of query.hip (csrc/Makefile): the same walks.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_scene.h"
#include "kernels.h"
#include "query_common.h"
#include "traverse.h"
#include "traverse_wide.h"
#include "wf_streams.h"  // wfLoad
#include "wide_node.h"

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
    if(L.admits(t, gid) && !query_rejects<TM>(sc, c, ccw) && !anyhit_ignores<TM>(sc, s, c.y, raySeed, VKRT_HOOK_UV(TM, u, v)))
      L.insert(t, gid, (int)s, u, v);
  }
}

// BVH2: the lane walk of query_common.h with the ray's box test against the list's bound and the triangle step above
template <int TM>
VKRT_DEV void traverse_multi(const DevScene& sc, f3 o, f3 d, float tmin, int* stk, int stride, MultiList& L, uint32_t raySeed)
{
  const f3 id = mk3(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
  TriRay<(TM & VKRT_TM_WATERTIGHT) != 0> tr;
  tr.set(d);
  const float4* __restrict__ tris = sc.tris;
  unsigned steps = sc.stepLimit;
  bvh2_lane_walk(
      sc, stk, stride, steps,
      [&](float4 q0, float4 q1, float4 q2, bool& h0, bool& h1, float& tn0, float& tn1) {
        h0 = box_test(o, id, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, tmin, L.boundT, tn0);
        h1 = box_test(o, id, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, tmin, L.boundT, tn1);
      },
      [&](unsigned s) { multi_test_triangle<TM>(sc, tr, o, d, tmin, s, tris, L, raySeed); });
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
// x 64 words).  Records behind a ray's count are miss records (query_common.h).
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
  const bool valid = queryRayValid(r0, r1) && (!(TM & VKRT_TM_FILTER) || sc.cullMask != 0u);
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
      query_write_hit(sc, out + 2 * j, __int_as_float(L.word(0, j)), __int_as_float(L.word(3, j)), __int_as_float(L.word(4, j)), L.word(2, j), L.word(1, j));
    else
      query_write_miss(out + 2 * j, r1.w);
  }
  if(counts)
    counts[i] = L.cnt;
}

static size_t multiLdsBytes(const DevQueryScene& sc, uint32_t maxHits) { return ((size_t)sc.stackCap + 5u * (size_t)maxHits) * 64 * sizeof(int); }

// n rays from `rays`, maxHits (1..VKRT_MULTIHIT_MAX, checked by the caller) records each into hits, counts may be NULL
hipError_t vkrt_launch_query_multi(const DevQueryScene& sc, const float4* rays, uint64_t n, uint32_t seed, bool filter, bool opaque, bool alpha,
                                   uint32_t maxHits, float4* hits, int* counts, hipStream_t stream)
{
  const size_t lds = multiLdsBytes(sc, maxHits);
  const bool wide = sc.layout == 1u;
  const int tm = query_tri_mode(sc, filter, opaque, alpha);
  return query_launch_chunks(n, [&](uint64_t first, uint64_t end, dim3 g) {
#define VKRT_QM(W, TM) hipLaunchKernelGGL((k_query_multi<W, TM>), g, dim3(64), lds, stream, sc, rays, first, end, seed, (int)maxHits, hits, counts)
#define VKRT_QM_TM(TM) do { if(wide) VKRT_QM(true, TM); else VKRT_QM(false, TM); } while(0)
    VKRT_QUERY_TM_SWITCH(tm, VKRT_QM_TM);
#undef VKRT_QM_TM
#undef VKRT_QM
  });
}
