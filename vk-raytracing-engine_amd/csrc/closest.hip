// closest.hip -- vkrt_closest_point (include/vkrt.h): per query point the nearest point of the scene's surface within a radius, as a
// vkrt_hit.  A distance-ordered walk of the world-space BVH -- both layouts -- with a lower bound of the squared point/box distance in
// the place of the ray/box test and Ericson's point/triangle function, evaluated in binary64, in the place of the ray/triangle test.
// The result is the smallest key (dist2, flattened triangle id) over the candidates, a property of the triangle set: the walk prunes a
// box only when its bound EXCEEDS the best dist2 so far, so an equally near triangle with a smaller id is still reached.
// Functions of its own, lane by lane: the ray walks (traverse.h, traverse_wide.h) are not touched.  The BVH2 loop, the records and the
// launch loop are those of query_common.h.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_scene.h"
#include "kernels.h"
#include "query_common.h"
#include "wf_streams.h"  // wfLoad
#include "wide_node.h"

// Margins of the box bound.  A bound must never exceed the binary64 dist2 of a triangle under the box.  The triangle the function sees is
// (p0, p0 + e1, p0 + e2) in exact arithmetic, while the builders boxed the binary32 sums p0 + e1 (or, watertight, the exact p1 whose
// binary32 difference p1 - p0 the function uses): a vertex can lie outside its box by half an ulp of its coordinate, 2^-24 |x|.  The
// decoded plane of a wide node is one fmaf away from the exact grid plane, another 2^-24 |x|.  So every per-axis gap is shortened by
// VKRT_CP_PAD_ABS x the largest |coordinate| of the box on that axis (2^-21: four times the sum of the two), and the binary32 rounding
// of the gap, its square and the two additions (2^-24 relative each) is covered by the relative factors; the constant term keeps a sum
// that rounded up into the subnormal range below the exact value.
#define VKRT_CP_PAD_ABS 4.76837158203125e-07f  // 2^-21
#define VKRT_CP_PAD_REL 0.99999904632568359375f  // 1 - 2^-20
#define VKRT_CP_PAD_MIN 1.17549435e-38f

// the walk's state of one query
struct CpState
{
  float qx, qy, qz;
  double d2;     // best key so far: (d2, gid); starts as (radius^2, -1), which admits dist2 < radius^2 only
  float d2Up;    // d2 rounded up to binary32: a box whose bound exceeds it holds no candidate
  float u, v;
  int gid, slot;
  unsigned steps;
  unsigned nodes, tris;  // COUNT
};

VKRT_DEV float cp_round_up(double x)
{
  const float f = (float)x;
  return ((double)f < x) ? __uint_as_float(__float_as_uint(f) + 1u) : f;  // (f >= 0 and finite here: the next binary32 up)
}

VKRT_DEV double cp_dot(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

// per-axis gap between the point and [lo, hi], shortened by the margins (>= 0)
VKRT_DEV float cp_gap(float q, float lo, float hi, float pad)
{
  const float g = fmaxf(fmaxf(lo - q, q - hi), 0.0f);
  return fmaxf(fmaf(g, VKRT_CP_PAD_REL, -pad), 0.0f);
}
VKRT_DEV float cp_bound(float gx, float gy, float gz)
{
  const float s = (gx * gx + gy * gy) + gz * gz;
  return fmaxf(fmaf(s, VKRT_CP_PAD_REL, -VKRT_CP_PAD_MIN), 0.0f);
}

// One triangle record against the query: the point/triangle function of include/vkrt.h (Ericson, Real-Time Collision Detection 5.1.5)
// in binary64 on the record's binary32 values, source order, no contraction (csrc/Makefile: -ffp-contract=off).
template <bool FILTER, bool COUNT>
VKRT_DEV void cp_test_triangle(const DevQueryScene& sc, CpState& S, unsigned s)
{
  const float4* __restrict__ tp = sc.tris + (size_t)s * VKRT_TRI_QUADS;
  const float4 a = tp[0];
  const float4 b = tp[1];
  const float4 c = tp[2];
  if(COUNT)
    S.tris++;
  if(FILTER)
  {
    if((sc.instances[__float_as_int(c.z)].vis & sc.cullMask) == 0u)
      return;
  }
  float e1x = a.w, e1y = b.x, e1z = b.y, e2x = b.z, e2y = b.w, e2z = c.x;
  if(sc.watertight)  // launch-uniform: the record holds (p0, p1, p2); the edges in binary32 are the bits of the default record
  {
    e1x = e1x - a.x; e1y = e1y - a.y; e1z = e1z - a.z;
    e2x = e2x - a.x; e2y = e2y - a.y; e2z = e2z - a.z;
  }
  const double ax = e1x, ay = e1y, az = e1z, bx = e2x, by = e2y, bz = e2z;
  const double apx = (double)S.qx - (double)a.x, apy = (double)S.qy - (double)a.y, apz = (double)S.qz - (double)a.z;
  const double d1 = cp_dot(ax, ay, az, apx, apy, apz), d2 = cp_dot(bx, by, bz, apx, apy, apz);
  const double bpx = apx - ax, bpy = apy - ay, bpz = apz - az;
  const double d3 = cp_dot(ax, ay, az, bpx, bpy, bpz), d4 = cp_dot(bx, by, bz, bpx, bpy, bpz);
  const double cpx = apx - bx, cpy = apy - by, cpz = apz - bz;
  const double d5 = cp_dot(ax, ay, az, cpx, cpy, cpz), d6 = cp_dot(bx, by, bz, cpx, cpy, cpz);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  double u, v;
  if(d1 <= 0.0 && d2 <= 0.0)
  {
    u = 0.0; v = 0.0;
  }
  else if(d3 >= 0.0 && d4 <= d3)
  {
    u = 1.0; v = 0.0;
  }
  else if(vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0)
  {
    u = d1 / (d1 - d3); v = 0.0;
  }
  else if(d6 >= 0.0 && d5 <= d6)
  {
    u = 0.0; v = 1.0;
  }
  else if(vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0)
  {
    u = 0.0; v = d2 / (d2 - d6);
  }
  else if(va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0)
  {
    const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    u = 1.0 - w; v = w;
  }
  else
  {
    const double den = 1.0 / ((va + vb) + vc);
    u = vb * den; v = vc * den;
  }
  const double dx = (apx - u * ax) - v * bx, dy = (apy - u * ay) - v * by, dz = (apz - u * az) - v * bz;
  const double dist2 = cp_dot(dx, dy, dz, dx, dy, dz);
  const int gid = __float_as_int(c.y) & 0x7fffffff;  // (bit 31: the dissolve flag of a scene built for that stage; a point has no any-hit stage)
  if(dist2 < S.d2 || (dist2 == S.d2 && gid < S.gid))  // (a NaN dist2 is no candidate)
  {
    S.d2 = dist2; S.d2Up = cp_round_up(dist2);
    S.u = (float)u; S.v = (float)v;
    S.gid = gid; S.slot = (int)s;
  }
}

// BVH2: the lane walk of query_common.h, near child = smaller bound
template <bool FILTER, bool COUNT>
VKRT_DEV void cp_walk_bvh2(const DevQueryScene& sc, CpState& S, int* stk, int stride)
{
  bvh2_lane_walk(
      sc, stk, stride, S.steps,
      [&](float4 q0, float4 q1, float4 q2, bool& h0, bool& h1, float& b0, float& b1) {
        if(COUNT)
          S.nodes++;
        b0 = cp_bound(cp_gap(S.qx, q0.x, q0.w, VKRT_CP_PAD_ABS * fmaxf(fabsf(q0.x), fabsf(q0.w))),
                      cp_gap(S.qy, q0.y, q1.x, VKRT_CP_PAD_ABS * fmaxf(fabsf(q0.y), fabsf(q1.x))),
                      cp_gap(S.qz, q0.z, q1.y, VKRT_CP_PAD_ABS * fmaxf(fabsf(q0.z), fabsf(q1.y))));
        b1 = cp_bound(cp_gap(S.qx, q1.z, q2.y, VKRT_CP_PAD_ABS * fmaxf(fabsf(q1.z), fabsf(q2.y))),
                      cp_gap(S.qy, q1.w, q2.z, VKRT_CP_PAD_ABS * fmaxf(fabsf(q1.w), fabsf(q2.z))),
                      cp_gap(S.qz, q2.x, q2.w, VKRT_CP_PAD_ABS * fmaxf(fabsf(q2.x), fabsf(q2.w))));
        h0 = !(b0 > S.d2Up);
        h1 = !(b1 > S.d2Up);
      },
      [&](unsigned s) { cp_test_triangle<FILTER, COUNT>(sc, S, s); });
}

#define VKRT_CP_SWAP(i, j)                     \
  do {                                         \
    const unsigned lo_ = min(k[i], k[j]);      \
    k[j] = max(k[i], k[j]);                    \
    k[i] = lo_;                                \
  } while(0)

// wide8.  A group G = (child base of a node, its pending internal children): G.y bits 0..23 = their ranks among the node's internal
// children (child = base + rank), 3 bits each, nearest first; bits 24..27 = how many.  As in traverse_wide.h the walk takes the nearest
// pending child of the current group, parks the rest of the group on the lane's stack column -- one entry per level, so the depth the
// build sized the column for is enough -- and tests the child's eight slots.  A parked child carries no bound: one that the best
// distance has overtaken since costs its node load and nothing more.
// Per node: the eight slot boxes decoded from the 8-bit planes (wide_node.h), a bound per slot, and one key per slot
//   leaf: bound bits & ~7 | slot      internal: the same | bit 31      empty, masked out (FILTER): 0xFFFFFFFF
// (a bound is >= 0, so its bits order as unsigned; clearing three bits only lowers it).  A 19-exchange network sorts the keys: leaves
// nearest first, then internal children nearest first.  The leaves' triangles are tested in that order, and the internal children that
// the best distance THEN still admits form the new group.
template <bool FILTER, bool COUNT>
VKRT_DEV void cp_walk_wide8(const DevQueryScene& sc, CpState& S, uint2* stk, int stride)
{
  const float4* __restrict__ nodes = sc.nodes;
  const int cap = (int)(sc.stackCap >> 1);
  uint2 G = make_uint2(0u, sc.rootRef == VKRT_TRAV_DONE ? 0u : 0x01000000u);
  int sp = 0;
  while((G.y >> 24) != 0u)
  {
    const unsigned child = G.x + (G.y & 7u);
    G.y = ((G.y & 0x00ffffffu) >> 3) | (((G.y >> 24) - 1u) << 24);
    if((G.y >> 24) != 0u)
    {
      if(sp < cap)
      {
        stk[sp * stride] = G;
        sp++;
      }
      else
        VKRT_TRAV_FAULT(sc);
    }
    if(--S.steps == 0u)
    {
      VKRT_TRAV_FAULT(sc);
      return;
    }
    const float4* __restrict__ np = nodes + (size_t)child * VKRT_WNODE_QUADS;
    const float4 q0 = np[0], q1 = np[1], q2 = np[2], q3 = np[3], q4 = np[4];
    uint2 slotMasks = make_uint2(0xffffffffu, 0xffffffffu);
    if(FILTER)
      slotMasks = sc.nodeMasks[child];
    if(COUNT)
      S.nodes++;
    const unsigned ew = __float_as_uint(q0.w);
    const unsigned imask = ew >> 24;
    const float sx = __uint_as_float((ew & 0xffu) << 23), sy = __uint_as_float(((ew >> 8) & 0xffu) << 23),
                sz = __uint_as_float(((ew >> 16) & 0xffu) << 23);
    // (the pad of the node's own extent serves its eight slots: every plane lies between the origin and origin + QMAX cells)
    const float padx = VKRT_CP_PAD_ABS * fmaxf(fabsf(q0.x), fabsf(fmaf((float)VKRT_WNODE_QMAX, sx, q0.x)));
    const float pady = VKRT_CP_PAD_ABS * fmaxf(fabsf(q0.y), fabsf(fmaf((float)VKRT_WNODE_QMAX, sy, q0.y)));
    const float padz = VKRT_CP_PAD_ABS * fmaxf(fabsf(q0.z), fabsf(fmaf((float)VKRT_WNODE_QMAX, sz, q0.z)));
    const unsigned lx[2] = {__float_as_uint(q2.x), __float_as_uint(q2.y)}, ly[2] = {__float_as_uint(q2.z), __float_as_uint(q2.w)};
    const unsigned lz[2] = {__float_as_uint(q3.x), __float_as_uint(q3.y)}, hx[2] = {__float_as_uint(q3.z), __float_as_uint(q3.w)};
    const unsigned hy[2] = {__float_as_uint(q4.x), __float_as_uint(q4.y)}, hz[2] = {__float_as_uint(q4.z), __float_as_uint(q4.w)};
    const unsigned meta[2] = {__float_as_uint(q1.z), __float_as_uint(q1.w)};
    const unsigned smask[2] = {slotMasks.x, slotMasks.y};
    unsigned k[8];
#pragma unroll
    for(int s = 0; s < 8; s++)
    {
      const int w = s >> 2, sh = 8 * (s & 3);
      const float gx = cp_gap(S.qx, fmaf((float)((lx[w] >> sh) & 0xffu), sx, q0.x), fmaf((float)((hx[w] >> sh) & 0xffu), sx, q0.x), padx);
      const float gy = cp_gap(S.qy, fmaf((float)((ly[w] >> sh) & 0xffu), sy, q0.y), fmaf((float)((hy[w] >> sh) & 0xffu), sy, q0.y), pady);
      const float gz = cp_gap(S.qz, fmaf((float)((lz[w] >> sh) & 0xffu), sz, q0.z), fmaf((float)((hz[w] >> sh) & 0xffu), sz, q0.z), padz);
      const unsigned key = (__float_as_uint(cp_bound(gx, gy, gz)) & ~7u) | (unsigned)s | (((imask >> s) & 1u) << 31);
      bool live = ((meta[w] >> sh) & 0xffu) != 0u;
      if(FILTER)
        live = live && (((smask[w] >> sh) & sc.cullMask) != 0u);
      k[s] = live ? key : 0xffffffffu;
    }
    VKRT_CP_SWAP(0, 2); VKRT_CP_SWAP(1, 3); VKRT_CP_SWAP(4, 6); VKRT_CP_SWAP(5, 7);
    VKRT_CP_SWAP(0, 4); VKRT_CP_SWAP(1, 5); VKRT_CP_SWAP(2, 6); VKRT_CP_SWAP(3, 7);
    VKRT_CP_SWAP(0, 1); VKRT_CP_SWAP(2, 3); VKRT_CP_SWAP(4, 5); VKRT_CP_SWAP(6, 7);
    VKRT_CP_SWAP(2, 4); VKRT_CP_SWAP(3, 5);
    VKRT_CP_SWAP(1, 4); VKRT_CP_SWAP(3, 6);
    VKRT_CP_SWAP(1, 2); VKRT_CP_SWAP(3, 4); VKRT_CP_SWAP(5, 6);
    const unsigned triBase = __float_as_uint(q1.y);
    G = make_uint2(__float_as_uint(q1.x), 0u);
    for(;;)
    {
      const unsigned key = k[0];
#pragma unroll
      for(int j = 0; j < 7; j++)
        k[j] = k[j + 1];
      k[7] = 0xffffffffu;
      if(key == 0xffffffffu)
        break;
      const bool inner = (key >> 31) != 0u;
      if(__uint_as_float(key & 0x7ffffff8u) > S.d2Up)
      {
        if(inner)
          break;  // (sorted: every internal child behind it is as far or farther)
        continue;
      }
      const unsigned s = key & 7u;
      if(inner)
      {
        const unsigned cnt = G.y >> 24;
        G.y = (G.y + 0x01000000u) | ((unsigned)__popc(imask & ((1u << s) - 1u)) << (3u * cnt));
      }
      else
      {
        const unsigned m = ((s < 4u ? meta[0] : meta[1]) >> (8u * (s & 3u))) & 0xffu;
        const unsigned firstSlot = triBase + (m & 31u), cnt = (unsigned)__popc(m >> 5);
        for(unsigned j = 0; j < cnt; j++)
        {
          if(--S.steps == 0u)
          {
            VKRT_TRAV_FAULT(sc);
            return;
          }
          cp_test_triangle<FILTER, COUNT>(sc, S, firstSlot + j);
        }
      }
    }
    if((G.y >> 24) == 0u)
    {
      if(sp == 0)
        return;
      sp--;
      G = stk[sp * stride];
    }
  }
}
#undef VKRT_CP_SWAP

// One thread per query, one wave per workgroup.  queries: one float4 each (point, radius); hits: 2 float4 each (vkrt_hit, query_common.h
// query_write_hit, t = the distance).  Queries [first, n).  Dynamic LDS: the stack columns (sc.stackCap x 64 words).  work (COUNT): two totals, nodes
// visited and triangle records tested.
template <bool WIDE, bool FILTER, bool COUNT>
__global__ __launch_bounds__(64)
void k_closest_point(const DevQueryScene sc, const float4* __restrict__ queries, uint64_t first, uint64_t n, float4* __restrict__ hits,
                     unsigned long long* __restrict__ work)
{
  extern __shared__ int lds_closest[];
  const uint64_t i = first + (uint64_t)blockIdx.x * 64u + threadIdx.x;
  if(i >= n)
    return;  // (no barrier and no cross-lane operation below: the walks are lane by lane)
  const float4 q = wfLoad(queries + i);
  // a query the walks never see: a non-finite point, a radius that is NaN, negative or zero, a cull mask of 0
  const bool valid = isfinite(q.x) && isfinite(q.y) && isfinite(q.z) && q.w > 0.0f && (!FILTER || sc.cullMask != 0u);
  CpState S;
  S.qx = q.x; S.qy = q.y; S.qz = q.z;
  S.d2 = (double)q.w * (double)q.w;
  S.u = 0.0f; S.v = 0.0f; S.gid = -1; S.slot = -1;
  S.steps = sc.stepLimit;
  S.nodes = 0u; S.tris = 0u;
  if(valid)
  {
    S.d2Up = cp_round_up(S.d2);
    if(WIDE)
      cp_walk_wide8<FILTER, COUNT>(sc, S, ((uint2*)lds_closest) + threadIdx.x, 64);
    else
      cp_walk_bvh2<FILTER, COUNT>(sc, S, lds_closest + threadIdx.x, 64);
  }
  if(valid && S.slot >= 0)
    query_write_hit(sc, hits + 2 * i, sqrtf((float)S.d2), S.u, S.v, S.slot, S.gid);
  else
    query_write_miss(hits + 2 * i, q.w);
  if(COUNT)
  {
    atomicAdd(work, (unsigned long long)S.nodes);
    atomicAdd(work + 1, (unsigned long long)S.tris);
  }
}

// n queries from `queries` into hits.  filter: walk with the cull mask (sc.cullMask, sc.nodeMasks).  work != NULL: the instrumented
// instantiation adds its totals there.
hipError_t vkrt_launch_closest_point(const DevQueryScene& sc, const float4* queries, uint64_t n, bool filter, float4* hits, unsigned long long* work,
                                     hipStream_t stream)
{
  const size_t lds = (size_t)sc.stackCap * 64 * sizeof(int);
  const bool wide = sc.layout == 1u;
  return query_launch_chunks(n, [&](uint64_t first, uint64_t end, dim3 g) {
#define VKRT_CP(W, F, C) hipLaunchKernelGGL((k_closest_point<W, F, C>), g, dim3(64), lds, stream, sc, queries, first, end, hits, work)
    if(work)
    {
      // (one instrumented kernel per layout, with the filter: a cull mask every node meets walks as the unfiltered kernel does)
      if(wide) VKRT_CP(true, true, true); else VKRT_CP(false, true, true);
    }
    else if(wide)
    {
      if(filter) VKRT_CP(true, true, false); else VKRT_CP(true, false, false);
    }
    else
    {
      if(filter) VKRT_CP(false, true, false); else VKRT_CP(false, false, false);
    }
#undef VKRT_CP
  });
}
