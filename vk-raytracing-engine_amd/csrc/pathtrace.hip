// pathtrace.hip -- the path-trace dispatch: replaces vkCmdTraceRaysKHR(W,H,1) over
// raytrace.rgen / .rchit / .rmiss / raytraceShadow.rmiss (reference hello_vulkan.cpp:1446,
// shaders/raytrace.rgen:24-146).
//
// Execution model (gfx950, wave64): persistent wavefronts.  Every lane owns one pixel at a time and
// runs the rgen sample/bounce loops as a state machine whose unit of work is ONE ray (closest-hit or
// shadow), so all live lanes of a wave are always inside the same BVH traversal loop.  Lanes whose
// pixel is finished are refilled from a global work counter with one wave-aggregated atomic
// (__ballot + popcount prefix); a wave exits when the counter is exhausted and all lanes are idle.
// Pixels are handed out in 8x8 tiles so the 64 pixels a fresh wave pulls are one screen tile.
// Per-lane traversal stacks live in LDS (entry k of lane l at stack[k*BLOCK + l]: bank-conflict free).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "device_math.h"
#include "device_scene.h"
#include "shade.h"
#include "traverse.h"
#include "traverse_wide.h"
#include "rgen.h"
#include "kernels.h"

#define VKRT_BLOCK 256


template <bool COUNT, int MINW, int TM>
__global__ __launch_bounds__(VKRT_BLOCK, MINW) void k_pathtrace(const TraceParams P)
{
  extern __shared__ int lds_stack[];
  int* stk = lds_stack + threadIdx.x;
  const unsigned lane = lane_id();

  LaneState L;
  bool active = false;
  bool exhausted = false;  // wave-uniform: work counter ran out
  unsigned nClosest = 0, nShadow = 0, nPixels = 0;
  TravCount tc;
  __shared__ float lut[512];
  ShadeStats st = shadeStatsInit(P.sc, lut);
  const uint32_t totalWork = P.tileCount * 64u;

  for(;;)
  {
    // ---- refill idle lanes (wave-aggregated dequeue) ------------------------------------------
    const unsigned long long idleMask = __ballot(!active);
    if(idleMask != 0ull && !exhausted)
    {
      const unsigned nIdle = (unsigned)__popcll(idleMask);
      // refill when the wave is empty or at least a quarter of it idles
      if(nIdle >= 16u || idleMask == ~0ull)
      {
        unsigned base = 0;
        const unsigned leader = (unsigned)__ffsll((long long)idleMask) - 1u;
        if(lane == leader)
          base = atomicAdd(P.workCounter, nIdle);
        base = (unsigned)__shfl((int)base, (int)leader);
        if(base + nIdle >= totalWork)
          exhausted = true;
        if(!active)
        {
          const unsigned w = base + (unsigned)__popcll(idleMask & ((1ull << lane) - 1ull));
          uint32_t x, y, lrow;
          if(pixelOfWork(P, w, 0u, x, y, lrow))
          {
            startPixel(P, L, x, y, lrow);
            active = true;
            nPixels++;
            if(P.pc.samples <= 0 || P.pc.depth <= 0)
            {  // degenerate launch: no rays, store the resolved (0/samples) value
              storePixel(P, L);
              active = false;
            }
          }
        }
      }
    }
    if(__ballot(active) == 0ull)
    {
      if(exhausted)
        break;
      continue;
    }

    // ---- one ray per live lane -------------------------------------------------------------------
    if(active)
    {
      f3 o = L.prd.rayOrigin, d;
      float tmin = 0.001f, tmax;
      const bool shadow = (L.stage == 1);
      if(shadow)
      {
        d = L.prd.shadowRayDir;
        tmax = L.prd.lightDist - 0.1f;  // rgen:94
        nShadow++;
      }
      else
      {
        d = L.prd.rayDirection;
        tmax = 10000.0f;
        nClosest++;
      }
      RayHit hit;
      traverse<COUNT, TM>(P.sc, o, d, tmin, tmax, shadow, stk, VKRT_BLOCK, hit, tc, L.prd.seed);

      bool shadowHit = false;
      bool accumulate = true;
      if(!shadow)
        accumulate = !afterClosestRay(P, L, hit, hit.slot >= 0 ? P.sc.triShade[hit.slot] : make_uint4(0u, 0u, 0u, 0u), d, st);
      else
        shadowHit = hit.slot >= 0;
      if(accumulate)
        active = accumulateAndAdvance(P, L, shadowHit);
    }
  }

  // ---- counters: block reduce, one atomic per counter per block ------------------------------------
  __shared__ unsigned long long red[VKRT_COUNTER_STRIDE * (VKRT_BLOCK / 64)];
  const unsigned vals[10] = {nClosest, nShadow, st.hits, st.diffuse, st.taps, nPixels, tc.nodes, tc.tris, tc.waveNodeSteps, tc.waveTriSteps};
  blockAddCounters(&P.counters->v[blockIdx.x % VKRT_COUNTER_SLOTS][0], vals, COUNT ? 10 : 6, red);
}

// ---- debug / test kernels --------------------------------------------------------------------------
__global__ __launch_bounds__(VKRT_BLOCK) void k_trace_rays(DevScene sc, unsigned n, const float* o, const float* d, float tmin,
                                                           float tmax, int anyHit, float* t, float* u, float* v, int* gid)
{
  extern __shared__ int lds_stack[];
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  RayHit hit;
  TravCount tc;
  const f3 ro = mk3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = mk3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
  // (test hook: the payload seed of these rays is 0, and the alpha-test stage of the frames is never theirs)
#define VKRT_DBG(W, TM) traverse_any<false, W, TM>(sc, ro, rd, tmin, tmax, anyHit != 0, lds_stack, (int)threadIdx.x, VKRT_BLOCK, hit, tc, 0u)
#define VKRT_DBG_WIDE(TM) VKRT_DBG(true, TM)
#define VKRT_DBG_BVH2(TM) VKRT_DBG(false, TM)
  if(sc.layout == 1u)
  {
    VKRT_TM_SWITCH4(frame_tri_mode(sc, false), VKRT_TM_DISSOLVE, 0, VKRT_DBG_WIDE)
  }
  else
  {
    VKRT_TM_SWITCH4(frame_tri_mode(sc, false), VKRT_TM_DISSOLVE, 0, VKRT_DBG_BVH2)
  }
#undef VKRT_DBG_BVH2
#undef VKRT_DBG_WIDE
#undef VKRT_DBG
  if(anyHit)
  {
    gid[i] = hit.slot >= 0 ? 0 : -1;
    t[i] = 0; u[i] = 0; v[i] = 0;
  }
  else
  {
    t[i] = hit.t; u[i] = hit.u; v[i] = hit.v;
    gid[i] = hit.slot >= 0 ? (__float_as_int(sc.tris[hit.slot * VKRT_TRI_QUADS + 2].y) & 0x7fffffff) : -1;
  }
}

__global__ void k_eval_math(int op, unsigned n, const float* a, const float* b, float* out)
{
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  float s, c;
  switch(op)
  {
    case 0: vk_sincos(a[i], &s, &c); out[i] = s; break;
    case 1: vk_sincos(a[i], &s, &c); out[i] = c; break;
    case 2: out[i] = sqrtf(a[i]); break;
    case 3: out[i] = a[i] / b[i]; break;
    case 4: out[i] = vk_pow5(a[i]); break;
    default: out[i] = normalize3(mk3(a[i], b[i], 0.0f)).x; break;
  }
}

// The BRDF tail of the hit shader on caller records (vkrt_debug_eval_shade; record layout in include/vkrt.h): one record per thread.
// The thread builds the HitMid closestHitFront hands over for an untextured material and runs closestHitLobe + closestHitTail, the
// functions of the frame kernels.  lights: VKRT_EVAL_SHADE_MAX_LIGHTS 32-byte records per thread; the thread fills the first
// lightsCount with the record's light, so whichever index the tail draws finds it.
__global__ __launch_bounds__(VKRT_BLOCK) void k_eval_shade(unsigned n, const float* in, float4* lights, float* out)
{
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  const float* p = in + 40u * (size_t)i;
  float* o = out + 20u * (size_t)i;
  const int lightsCount = __float_as_int(p[35]);
  if(lightsCount < 1 || lightsCount > VKRT_EVAL_SHADE_MAX_LIGHTS)  // (the host refuses such a batch; never index past the thread's lights)
  {
    for(int k = 0; k < 20; k++)
      o[k] = 0.0f;
    return;
  }
  float4* lq = lights + 2u * VKRT_EVAL_SHADE_MAX_LIGHTS * (size_t)i;
  const float4 l0 = make_float4(p[24], p[25], p[26], p[27]), l1 = make_float4(p[28], p[29], p[30], p[31]);
  for(int k = 0; k < lightsCount; k++)
  {
    lq[2 * k] = l0;
    lq[2 * k + 1] = l1;
  }
  DevScene sc = {};
  sc.lights = (const GltfLight*)lq;
  PushConstantRay pc = {};
  pc.lightsCount = lightsCount;
  Payload prd = {};
  prd.seed = __float_as_uint(p[32]);
  prd.depth = __float_as_uint(p[33]);
  prd.isSpecular = __float_as_uint(p[34]) != 0u;
  HitMid mid;
  mid.worldPos = mk3(p[0], p[1], p[2]); mid.N = mk3(p[3], p[4], p[5]);
  mid.tangent = mk3(p[6], p[7], p[8]); mid.binormal = mk3(p[9], p[10], p[11]);
  mid.V = normalize3(-mk3(p[12], p[13], p[14]));
  mid.baseColor = mk3(p[15], p[16], p[17]);
  mid.emittance = (prd.depth == 0 || prd.isSpecular) ? mk3(p[21], p[22], p[23]) : mk3(0.0f);  // rchit:83
  mid.metalU = p[19]; mid.roughU = p[20];
  mid.retap = 0u;
  ShadeStats st;
  st.hits = 0; st.diffuse = 0; st.taps = 0; st.lut = nullptr;
  const bool diffuse = closestHitLobe(mid, prd);
  closestHitTail(sc, pc, mid, diffuse, prd, st);
  o[0] = prd.hitValue.x; o[1] = prd.hitValue.y; o[2] = prd.hitValue.z;
  o[3] = prd.rayOrigin.x; o[4] = prd.rayOrigin.y; o[5] = prd.rayOrigin.z;
  o[6] = prd.rayDirection.x; o[7] = prd.rayDirection.y; o[8] = prd.rayDirection.z;
  o[9] = prd.weight.x; o[10] = prd.weight.y; o[11] = prd.weight.z;
  o[12] = prd.isSpecular ? 1.0f : 0.0f;
  // (the specular branch leaves lightDist / shadowRayDir as the payload held them: 0 here, as in the oracle's record call)
  o[13] = prd.lightDist;
  o[14] = prd.shadowRayDir.x; o[15] = prd.shadowRayDir.y; o[16] = prd.shadowRayDir.z;
  o[17] = __uint_as_float(prd.seed);
  o[18] = 0.0f; o[19] = 0.0f;
}

// ---- launch wrappers (called from the api_*.cpp units) ------------------------------------------------------
// MINW = minimum waves per SIMD the register allocator must allow: 3 measured +34 % over the unconstrained build and
// level with 4 (profiles/r01_experiments.md #2, #3), so the product build carries that one variant.
hipError_t vkrt_launch_pathtrace(const TraceParams& P, unsigned gridBlocks, bool count, hipStream_t stream)
{
  const size_t lds = (size_t)P.sc.stackCap * VKRT_BLOCK * sizeof(int);
  const dim3 g(gridBlocks), b(VKRT_BLOCK);
// (With the alpha-test stage the kernel does not fit the 168 VGPRs of MINW = 3 -- its siblings already spill 26 to 28 there -- so those
// instantiations ask for two waves per SIMD and keep everything in registers.)
#define VKRT_MEGA(TM)                                                                                        \
  do {                                                                                                       \
    if(count) hipLaunchKernelGGL((k_pathtrace<true, 1, TM>), g, b, lds, stream, P);                         \
    else hipLaunchKernelGGL((k_pathtrace<false, ((TM) & VKRT_TM_ALPHA) ? 2 : 3, TM>), g, b, lds, stream, P); \
  } while(0)
  VKRT_FRAME_TM_SWITCH(frame_tri_mode(P.sc, false), VKRT_TM_DISSOLVE, VKRT_MEGA)
#undef VKRT_MEGA
  return hipGetLastError();
}

int vkrt_pathtrace_block_size() { return VKRT_BLOCK; }

hipError_t vkrt_pathtrace_occupancy(size_t ldsBytes, int* blocksPerCU)
{
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocksPerCU, k_pathtrace<false, 3, 0>, VKRT_BLOCK, ldsBytes);
}

hipError_t vkrt_launch_trace_rays(const DevScene& sc, unsigned n, const float* o, const float* d, float tmin, float tmax, int anyHit,
                                  float* t, float* u, float* v, int* gid, hipStream_t stream)
{
  const size_t lds = (size_t)sc.stackCap * VKRT_BLOCK * sizeof(int);
  hipLaunchKernelGGL(k_trace_rays, dim3((n + VKRT_BLOCK - 1) / VKRT_BLOCK), dim3(VKRT_BLOCK), lds, stream, sc, n, o, d, tmin, tmax,
                     anyHit, t, u, v, gid);
  return hipGetLastError();
}

hipError_t vkrt_launch_eval_math(int op, unsigned n, const float* a, const float* b, float* out, hipStream_t stream)
{
  hipLaunchKernelGGL(k_eval_math, dim3((n + 255) / 256), dim3(256), 0, stream, op, n, a, b, out);
  return hipGetLastError();
}

hipError_t vkrt_launch_eval_shade(unsigned n, const float* in, float4* lights, float* out, hipStream_t stream)
{
  hipLaunchKernelGGL(k_eval_shade, dim3((n + VKRT_BLOCK - 1) / VKRT_BLOCK), dim3(VKRT_BLOCK), 0, stream, n, in, lights, out);
  return hipGetLastError();
}
