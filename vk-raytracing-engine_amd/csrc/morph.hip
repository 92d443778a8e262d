// morph.hip -- morph targets (glTF blend shapes) inside the library: the device side of vkrt_scene_add_morph /
// vkrt_scene_morph_vertices (include/vkrt.h).
//
// A morphed glTF primitive carries, per target, a displacement of POSITION, NORMAL and TANGENT per vertex, and is posed from a vector
// of weights: base + sum(w[k] * delta[k]).  k_morph_live writes the result straight into the scene's live arrays (DevScene::positions
// and the position, normal and tangent words of DevScene::vertexPN, with the store shapes of k_skin); k_morph_bind writes it into the
// bind pose of the skin that contains the morph's range (the store shapes of k_skin_capture), so that the skin's next pose carries the
// morphed shape into the scene: glTF's order, morph then skin.  The base shape is captured when the morph is added (skin.hip's
// k_skin_capture from the live arrays, device copies from a skin's bind pose).
//
// One lane per vertex, pure streaming: 40 B of base read, 12 B per attribute of every target whose weight is not zero, 52 B (live) or
// 40 B (bind) written.  The deltas are vec3 at dword alignment, target-major: lane i of target k reads floats 3 (k count + i) .. + 2,
// so a wave's loads for one target are one contiguous span of 768 B, as its position loads and stores are.  The weights are read by
// the wave as a whole, 64 per load, and a ballot of `w != 0` lists the targets in use: a target that is switched off costs one bit of
// that mask and no memory traffic, and the loop over the others is the same in every lane.
//
// Arithmetic (binary32, source order, no contraction: the Makefile's -ffp-contract=off): see include/vkrt.h.
#include <hip/hip_runtime.h>

#include "device_scene.h"
#include "morph.h"

namespace vkrt {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f3 __attribute__((ext_vector_type(3)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f3u __attribute__((ext_vector_type(3), aligned(4)));  // the scene's own vec3 positions, and the deltas

static_assert(VKRT_VERTEX_QUADS == 3, "the morph kernels write the three float4 of a vertex record");

constexpr unsigned kBlock = 256;

// skin.hip's rule: a zero or overflowing length leaves the vector as it is
__device__ __forceinline__ f3 normalizeGuarded(f3 a)
{
  const float d = (a.x * a.x + a.y * a.y) + a.z * a.z;
  if(d > 0.0f && d < __builtin_inff())
  {
    const float inv = 1.0f / sqrtf(d);
    return a * inv;
  }
  return a;
}

struct Morphed
{
  f3 p, n, t;
  float tw;
};

// vertex i of the morph: the captured base, then target after target in index order.
// The weights are read 64 at a time, one per lane, and the targets in use come out of a ballot: the loop runs once per non-zero
// weight, its count and every branch in it are wave-uniform, and a weight reaches the lanes through a scalar register (readlane).
// Every lane of the wave must be here (the callers clamp i instead of returning early): the ballot and the readlane need them.
// The three loads of a target are issued before the first of its sums; an attribute without deltas sums zeros that are dropped.
__device__ __forceinline__ Morphed morphVertex(uint32_t i, uint32_t count, uint32_t targetCount, const float4* __restrict__ basePN,
                                               const float2* __restrict__ baseNyz, const float4* __restrict__ baseTan, const float* __restrict__ dPos,
                                               const float* __restrict__ dNrm, const float* __restrict__ dTan, const float* __restrict__ weights)
{
  const float4 b0 = basePN[i];
  const float2 b1 = baseNyz[i];
  const float4 b2 = baseTan[i];
  const f3 p0 = {b0.x, b0.y, b0.z}, n0 = {b0.w, b1.x, b1.y}, t0 = {b2.x, b2.y, b2.z};
  f3 P = p0, N = n0, T = t0;
  const uint32_t lane = threadIdx.x & 63u;
  bool any = false;
  for(uint32_t k0 = 0; k0 < targetCount; k0 += 64)
  {
    const float mine = k0 + lane < targetCount ? weights[k0 + lane] : 0.0f;
    unsigned long long inUse = __ballot(mine != 0.0f);  // (a NaN weight of a device array is "not zero": it is used as given)
    any = any || inUse != 0;
    while(inUse)
    {
      const uint32_t b = (uint32_t)__builtin_ctzll(inUse);
      inUse &= inUse - 1;
      const float w = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine), (int)b));
      const size_t at = 3 * ((size_t)(k0 + b) * count + i);
      f3 dp = {0.0f, 0.0f, 0.0f}, dn = dp, dt = dp;
      if(dPos)
        dp = *(const f3u*)(dPos + at);
      if(dNrm)
        dn = *(const f3u*)(dNrm + at);
      if(dTan)
        dt = *(const f3u*)(dTan + at);
      P = P + w * dp;
      N = N + w * dn;
      T = T + w * dt;
    }
  }
  Morphed out;
  out.p = dPos ? P : p0;
  out.n = dNrm ? (any ? normalizeGuarded(N) : N) : n0;
  out.t = dTan ? (any ? normalizeGuarded(T) : T) : t0;
  out.tw = b2.w;
  return out;
}

__global__ __launch_bounds__(kBlock) void k_morph_live(uint32_t first, uint32_t count, uint32_t targetCount, const float4* __restrict__ basePN,
                                                       const float2* __restrict__ baseNyz, const float4* __restrict__ baseTan,
                                                       const float* __restrict__ dPos, const float* __restrict__ dNrm, const float* __restrict__ dTan,
                                                       const float* __restrict__ weights, float* __restrict__ positions, float4* __restrict__ vertexPN)
{
  const uint32_t at = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = at < count ? at : count - 1;  // (the lanes past the end redo the last vertex and store nothing)
  const Morphed m = morphVertex(i, count, targetCount, basePN, baseNyz, baseTan, dPos, dNrm, dTan, weights);
  if(at >= count)
    return;
  const size_t v = (size_t)first + i;
  float* rec = (float*)(vertexPN + VKRT_VERTEX_QUADS * v);  // 48 B, 16-byte aligned
  *(f3u*)(positions + 3 * v) = m.p;
  *(f4*)rec = f4{m.p.x, m.p.y, m.p.z, m.n.x};        // quad 0 = position.xyz, normal.x
  *(f2*)(rec + 4) = f2{m.n.y, m.n.z};                // quad 1 = normal.yz, uv (kept)
  *(f4*)(rec + 8) = f4{m.t.x, m.t.y, m.t.z, m.tw};   // quad 2 = tangent, its handedness as captured
}

__global__ __launch_bounds__(kBlock) void k_morph_bind(uint32_t count, uint32_t targetCount, const float4* __restrict__ basePN,
                                                       const float2* __restrict__ baseNyz, const float4* __restrict__ baseTan,
                                                       const float* __restrict__ dPos, const float* __restrict__ dNrm, const float* __restrict__ dTan,
                                                       const float* __restrict__ weights, float4* __restrict__ bindPN, float2* __restrict__ bindNyz,
                                                       float4* __restrict__ bindTan)
{
  const uint32_t at = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = at < count ? at : count - 1;  // (as in k_morph_live)
  const Morphed m = morphVertex(i, count, targetCount, basePN, baseNyz, baseTan, dPos, dNrm, dTan, weights);
  if(at >= count)
    return;
  bindPN[i] = make_float4(m.p.x, m.p.y, m.p.z, m.n.x);
  bindNyz[i] = make_float2(m.n.y, m.n.z);
  bindTan[i] = make_float4(m.t.x, m.t.y, m.t.z, m.tw);
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

size_t deltaBytes(uint32_t count, uint32_t targetCount) { return align16((size_t)targetCount * count * 3 * sizeof(float)); }

}  // namespace

size_t morph_bytes(uint32_t count, uint32_t targetCount, bool hasPos, bool hasNrm, bool hasTan)
{
  return 2 * (size_t)count * 16 + align16((size_t)count * 8) + ((size_t)hasPos + (size_t)hasNrm + (size_t)hasTan) * deltaBytes(count, targetCount);
}

void morph_carve(void* mem, uint32_t first, uint32_t count, uint32_t targetCount, bool hasPos, bool hasNrm, bool hasTan, MorphArrays& out)
{
  char* at = (char*)mem;
  out.first = first;
  out.count = count;
  out.targetCount = targetCount;
  out.basePN = (float4*)at;   at += (size_t)count * 16;
  out.baseTan = (float4*)at;  at += (size_t)count * 16;
  out.baseNyz = (float2*)at;  at += align16((size_t)count * 8);
  out.dPos = out.dNrm = out.dTan = nullptr;
  if(hasPos)
    out.dPos = (float*)at, at += deltaBytes(count, targetCount);
  if(hasNrm)
    out.dNrm = (float*)at, at += deltaBytes(count, targetCount);
  if(hasTan)
    out.dTan = (float*)at;
}

hipError_t launch_morph_live(float* positions, float4* vertexPN, const MorphArrays& m, const float* weights, hipStream_t stream)
{
  if(m.count == 0)
    return hipSuccess;
  hipLaunchKernelGGL(k_morph_live, dim3((m.count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, m.first, m.count, m.targetCount, m.basePN, m.baseNyz,
                     m.baseTan, m.dPos, m.dNrm, m.dTan, weights, positions, vertexPN);
  return hipGetLastError();
}

hipError_t launch_morph_bind(float4* bindPN, float2* bindNyz, float4* bindTan, const MorphArrays& m, const float* weights, hipStream_t stream)
{
  if(m.count == 0)
    return hipSuccess;
  hipLaunchKernelGGL(k_morph_bind, dim3((m.count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, m.count, m.targetCount, m.basePN, m.baseNyz, m.baseTan,
                     m.dPos, m.dNrm, m.dTan, weights, bindPN, bindNyz, bindTan);
  return hipGetLastError();
}

}  // namespace vkrt
