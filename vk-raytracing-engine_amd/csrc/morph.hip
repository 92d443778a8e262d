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

constexpr unsigned kBlock = 256;

// vertex i of the morph: the captured base, then target after target in index order.
// The weights are read 64 at a time, one per lane, and the targets in use come out of a ballot: the loop runs once per non-zero
// weight, its count and every branch in it are wave-uniform, and a weight reaches the lanes through a scalar register (readlane).
// Every lane of the wave must be here (the callers clamp i instead of returning early): the ballot and the readlane need them.
// The three loads of a target are issued before the first of its sums; an attribute without deltas sums zeros that are dropped.
__device__ __forceinline__ PoseVertex morphVertex(uint32_t i, uint32_t count, uint32_t targetCount, const Pose& base, const float* __restrict__ dPos,
                                                  const float* __restrict__ dNrm, const float* __restrict__ dTan, const float* __restrict__ weights)
{
  const PoseVertex b = pose_load(base, i);
  f3 P = b.p, N = b.n, T = b.t;
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
  return PoseVertex{dPos ? P : b.p, dNrm ? (any ? normalizeGuarded(N) : N) : b.n, dTan ? (any ? normalizeGuarded(T) : T) : b.t, b.tw};
}

__global__ __launch_bounds__(kBlock) void k_morph_live(uint32_t first, uint32_t count, uint32_t targetCount, Pose base, const float* __restrict__ dPos,
                                                       const float* __restrict__ dNrm, const float* __restrict__ dTan,
                                                       const float* __restrict__ weights, float* __restrict__ positions, float4* __restrict__ vertexPN)
{
  const uint32_t at = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = at < count ? at : count - 1;  // (the lanes past the end redo the last vertex and store nothing)
  const PoseVertex m = morphVertex(i, count, targetCount, base, dPos, dNrm, dTan, weights);
  if(at >= count)
    return;
  live_store(positions, vertexPN, (size_t)first + i, m);
}

__global__ __launch_bounds__(kBlock) void k_morph_bind(uint32_t count, uint32_t targetCount, float4* __restrict__ basePN, float2* __restrict__ baseNyz,
                                                       float4* __restrict__ baseTan, const float* __restrict__ dPos, const float* __restrict__ dNrm,
                                                       const float* __restrict__ dTan, const float* __restrict__ weights, float4* __restrict__ bindPN,
                                                       float2* __restrict__ bindNyz, float4* __restrict__ bindTan)
{
  // (two poses as six pointer arguments: with two Pose arguments the compiler fetches the kernel arguments in other pieces)
  const Pose base = {basePN, baseTan, baseNyz}, bind = {bindPN, bindTan, bindNyz};
  const uint32_t at = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = at < count ? at : count - 1;  // (as in k_morph_live)
  const PoseVertex m = morphVertex(i, count, targetCount, base, dPos, dNrm, dTan, weights);
  if(at >= count)
    return;
  pose_store(bind, i, m);
}

size_t deltaBytes(uint32_t count, uint32_t targetCount) { return align16((size_t)targetCount * count * 3 * sizeof(float)); }

}  // namespace

size_t morph_bytes(uint32_t count, uint32_t targetCount, bool hasPos, bool hasNrm, bool hasTan)
{
  return pose_bytes(count) + ((size_t)hasPos + (size_t)hasNrm + (size_t)hasTan) * deltaBytes(count, targetCount);
}

void morph_carve(void* mem, uint32_t first, uint32_t count, uint32_t targetCount, bool hasPos, bool hasNrm, bool hasTan, MorphArrays& out)
{
  out.first = first;
  out.count = count;
  out.targetCount = targetCount;
  char* at = pose_carve((char*)mem, count, out.base);
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
  hipLaunchKernelGGL(k_morph_live, dim3((m.count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, m.first, m.count, m.targetCount, m.base, m.dPos, m.dNrm,
                     m.dTan, weights, positions, vertexPN);
  return hipGetLastError();
}

hipError_t launch_morph_bind(Pose bind, const MorphArrays& m, const float* weights, hipStream_t stream)
{
  if(m.count == 0)
    return hipSuccess;
  hipLaunchKernelGGL(k_morph_bind, dim3((m.count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, m.count, m.targetCount, m.base.pn, m.base.nyz, m.base.tan,
                     m.dPos, m.dNrm, m.dTan, weights, bind.pn, bind.nyz, bind.tan);
  return hipGetLastError();
}

}  // namespace vkrt
