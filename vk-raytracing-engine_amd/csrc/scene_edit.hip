// scene_edit.hip -- editing a live scene's lights, materials and textures: the device side of vkrt_scene_update_lights,
// vkrt_scene_update_materials and vkrt_scene_update_texture (include/vkrt.h).
//
// Lights and materials are small tables whose new records the host has in hand: they travel as kernel arguments, 16 B per lane, like
// the instance records of vkrt_scene_update_nodes (refit.hip k_rf_instances).  A texture is the one table that is rebuilt here:
//   k_se_level0    one lane per level-0 texel: the pool word (4 B per lane, consecutive lanes consecutive words) and the 16-B footprint
//                  record {(x,y), (x+1,y), (x,y+1), (x+1,y+1)} with wrap-around as one 16-byte store per lane, 1 KiB per wave and store.
//                  The four reads of a lane overlap its neighbours': each source texel comes from HBM once
//   k_se_mip       one lane per texel of level L, blitted from level L - 1 with the arithmetic of pack_scene (texture_pack.h
//                  vkrt_mip_texel: binary32 in source order, IEEE division; this unit is built with -ffp-contract=off like all of them)
//   k_se_mip_tail  one workgroup for every level whose source has at most kTailTexels texels, level after level with a barrier between
//                  them: a 2048 x 2048 texture takes 1 + 7 + 1 launches instead of 1 + 11
// Both mip kernels keep the 512-entry decode table and the 256 thresholds of the sRGB encode (texture_pack.h vkrt_srgb_quantise) in
// 3 KiB of LDS: a texel reads 16 decode entries and, in an sRGB texture, 24 thresholds.  No atomics, no scratch; a lane writes its own
// texel only.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>

#include "scene_edit.h"
#include "texture_pack.h"

namespace vkrt {

constexpr uint32_t kLightsPerLaunch = 120;    // 16 + 120 x 32 B of kernel arguments (limit 4 KiB)
constexpr uint32_t kMaterialsPerLaunch = 20;  // 16 + 20 x 192 B
constexpr uint32_t kTailTexels = 256;         // a level that is read from at most this many texels is made by k_se_mip_tail
static_assert(sizeof(GltfLight) == 2 * sizeof(uint4) && sizeof(DevMaterial) == 8 * sizeof(uint4) && sizeof(DevShadeMaterial) == 4 * sizeof(uint4), "quads");

// (outside the anonymous namespace: tools/kernel_resources.py reads a kernel's name off its demangled signature)
struct LightBatch
{
  uint32_t first, count, pad[2];
  uint4 quad[2 * kLightsPerLaunch];
};
struct MaterialBatch
{
  uint32_t first, count, pad[2];
  uint4 quad[12 * kMaterialsPerLaunch];  // per material: the eight quads of its DevMaterial, the four of its DevShadeMaterial
};
struct MipTail
{
  uint32_t count, srgb;  // levels listed, the first is read only
  uint32_t at[VKRT_MAX_MIPS], w[VKRT_MAX_MIPS], h[VKRT_MAX_MIPS];
};

namespace {

constexpr unsigned kBlock = 256;

__global__ __launch_bounds__(kBlock) void k_se_lights(LightBatch b, uint4* table)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i < 2u * b.count)
    table[2 * (size_t)b.first + i] = b.quad[i];
}

__global__ __launch_bounds__(kBlock) void k_se_materials(MaterialBatch b, uint4* materials, uint4* shadeMaterials)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= 12u * b.count)
    return;
  const uint32_t m = i / 12u, q = i % 12u;
  const uint4 v = b.quad[i];
  if(q >= 8u)
    shadeMaterials[4 * (size_t)(b.first + m) + (q - 8u)] = v;
  else if(q != 3u)
    materials[8 * (size_t)(b.first + m) + q] = v;
  else  // (emissiveTexture, pad, alphaMode, alphaCutoff): the second half is vkrt_scene_set_material_alpha's
    *reinterpret_cast<uint2*>(&materials[8 * (size_t)(b.first + m) + 3]) = make_uint2(v.x, v.y);
}

// pool, quads: at the texture's level 0 / first footprint record
__global__ __launch_bounds__(kBlock) void k_se_level0(uint32_t w, uint32_t h, const uint32_t* __restrict__ src, uint32_t* __restrict__ pool,
                                                      uint4* __restrict__ quads)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= w * h)
    return;
  if(!quads)
  {
    pool[i] = src[i];
    return;
  }
  uint32_t q[4];
  vkrt_footprint(src, w, h, i % w, i / w, q);
  pool[i] = q[0];
  quads[i] = make_uint4(q[0], q[1], q[2], q[3]);
}

__device__ inline void loadTables(float* sLut, float* sT, const float* __restrict__ lut512, const float* __restrict__ encodeT)
{
  for(uint32_t k = threadIdx.x; k < 512u; k += kBlock) sLut[k] = lut512[k];
  for(uint32_t k = threadIdx.x; k < (uint32_t)VKRT_SRGB_THRESHOLDS; k += kBlock) sT[k] = encodeT[k];
  __syncthreads();
}

// level (dstAt, dw x dh) of the pool from level (srcAt, sw x sh)
__global__ __launch_bounds__(kBlock) void k_se_mip(uint32_t* pool, uint32_t srcAt, uint32_t sw, uint32_t sh, uint32_t dstAt, uint32_t dw, uint32_t dh,
                                                   uint32_t srgb, const float* __restrict__ lut512, const float* __restrict__ encodeT)
{
  __shared__ float sLut[512], sT[VKRT_SRGB_THRESHOLDS];
  loadTables(sLut, sT, lut512, encodeT);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= dw * dh)
    return;
  pool[(size_t)dstAt + i] = vkrt_mip_texel(pool + srcAt, sw, sh, dw, dh, i % dw, i / dw, srgb != 0u, sLut, sT);
}

__global__ __launch_bounds__(kBlock) void k_se_mip_tail(uint32_t* pool, MipTail t, const float* __restrict__ lut512, const float* __restrict__ encodeT)
{
  __shared__ float sLut[512], sT[VKRT_SRGB_THRESHOLDS];
  loadTables(sLut, sT, lut512, encodeT);
  for(uint32_t L = 1; L < t.count; L++)
  {
    const uint32_t dw = t.w[L], dh = t.h[L];
    for(uint32_t i = threadIdx.x; i < dw * dh; i += kBlock)
      pool[(size_t)t.at[L] + i] = vkrt_mip_texel(pool + t.at[L - 1], t.w[L - 1], t.h[L - 1], dw, dh, i % dw, i / dw, t.srgb != 0u, sLut, sT);
    __syncthreads();  // the level just written is the next one's source (one workgroup: the barrier orders its global stores and loads)
  }
}

}  // namespace

hipError_t launch_light_records(GltfLight* table, uint32_t first, uint32_t count, const GltfLight* src, hipStream_t stream)
{
  for(uint32_t done = 0; done < count; done += kLightsPerLaunch)
  {
    LightBatch b;
    b.first = first + done;
    b.count = std::min(kLightsPerLaunch, count - done);
    memcpy(b.quad, src + done, (size_t)b.count * sizeof(GltfLight));
    hipLaunchKernelGGL(k_se_lights, dim3((2 * b.count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, b, (uint4*)table);
  }
  return hipGetLastError();
}

hipError_t launch_material_records(DevMaterial* materials, DevShadeMaterial* shadeMaterials, uint32_t first, uint32_t count, const DevMaterial* src,
                                   const DevShadeMaterial* shadeSrc, hipStream_t stream)
{
  for(uint32_t done = 0; done < count; done += kMaterialsPerLaunch)
  {
    MaterialBatch b;
    b.first = first + done;
    b.count = std::min(kMaterialsPerLaunch, count - done);
    for(uint32_t k = 0; k < b.count; k++)
    {
      memcpy(&b.quad[12 * k], src + done + k, sizeof(DevMaterial));
      memcpy(&b.quad[12 * k + 8], shadeSrc + done + k, sizeof(DevShadeMaterial));
    }
    hipLaunchKernelGGL(k_se_materials, dim3((12 * b.count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, b, (uint4*)materials, (uint4*)shadeMaterials);
  }
  return hipGetLastError();
}

hipError_t launch_texture_image(uint32_t* pool, uint4* quads, const TextureSlot& t, const uint32_t* texels, const float* lut512, const float* encodeT,
                                hipStream_t stream)
{
  const uint32_t n0 = t.width * t.height;  // (a pool holds fewer than 2^30 texels)
  hipLaunchKernelGGL(k_se_level0, dim3((n0 + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, t.width, t.height, texels, pool + t.levelOffset[0],
                     quads ? quads + t.quadFirst : nullptr);
  uint32_t w = t.width, h = t.height, L = 1;
  for(; L < t.levels && w * h > kTailTexels; L++)
  {
    const uint32_t dw = std::max(1u, w / 2), dh = std::max(1u, h / 2);
    hipLaunchKernelGGL(k_se_mip, dim3((dw * dh + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pool, t.levelOffset[L - 1], w, h, t.levelOffset[L], dw, dh,
                       t.srgb ? 1u : 0u, lut512, encodeT);
    w = dw; h = dh;
  }
  if(L < t.levels)
  {
    MipTail tail{};
    tail.srgb = t.srgb ? 1u : 0u;
    for(uint32_t k = L - 1; k < t.levels; k++)
    {
      tail.at[tail.count] = t.levelOffset[k];
      tail.w[tail.count] = w; tail.h[tail.count] = h;
      tail.count++;
      w = std::max(1u, w / 2); h = std::max(1u, h / 2);
    }
    hipLaunchKernelGGL(k_se_mip_tail, dim3(1), dim3(kBlock), 0, stream, pool, tail, lut512, encodeT);
  }
  return hipGetLastError();
}

}  // namespace vkrt
