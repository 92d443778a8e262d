// scene_edit.h -- editing a live scene's lights, materials and textures (scene_edit.hip): the device side of vkrt_scene_update_lights,
// vkrt_scene_update_materials and vkrt_scene_update_texture.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "device_scene.h"

namespace vkrt {

// Records [first, first + count) of the light table from a host array: they travel as kernel arguments of launches on `stream` (like
// upload_instances' records: nothing staged, no synchronisation).
hipError_t launch_light_records(GltfLight* table, uint32_t first, uint32_t count, const GltfLight* src, hipStream_t stream);

// Records [first, first + count) of both material tables from host arrays, as kernel arguments of launches on `stream`.  Words 14 and 15
// of a DevMaterial (alphaMode, alphaCutoff) are not written: they stay what vkrt_scene_set_material_alpha made them.
hipError_t launch_material_records(DevMaterial* materials, DevShadeMaterial* shadeMaterials, uint32_t first, uint32_t count, const DevMaterial* src,
                                   const DevShadeMaterial* shadeSrc, hipStream_t stream);

// One texture of the pools, as the host copy of the scene's tables describes it
struct TextureSlot
{
  uint32_t width, height;
  bool srgb;
  uint32_t levels;                      // >= 1
  uint32_t levelOffset[VKRT_MAX_MIPS];  // first texel of each level in the RGBA8 pool
  uint32_t quadFirst;                   // first footprint record (read when the scene has that pool)
};

// The whole image of one texture from width x height RGBA8 texels in device memory (4-byte aligned): level 0 of the pool, the footprint
// records (quads != nullptr) and every mip level, bit for bit what pack_scene makes of the same texels (texture_pack.h).  Enqueued on
// `stream`: one launch for level 0 and the footprints, one per mip level while the level it reads has more than kTailTexels texels, one
// for all the levels behind (at most 1 + VKRT_MAX_MIPS in all); no allocation, no synchronisation.  lut512: DevScene::srgbLut;
// encodeT: the thresholds of make_srgb_encode_table on the device.
hipError_t launch_texture_image(uint32_t* pool, uint4* quads, const TextureSlot& t, const uint32_t* texels, const float* lut512, const float* encodeT,
                                hipStream_t stream);

}  // namespace vkrt
