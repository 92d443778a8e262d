// api_edit.cpp -- editing a live scene (include/vkrt.h): vkrt_scene_update_lights, vkrt_scene_update_materials, vkrt_scene_update_texture
// and the readers of the three tables.  The argument rules are entry_checks.h's, the material records scene_pack.h's, the kernels
// scene_edit.h's.
#include "scene_edit.h"
#include "scene_pack.h"
#include "scene_state.h"

using namespace vkrt;

extern "C" {

int vkrt_scene_update_lights(vkrt_scene* s, const vkrt_light_update* u, void* hip_stream)
{
  CHECK_TRY(check_light_update_desc(u, err));
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_scene_update_lights: scene is NULL");
  CHECK_TRY(check_light_update_range(*u, s->lightCount, err));
  if(u->count == 0)
    return VKRT_OK;
  RC_TRY(enter(s));
  GltfLight* table = const_cast<GltfLight*>(s->dev.lights);
  hipStream_t stream = (hipStream_t)hip_stream;
  // stream-ordered either way, no allocation, no wait: host records as kernel arguments, a device array as one device copy
  if(u->memory == VKRT_MEMORY_HOST)
    HIP_TRY(launch_light_records(table, u->first, u->count, u->lights, stream));
  else
    HIP_TRY(hipMemcpyAsync(table + u->first, u->lights, (size_t)u->count * sizeof(GltfLight), hipMemcpyDeviceToDevice, stream));
  return VKRT_OK;
}

int vkrt_scene_update_materials(vkrt_scene* s, uint32_t first, uint32_t count, const GltfPBRMaterial* materials, void* hip_stream)
{
  const char* who = "vkrt_scene_update_materials";
  CHECK_TRY(check_material_update_values(who, count, materials, s ? (uint32_t)s->textures.size() : 0u, err));
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  CHECK_TRY(check_material_range(who, first, count, s->materialCount, err));
  // every record before anything changes (a refused call leaves the scene as it was)
  std::vector<DevMaterial> mats(count);
  std::vector<DevShadeMaterial> shade(count);
  for(uint32_t i = 0; i < count; i++)
  {
    std::string err;
    if(const int rc = make_material(materials[i], s->textures.data(), (uint32_t)s->textures.size(), s->texQuadFirst.data(), s->dev.texQuads != nullptr, mats[i],
                                    shade[i], err);
       rc != VKRT_OK)
      return fail(rc, "%s: materials[%u]: %s", who, i, err.c_str());
  }
  if(count == 0)
    return VKRT_OK;
  RC_TRY(enter(s));
  HIP_TRY(launch_material_records(const_cast<DevMaterial*>(s->dev.materials), const_cast<DevShadeMaterial*>(s->dev.shadeMaterials), first, count, mats.data(),
                                  shade.data(), (hipStream_t)hip_stream));
  // the host builder's copy follows; a material that the tree's triangle flags do not cover asks for a rebuild (the header's dissolve rule)
  for(uint32_t i = 0; i < count; i++)
  {
    const float a = materials[i].pbrBaseColorFactor[3];
    s->materialAlpha[(size_t)first + i] = a;
    if(s->built && !s->builtNonOpaque.empty() && a < 1.0f && !s->builtNonOpaque[(size_t)first + i])
      s->dissolveRebuild = true;
  }
  return VKRT_OK;
}

int vkrt_scene_update_texture(vkrt_scene* s, const vkrt_texture_update* u, void* hip_stream)
{
  const char* who = "vkrt_scene_update_texture";
  CHECK_TRY(check_texture_update_desc(u, err));
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  CHECK_TRY(check_texture_index(who, u->texture, (uint32_t)s->textures.size(), err));
  const DevTexture& tx = s->textures[u->texture];
  CHECK_TRY(check_texture_update_image(*u, tx.width, tx.height, err));
  RC_TRY(enter(s));
  TextureSlot slot{};
  slot.width = tx.width;
  slot.height = tx.height;
  slot.srgb = (tx.srgb & 1u) != 0u;
  slot.levels = tx.srgb >> 8;
  std::copy_n(&s->texMips[(size_t)u->texture * VKRT_MAX_MIPS], VKRT_MAX_MIPS, slot.levelOffset);
  slot.quadFirst = s->texQuadFirst[u->texture];
  hipStream_t stream = (hipStream_t)hip_stream;
  const void* texels = u->rgba8;
  const bool staged = u->memory == VKRT_MEMORY_HOST;
  if(staged)
    HIP_TRY(s->vertexStage.putBytes(u->rgba8, (size_t)tx.width * tx.height * 4, &texels, stream));
  // one device path for both memory kinds: level 0 and the footprints, then the mip chain, in stream order
  HIP_TRY(launch_texture_image(const_cast<uint32_t*>(s->dev.texels), const_cast<uint4*>(s->dev.texQuads), slot, (const uint32_t*)texels, s->dev.srgbLut,
                               s->srgbEncode, stream));
  if(staged)
    HIP_TRY(hipStreamSynchronize(stream));  // (the staging buffer's rule, dev_buffer.h)
  return VKRT_OK;
}

int vkrt_debug_read_lights(vkrt_scene* s, uint32_t first, uint32_t count, void* out, uint64_t bytes)
{
  const char* who = "vkrt_debug_read_lights";
  if(!s || !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
  if((uint64_t)first + count > s->lightCount)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: lights [%u, %llu) outside the scene's %u lights", who, first, (unsigned long long)first + count, s->lightCount);
  if(bytes != (uint64_t)count * sizeof(GltfLight))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: bytes %llu != %zu x %u records", who, (unsigned long long)bytes, sizeof(GltfLight), count);
  RC_TRY(enter(s));
  HIP_TRY(readBack(out, s->dev.lights + first, (size_t)count * sizeof(GltfLight)));
  return VKRT_OK;
}

int vkrt_debug_read_materials(vkrt_scene* s, uint32_t first, uint32_t count, void* out, uint64_t bytes)
{
  const char* who = "vkrt_debug_read_materials";
  if(!s || !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
  CHECK_TRY(check_material_range(who, first, count, s->materialCount, err));
  constexpr size_t kRecord = sizeof(DevMaterial) + sizeof(DevShadeMaterial);
  if(bytes != (uint64_t)count * kRecord)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: bytes %llu != %zu x %u records", who, (unsigned long long)bytes, kRecord, count);
  RC_TRY(enter(s));
  std::vector<DevMaterial> mats(count);
  std::vector<DevShadeMaterial> shade(count);
  HIP_TRY(readBack(mats.data(), s->dev.materials + first, (size_t)count * sizeof(DevMaterial)));
  HIP_TRY(readBack(shade.data(), s->dev.shadeMaterials + first, (size_t)count * sizeof(DevShadeMaterial)));
  for(uint32_t i = 0; i < count; i++)
  {
    memcpy((char*)out + i * kRecord, &mats[i], sizeof(DevMaterial));
    memcpy((char*)out + i * kRecord + sizeof(DevMaterial), &shade[i], sizeof(DevShadeMaterial));
  }
  return VKRT_OK;
}

int vkrt_debug_read_texture(vkrt_scene* s, uint32_t texture, uint32_t level, void* texels, uint64_t texel_bytes, void* quads, uint64_t quad_bytes)
{
  const char* who = "vkrt_debug_read_texture";
  if(!s || !texels)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
  CHECK_TRY(check_texture_index(who, texture, (uint32_t)s->textures.size(), err));
  const DevTexture& tx = s->textures[texture];
  if(level >= (tx.srgb >> 8))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: level %u outside texture %u's %u levels", who, level, texture, tx.srgb >> 8);
  const uint64_t n = (uint64_t)std::max(1u, tx.width >> level) * std::max(1u, tx.height >> level);
  if(texel_bytes != n * 4)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: texel_bytes %llu != 4 x %llu texels", who, (unsigned long long)texel_bytes, (unsigned long long)n);
  if(quads && level != 0)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: quads with level %u (the footprint records are level 0's)", who, level);
  if(quads && quad_bytes != n * 16)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: quad_bytes %llu != 16 x %llu records", who, (unsigned long long)quad_bytes, (unsigned long long)n);
  if(quads && !s->dev.texQuads)
    return fail(VKRT_ERR_UNSUPPORTED, "%s: the scene has no footprint pool", who);
  RC_TRY(enter(s));
  HIP_TRY(readBack(texels, s->dev.texels + s->texMips[(size_t)texture * VKRT_MAX_MIPS + level], (size_t)n * 4));
  if(quads)
    HIP_TRY(readBack(quads, s->dev.texQuads + s->texQuadFirst[texture], (size_t)n * 16));
  return VKRT_OK;
}

}  // extern "C"
