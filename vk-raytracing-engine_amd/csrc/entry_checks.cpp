// entry_checks.cpp -- the argument rules of the node-update, visibility, material-alpha, scene-edit, query and frame entry points (entry_checks.h):
// host-only, no HIP type.
#include "entry_checks.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace vkrt {

namespace {

int refuse(int code, std::string& err, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int refuse(int code, std::string& err, const char* fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  err = buf;
  return code;
}

const int kBad = VKRT_ERR_INVALID_ARGUMENT;
const char* const kNodeUpdate = "vkrt_scene_update_node_transforms";

}  // namespace

int check_node_range(const char* who, uint32_t first, uint32_t count, size_t nodeCount, std::string& err)
{
  if((uint64_t)first + count <= nodeCount)
    return VKRT_OK;
  return refuse(kBad, err, "%s%snodes [%u, %llu) outside the scene's %zu nodes", who ? who : "", who ? ": " : "", first, (unsigned long long)first + count, nodeCount);
}

int check_prim_mesh_kept(uint32_t node, int32_t given, int32_t kept, std::string& err)
{
  return given != kept ? refuse(kBad, err, "node %u: primMesh %d != %d (an update moves instances, it does not change their geometry)", node, given, kept) : VKRT_OK;
}

int check_node_update_desc(const vkrt_node_update* u, std::string& err)
{
  const char* who = kNodeUpdate;
  if(!u)
    return refuse(kBad, err, "%s: update is NULL", who);
  if(u->struct_size < sizeof(vkrt_node_update))
    return refuse(kBad, err, "%s: vkrt_node_update.struct_size %u < %zu (ABI mismatch)", who, u->struct_size, sizeof(vkrt_node_update));
  if(u->memory != VKRT_MEMORY_HOST && u->memory != VKRT_MEMORY_DEVICE)
    return refuse(kBad, err, "%s: memory %u is neither VKRT_MEMORY_HOST nor VKRT_MEMORY_DEVICE", who, u->memory);
  if(u->node_indices && u->first != 0)
    return refuse(kBad, err, "%s: first is %u with node_indices given (a sparse update takes first = 0)", who, u->first);
  return VKRT_OK;
}

int check_node_update_range(const vkrt_node_update& u, size_t nodeCount, std::string& err)
{
  const char* who = kNodeUpdate;
  const size_t n = u.count;
  if(!u.node_indices)
    if(const int rc = check_node_range(who, u.first, u.count, nodeCount, err); rc != VKRT_OK)
      return rc;
  if(n && !u.world_matrices)
    return refuse(kBad, err, "%s: world_matrices is NULL", who);
  if(u.memory != VKRT_MEMORY_HOST)
  {
    if(((uintptr_t)u.world_matrices & 15u) != 0)
      return refuse(kBad, err, "%s: world_matrices %p is not 16-byte aligned", who, (const void*)u.world_matrices);
    if(((uintptr_t)u.node_indices & 3u) != 0)
      return refuse(kBad, err, "%s: node_indices %p is not 4-byte aligned", who, (const void*)u.node_indices);
    return VKRT_OK;
  }
  // the rules of vkrt_scene_update_nodes, checked for every entry before anything changes
  if(u.node_indices)
    for(size_t k = 0; k < n; k++)
      if(u.node_indices[k] >= nodeCount)
        return refuse(kBad, err, "%s: node_indices[%zu] is %u, outside the scene's %zu nodes", who, k, u.node_indices[k], nodeCount);
  for(size_t k = 0; k < 16 * n; k++)
    if(!std::isfinite(u.world_matrices[k]))
      return refuse(kBad, err, "%s: world_matrices[%zu] (entry %zu, node %u) is not finite", who, k, k / 16,
                    u.node_indices ? u.node_indices[k / 16] : u.first + (uint32_t)(k / 16));
  return VKRT_OK;
}

int check_visibility_values(const char* who, uint32_t count, const vkrt_instance_visibility* vis, std::string& err)
{
  if(count && !vis)
    return refuse(kBad, err, "%s: vis is NULL", who);
  for(uint32_t i = 0; i < count; i++)
  {
    if(vis[i].mask == 0)
      return refuse(kBad, err, "%s: entry %u: mask 0 (hide an instance from every ray with a zero-scale transform)", who, i);
    if(vis[i].flags & ~(VKRT_INSTANCE_FACING_CULL_DISABLE | VKRT_INSTANCE_FLIP_FACING))
      return refuse(kBad, err, "%s: entry %u: unknown flag bits 0x%x", who, i, (unsigned)vis[i].flags);
    if(vis[i].reserved != 0)
      return refuse(kBad, err, "%s: entry %u: reserved is not 0", who, i);
  }
  return VKRT_OK;
}

int check_alpha_values(const char* who, uint32_t count, const vkrt_material_alpha* alpha, std::string& err)
{
  if(count && !alpha)
    return refuse(kBad, err, "%s: alpha is NULL", who);
  for(uint32_t i = 0; i < count; i++)
  {
    if(alpha[i].mode != VKRT_ALPHA_OPAQUE && alpha[i].mode != VKRT_ALPHA_MASK)
      return refuse(kBad, err, "%s: entry %u: mode %u is neither VKRT_ALPHA_OPAQUE nor VKRT_ALPHA_MASK", who, i, alpha[i].mode);
    if(!std::isfinite(alpha[i].cutoff) || alpha[i].cutoff < 0.0f)
      return refuse(kBad, err, "%s: entry %u: cutoff %g is not a finite number >= 0", who, i, (double)alpha[i].cutoff);
  }
  return VKRT_OK;
}

int check_material_range(const char* who, uint32_t first, uint32_t count, uint32_t materialCount, std::string& err)
{
  if((uint64_t)first + count <= materialCount)
    return VKRT_OK;
  return refuse(kBad, err, "%s: materials [%u, %llu) outside the scene's %u materials", who, first, (unsigned long long)first + count, materialCount);
}

int check_light_update_desc(const vkrt_light_update* u, std::string& err)
{
  const char* who = "vkrt_scene_update_lights";
  if(!u)
    return refuse(kBad, err, "%s: update is NULL", who);
  if(u->struct_size < sizeof(vkrt_light_update))
    return refuse(kBad, err, "%s: vkrt_light_update.struct_size %u < %zu (ABI mismatch)", who, u->struct_size, sizeof(vkrt_light_update));
  if(u->memory != VKRT_MEMORY_HOST && u->memory != VKRT_MEMORY_DEVICE)
    return refuse(kBad, err, "%s: memory %u is neither VKRT_MEMORY_HOST nor VKRT_MEMORY_DEVICE", who, u->memory);
  return VKRT_OK;
}

int check_light_update_range(const vkrt_light_update& u, uint32_t lightCount, std::string& err)
{
  const char* who = "vkrt_scene_update_lights";
  if((uint64_t)u.first + u.count > lightCount)
    return refuse(kBad, err, "%s: lights [%u, %llu) outside the scene's %u lights", who, u.first, (unsigned long long)u.first + u.count, lightCount);
  if(u.count && !u.lights)
    return refuse(kBad, err, "%s: lights is NULL", who);
  if(u.memory != VKRT_MEMORY_HOST && ((uintptr_t)u.lights & 15u) != 0)
    return refuse(kBad, err, "%s: lights %p is not 16-byte aligned", who, (const void*)u.lights);
  return VKRT_OK;
}

int check_material_update_values(const char* who, uint32_t count, const GltfPBRMaterial* materials, uint32_t textureCount, std::string& err)
{
  if(count && !materials)
    return refuse(kBad, err, "%s: materials is NULL", who);
  if(textureCount > 0)
    for(uint32_t i = 0; i < count; i++)
    {
      const int32_t t[4] = {materials[i].pbrBaseColorTexture, materials[i].metallicRoughnessTexture, materials[i].normalTexture, materials[i].emissiveTexture};
      for(int k = 0; k < 4; k++)
        if(t[k] >= (int32_t)textureCount)
          return refuse(kBad, err, "%s: materials[%u]: texture index %d out of range (the scene has %u textures)", who, i, t[k], textureCount);
    }
  return VKRT_OK;
}

int check_texture_update_desc(const vkrt_texture_update* u, std::string& err)
{
  const char* who = "vkrt_scene_update_texture";
  if(!u)
    return refuse(kBad, err, "%s: update is NULL", who);
  if(u->struct_size < sizeof(vkrt_texture_update))
    return refuse(kBad, err, "%s: vkrt_texture_update.struct_size %u < %zu (ABI mismatch)", who, u->struct_size, sizeof(vkrt_texture_update));
  if(u->memory != VKRT_MEMORY_HOST && u->memory != VKRT_MEMORY_DEVICE)
    return refuse(kBad, err, "%s: memory %u is neither VKRT_MEMORY_HOST nor VKRT_MEMORY_DEVICE", who, u->memory);
  return VKRT_OK;
}

int check_texture_index(const char* who, uint32_t texture, uint32_t textureCount, std::string& err)
{
  return texture >= textureCount ? refuse(kBad, err, "%s: texture %u outside the scene's %u textures", who, texture, textureCount) : VKRT_OK;
}

int check_texture_update_image(const vkrt_texture_update& u, uint32_t width, uint32_t height, std::string& err)
{
  const char* who = "vkrt_scene_update_texture";
  if(u.width != width || u.height != height)
    return refuse(kBad, err, "%s: width x height %ux%u: texture %u is %ux%u (an update replaces the whole image)", who, u.width, u.height, u.texture, width, height);
  if(!u.rgba8)
    return refuse(kBad, err, "%s: rgba8 is NULL", who);
  if(u.memory != VKRT_MEMORY_HOST && ((uintptr_t)u.rgba8 & 15u) != 0)
    return refuse(kBad, err, "%s: rgba8 %p is not 16-byte aligned", who, (const void*)u.rgba8);
  return VKRT_OK;
}

int check_query_opts(const vkrt_query_opts* q, const char* who, std::string& err)
{
  if(!q)
    return refuse(kBad, err, "%s: opts is NULL", who);
  if(q->struct_size < sizeof(vkrt_query_opts))
    return refuse(kBad, err, "%s: vkrt_query_opts.struct_size %u < %zu (ABI mismatch)", who, q->struct_size, sizeof(vkrt_query_opts));
  const uint32_t known = VKRT_RAY_OPAQUE | VKRT_RAY_CULL_BACK_FACING | VKRT_RAY_CULL_FRONT_FACING;
  if(q->ray_flags & ~known)
    return refuse(kBad, err, "%s: ray_flags 0x%x has bits outside OPAQUE | CULL_BACK_FACING | CULL_FRONT_FACING", who, q->ray_flags);
  if((q->ray_flags & VKRT_RAY_CULL_BACK_FACING) && (q->ray_flags & VKRT_RAY_CULL_FRONT_FACING))
    return refuse(kBad, err, "%s: ray_flags: CULL_BACK_FACING and CULL_FRONT_FACING together", who);
  if(q->cull_mask > 0xFFu)
    return refuse(kBad, err, "%s: cull_mask 0x%x > 0xFF", who, q->cull_mask);
  return VKRT_OK;
}

int check_point_opts(const vkrt_query_opts* opts, const char* who, vkrt_query_opts& q, std::string& err)
{
  q = vkrt_query_opts{sizeof(vkrt_query_opts), 0u, 0xFFu, 0u};
  if(!opts)
    return VKRT_OK;
  if(const int rc = check_query_opts(opts, who, err); rc != VKRT_OK)
    return rc;
  if(opts->ray_flags != 0u)
    return refuse(kBad, err, "%s: ray_flags 0x%x: a point query takes no ray flag", who, opts->ray_flags);
  q = *opts;
  return VKRT_OK;
}

int check_max_hits(uint32_t maxHits, std::string& err)
{
  const bool bad = maxHits == 0u || maxHits > VKRT_MULTIHIT_MAX;
  return bad ? refuse(kBad, err, "vkrt_intersect_multi: max_hits %u outside 1..%d (VKRT_MULTIHIT_MAX)", maxHits, VKRT_MULTIHIT_MAX) : VKRT_OK;
}

int check_query_arrays(const char* who, uint32_t n, std::initializer_list<QueryArray> arrays, const char* alignText, std::string& err)
{
  if(n == 0)
    return VKRT_OK;
  for(const QueryArray& a : arrays)
    if(!a.p && !a.mayBeNull)
      return refuse(kBad, err, "%s: NULL array", who);
  for(const QueryArray& a : arrays)
    if(((uintptr_t)a.p & (a.align - 1u)) != 0u)
      return refuse(kBad, err, "%s: misaligned array %s", who, alignText);
  return VKRT_OK;
}

int check_shard(const vkrt_shard* shard, std::string& err)
{
  if(shard->full_width == 0 || shard->full_height == 0)
    return refuse(kBad, err, "empty launch size");
  if(shard->shard_count > 1 && (shard->strip_rows == 0 || shard->shard_index >= shard->shard_count))
    return refuse(kBad, err, "bad shard (strip_rows %u, %u of %u)", shard->strip_rows, shard->shard_index, shard->shard_count);
  return VKRT_OK;
}

int shard_tiles(const vkrt_shard* shard, uint32_t& tileCount, std::string& err)
{
  const uint64_t tiles = (uint64_t)((shard->full_width + 7) / 8) * ((vkrt_shard_rows(shard) + 7) / 8);
  if(tiles * 64 >= 0xFFFFFFFFull)
    return refuse(VKRT_ERR_UNSUPPORTED, err, "launch too large");
  tileCount = (uint32_t)tiles;
  return VKRT_OK;
}

int check_frame_count(uint32_t nFrames, int32_t firstFrame, std::string& err)
{
  return nFrames > 65536u || (int64_t)firstFrame + (int64_t)nFrames > 0x7fffffffll ? refuse(kBad, err, "n_frames %u out of range", nFrames) : VKRT_OK;
}

int check_lights_count(const char* what, int32_t lightsCount, uint32_t lightCount, std::string& err)
{
  return lightsCount < 0 || (uint32_t)lightsCount > lightCount ? refuse(kBad, err, "%s %d outside [0,%u]", what, lightsCount, lightCount) : VKRT_OK;
}

int check_samples_depth(const char* what, int32_t samples, int32_t depth, std::string& err)
{
  return samples < 0 || depth < 0 || depth > 99 ? refuse(kBad, err, "%s out of range", what) : VKRT_OK;
}

}  // namespace vkrt

extern "C" uint32_t vkrt_shard_rows(const vkrt_shard* sh)
{
  if(!sh)
    return 0;
  if(sh->strip_rows == 0 || sh->shard_count <= 1)
    return (sh->shard_count <= 1 || sh->shard_index == 0) ? sh->full_height : 0;
  const uint32_t strips = (sh->full_height + sh->strip_rows - 1) / sh->strip_rows;
  uint32_t rows = 0;
  for(uint32_t s = sh->shard_index; s < strips; s += sh->shard_count)
  {
    const uint32_t y0 = s * sh->strip_rows;
    rows += std::min(sh->strip_rows, sh->full_height - y0);
  }
  return rows;
}
