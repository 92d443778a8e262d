// scene_records.h -- the scene records that vkrt_scene_create packs on the host (scene_pack.cpp) and the kernels read (device_scene.h
// includes this file).  Fixed-width integers, floats and GltfPBRMaterial only: no HIP type, so host-only code can fill them.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/vkrt_host_device.h"

// One TLAS instance (hello_vulkan.cpp:1035-1043): object->world rows + inverse 3x3 + primMesh.
struct DevInstance
{
  float o2w[12];  // row-major 3x4
  float w2o[9];   // row-major 3x3 inverse of the upper-left block
  int32_t primMesh;
  uint32_t vis;  // ray-query visibility (vkrt_scene_set_instance_visibility): bits 0-7 mask, bits 8-15 vkrt_instance_flags, VKRT_VIS_MIRRORED
  int32_t pad;
};
static_assert(sizeof(DevInstance) == 96, "DevInstance");
#define VKRT_VIS_CULL_DISABLE 0x100u  // VKRT_INSTANCE_FACING_CULL_DISABLE << 8
#define VKRT_VIS_FLIP 0x200u          // VKRT_INSTANCE_FLIP_FACING << 8
#define VKRT_VIS_MIRRORED 0x10000u    // the object->world 3x3 has a negative determinant (set on the host with the record)

// Shading-side repack (done once at upload; the API still takes the reference's SoA arrays):
// the per-CU L1/TA processes one 16-byte lane-load per tag lookup, so records are laid out for few,
// wide, aligned loads instead of the ~70 dword loads per hit that the raw SoA layout needs.
//   vertex  : 3 x float4 = (pos.xyz, nrm.x) (nrm.y, nrm.z, uv.x, uv.y) (tangent.xyzw): 48 bytes, one or two cache lines per vertex
//             (round 4: the tangent used to live in an array of its own, a third line per vertex)
//   material: 128 bytes = GltfPBRMaterial (52 B) padded to four aligned float4 + the descriptors of its four
//             textures (base colour, metallic-roughness, normal, emissive), so a hit reaches its texels in
//             one hop from the material record instead of two (no separate descriptor-table lookup)
#define VKRT_VERTEX_QUADS 3
#define VKRT_VERTEX_BYTES 48u
struct DevTexRef
{
  uint32_t offset;  // first texel in the RGBA8 pool (0 when invalid)
  uint32_t wh;      // width | height << 16 (1 | 1 << 16 when invalid)
  uint32_t flags;   // bit 0: index refers to an uploaded texture; bit 1: sRGB
  uint32_t quads;   // first record of the texture's level 0 in the footprint pool (DevScene::texQuads; 0 when invalid or no such pool)
};
#define VKRT_TEXREF_BASE 0
#define VKRT_TEXREF_MR 1
#define VKRT_TEXREF_NORMAL 2
#define VKRT_TEXREF_EMISSIVE 3
struct DevMaterial
{
  GltfPBRMaterial m;
  int32_t pad;
  uint32_t alphaMode;  // vkrt_alpha_mode (vkrt_scene_set_material_alpha); with alphaCutoff one aligned 8-byte load of the ray queries'
  float alphaCutoff;   // alpha-test stage (traverse.h alpha_ignores), which alone reads the two
  DevTexRef tex[4];
};
static_assert(sizeof(DevMaterial) == 128 && offsetof(DevMaterial, alphaMode) == 56, "DevMaterial");
// The hit shader's view of a material (shade.h closestHitFront): the factors raytrace.rchit reads and the four texture references
// in 64 bytes = four aligned 16-byte loads per hit (DevMaterial: eight).
//   f = (baseColor.xyz, metallic, roughness, emissive.xyz)   ref[2 k], ref[2 k + 1] = reference k (VKRT_TEXREF_*):
//   dims = (width - 1) | used << 15 | (height - 1) << 16 | valid << 31   (used: the material's texture index is > -1; valid: it
//          names an uploaded texture; an invalid reference has width = height = 1), sides up to 32768
//   base = first record of the texture in the footprint pool (DevScene::texQuads), or its first texel when the scene has no such
//          pool; | sRGB << 31
struct DevShadeMaterial
{
  float f[8];
  uint32_t ref[8];
};
static_assert(sizeof(DevShadeMaterial) == 64, "DevShadeMaterial");

#define VKRT_MAX_MIPS 16
struct DevTexture
{
  uint32_t offset;  // first texel of level 0 in the RGBA8 pool
  uint32_t width, height;
  uint32_t srgb;    // bit 0: sRGB; bits 8..: number of mip levels (>= 1); level offsets in DevScene::texMips
};
