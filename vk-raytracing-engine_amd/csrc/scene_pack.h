// scene_pack.h -- what vkrt_scene_create does before it touches the device: the checks of a vkrt_scene_desc and the tables the kernels
// read, packed into plain vectors (scene_pack.cpp).  No HIP type: tests/test_scene_pack.py compiles it with g++.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/vkrt.h"
#include "scene_records.h"
#include "texture_pack.h"

namespace vkrt {

constexpr vkrt_material_alpha kDefaultAlpha = {VKRT_ALPHA_OPAQUE, 0.5f};  // glTF's defaults; the reference treats every material as opaque
constexpr vkrt_instance_visibility kDefaultVisibility = {0xFF, VKRT_INSTANCE_FACING_CULL_DISABLE, 0};  // the reference's TLAS (hello_vulkan.cpp:1040-1041)

// The tables of a scene in upload order of their device copies (DevScene names each)
struct PackedScene
{
  std::vector<float> vertexPN;             // VKRT_VERTEX_QUADS x 4 floats per vertex: (position, normal, uv, tangent) (rchit:41-66)
  std::vector<uint32_t> primMeshes;        // 4 words per primitive-mesh (DevSurfaceScene::primMeshes; rchit:34-40 per record)
  std::vector<DevInstance> instances;      // one per node, with kDefaultVisibility
  std::vector<DevMaterial> materials;      // with the descriptors of their textures folded in and kDefaultAlpha
  std::vector<DevShadeMaterial> shadeMaterials;
  std::vector<DevTexture> textures;
  std::vector<uint32_t> texMips;           // [texture][VKRT_MAX_MIPS]
  std::vector<uint32_t> texels;            // RGBA8 pool, every level (one white texel when the scene has no texture)
  std::vector<uint32_t> texQuads;          // footprint pool, 4 words per record; empty = the scene has none
  float srgbLut[512];
  // what an edit of the live scene needs besides (vkrt_scene_update_materials, vkrt_scene_update_texture): each texture's first record in
  // the footprint pool, and the thresholds of the sRGB encode (make_srgb_encode_table)
  std::vector<uint32_t> texQuadFirst;
  float srgbEncode[VKRT_SRGB_THRESHOLDS];
};

// node transforms: vkrt_scene_create and vkrt_scene_update_nodes refuse the same ones
int check_transform(const vkrt_node& n, uint32_t i, std::string& err);
// VKRT_OK, or VKRT_ERR_INVALID_ARGUMENT with the reason in err
int validate_scene(const vkrt_scene_desc* d, std::string& err);
// The tables of a validated scene.  texQuadsAllowed = false: no footprint pool (the VKRT_TEX_QUADS=0 test hook).  VKRT_ERR_UNSUPPORTED
// with the reason in err for a referenced texture side above 32768, a pool of 2^31 records and tables of 4 GiB.
int pack_scene(const vkrt_scene_desc* d, bool texQuadsAllowed, PackedScene& out, std::string& err);
// The DevMaterial and DevShadeMaterial of one material, with kDefaultAlpha: the same code at vkrt_scene_create (pack_scene calls it per
// material) and at vkrt_scene_update_materials, so that an updated record is bit for bit the one a scene created with the material gets.
// table: the scene's DevTexture records; quadFirst: each texture's first footprint record (read when wantQuads, the scene has that pool).
// An index outside [0, textureCount) makes the 1x1 invalid reference.  VKRT_ERR_UNSUPPORTED with the reason in err for a referenced
// texture side above 32768 and a base of 2^31 and more.
int make_material(const GltfPBRMaterial& m, const DevTexture* table, uint32_t textureCount, const uint32_t* quadFirst, bool wantQuads, DevMaterial& mat,
                  DevShadeMaterial& sm, std::string& err);
// The 8-bit code pack_scene gives a filtered linear colour value of an sRGB texture: powf, clamp, * 255 + 0.5, truncation
uint32_t srgb_encode_code(float v);
// T[0] = 0; T[q], q = 1..255: the smallest binary32 v >= 0 with srgb_encode_code(v) >= q, found by bisection over bit patterns.  The device
// quantises with these (texture_pack.h vkrt_srgb_quantise) instead of evaluating the curve
void make_srgb_encode_table(float T[VKRT_SRGB_THRESHOLDS]);
// gl_ObjectToWorldEXT / gl_WorldToObjectEXT of one node (rchit:72-76) and its ray-query visibility: the same code at vkrt_scene_create,
// vkrt_scene_update_nodes and vkrt_scene_set_instance_visibility, so that a moved scene's records are bit for bit those of a scene
// created with the moved nodes
void make_instance(const vkrt_node& node, const vkrt_instance_visibility& vis, DevInstance& in);
// World-space bounds of the instanced geometry, conservatively from the corners of every node's local box, and whether the scene has
// large triangles (the any-hit order heuristic asks whether a ray ends outside the bounds; nothing else reads them)
void scene_bounds(const std::vector<float>& positions, const std::vector<uint32_t>& indices, const std::vector<vkrt_prim_mesh>& primMeshes,
                  const std::vector<vkrt_node>& nodes, float lo[3], float hi[3], bool& hasLargeTriangles);

}  // namespace vkrt
