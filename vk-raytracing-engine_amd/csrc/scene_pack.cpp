// scene_pack.cpp -- host side of vkrt_scene_create (scene_pack.h): scene checks, the interleaved vertex records, instance records,
// the texel pool with its mip chains, the footprint pool and the material records.  Plain C++, nothing of the device.
#include "scene_pack.h"
#include "bvh_host.h"
#include "instance_record.h"
#include "texture_pack.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace vkrt {
namespace {

int fail(std::string& err, int code, const char* fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  err = buf;
  return code;
}

// Mip chain of one RGBA8 image as nvvk::cmdGenerateMipmaps builds it (hello_vulkan.cpp:496): level L is blitted from level
// L - 1 with VK_FILTER_LINEAR to max(1, size / 2).  vkCmdBlitImage semantics: destination texel centre x + 0.5 maps to the
// unnormalised source coordinate (x + 0.5) * srcSize / dstSize, filtered bilinearly around it with clamp-to-edge; an sRGB
// image is filtered in linear space and re-encoded.  Even sizes reduce to the 2x2 box average.
float srgbEncode(float c) { return c <= 0.0031308f ? 12.92f * c : 1.055f * powf(c, 1.0f / 2.4f) - 0.055f; }
void downsampleLevel(const uint32_t* src, uint32_t sw, uint32_t sh, uint32_t* dst, uint32_t dw, uint32_t dh, bool srgb, const float* lut512)
{
  // (the filter is texture_pack.h's, which k_se_mip runs on the device for vkrt_scene_update_texture; the encode is the curve itself)
  for(uint32_t y = 0; y < dh; y++)
    for(uint32_t x = 0; x < dw; x++)
    {
      float f[4];
      vkrt_mip_filter(src, sw, sh, dw, dh, x, y, srgb, lut512, f);
      uint32_t out = 0;
      for(int c = 0; c < 4; c++)
      {
        float v = f[c];
        if(srgb && c < 3) v = srgbEncode(v);
        v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
        out |= (uint32_t)(v * 255.0f + 0.5f) << (8 * c);
      }
      dst[(size_t)y * dw + x] = out;
    }
}

}  // namespace

int check_transform(const vkrt_node& n, uint32_t i, std::string& err)
{
  for(int k = 0; k < 16; k++)
    if(!std::isfinite(n.worldMatrix[k]))
      return fail(err, VKRT_ERR_INVALID_ARGUMENT, "node %u: worldMatrix[%d] is not finite", i, k);
  return VKRT_OK;
}

int validate_scene(const vkrt_scene_desc* d, std::string& err)
{
  const int bad = VKRT_ERR_INVALID_ARGUMENT;
  if(!d)
    return fail(err, bad, "desc is NULL");
  if(d->struct_size != sizeof(vkrt_scene_desc))
    return fail(err, bad, "vkrt_scene_desc.struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(vkrt_scene_desc));
  if(d->vertex_count && (!d->positions || !d->normals || !d->tangents || !d->texcoords0))
    return fail(err, bad, "vertex arrays missing");
  if(d->index_count && !d->indices)
    return fail(err, bad, "indices missing");
  if(d->material_count == 0 || !d->materials)
    return fail(err, bad, "at least one material is required (nvh::GltfScene appends a default one)");
  if(d->light_count == 0 || !d->lights)
    return fail(err, bad, "at least one light is required (hello_vulkan.cpp:247 adds 8 fallback lights)");
  if((d->prim_mesh_count && !d->prim_meshes) || (d->node_count && !d->nodes) || (d->texture_count && !d->textures))
    return fail(err, bad, "array pointer missing");
  for(uint32_t i = 0; i < d->prim_mesh_count; i++)
  {
    const vkrt_prim_mesh& p = d->prim_meshes[i];
    if((uint64_t)p.firstIndex + p.indexCount > d->index_count || (uint64_t)p.vertexOffset + p.vertexCount > d->vertex_count)
      return fail(err, bad, "primMesh %u: range outside the index/vertex arrays", i);
    if(p.materialIndex >= (int32_t)d->material_count)
      return fail(err, bad, "primMesh %u: materialIndex %d out of range", i, p.materialIndex);
    const uint32_t triIdx = (p.indexCount / 3) * 3;
    for(uint32_t k = 0; k < triIdx; k++)
      if(d->indices[p.firstIndex + k] >= p.vertexCount)
        return fail(err, bad, "primMesh %u: index %u >= vertexCount %u", i, d->indices[p.firstIndex + k], p.vertexCount);
  }
  for(uint32_t i = 0; i < d->node_count; i++)
  {
    if(d->nodes[i].primMesh < 0 || (uint32_t)d->nodes[i].primMesh >= d->prim_mesh_count)
      return fail(err, bad, "node %u: primMesh %d out of range", i, d->nodes[i].primMesh);
    if(check_transform(d->nodes[i], i, err) != VKRT_OK)
      return bad;
  }
  // the builders compare and quantise boxes: NaN / inf coordinates have no place in an acceleration structure (a Vulkan driver is
  // free to drop such triangles; here they are refused up front)
  for(size_t i = 0; i < (size_t)d->vertex_count * 3; i++)
    if(!std::isfinite(d->positions[i]))
      return fail(err, bad, "positions[%zu] (vertex %zu) is not finite", i, i / 3);
  for(uint32_t i = 0; i < d->material_count; i++)
  {
    const GltfPBRMaterial& m = d->materials[i];
    const int32_t t[4] = {m.pbrBaseColorTexture, m.metallicRoughnessTexture, m.normalTexture, m.emissiveTexture};
    for(int k = 0; k < 4; k++)
      if(t[k] >= (int32_t)d->texture_count && d->texture_count > 0)
        return fail(err, bad, "material %u: texture index %d out of range", i, t[k]);
  }
  for(uint32_t i = 0; i < d->texture_count; i++)
    if(!d->textures[i].rgba8 || d->textures[i].width == 0 || d->textures[i].height == 0)
      return fail(err, bad, "texture %u: empty", i);
  return VKRT_OK;
}

void make_instance(const vkrt_node& node, const vkrt_instance_visibility& vis, DevInstance& in)
{
  // (the arithmetic is instance_record.h's, which k_nu_transforms runs on the device for vkrt_scene_update_node_transforms)
  memset(&in, 0, sizeof in);
  vkrt_instance_rows(node.worldMatrix, in.o2w);
  vkrt_invert3x3_rows(in.o2w, in.w2o);
  in.primMesh = node.primMesh;
  in.vis = (uint32_t)vis.mask | ((uint32_t)vis.flags << 8) | vkrt_mirrored_bit(in.o2w);
}

uint32_t srgb_encode_code(float v)
{
  v = srgbEncode(v);
  v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
  return (uint32_t)(v * 255.0f + 0.5f);
}

void make_srgb_encode_table(float T[VKRT_SRGB_THRESHOLDS])
{
  // non-negative binary32 values order like their bit patterns: bisect on those.  The code of 0 is 0 and the code of 1 is 255, so every
  // q in 1..255 has a threshold in (0, 1]
  T[0] = 0.0f;
  for(uint32_t q = 1; q < VKRT_SRGB_THRESHOLDS; q++)
  {
    uint32_t lo = 0u, hi = 0x3f800000u;  // code(lo) < q <= code(hi)
    while(hi - lo > 1u)
    {
      const uint32_t mid = lo + (hi - lo) / 2u;
      float v;
      memcpy(&v, &mid, 4);
      (srgb_encode_code(v) >= q ? hi : lo) = mid;
    }
    memcpy(&T[q], &hi, 4);
  }
}

int make_material(const GltfPBRMaterial& m, const DevTexture* table, uint32_t textureCount, const uint32_t* quadFirst, bool wantQuads, DevMaterial& mat,
                  DevShadeMaterial& sm, std::string& err)
{
  memset(&mat, 0, sizeof mat);
  mat.m = m;
  mat.alphaMode = kDefaultAlpha.mode;
  mat.alphaCutoff = kDefaultAlpha.cutoff;
  memset(&sm, 0, sizeof sm);
  for(int k = 0; k < 3; k++)
  {
    sm.f[k] = mat.m.pbrBaseColorFactor[k];
    sm.f[5 + k] = mat.m.emissiveFactor[k];
  }
  sm.f[3] = mat.m.metallicFactor;
  sm.f[4] = mat.m.roughnessFactor;
  const int idx[4] = {mat.m.pbrBaseColorTexture, mat.m.metallicRoughnessTexture, mat.m.normalTexture, mat.m.emissiveTexture};
  for(int k = 0; k < 4; k++)
  {
    DevTexRef& r = mat.tex[k];
    r = DevTexRef{0u, 1u | (1u << 16), 0u, 0u};
    if(idx[k] >= 0 && (uint32_t)idx[k] < textureCount)
    {
      const DevTexture& t = table[(size_t)idx[k]];
      if(t.width == 0u || t.height == 0u || t.width > 32768u || t.height > 32768u)
        return fail(err, VKRT_ERR_UNSUPPORTED, "texture %d is %ux%u (supported: 1..32768 per side)", idx[k], t.width, t.height);
      r = DevTexRef{t.offset, t.width | (t.height << 16), 1u | ((t.srgb & 1u) ? 2u : 0u), wantQuads ? quadFirst[(size_t)idx[k]] : 0u};
    }
    // (the reference order of DevShadeMaterial is VKRT_TEXREF_*: BASE, MR, NORMAL, EMISSIVE = the order of idx[])
    const uint32_t base = wantQuads ? r.quads : r.offset;
    if(base >> 31)
      return fail(err, VKRT_ERR_UNSUPPORTED, "texture pool of 2^31 records and more is not supported");
    sm.ref[2 * k] = ((r.wh & 0xffffu) - 1u) | (idx[k] > -1 ? 1u << 15 : 0u) | (((r.wh >> 16) - 1u) << 16) | ((r.flags & 1u) << 31);
    sm.ref[2 * k + 1] = base | ((r.flags & 2u) << 30);
  }
  return VKRT_OK;
}

int pack_scene(const vkrt_scene_desc* d, bool texQuadsAllowed, PackedScene& out, std::string& err)
{
  // (normals / uv travel inside vertexPN; the ePrimLookup indirection of hello_vulkan.cpp:363-368 is resolved per triangle
  // at build time into triShade, so neither is uploaded in its raw form)
  out.vertexPN.resize((size_t)d->vertex_count * 4 * VKRT_VERTEX_QUADS);
  for(uint32_t v = 0; v < d->vertex_count; v++)
  {
    float* o = &out.vertexPN[(size_t)v * 4 * VKRT_VERTEX_QUADS];
    o[0] = d->positions[3 * (size_t)v]; o[1] = d->positions[3 * (size_t)v + 1]; o[2] = d->positions[3 * (size_t)v + 2];
    o[3] = d->normals[3 * (size_t)v]; o[4] = d->normals[3 * (size_t)v + 1]; o[5] = d->normals[3 * (size_t)v + 2];
    o[6] = d->texcoords0[2 * (size_t)v]; o[7] = d->texcoords0[2 * (size_t)v + 1];
    for(int k = 0; k < 4; k++) o[8 + k] = d->tangents[4 * (size_t)v + k];
  }
  out.primMeshes.resize((size_t)d->prim_mesh_count * 4);
  for(uint32_t m = 0; m < d->prim_mesh_count; m++)
  {
    const vkrt_prim_mesh& pm = d->prim_meshes[m];
    const uint32_t w[4] = {pm.firstIndex, pm.vertexOffset, pm.indexCount / 3u, (uint32_t)std::max(0, pm.materialIndex)};
    memcpy(&out.primMeshes[(size_t)m * 4], w, sizeof w);
  }
  out.instances.resize(d->node_count);
  for(uint32_t n = 0; n < d->node_count; n++)
    make_instance(d->nodes[n], kDefaultVisibility, out.instances[n]);
  // textures: RGBA8 pool + table + sRGB decode table
  float* lut = out.srgbLut;
  for(int i = 0; i < 256; i++)
  {
    const float c = (float)i / 255.0f;
    lut[i] = (c <= 0.04045f) ? c / 12.92f : powf((c + 0.055f) / 1.055f, 2.4f);
    lut[256 + i] = c;
  }
  std::vector<DevTexture>& table = out.textures;
  std::vector<uint32_t>&mipTable = out.texMips, &pool = out.texels, &quads = out.texQuads;
  table.resize(d->texture_count);
  mipTable.assign((size_t)d->texture_count * VKRT_MAX_MIPS, 0u);
  pool.clear();
  // footprint pool (DevScene::texQuads): 16 bytes per level-0 texel; built when it stays below 2 GiB and the caller allows it (without
  // it the path tracer gathers the four texels of a tap one by one, as it did up to round 3; same values either way)
  std::vector<uint32_t> quadFirst(d->texture_count, 0u);  // (kept in out.texQuadFirst)
  uint64_t quadTotal = 1;  // record 0 = white dummy (hits without a texture read it and discard it)
  for(uint32_t t = 0; t < d->texture_count; t++)
  {
    quadFirst[t] = (uint32_t)std::min<uint64_t>(quadTotal, 0xffffffffull);
    quadTotal += (uint64_t)d->textures[t].width * d->textures[t].height;
  }
  const bool wantQuads = quadTotal * 16ull < (2ull << 30) && texQuadsAllowed;
  quads.clear();
  if(wantQuads)
    quads.assign((size_t)quadTotal * 4, 0xffffffffu);
  for(uint32_t t = 0; t < d->texture_count; t++)
  {
    const vkrt_texture& tx = d->textures[t];
    const size_t n = (size_t)tx.width * tx.height;
    size_t at = pool.size();
    pool.resize(at + n);
    memcpy(&pool[at], tx.rgba8, n * 4);
    // (the footprints are texture_pack.h's, which k_se_level0 writes on the device, read from the pool's aligned copy of level 0)
    if(wantQuads)
      for(uint32_t y = 0; y < tx.height; y++)
        for(uint32_t x = 0; x < tx.width; x++)
          vkrt_footprint(&pool[at], tx.width, tx.height, x, y, &quads[((size_t)quadFirst[t] + (size_t)y * tx.width + x) * 4]);
    // the mip chain behind level 0 (sampled by the hybrid G-buffer's implicit-LOD texture(); the path tracer reads level 0)
    uint32_t levels = 1, w = tx.width, h = tx.height;
    mipTable[(size_t)t * VKRT_MAX_MIPS] = (uint32_t)at;
    while((w > 1 || h > 1) && levels < VKRT_MAX_MIPS)
    {
      const uint32_t dw = std::max(1u, w / 2), dh = std::max(1u, h / 2);
      const size_t to = pool.size();
      pool.resize(to + (size_t)dw * dh);
      downsampleLevel(&pool[at], w, h, &pool[to], dw, dh, tx.is_srgb != 0, lut);
      mipTable[(size_t)t * VKRT_MAX_MIPS + levels] = (uint32_t)to;
      at = to; w = dw; h = dh;
      levels++;
    }
    table[t] = DevTexture{mipTable[(size_t)t * VKRT_MAX_MIPS], tx.width, tx.height, (tx.is_srgb ? 1u : 0u) | (levels << 8)};
  }
  if(pool.empty())
    pool.push_back(0xffffffffu);  // shading always issues its texel loads (to texel 0 when a material has no texture)
  // materials, with the descriptors of their textures folded in (DevMaterial)
  out.materials.resize(d->material_count);
  out.shadeMaterials.resize(d->material_count);
  for(uint32_t i = 0; i < d->material_count; i++)
    if(const int rc = make_material(d->materials[i], table.data(), d->texture_count, quadFirst.data(), wantQuads, out.materials[i], out.shadeMaterials[i], err);
       rc != VKRT_OK)
      return rc;
  out.texQuadFirst = quadFirst;
  make_srgb_encode_table(out.srgbEncode);
  // the hit shader addresses its tables with 32-bit byte offsets (shade.h BufView): refuse what does not fit
  if((uint64_t)pool.size() * 4 >= (4ull << 30) || (uint64_t)d->vertex_count * VKRT_VERTEX_BYTES >= (4ull << 30) || (uint64_t)d->material_count * 128 >= (4ull << 30) ||
     (uint64_t)d->node_count * 96 >= (4ull << 30))
    return fail(err, VKRT_ERR_UNSUPPORTED, "scene tables of 4 GiB and more are not supported (texel pool %zu texels, %u vertices)", pool.size(), d->vertex_count);
  return VKRT_OK;
}

void scene_bounds(const std::vector<float>& positions, const std::vector<uint32_t>& indices, const std::vector<vkrt_prim_mesh>& primMeshes,
                  const std::vector<vkrt_node>& nodes, float sceneLo[3], float sceneHi[3], bool& hasLargeTriangles)
{
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  std::vector<float> meshBox(primMeshes.size() * 6);
  for(size_t m = 0; m < primMeshes.size(); m++)
  {
    const vkrt_prim_mesh& pm = primMeshes[m];
    float* b = &meshBox[m * 6];
    for(int k = 0; k < 3; k++) { b[k] = INFINITY; b[3 + k] = -INFINITY; }
    for(uint32_t v = 0; v < pm.vertexCount; v++)
      for(int k = 0; k < 3; k++)
      {
        const float x = positions[3 * (size_t)(pm.vertexOffset + v) + k];
        b[k] = std::min(b[k], x); b[3 + k] = std::max(b[3 + k], x);
      }
  }
  for(const vkrt_node& n : nodes)
  {
    const float* b = &meshBox[(size_t)n.primMesh * 6];
    if(!(b[0] <= b[3]))
      continue;
    for(int c = 0; c < 8; c++)
    {
      const float p[3] = {(c & 1) ? b[3] : b[0], (c & 2) ? b[4] : b[1], (c & 4) ? b[5] : b[2]};
      for(int k = 0; k < 3; k++)
      {
        const float w = n.worldMatrix[k] * p[0] + n.worldMatrix[4 + k] * p[1] + n.worldMatrix[8 + k] * p[2] + n.worldMatrix[12 + k];
        lo[k] = std::min(lo[k], w); hi[k] = std::max(hi[k], w);
      }
    }
  }
  for(int k = 0; k < 3; k++)
  {
    const float pad = 1e-3f * std::max(1e-6f, hi[k] - lo[k]);
    sceneLo[k] = lo[k] - pad; sceneHi[k] = hi[k] + pad;
  }
  // "large" = a triangle of more than 1 % of the largest face of the scene's box (world space, every instance)
  const double ex = (double)hi[0] - lo[0], ey = (double)hi[1] - lo[1], ez = (double)hi[2] - lo[2];
  const double face = std::max(ex * ey, std::max(ey * ez, ez * ex));
  double maxArea = 0.0;
  for(const vkrt_node& n : nodes)
  {
    const vkrt_prim_mesh& pm = primMeshes[(size_t)n.primMesh];
    const float* M = n.worldMatrix;
    for(uint32_t t = 0; t + 3 <= pm.indexCount; t += 3)
    {
      double w[3][3];
      for(int v = 0; v < 3; v++)
      {
        const float* p = &positions[3 * (size_t)(indices[pm.firstIndex + t + v] + pm.vertexOffset)];
        for(int k = 0; k < 3; k++) w[v][k] = (double)M[k] * p[0] + (double)M[4 + k] * p[1] + (double)M[8 + k] * p[2] + (double)M[12 + k];
      }
      const double a[3] = {w[1][0] - w[0][0], w[1][1] - w[0][1], w[1][2] - w[0][2]}, b[3] = {w[2][0] - w[0][0], w[2][1] - w[0][1], w[2][2] - w[0][2]};
      const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
      maxArea = std::max(maxArea, 0.5 * std::sqrt(cx * cx + cy * cy + cz * cz));
    }
  }
  hasLargeTriangles = face > 0.0 && maxArea > 0.01 * face;
}

}  // namespace vkrt
