// texel.h -- the texture() fetch of the hit group (bilinear, REPEAT, LOD 0: hello_vulkan.cpp:448-454) in the three steps shade.h issues
// it in, the buffer-descriptor loads they go through, and glTF's alpha on top of them (materialAlpha): what the hit shader (shade.h),
// vkrt_hit_surface (surface.hip) and the alpha-test stage of the ray-query walks (traverse.h alpha_ignores) share.
#pragma once
#include "device_math.h"
#include "device_scene.h"

struct f4 { float x, y, z, w; };

// Gathers of the hit shader go through buffer descriptors (four SGPRs built from a kernel-argument pointer) with a 32-bit byte
// offset per lane instead of a 64-bit flat address per lane: one VGPR per address instead of two.  The shader holds 16 texel
// addresses + 8 record addresses at its register peak (profiles/r04_experiments.md #114).  Every table is < 4 GiB (vkrt_scene_create refuses larger ones);
// the range check of the descriptor is left open (all ones): indices are validated at upload, as before.
typedef unsigned vkrt_v4u __attribute__((ext_vector_type(4)));
struct BufView { __amdgpu_buffer_rsrc_t r; };
VKRT_DEV BufView bufView(const void* p) { return BufView{__builtin_amdgcn_make_buffer_rsrc((void*)p, 0, (int)0xffffffffu, 0x00020000)}; }
VKRT_DEV float4 bufLoad4(BufView b, uint32_t byteOffset)
{
  const vkrt_v4u v = __builtin_amdgcn_raw_buffer_load_b128(b.r, (int)byteOffset, 0, 0);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
VKRT_DEV uint32_t bufLoad1(BufView b, uint32_t byteOffset) { return __builtin_amdgcn_raw_buffer_load_b32(b.r, (int)byteOffset, 0, 0); }

// i mod n in [0, n) for n > 0 (REPEAT addressing); power-of-two sizes take the mask path
VKRT_DEV int wrapi(int i, int n)
{
  if((n & (n - 1)) == 0)
    return i & (n - 1);
  int m = i % n;
  return m < 0 ? m + n : m;
}

// texture(): bilinear, REPEAT, LOD 0, RGBA8 UNORM / sRGB (hello_vulkan.cpp:448-454), split in three steps so a hit can
// issue the texel loads of all its textures back to back: footprint (addresses + weights), 4 loads, decode + blend.
struct TexTap
{
  uint32_t i00, i10, i01, i11;  // texel indices into the pool
  float ax, ay;
  uint32_t lutBase;             // 0: sRGB decode, 256: UNORM decode (rgb; alpha is always UNORM)
  bool white;                   // index out of range: 1x1 white dummy (hello_vulkan.cpp:468-472)
};
// first half: the weights, lutBase / white, and the wrapped texel (x0, y0) of the footprint's corner
VKRT_DEV void texFootprintOrigin(uint32_t width, uint32_t height, bool srgb, bool valid, float u, float v, TexTap& t, int& x0, int& y0)
{
  float fx = u * (float)width - 0.5f;
  float fy = v * (float)height - 0.5f;
  if(!(fabsf(fx) < 1.0e9f)) fx = 0.0f;
  if(!(fabsf(fy) < 1.0e9f)) fy = 0.0f;
  const float flx = floorf(fx), fly = floorf(fy);
  t.ax = fx - flx; t.ay = fy - fly;
  x0 = wrapi((int)flx, (int)width); y0 = wrapi((int)fly, (int)height);
  t.lutBase = srgb ? 0u : 256u;
  t.white = !valid;
}
// second half: the four texel indices of the footprint at (x0, y0), or texel 0 four times for a tap nobody wants
VKRT_DEV void texFootprintTexels(uint32_t offset, uint32_t width, uint32_t height, bool live, int x0, int y0, TexTap& t)
{
  const int w = (int)width, h = (int)height;
  const int x1 = x0 + 1 == w ? 0 : x0 + 1, y1 = y0 + 1 == h ? 0 : y0 + 1;
  const uint32_t r0 = offset + (uint32_t)y0 * width, r1 = offset + (uint32_t)y1 * width;
  t.i00 = live ? r0 + (uint32_t)x0 : 0u; t.i10 = live ? r0 + (uint32_t)x1 : 0u;
  t.i01 = live ? r1 + (uint32_t)x0 : 0u; t.i11 = live ? r1 + (uint32_t)x1 : 0u;
}
VKRT_DEV void texFootprint(uint32_t offset, uint32_t width, uint32_t height, bool srgb, bool valid, bool want, float u, float v, TexTap& t)
{
  int x0, y0;
  texFootprintOrigin(width, height, srgb, valid, u, v, t, x0, y0);
  texFootprintTexels(offset, width, height, want && valid, x0, y0, t);
}
VKRT_DEV f4 texelDecode(const float* lut, uint32_t p, uint32_t base)
{
  f4 o;
  o.x = lut[base + (p & 255u)]; o.y = lut[base + ((p >> 8) & 255u)]; o.z = lut[base + ((p >> 16) & 255u)];
  o.w = lut[256u + (p >> 24)];
  return o;
}
VKRT_DEV f4 texBlend(const float* lut, const TexTap& tp, uint32_t p00, uint32_t p10, uint32_t p01, uint32_t p11)
{
  f4 r;
  if(tp.white)
  {
    r.x = r.y = r.z = r.w = 1.0f;
    return r;
  }
  const f4 t00 = texelDecode(lut, p00, tp.lutBase), t10 = texelDecode(lut, p10, tp.lutBase);
  const f4 t01 = texelDecode(lut, p01, tp.lutBase), t11 = texelDecode(lut, p11, tp.lutBase);
  const float ax = tp.ax, ay = tp.ay, bx = 1.0f - ax, by = 1.0f - ay;
  r.x = (t00.x * bx + t10.x * ax) * by + (t01.x * bx + t11.x * ax) * ay;
  r.y = (t00.y * bx + t10.y * ax) * by + (t01.y * bx + t11.y * ax) * ay;
  r.z = (t00.z * bx + t10.z * ax) * by + (t01.z * bx + t11.z * ax) * ay;
  r.w = (t00.w * bx + t10.w * ax) * by + (t01.w * bx + t11.w * ax) * ay;
  return r;
}

// The texture coordinate raytrace.rchit:68-79 interpolates at barycentrics (u, v): b = (1 - u - v, u, v), each component
// (uv0 * b.x + uv1 * b.y) + uv2 * b.z in binary32 without contraction.  q0, q1, q2: the second quads of the three vertex records
// (nrm.y, nrm.z, uv.x, uv.y).
VKRT_DEV void texcoordAt(const float4 q0, const float4 q1, const float4 q2, const float u, const float v, float& tu, float& tv)
{
  const f3 b = mk3(1.0f - u - v, u, v);  // rchit:68
  tu = (q0.z * b.x + q1.z * b.y) + q2.z * b.z;
  tv = (q0.w * b.x + q1.w * b.y) + q2.w * b.z;
}

// glTF's alpha: pbrBaseColorFactor.a (DevMaterial; the hit shader's 64-byte record drops it) times the .a of the base colour tap, which
// is the tap closestHitFront takes (same footprint, same texels).  LAZY = false (vkrt_hit_surface): the tap is issued whether or not
// the material has the texture, exactly as closestHitFront issues it (a tap nobody wants reads record 0), so the two merge.  LAZY = true
// (the walks): a material without the texture returns after its two record loads.  The value is the same either way.
// A table as materialAlpha loads from it, 16 or 4 bytes at a byte offset: through a buffer descriptor (four SGPRs per table, one VGPR per
// address: the hit shader's way) or, PLAIN, through the table's pointer (the walks, which have no SGPRs to spare for four more descriptors)
template <bool PLAIN> struct TabView;
template <> struct TabView<false> { BufView b; };
template <> struct TabView<true> { const char* p; };
template <bool PLAIN>
VKRT_DEV TabView<PLAIN> tabView(const void* table)
{
  if constexpr(PLAIN)
    return TabView<true>{(const char*)table};
  else
    return TabView<false>{bufView(table)};
}
VKRT_DEV float4 tabLoad4(TabView<false> t, uint32_t byteOffset) { return bufLoad4(t.b, byteOffset); }
VKRT_DEV float4 tabLoad4(TabView<true> t, uint32_t byteOffset) { return *(const float4*)(t.p + byteOffset); }
VKRT_DEV uint32_t tabLoad1(TabView<false> t, uint32_t byteOffset) { return bufLoad1(t.b, byteOffset); }
VKRT_DEV uint32_t tabLoad1(TabView<true> t, uint32_t byteOffset) { return *(const uint32_t*)(t.p + byteOffset); }

template <bool LAZY>
VKRT_DEV float materialAlpha(const DevScene& sc, const uint32_t matIndex, const float tu, const float tv, const float* lut)
{
  const float factor = __uint_as_float(tabLoad1(tabView<LAZY>(sc.materials), 128u * matIndex + 12u));
  const float4 ref01 = tabLoad4(tabView<LAZY>(sc.shadeMaterials), 64u * matIndex + 32u);
  const uint32_t dimB = __float_as_uint(ref01.x), baseB = __float_as_uint(ref01.y);
  const bool wantB = (dimB & 0x8000u) != 0u;
  if(LAZY && !wantB)
    return factor;
  TexTap tB;
  texFootprint(sc.texQuads ? 0u : (baseB & 0x7fffffffu), (dimB & 0x7fffu) + 1u, ((dimB >> 16) & 0x7fffu) + 1u, (baseB >> 31) != 0u, (dimB >> 31) != 0u, wantB,
               tu, tv, tB);
  uint32_t c00, c10, c01, c11;
  if(sc.texQuads)
  {
    const uint32_t rec = (wantB && (dimB >> 31) != 0u) ? tB.i00 + (baseB & 0x7fffffffu) : 0u;
    const float4 q = tabLoad4(tabView<LAZY>(sc.texQuads), 16u * rec);
    c00 = __float_as_uint(q.x); c10 = __float_as_uint(q.y); c01 = __float_as_uint(q.z); c11 = __float_as_uint(q.w);
  }
  else
  {
    const TabView<LAZY> tex = tabView<LAZY>(sc.texels);
    c00 = tabLoad1(tex, 4u * tB.i00); c10 = tabLoad1(tex, 4u * tB.i10); c01 = tabLoad1(tex, 4u * tB.i01); c11 = tabLoad1(tex, 4u * tB.i11);
  }
  if(!wantB)
    return factor;
  return factor * texBlend(lut, tB, c00, c10, c01, c11).w;
}
