// texture_pack.h -- the arithmetic of one texel of the texture tables, once, for the host (pack_scene in scene_pack.cpp) and for the device
// (k_se_level0, k_se_mip, k_se_mip_tail in scene_edit.hip): a texture that vkrt_scene_update_texture rebuilds on the device is bit for bit
// the one vkrt_scene_create packs from the same texels on the host.  Fixed-width integers and floats only, no HIP type: host-only code
// includes it (tests compile it with g++).
//
// Every operation below is IEEE binary32 in source order (the translation units that include this are built with -ffp-contract=off;
// binary32 division and the conversions are correctly rounded on either side), with one exception that is not arithmetic at all: the sRGB
// encode of a filtered value.  The host calls powf, which the device cannot reproduce bit for bit, so the device does not compute it: it
// looks the 8-bit result up in a table of thresholds that the host derived from its own function (vkrt_srgb_quantise below).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VKRT_TP_HD __host__ __device__ inline
#else
#define VKRT_TP_HD inline
#endif

#define VKRT_SRGB_THRESHOLDS 256  // T[0] = 0 (every value reaches code 0), T[q] for q = 1..255

// The footprint record of level-0 texel (x, y): the texels (x, y) (x+1, y) (x, y+1) (x+1, y+1) with REPEAT wrap-around
VKRT_TP_HD void vkrt_footprint(const uint32_t* src, uint32_t w, uint32_t h, uint32_t x, uint32_t y, uint32_t q[4])
{
  const uint32_t x1 = x + 1 == w ? 0 : x + 1, y1 = y + 1 == h ? 0 : y + 1;
  q[0] = src[(size_t)y * w + x];
  q[1] = src[(size_t)y * w + x1];
  q[2] = src[(size_t)y1 * w + x];
  q[3] = src[(size_t)y1 * w + x1];
}

// Texel (x, y) of a dw x dh level blitted from the sw x sh level before it, before quantisation: vkCmdBlitImage with VK_FILTER_LINEAR.
// The destination centre x + 0.5 maps to the unnormalised source coordinate (x + 0.5) * sw / dw, filtered bilinearly around it with
// clamp-to-edge; colour channels of an sRGB image are filtered on decoded values (lut512[0..255], lut512[256..511] is the UNORM ramp).
VKRT_TP_HD void vkrt_mip_filter(const uint32_t* src, uint32_t sw, uint32_t sh, uint32_t dw, uint32_t dh, uint32_t x, uint32_t y, bool srgb,
                                const float* lut512, float v[4])
{
  const float fu = ((float)x + 0.5f) * ((float)sw / (float)dw) - 0.5f, fv = ((float)y + 0.5f) * ((float)sh / (float)dh) - 0.5f;
  const float flx = floorf(fu), fly = floorf(fv), ax = fu - flx, ay = fv - fly;
  const int ix = (int)flx, iy = (int)fly, nx = (int)sw, ny = (int)sh;
  const int x0 = ix < 0 ? 0 : (ix >= nx ? nx - 1 : ix), x1 = ix + 1 < 0 ? 0 : (ix + 1 >= nx ? nx - 1 : ix + 1);
  const int y0 = iy < 0 ? 0 : (iy >= ny ? ny - 1 : iy), y1 = iy + 1 < 0 ? 0 : (iy + 1 >= ny ? ny - 1 : iy + 1);
  const uint32_t p[4] = {src[(size_t)y0 * sw + x0], src[(size_t)y0 * sw + x1], src[(size_t)y1 * sw + x0], src[(size_t)y1 * sw + x1]};
  for(int c = 0; c < 4; c++)
  {
    const uint32_t base = (srgb && c < 3) ? 0u : 256u;
    const float t00 = lut512[base + ((p[0] >> (8 * c)) & 255u)], t10 = lut512[base + ((p[1] >> (8 * c)) & 255u)];
    const float t01 = lut512[base + ((p[2] >> (8 * c)) & 255u)], t11 = lut512[base + ((p[3] >> (8 * c)) & 255u)];
    v[c] = (t00 * (1.0f - ax) + t10 * ax) * (1.0f - ay) + (t01 * (1.0f - ax) + t11 * ax) * ay;
  }
}

// a filtered UNORM value (alpha, and every channel of a linear image) as its 8-bit code
VKRT_TP_HD uint32_t vkrt_unorm_quantise(float v)
{
  v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
  return (uint32_t)(v * 255.0f + 0.5f);
}

// A filtered linear colour value as its 8-bit sRGB code without evaluating the curve: T[q] is the smallest binary32 v >= 0 whose code
// under the host's own encode (scene_pack.h srgb_encode_code: powf, clamp, * 255 + 0.5, truncation) is >= q, so the code of v is the
// number of q in 1..255 with v >= T[q] -- exactly, as long as the host's code is non-decreasing in v, which tests/test_scene_edit_pack.py
// checks over every binary32 value of [0, 1].  T is non-decreasing and T[0] = 0: eight comparisons find the last entry that v reaches.
// (A negative v, which the filter cannot produce from a table of non-negative values, gets code 0 like on the host.)
VKRT_TP_HD uint32_t vkrt_srgb_quantise(const float* T, float v)
{
  uint32_t q = 0;
  for(uint32_t step = VKRT_SRGB_THRESHOLDS / 2; step > 0; step >>= 1)
    q += v >= T[q + step] ? step : 0u;
  return q;
}

// texel (x, y) of a mip level as the device makes it, and as the host makes it up to the encode (pack_scene calls the curve itself)
VKRT_TP_HD uint32_t vkrt_mip_texel(const uint32_t* src, uint32_t sw, uint32_t sh, uint32_t dw, uint32_t dh, uint32_t x, uint32_t y, bool srgb,
                                   const float* lut512, const float* T)
{
  float v[4];
  vkrt_mip_filter(src, sw, sh, dw, dh, x, y, srgb, lut512, v);
  uint32_t out = vkrt_unorm_quantise(v[3]) << 24;
  for(int c = 0; c < 3; c++)
    out |= (srgb ? vkrt_srgb_quantise(T, v[c]) : vkrt_unorm_quantise(v[c])) << (8 * c);
  return out;
}
