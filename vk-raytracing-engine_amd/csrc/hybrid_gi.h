// hybrid_gi.h -- the GI path of the hybrid mode (raytraceHybrid.rgen:172-282) and the pixel's store (:266-282, :36-48) for the two
// places that run it: k_hybrid's in-kernel loop (hybrid.hip; megakernel mode) and the wavefront streams (k_hy_gi_init and the HYBRID
// shade functions, wavefront.hip; the default).  That the two are the same function of the pixel, bit for bit, is a tested contract
// (tests/test_hybrid.py): every rule of the path has its one definition here, compiled into both translation units.
#pragma once
#include "device_math.h"
#include "device_scene.h"
#include "kernels.h"  // HybridGi
#include "rgen.h"
#include "shade.h"

// What raytraceHybrid.rgen reads of a pixel from the G-buffer (:57-78)
struct GbufferPixel
{
  f3 worldPos, worldNrm, albedo;
  float roughness, metalness;
  bool shaded;  // rgen:67 -- position and normal all zero: the raster pass's clear values, nothing to light
};
VKRT_DEV GbufferPixel loadGbufferPixel(const HybridGi& G, size_t p)
{
  const float4 pixelImg = G.color[p], pixelPos = G.position[p], pixelNorm = G.normal[p];
  const float2 rm = G.rough[p];
  GbufferPixel g;
  g.worldPos = mk3(pixelPos.x, pixelPos.y, pixelPos.z); g.worldNrm = mk3(pixelNorm.x, pixelNorm.y, pixelNorm.z);
  g.shaded = !(g.worldPos.x == 0.0f && g.worldPos.y == 0.0f && g.worldPos.z == 0.0f && g.worldNrm.x == 0.0f && g.worldNrm.y == 0.0f &&
               g.worldNrm.z == 0.0f);
  g.albedo = mk3(pixelImg.w, pixelPos.w, pixelNorm.w);
  g.roughness = rm.x; g.metalness = rm.y;
  return g;
}

// rgen:172-204 -- the first ray of a shaded pixel's GI path into prd (whose seed is the pixel's, after the direct part) and the
// path weight it starts with: a hemisphere sample weighted by the albedo, or the mirror reflection of the view ray
VKRT_DEV void giFirstRay(const TraceParams& P, const GbufferPixel& g, Payload& prd, f3& curWeight)
{
  f3 direction;
  const float ratio = g.metalness * (1.0f - g.roughness);
  if(ratio < 0.8f)
  {
    prd.isSpecular = false;
    f3 tangent, binormal;
    createCoordinateSystem(g.worldNrm, tangent, binormal);
    direction = normalize3(samplingHemisphere(prd.seed, tangent, binormal, g.worldNrm));
    curWeight = g.albedo;
  }
  else
  {
    prd.isSpecular = true;
    const f3 V = normalize3(cameraOrigin(P) - g.worldPos);
    direction = normalize3(glsl_reflect(-V, g.worldNrm));
    curWeight = mk3(1.0f);
  }
  prd.hitValue = mk3(0.0f);
  prd.rayOrigin = g.worldPos;
  prd.rayDirection = direction;
  prd.depth = 1;
  prd.weight = mk3(0.0f);
}

// rgen:240-266 -- one finished segment of the GI path: (contrib, nextWeight) are its segmentTerms, lightDist the length of its
// shadow ray (read for a diffuse segment at depth 1 only, which always traced one: rgen:253-264).  false: the path is complete.
VKRT_DEV bool giSegmentStep(const PushConstantRay& pc, Payload& prd, f3& curWeight, f3& hitValue, float& hitDists, bool shadowHit, f3 contrib,
                            f3 nextWeight, float lightDist)
{
  if(!shadowHit)
    hitValue = hitValue + contrib;
  if(prd.depth == 1u && !prd.isSpecular)
    hitDists = shadowHit ? 0.5f * lightDist : lightDist;
  curWeight = nextWeight;
  prd.depth++;
  return prd.depth < (uint32_t)pc.depth;
}

// rgen:266-282 + 36-48 -- the pixel's value is complete: (hitValue, alpha) into the accumulation image and, for a pixel whose GI
// path ran (`gi`: shaded, useGI), the REBLUR front-end record of its radiance and hit distance
VKRT_DEV void hybridStorePixel(const TraceParams& P, const HybridGi& G, size_t p, bool gi, f3 hitValue, float hitDists, float alpha)
{
  float4 color = make_float4(0.0f, 0.0f, 0.0f, alpha);
  if(gi)
  {
    color.x = hitValue.x; color.y = hitValue.y; color.z = hitValue.z;
    if(G.nrdRadHitD)
    {  // rgen:273-281: hitDistParams (3, 1, 20, -25), rgba16f store
      const float roughness = G.rough[p].x;
      const float viewZ = G.nrdViewZ[p];
      const float t = glsl_clamp(exp2f(-25.0f * roughness * roughness), 0.0f, 1.0f);
      const float f = (3.0f + fabsf(viewZ) * 1.0f) * (1.0f * (1.0f - t) + 20.0f * t);
      float normHitDist = glsl_clamp(hitDists / f, 0.0f, 1.0f);
      f3 rad = hitValue;
      const bool bad = isnan(rad.x) || isnan(rad.y) || isnan(rad.z) || isinf(rad.x) || isinf(rad.y) || isinf(rad.z);
      rad = bad ? mk3(0.0f) : mk3(glsl_clamp(rad.x, 0.0f, 65504.0f), glsl_clamp(rad.y, 0.0f, 65504.0f), glsl_clamp(rad.z, 0.0f, 65504.0f));
      normHitDist = (isnan(normHitDist) || isinf(normHitDist)) ? 0.0f : glsl_clamp(normHitDist, 0.0f, 1.0f);
      if(normHitDist != 0.0f)
        normHitDist = glsl_max(normHitDist, 1e-7f);
      const float Y = (rad.x * 0.25f + rad.y * 0.5f) + rad.z * 0.25f;
      const float Co = (rad.x * 0.5f + rad.y * 0.0f) + rad.z * -0.5f;
      const float Cg = (rad.x * -0.25f + rad.y * 0.5f) + rad.z * -0.25f;
      G.nrdRadHitD[p] = make_float4(quantizeHalf(Y), quantizeHalf(Co), quantizeHalf(Cg), quantizeHalf(normHitDist));
    }
  }
  if(P.pc.frame > 0)  // accumulateFrames, rgen:36-48 (all four channels)
  {
    const float a = 1.0f / (float)(P.pc.frame + 1);
    const float4 old = G.accum[p];
    G.accum[p] = make_float4(old.x * (1.0f - a) + color.x * a, old.y * (1.0f - a) + color.y * a, old.z * (1.0f - a) + color.z * a,
                             old.w * (1.0f - a) + color.w * a);
  }
  else
    G.accum[p] = color;
}
