// rgen.h -- the ray-generation program (reference shaders/raytrace.rgen:24-146) as a per-path state
// machine shared by the megakernel (pathtrace.hip) and the wavefront kernels (wavefront.hip).
// One "path" = one pixel; its unit of work is one ray (closest-hit or shadow).
// Also the pixel front end of every frame kernel (pathtrace.hip, wavefront.hip, hybrid.hip): the tile-major work index -> pixel decode
// (pixelOfWork) and its inverse (pixelSlot), the seed index rule (pixelSeed), the camera origin and the lane setup of a pixel.
#pragma once
#include "device_math.h"
#include "device_scene.h"
#include "shade.h"

struct LaneState
{
  Payload prd;
  f3 curWeight, hitValue, hitValues;
  f3 camOrigin;
  uint32_t px;       // global pixel column (gl_LaunchIDEXT.x)
  uint32_t lrow;     // row in the shard-local buffer; gl_LaunchIDEXT.y = globalRow(P, lrow)
  int smpl;
  int stage;         // 0: next ray is the closest-hit ray, 1: next ray is the shadow ray
};

// shard-local row -> global row (include/vkrt.h vkrt_shard)
VKRT_DEV uint32_t globalRow(const TraceParams& P, uint32_t lrow)
{
  if(P.stripRows == 0u)
    return lrow;
  const uint32_t s = lrow / P.stripRows, r = lrow % P.stripRows;
  return (s * P.shardCount + P.shardIndex) * P.stripRows + r;
}

// Tile-major work index -> pixel.  Work item w of a launch belongs to the 8x8 tile tileFirst + w / 64 of the shard (tiles row by row,
// tilesX to a row) and to pixel w % 64 inside it (row by row): column x, shard-local row lrow, global row y.  false: w is past the
// launch's tiles, or the pixel of a partial tile lies outside the shard or the image.
VKRT_DEV bool pixelOfWork(const TraceParams& P, unsigned w, unsigned tileFirst, uint32_t& x, uint32_t& y, uint32_t& lrow)
{
  if(w >= P.tileCount * 64u)
    return false;
  const unsigned tile = tileFirst + (w >> 6), inTile = w & 63u;
  x = (tile % P.tilesX) * 8u + (inTile & 7u);
  lrow = (tile / P.tilesX) * 8u + (inTile >> 3);
  if(x >= P.fullW || lrow >= P.localRows)
    return false;
  y = globalRow(P, lrow);
  return y < P.fullH;
}
// ... and back: tile * 64 + inTile of pixel (x, lrow), its tile-major index in the shard (the pixel's sample-state record)
VKRT_DEV unsigned pixelSlot(const TraceParams& P, uint32_t x, uint32_t lrow)
{
  return (((lrow >> 3) * P.tilesX + (x >> 3)) << 6) | ((lrow & 7u) << 3) | (x & 7u);
}

// the index the pixel's random sequence is seeded with (raytrace.rgen:28, raytraceHybrid.rgen:55; flags bit 0: VKRT_TRACE_SEED_INDEX_ROW_MAJOR)
VKRT_DEV uint32_t pixelSeed(const TraceParams& P, uint32_t x, uint32_t y)
{
  const uint32_t index = (P.flags & 1u) ? (y * P.fullW + x) : (y * x + x);
  return tea(index, P.seed);
}

// raytrace.rgen:30 -- viewInverse * (0, 0, 0, 1) (launch-uniform; cheaper to recompute than to carry)
VKRT_DEV f3 cameraOrigin(const TraceParams& P)
{
  float origin[4];
  mat4MulVec4(P.viewInverse, 0.0f, 0.0f, 0.0f, 1.0f, origin);
  return mk3(origin[0], origin[1], origin[2]);
}

// raytrace.rgen:42-60 -- start sample `smpl` of the lane's pixel
VKRT_DEV void startSample(const TraceParams& P, LaneState& L)
{
  const float r1 = rnd(L.prd.seed);
  const float r2 = rnd(L.prd.seed);
  const float jx = P.pc.frame == 0 ? 0.5f : r1, jy = P.pc.frame == 0 ? 0.5f : r2;
  const float pcx = (float)L.px + jx, pcy = (float)globalRow(P, L.lrow) + jy;  // (the global row is only needed here: two integer
                                                                               //  divisions per sample when sharded, not per ray)
  const float inU = pcx / (float)P.fullW, inV = pcy / (float)P.fullH;
  const float dx = inU * 2.0f - 1.0f, dy = inV * 2.0f - 1.0f;
  float target[4], direction[4];
  mat4MulVec4(P.projInverse, dx, dy, 1.0f, 1.0f, target);
  const f3 tn = normalize3(mk3(target[0], target[1], target[2]));
  mat4MulVec4(P.viewInverse, tn.x, tn.y, tn.z, 0.0f, direction);
  L.prd.hitValue = mk3(0.0f);
  L.prd.rayOrigin = L.camOrigin;
  L.prd.rayDirection = mk3(direction[0], direction[1], direction[2]);
  L.prd.depth = 0;
  L.prd.weight = mk3(0.0f);
  L.curWeight = mk3(1.0f);
  L.hitValue = mk3(0.0f);
  L.stage = 0;
}

// raytrace.rgen:27-30 -- bind a pixel to the lane: what depends neither on the seed nor on the sum over the samples so far.
// prd.isSpecular is reset here for every sample the sample-synchronous schedule starts (k_wf_sample_init), while a pixel that walks
// through its samples at its own pace carries the bit of a sample's last segment into the next sample.  Nothing reads it there: at
// depth 0 the emission rule of the hit shader (`depth == 0 || isSpecular`, rchit:83) holds whatever the bit says and closestHitTail
// sets it on both of its branches; a miss leaves it alone but sets depth 100, which decides the shadow-ray test (rgen:79) by itself
// and ends the sample, so the bit reaches the next sample's depth 0 unread again.
VKRT_DEV void bindPixel(const TraceParams& P, LaneState& L, uint32_t x, uint32_t lrow)
{
  L.px = x; L.lrow = lrow;
  L.prd.isSpecular = false;
  L.prd.lightDist = 0.0f;
  L.prd.shadowRayDir = mk3(0.0f);
  L.camOrigin = cameraOrigin(P);
}

// raytrace.rgen:27-60 -- the first sample of pixel (x, y), y == globalRow(P, lrow)
VKRT_DEV void startPixel(const TraceParams& P, LaneState& L, uint32_t x, uint32_t y, uint32_t lrow)
{
  bindPixel(P, L, x, lrow);
  L.prd.seed = pixelSeed(P, x, y);
  L.hitValues = mk3(0.0f);
  L.smpl = 0;
  startSample(P, L);
}

// raytrace.rgen:120,136-145 -- resolve and store the pixel
VKRT_DEV void storePixel(const TraceParams& P, const LaneState& L)
{
  const f3 res = L.hitValues / (float)P.pc.samples;
  float4* dst = (float4*)P.image + ((size_t)L.lrow * P.fullW + L.px);
  if(P.pc.frame > 0 && !(P.flags & VKRT_FLAG_STORE_STAGED))  // (a frame in flight leaves `res` in its staging plane; blendPixel follows in frame order)
  {
    const float a = 1.0f / (float)(P.pc.frame + 1);
    const float4 old = *dst;
    const f3 m = glsl_mix(mk3(old.x, old.y, old.z), res, a);
    *dst = make_float4(m.x, m.y, m.z, 1.0f);
  }
  else
    *dst = make_float4(res.x, res.y, res.z, 1.0f);
}

// raytrace.rgen:136-145 for a pixel whose value `res` was staged (frames in flight): same operations as storePixel's
VKRT_DEV void blendPixel(float4* dst, float4 staged, int frame)
{
  if(frame > 0)
  {
    const float a = 1.0f / (float)(frame + 1);
    const float4 old = *dst;
    const f3 m = glsl_mix(mk3(old.x, old.y, old.z), mk3(staged.x, staged.y, staged.z), a);
    *dst = make_float4(m.x, m.y, m.z, 1.0f);
  }
  else
    *dst = make_float4(staged.x, staged.y, staged.z, 1.0f);
}

// After the closest-hit ray of the current segment: run rchit / rmiss (raytrace.rgen:64-75).
// Returns true when a shadow ray has to be traced before the segment can be accumulated (rgen:79).
// `ts`: the hit triangle's shading record (sc.triShade[hit.slot]); ignored on a miss.
VKRT_DEV bool afterClosestRay(const TraceParams& P, LaneState& L, const RayHit& hit, const uint4 ts, f3 rayDir, ShadeStats& st)
{
  if(hit.slot >= 0)
    closestHitShader(P.sc, P.pc, hit, ts, rayDir, L.prd, st);
  else
    missShader(P.pc, L.prd);
  if(!L.prd.isSpecular && L.prd.depth != 100u)
  {
    L.stage = 1;
    return true;
  }
  return false;
}

// raytrace.rgen:99-102,115 -- the two products of a finished segment: its clamped radiance contribution and the path
// weight after it.  Split from the bookkeeping below so the wavefront pipeline can carry (contrib, nextWeight) across
// the shadow ray instead of (prd.hitValue, curWeight, prd.weight); the float operations are the same.
VKRT_DEV void segmentTerms(const Payload& prd, f3 curWeight, f3& contrib, f3& nextWeight)
{
  const f3 q = prd.hitValue * curWeight;
  contrib = mk3(glsl_min(q.x, 10.0f), glsl_min(q.y, 10.0f), glsl_min(q.z, 10.0f));
  nextWeight = curWeight * prd.weight;
}

// raytrace.rgen:99-120 -- accumulate the segment, advance depth / sample, up to the point where the next sample would start.
enum SegmentStep
{
  SEG_PIXEL_DONE = 0,  // the pixel is complete (its value has been stored)
  SEG_CONTINUE = 1,    // the sample goes on with its next segment
  SEG_SAMPLE_END = 2   // the sample is in hitValues and smpl names the next one, which the caller starts (startSample)
};
VKRT_DEV SegmentStep stepSegment(const TraceParams& P, LaneState& L, bool shadowHit, f3 contrib, f3 nextWeight)
{
  L.stage = 0;
  if(!shadowHit)  // rgen:99-102
    L.hitValue = L.hitValue + contrib;
  L.curWeight = nextWeight;  // rgen:115
  L.prd.depth++;
  if(L.prd.depth < (uint32_t)P.pc.depth)
    return SEG_CONTINUE;
  L.hitValues = L.hitValues + L.hitValue;
  L.smpl++;
  if(L.smpl < P.pc.samples)
    return SEG_SAMPLE_END;
  storePixel(P, L);
  return SEG_PIXEL_DONE;
}

// stepSegment for a path that walks through its samples at its own pace: the next sample starts at once.  Returns false when the
// pixel is complete (its value has been stored).
VKRT_DEV bool advanceSegment(const TraceParams& P, LaneState& L, bool shadowHit, f3 contrib, f3 nextWeight)
{
  const SegmentStep step = stepSegment(P, L, shadowHit, contrib, nextWeight);
  if(step == SEG_SAMPLE_END)
    startSample(P, L);
  return step != SEG_PIXEL_DONE;
}

VKRT_DEV bool accumulateAndAdvance(const TraceParams& P, LaneState& L, bool shadowHit)
{
  f3 contrib, nextWeight;
  segmentTerms(L.prd, L.curWeight, contrib, nextWeight);
  return advanceSegment(P, L, shadowHit, contrib, nextWeight);
}
