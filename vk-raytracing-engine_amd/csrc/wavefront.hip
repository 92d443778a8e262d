// wavefront.hip -- the path-trace dispatch as a wavefront pipeline (default execution mode).
// Replaces vkCmdTraceRaysKHR(W,H,1) over raytrace.rgen/.rchit/.rmiss/raytraceShadow.rmiss
// (reference hello_vulkan.cpp:1446) exactly like pathtrace.hip, with the same per-path state machine
// (rgen.h) and therefore the same results; the work is re-scheduled for gfx950:
//
//   k_wf_init          one thread per pixel, in tile order like every per-pixel kernel here (rgen.h pixelOfWork): rgen prologue
//                      (seed, camera ray of sample 0) -> closest-ray stream.
//   k_wf_traverse      one thread per queued ray, batch-synchronous: the 64 rays of a wave start together, so the
//                      top tree levels are fetched as coalesced/broadcast loads; lanes that finish early take over
//                      pending subtrees of their neighbours (traverse_share.h).  Workgroups are one wave and
//                      homogeneous in ray kind: closest-hit rays first (rgen:64-75), then shadow rays (rgen:85-97, any-hit).
//                      Per-lane stacks in LDS.  Software stand-in for traceRayEXT.
//   k_wf_shade         one launch for the three result streams: rchit / rmiss, the segment accumulation (rgen:99-120),
//                      the next ray(s) of the path.
//
// Path records MOVE with their queue position: a round reads the records of its input streams front to back
// and every surviving path writes its new record at the position a block-aggregated ballot compaction assigns
// it in the next round's stream (ping-pong buffers).  All record traffic is therefore sequential; the state is
// kept as structure-of-arrays planes of float4, so the 64 lanes of a wave read 1 KB contiguous per plane.
// (The first version kept records in place and queued path ids: every record access was a random 16-byte gather
// and the shade kernels ran at memory-system throughput, r01_experiments.md #24.)
//
// Three streams (round 2).  The shadow ray of a diffuse segment and the closest-hit ray of the NEXT segment start at the same
// point and neither needs the other's result: only the accumulation `hitValue += contrib` (rgen:99-102) waits for the shadow
// ray.  A diffuse hit that is not the last segment of its sample therefore emits ONE "pair" record carrying both rays; they
// are traced in the same round and the next shade step first finishes segment k (accumulate, weight, depth++), then shades
// segment k+1's hit.  The rays traced, their order per path and every float operation are those of rgen's loop; only the
// round in which a ray is traced changes.  A frame needs samples * (depth + 1) rounds instead of 2 * samples * depth
// (144 instead of 256 on the bench workload), each with ~1.8x the rays, and a diffuse segment moves ~35 % fewer record bytes
// (one record instead of a shadow record followed by a closest record).
//
// The launches of a frame are enqueued back to back; stream counts stay on the device (no host synchronisation inside a frame).
// How many rounds a frame has, what each of its steps launches in the three schedules and how the frames of a call are dealt to
// lanes is decided in wf_schedule.h, which the host half of this file only carries out.
//
// Sample-synchronous schedule (VKRT_OPT_WF_SAMPLE_SYNC, VKRT_FLAG_SAMPLE_SYNC).  A sample takes at most depth + 1 rounds, so the
// round count above already lets every pixel of a frame trace sample s in the rounds [s (depth + 1), (s + 1) (depth + 1)): a path
// whose sample ends leaves (hitValues, seed) in its pixel's sample-state record instead of starting the next sample at once, and
// k_wf_sample_init starts sample s of ALL pixels in front of round s (depth + 1), in tile order like k_wf_init.  The camera rays of
// a sample are then traced as whole 8x8 tiles per wave instead of scattered among bounce rays of every depth, and their hits are
// shaded 64 neighbouring pixels to a wave.  Paths, random draws and float operations are those of the other schedule (option 0:
// pixels walk through their samples at their own pace); only the round in which a ray is traced changes.
//
// Camera rounds (VKRT_OPT_WF_CAMERA_ROUNDS, VKRT_FLAG_CAMERA_ROUNDS; the default where the sharing wave runs).  In that schedule the
// streams are empty in front of a sample's first round -- the round before it traced the last shadow rays of the previous sample and
// its shade step emitted nothing -- so the round holds camera rays only, one per pixel, and everything in their records but the hit
// follows from the pixel index, the launch constants and the sample state.  The record is therefore never written:
//
//   k_wf_traverse_camera   (wf_traverse.hip) one wave per 8x8 tile: pixel -> sample state (sample 0: the pixel's seed) -> bindPixel +
//                          startSample -> the walk of k_wf_traverse -> H0 / H1 at the pixel's slot of the C stream.
//   k_wf_shade_camera      one thread per pixel: the same state again, H0 / H1, then the code of k_wf_shade's C workgroups.
//
// A frame then has no k_wf_init and no k_wf_sample_init (wf_schedule.h wfStep).  Per pixel and sample the first round moves 96 B
// (traversal: 16 in, 32 out; shade: 16 + 32 in) instead of 256 B (init: 16 in, 80 out; traversal: 32 in, 32 out; shade: 96 in), and
// the frame has `samples` launches fewer.  Same functions, draws and float operations: only where a value comes from changes.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "device_math.h"
#include "device_scene.h"
#include "kernels.h"
#include "rgen.h"
#include "hybrid_gi.h"
#include "shade.h"
#include "traverse.h"
#include "traverse_wide.h"
#include "traverse_share.h"

#define WF_BLOCK 256
#define VKRT_FLAG_COUNT_WORK 2u  // = VKRT_TRACE_COUNT_TRAVERSAL (include/vkrt.h)

#include "wf_streams.h"

VKRT_DEV unsigned packFlags(const LaneState& L)
{
  return (L.prd.depth & 0xffu) | (((unsigned)L.smpl & 0xffffu) << 8) | ((L.prd.isSpecular ? 1u : 0u) << 25);
}

// state common to all streams (S0..S2) -> lane
VKRT_DEV void loadCommon(const TraceParams& P, const WfBuffers& B, int parity, int type, unsigned i, LaneState& L)
{
  const float4 s0 = wfLoad(rec(B, parity, type, WF_S0, i)), s1 = wfLoad(rec(B, parity, type, WF_S1, i)), s2 = wfLoad(rec(B, parity, type, WF_S2, i));
  const unsigned flags = __float_as_uint(s1.w), pix = __float_as_uint(s2.w);
  L.curWeight = mk3(s0.x, s0.y, s0.z); L.prd.seed = __float_as_uint(s0.w);
  L.hitValue = mk3(s1.x, s1.y, s1.z);
  L.prd.depth = flags & 0xffu; L.smpl = (int)((flags >> 8) & 0xffffu);
  L.prd.isSpecular = ((flags >> 25) & 1u) != 0u;
  L.hitValues = mk3(s2.x, s2.y, s2.z);
  L.px = pix & 0xffffu; L.lrow = pix >> 16;
  L.camOrigin = cameraOrigin(P);
  L.prd.lightDist = 0.0f;
  L.prd.shadowRayDir = mk3(0.0f);
  L.prd.hitValue = mk3(0.0f);
  L.prd.weight = mk3(0.0f);
  L.stage = 0;
}

VKRT_DEV void storeState(const WfBuffers& B, int parity, int type, unsigned i, const LaneState& L, f3 weight)
{
  wfStore(rec(B, parity, type, WF_S0, i), make_float4(weight.x, weight.y, weight.z, __uint_as_float(L.prd.seed)));
  wfStore(rec(B, parity, type, WF_S1, i), make_float4(L.hitValue.x, L.hitValue.y, L.hitValue.z, __uint_as_float(packFlags(L))));
  wfStore(rec(B, parity, type, WF_S2, i), make_float4(L.hitValues.x, L.hitValues.y, L.hitValues.z, __uint_as_float(L.px | (L.lrow << 16))));
}

// a path whose next ray is the closest-hit ray (rgen:64-75) -> slot i of stream C
VKRT_DEV void storeClosest(const WfBuffers& B, int parity, unsigned i, const LaneState& L)
{
  wfStore(rec(B, parity, WF_C, WF_R0, i), make_float4(L.prd.rayOrigin.x, L.prd.rayOrigin.y, L.prd.rayOrigin.z, 10000.0f));
  wfStore(rec(B, parity, WF_C, WF_R1, i), make_float4(L.prd.rayDirection.x, L.prd.rayDirection.y, L.prd.rayDirection.z, 0.0f));
  storeState(B, parity, WF_C, i, L, L.curWeight);
}

// a path waiting for the shadow ray of its current segment (rgen:85-97) -> slot i of stream S (last segment of the sample)
// or, with the closest-hit ray of the next segment riding along, of stream P
VKRT_DEV void storeShadow(const WfBuffers& B, int parity, int type, unsigned i, const LaneState& L, f3 contrib, f3 nextWeight)
{
  wfStore(rec(B, parity, type, WF_R0, i), make_float4(L.prd.rayOrigin.x, L.prd.rayOrigin.y, L.prd.rayOrigin.z, L.prd.lightDist - 0.1f));
  wfStore(rec(B, parity, type, WF_R1, i), make_float4(L.prd.shadowRayDir.x, L.prd.shadowRayDir.y, L.prd.shadowRayDir.z, L.prd.lightDist));
  if(type == WF_P)
    wfStore(rec(B, parity, type, WF_R2, i), make_float4(L.prd.rayDirection.x, L.prd.rayDirection.y, L.prd.rayDirection.z, 0.0f));
  storeState(B, parity, type, i, L, nextWeight);
  wfStore(rec(B, parity, type, WF_S3, i), make_float4(contrib.x, contrib.y, contrib.z, 0.0f));
}

// rgen:99-120 for a segment of the path tracer that is complete (no shadow ray, or the ray is back): the stream the path's next
// record goes to -- WF_C, or -1 when the pixel is stored or, in the sample-synchronous schedule, waits for k_wf_sample_init
VKRT_DEV int finishSegment(const TraceParams& P, const WfBuffers& B, LaneState& L, bool shadowHit, f3 contrib, f3 nextWeight)
{
  const SegmentStep step = stepSegment(P, L, shadowHit, contrib, nextWeight);
  if(step == SEG_SAMPLE_END)
  {
    if(P.flags & VKRT_FLAG_SAMPLE_SYNC)  // launch-uniform
    {
      wfStore(B.sampleState + pixelSlot(P, L.px, L.lrow), make_float4(L.hitValues.x, L.hitValues.y, L.hitValues.z, __uint_as_float(L.prd.seed)));
      return -1;
    }
    startSample(P, L);
  }
  return step == SEG_PIXEL_DONE ? -1 : WF_C;
}

// Block-aggregated slot assignment in the next round's streams: ballot + popcount inside each wave, wave totals
// combined through LDS, ONE global atomic per workgroup and stream (the count is a single word: per-wave atomics
// serialise near 88/us, MI355X_MICROARCH.md "dequeue").  Must be called by every thread of the block; `to` = the stream the
// thread's path goes to (WF_C / WF_S / WF_P) or -1; returns its slot there.  The slots of a block are contiguous per stream,
// in lane order.  wsum: LDS [WF_TYPES * (nw + 1)].
VKRT_DEV unsigned claimSlots(const WfBuffers& B, int parity, int to, unsigned lane, unsigned* wsum)
{
  const unsigned wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const unsigned long long m[WF_TYPES] = {__ballot(to == WF_C), __ballot(to == WF_S), __ballot(to == WF_P)};
  if(lane == 0)
  {
#pragma unroll
    for(int t = 0; t < WF_TYPES; t++) wsum[t * (nw + 1) + wave] = (unsigned)__popcll(m[t]);
  }
  __syncthreads();
  if(threadIdx.x < WF_TYPES)
  {
    unsigned* w = wsum + threadIdx.x * (nw + 1);
    unsigned tot = 0;
    for(unsigned k = 0; k < nw; k++)
    {
      const unsigned c = w[k];
      w[k] = tot;
      tot += c;
    }
    w[nw] = tot ? atomicAdd(countOf(B, parity, (int)threadIdx.x), tot) : 0u;
  }
  __syncthreads();
  if(to < 0)
    return 0u;
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long mine = to == WF_C ? m[0] : to == WF_S ? m[1] : m[2];
  return wsum[to * (nw + 1) + nw] + wsum[to * (nw + 1) + wave] + (unsigned)__popcll(mine & below);
}

// ---- init: raytrace.rgen:27-60 for every pixel of the shard -------------------------------------------------
__global__ __launch_bounds__(WF_BLOCK) void k_wf_init(const TraceParams P, const WfBuffers B)
{
  const unsigned lane = lane_id();
  const unsigned w = blockIdx.x * blockDim.x + threadIdx.x;  // tile-major work index
  bool alive = false;
  unsigned nPixels = 0;
  LaneState L;
  uint32_t x, y, lrow;
  if(pixelOfWork(P, w, P.tileFirst, x, y, lrow))
  {
    startPixel(P, L, x, y, lrow);
    nPixels = 1;
    if(P.pc.samples <= 0 || P.pc.depth <= 0)
      storePixel(P, L);  // degenerate launch: no rays
    else
      alive = true;
  }
  __shared__ unsigned wsum[WF_TYPES * (WF_BLOCK / 64 + 1)];
  const unsigned slot = claimSlots(B, 0, alive ? WF_C : -1, lane, wsum);
  if(alive)
    storeClosest(B, 0, slot, L);
  __shared__ unsigned long long red[VKRT_COUNTER_STRIDE * (WF_BLOCK / 64)];
  const unsigned vals[6] = {0, 0, 0, 0, 0, nPixels};
  blockAddCounters(&P.counters->v[blockIdx.x % VKRT_COUNTER_SLOTS][0], vals, 6, red);
}

// ---- sample init (sample-synchronous schedule): raytrace.rgen:42-60 of sample `smpl` >= 1 for every pixel of the shard ----------
// The twin of k_wf_init, in front of round `round` = smpl * (depth + 1): one thread per pixel in tile order, so a wave is one 8x8
// tile.  The C stream of the round's parity is empty here: the traversal launch of round - 1 cleared its count and no path of
// sample smpl - 1 emitted a record in the shade step of round - 1 (every one of them had ended its sample by then).
// The sample state is (hitValues, seed); the rest of the lane is bindPixel's (rgen.h, which also says why prd.isSpecular is not carried).
__global__ __launch_bounds__(WF_BLOCK) void k_wf_sample_init(const TraceParams P, const WfBuffers B, const int round, const int smpl)
{
  const unsigned lane = lane_id();
  const unsigned w = blockIdx.x * blockDim.x + threadIdx.x;  // tile-major work index
  bool alive = false;
  LaneState L;
  uint32_t x, y, lrow;
  if(pixelOfWork(P, w, P.tileFirst, x, y, lrow))
  {
    const float4 st = wfLoad(B.sampleState + pixelSlot(P, x, lrow));  // written once, read once
    bindPixel(P, L, x, lrow);
    L.prd.seed = __float_as_uint(st.w);
    L.hitValues = mk3(st.x, st.y, st.z);
    L.smpl = smpl;
    startSample(P, L);
    alive = true;
  }
  __shared__ unsigned wsum[WF_TYPES * (WF_BLOCK / 64 + 1)];
  const unsigned slot = claimSlots(B, round & 1, alive ? WF_C : -1, lane, wsum);
  if(alive)
    storeClosest(B, round & 1, slot, L);
}

// ---- hybrid mode: the GI path of raytraceHybrid.rgen:172-282 on the same streams ----------------------------------------------
// A pixel's GI path is one sample that starts at depth 1 from the G-buffer position; its record is the path tracer's, with the
// S2 plane (unused: there is no sum over samples) carrying hitDists (.x, rgen:253-264) and the visibility term of the direct
// part (.y, the alpha of the accumulation image).  HYBRID instantiations of the shade functions end a sample with hybridStorePixel
// instead of storePixel and keep hitDists; everything else -- rays, shaders, compaction -- is shared with the path tracer, and the
// rules of the GI path itself with k_hybrid, which runs it in-kernel in the megakernel mode (hybrid_gi.h).
// rgen:240-266 for one finished segment of the GI path (hybrid_gi.h); false = the path is complete and the pixel stored
VKRT_DEV bool advanceSegmentHybrid(const TraceParams& P, const HybridGi& G, LaneState& L, bool shadowHit, f3 contrib, f3 nextWeight, float lightDist)
{
  L.stage = 0;
  if(giSegmentStep(P.pc, L.prd, L.curWeight, L.hitValue, L.hitValues.x, shadowHit, contrib, nextWeight, lightDist))
    return true;
  hybridStorePixel(P, G, (size_t)L.lrow * P.fullW + L.px, true, L.hitValue, L.hitValues.x, L.hitValues.y);
  return false;
}

// ---- shade, results of streams C and P: [finish segment k,] rchit / rmiss of the traced closest-hit ray, then the next ray(s) ----
// (Regrouping the 256 results of a workgroup by lobe through LDS between the hit shader's front half and its diffuse / specular
// tail -- closestHitFront / closestHitLobe / closestHitTail in shade.h -- so that a wave runs one branch only was built and
// measured in round 2: bit-identical images, ~30 % fewer VALU instructions, no change in kernel time (5.94 vs 5.91 ms per
// 4-spp frame): the stage is bound by its stream traffic to HBM and the latency of its gathers, not by issue.  Removed again;
// profiles/r02_experiments.md #52.)
// LDS of a shade workgroup (one allocation for the kernel: the C and the pair instantiation of shadeHitBlock share it)
struct ShadeLds
{
  float lut[512];
  unsigned wsum[WF_TYPES * (WF_BLOCK / 64 + 1)];
};

// pixelOfWork (rgen.h) where 64 consecutive work items are one wave, as in the 256-thread workgroups here: the tile is the wave's, so
// its column and row -- two integer divisions -- are found once on the scalar unit instead of in every lane.  Same x, y, lrow.
VKRT_DEV bool pixelOfWave(const TraceParams& P, unsigned w, unsigned tileFirst, uint32_t& x, uint32_t& y, uint32_t& lrow)
{
  if(w >= P.tileCount * 64u)
    return false;
  const unsigned tile = (unsigned)__builtin_amdgcn_readfirstlane((int)(tileFirst + (w >> 6))), inTile = w & 63u;
  x = (tile % P.tilesX) * 8u + (inTile & 7u);
  lrow = (tile / P.tilesX) * 8u + (inTile >> 3);
  if(x >= P.fullW || lrow >= P.localRows)
    return false;
  y = globalRow(P, lrow);
  return y < P.fullH;
}

// CAMERA (k_wf_shade_camera, a camera round of VKRT_FLAG_CAMERA_ROUNDS): the records are the camera rays of sample `smpl`, one per pixel
// of the launch, and only their H0 / H1 planes exist: record qi belongs to the pixel with tile-major work index qi, and its state is
// made from the pixel's sample state as k_wf_traverse_camera made the ray (`count` is not read).
template <bool PAIR, bool HYBRID, bool CAMERA = false>
VKRT_DEV void shadeHitBlock(const TraceParams& P, const WfBuffers& B, const HybridGi& G, const int par, const unsigned count, const unsigned block, ShadeLds& lds,
                            const int smpl = 0)
{
  const int type = PAIR ? WF_P : WF_C;
  const unsigned lane = lane_id();
  const unsigned qi = block * WF_BLOCK + threadIdx.x;
  ShadeStats st = shadeStatsInit<WF_BLOCK>(P.sc, lds.lut);
  unsigned* wsum = lds.wsum;
  int to = -1;
  LaneState L;
  f3 contrib = mk3(0.0f), nextWeight = mk3(0.0f);
  uint32_t x = 0, y = 0, lrow = 0;
  if(CAMERA ? pixelOfWave(P, qi, P.tileFirst, x, y, lrow) : qi < count)
  {
    if(CAMERA)
    {
      bindPixel(P, L, x, lrow);
      if(smpl == 0)  // launch-uniform: raytrace.rgen:27-28
      {
        L.prd.seed = pixelSeed(P, x, y);
        L.hitValues = mk3(0.0f);
      }
      else
      {
        // (pixelSlot(P, x, lrow) is the pixel's tile-major index in the shard, which is what qi counts from the launch's first tile)
        const float4 s = wfLoad(B.sampleState + (P.tileFirst * 64u + qi));  // this lane is the pixel's only one in the launch: it may write it again below
        L.prd.seed = __float_as_uint(s.w);
        L.hitValues = mk3(s.x, s.y, s.z);
      }
      L.smpl = smpl;
      startSample(P, L);
    }
    else
      loadCommon(P, B, par, type, qi, L);
    const float4 h = wfLoad(rec(B, par, type, WF_H0, qi)), t4 = wfLoad(rec(B, par, type, WF_H1, qi));
    if(!CAMERA)
    {
      const float4 rd = wfLoad(rec(B, par, type, PAIR ? WF_R2 : WF_R1, qi));
      L.prd.rayDirection = mk3(rd.x, rd.y, rd.z);  // direction of the closest-hit ray that was traced
    }
    L.prd.rayOrigin = mk3(0.0f);                 // rchit / rmiss do not read it
    if(PAIR)
    {
      // finish segment k first (rgen:99-116): its shadow ray came back with this record.  S0 holds the weight after it;
      // the segment is never the last of its sample (emission rule below), so advanceSegment only accumulates and steps depth
      const float4 s3 = wfLoad(rec(B, par, WF_P, WF_S3, qi));
      const bool shadowHit = __float_as_int(h.x) != 0;
      if(HYBRID)
        (void)advanceSegmentHybrid(P, G, L, shadowHit, mk3(s3.x, s3.y, s3.z), L.curWeight, L.prd.depth == 1u ? wfLoad(rec(B, par, WF_P, WF_R1, qi)).w : 0.0f);
      else
        (void)advanceSegment(P, L, shadowHit, mk3(s3.x, s3.y, s3.z), L.curWeight);
    }
    RayHit hit;
    hit.t = h.x; hit.u = h.y; hit.v = h.z; hit.slot = __float_as_int(h.w);  // instance id of the hit (>= 0) or -1; t is not used by the shaders
    const uint4 ts = make_uint4(__float_as_uint(t4.x), __float_as_uint(t4.y), __float_as_uint(t4.z), __float_as_uint(t4.w));
    if(hit.slot >= 0)
      closestHitShaderInst(P.sc, P.pc, hit, (uint32_t)hit.slot, ts, L.prd.rayDirection, L.prd, st);
    else
      missShader(P.pc, L.prd);
    segmentTerms(L.prd, L.curWeight, contrib, nextWeight);
    // VKRT_OPT_SKIP_DEAD_SHADOW_RAYS (launch-uniform, path-tracing mode only): rgen:99-102 adds `contrib` when the shadow ray is
    // not occluded; a contribution of exactly (+-0, +-0, +-0) -- light behind the surface and no emission, or a zero weight --
    // leaves hitValue bit for bit as it is either way (x + 0 = x; the sum is never -0), so the ray need not be traced
    const bool dead = !HYBRID && (P.flags & VKRT_FLAG_SKIP_DEAD_SHADOW) != 0u && contrib.x == 0.0f && contrib.y == 0.0f && contrib.z == 0.0f;
    if(!L.prd.isSpecular && L.prd.depth != 100u && !dead)  // rgen:79: a shadow ray decides whether this segment contributes
      to = (L.prd.depth + 1u < (uint32_t)P.pc.depth) ? WF_P : WF_S;  // not the last segment: the next closest-hit ray rides along
    else if(HYBRID)
      to = advanceSegmentHybrid(P, G, L, false, contrib, nextWeight, 0.0f) ? WF_C : -1;
    else
      to = finishSegment(P, B, L, false, contrib, nextWeight);
  }
  const unsigned slot = claimSlots(B, par ^ 1, to, lane, wsum);
  if(to == WF_C)
    storeClosest(B, par ^ 1, slot, L);
  else if(to == WF_P)  // (one call per stream: with the type a constant every plane's base is uniform and a store needs the lane's 32-bit offset only)
    storeShadow(B, par ^ 1, WF_P, slot, L, contrib, nextWeight);
  else if(to == WF_S)
    storeShadow(B, par ^ 1, WF_S, slot, L, contrib, nextWeight);
  if(P.flags & VKRT_FLAG_COUNT_WORK)  // launch-uniform: hit / lobe / texture-tap tallies are instrumentation, not needed for the ray rate
  {
    __shared__ unsigned long long red[VKRT_COUNTER_STRIDE * (WF_BLOCK / 64)];
    const unsigned vals[5] = {0, 0, st.hits, st.diffuse, st.taps};
    blockAddCounters(&P.counters->v[blockIdx.x % VKRT_COUNTER_SLOTS][0], vals, 5, red);
  }
}

// ---- shade, results of stream S: the last segment of a sample (rgen:99-120), next sample or pixel store (light; many waves) ----
template <bool HYBRID>
VKRT_DEV void shadeShadowBlock(const TraceParams& P, const WfBuffers& B, const HybridGi& G, const int par, const unsigned count, const unsigned block, ShadeLds& lds)
{
  const unsigned lane = lane_id();
  const unsigned qi = block * WF_BLOCK + threadIdx.x;
  unsigned* wsum = lds.wsum;
  bool toClosest = false;
  LaneState L;
  if(qi < count)
  {
    loadCommon(P, B, par, WF_S, qi, L);  // S0 holds the weight after this segment
    const float4 h = wfLoad(rec(B, par, WF_S, WF_H0, qi)), s3 = wfLoad(rec(B, par, WF_S, WF_S3, qi));
    L.prd.rayOrigin = mk3(0.0f);     // the sample ends here: startSample sets the next ray (now, or in k_wf_sample_init), or the pixel is stored
    L.prd.rayDirection = mk3(0.0f);
    const bool shadowHit = __float_as_int(h.w) >= 0;
    if(HYBRID)
      toClosest = advanceSegmentHybrid(P, G, L, shadowHit, mk3(s3.x, s3.y, s3.z), L.curWeight, L.prd.depth == 1u ? wfLoad(rec(B, par, WF_S, WF_R1, qi)).w : 0.0f);
    else
      toClosest = finishSegment(P, B, L, shadowHit, mk3(s3.x, s3.y, s3.z), L.curWeight) == WF_C;
  }
  const unsigned slot = claimSlots(B, par ^ 1, toClosest ? WF_C : -1, lane, wsum);
  if(toClosest)
    storeClosest(B, par ^ 1, slot, L);
}

// One launch shades the three result streams of a round: the heavy workgroups (C, then P) are dispatched first, the light
// shadow-result workgroups fill in behind them.
// WF_SCALAR_FP32 on the shade kernels: with frames in flight they are bound by VALU issue, where a packed FP32 instruction takes the two
// slots of the two scalar ones it replaces and the v_mov_b32 that pair its operands in adjacent registers come on top (k_wf_shade: 661
// moves with packed FP32, 437 without; profiles/shade_isa.json).  The attribute takes the packed opcodes from these kernels' target, so
// the SLP vectoriser, which the unit keeps for its other kernels, finds nothing to form there.  Same operations, same results.
#if defined(__HIP_DEVICE_COMPILE__)
#define WF_SCALAR_FP32 __attribute__((target("no-packed-fp32-ops")))
#else
#define WF_SCALAR_FP32  // (the host pass only sees the kernels' stubs, and its target has no such feature)
#endif
template <bool HYBRID>
VKRT_DEV void shadeRound(const TraceParams& P, const WfBuffers& B, const HybridGi& G, const int round)
{
  const int par = round & 1;
  const unsigned cC = *countOf(B, par, WF_C), cS = *countOf(B, par, WF_S), cP = *countOf(B, par, WF_P);
  const unsigned nC = (cC + WF_BLOCK - 1) / WF_BLOCK, nP = (cP + WF_BLOCK - 1) / WF_BLOCK, nS = (cS + WF_BLOCK - 1) / WF_BLOCK;
  unsigned blk = blockIdx.x;
  __shared__ ShadeLds lds;
  if(blk < nC)
    shadeHitBlock<false, HYBRID>(P, B, G, par, cC, blk, lds);
  else if((blk -= nC) < nP)
    shadeHitBlock<true, HYBRID>(P, B, G, par, cP, blk, lds);
  else if((blk -= nP) < nS)
    shadeShadowBlock<HYBRID>(P, B, G, par, cS, blk, lds);
}
WF_SCALAR_FP32 __global__ __launch_bounds__(WF_BLOCK) void k_wf_shade(const TraceParams P, const WfBuffers B, const int round)
{
  const HybridGi none{};
  shadeRound<false>(P, B, none, round);
}
WF_SCALAR_FP32 __global__ __launch_bounds__(WF_BLOCK) void k_wf_shade_hybrid(const TraceParams P, const WfBuffers B, const HybridGi G, const int round)
{
  shadeRound<true>(P, B, G, round);
}
// shade step of a camera round (k_wf_traverse_camera traced it): one thread per pixel of the sub-frame in tile order; reads no stream counts
WF_SCALAR_FP32 __global__ __launch_bounds__(WF_BLOCK) void k_wf_shade_camera(const TraceParams P, const WfBuffers B, const int round, const int smpl)
{
  const HybridGi none{};
  __shared__ ShadeLds lds;
  shadeHitBlock<false, false, true>(P, B, none, round & 1, 0u, blockIdx.x, lds, smpl);
}

// First ray of the GI path of every shaded pixel (raytraceHybrid.rgen:172-204), or the pixel's final value when there is no path
// to trace.  tmp: (seed after the direct part, visibility) per pixel, left by k_hybrid.
__global__ __launch_bounds__(WF_BLOCK) void k_hy_gi_init(const TraceParams P, const WfBuffers B, const HybridGi G, const uint2* tmp)
{
  const unsigned lane = lane_id();
  const unsigned w = blockIdx.x * blockDim.x + threadIdx.x;  // tile-major work index
  bool alive = false;
  LaneState L;
  uint32_t x, y, lrow;
  if(pixelOfWork(P, w, P.tileFirst, x, y, lrow))
  {
    const size_t p = (size_t)lrow * P.fullW + x;
    const GbufferPixel g = loadGbufferPixel(G, p);
    const uint2 t = tmp[p];
    const float alpha = __uint_as_float(t.y);
    if(g.shaded)
    {
      bindPixel(P, L, x, lrow);
      L.prd.seed = t.x;
      giFirstRay(P, g, L.prd, L.curWeight);
      L.hitValue = mk3(0.0f);
      L.hitValues = mk3(0.0f, alpha, 0.0f);  // .x hitDists, .y visibility
      L.smpl = 0;
      L.stage = 0;
      alive = L.prd.depth < (uint32_t)P.pc.depth;
    }
    if(!alive)  // no path to trace: the pixel's value is final
      hybridStorePixel(P, G, p, g.shaded, mk3(0.0f), 0.0f, alpha);
  }
  __shared__ unsigned wsum[WF_TYPES * (WF_BLOCK / 64 + 1)];
  const unsigned slot = claimSlots(B, 0, alive ? WF_C : -1, lane, wsum);
  if(alive)
    storeClosest(B, 0, slot, L);
}

// ---- frames in flight: ordered blend of a staged frame (raytrace.rgen:136-145) ---------------------------------------------------
// One thread per pixel of the lane's tiles (tile-major, as k_wf_init): image = mix(image, staged, 1 / (frame + 1)), or the plain
// store of frame 0.  Launched at the end of a frame on the frame's own lane, behind the blend of the frame before it.
__global__ __launch_bounds__(WF_BLOCK) void k_wf_blend(const TraceParams P, const float4* stage)
{
  uint32_t x, y, lrow;
  if(pixelOfWork(P, blockIdx.x * blockDim.x + threadIdx.x, P.tileFirst, x, y, lrow))
  {
    const size_t p = (size_t)lrow * P.fullW + x;
    blendPixel((float4*)P.image + p, stage[p], P.pc.frame);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
#define WF_CTRL_BYTES (256 * VKRT_WF_MAX_LANES)  // 64 count words per lane
size_t vkrt_wf_state_bytes(uint32_t pathCapacity, int groups)
{
  const size_t g = (size_t)std::max(groups, 1);
  return g * pathCapacity * 2 * WF_SLOTS * sizeof(float4) + (g > 1 ? g * pathCapacity * sizeof(float4) : 0) + g * pathCapacity * sizeof(float4) +
         WF_CTRL_BYTES;  // streams + staging planes + sample-state planes + counts
}

void vkrt_wf_carve(void* base, uint32_t pathCapacity, int groups, WfBuffers* B)
{
  const size_t g = (size_t)std::max(groups, 1);
  char* p = (char*)base;
  B->ctrl = (unsigned*)p;
  p += WF_CTRL_BYTES;
  B->planes = (float4*)p;
  p += g * pathCapacity * 2 * WF_SLOTS * sizeof(float4);
  B->stage = g > 1 ? (float4*)p : nullptr;
  p += g > 1 ? g * pathCapacity * sizeof(float4) : 0;
  B->sampleState = (float4*)p;
  B->capacity = pathCapacity;
  B->groups = (uint32_t)g;
}

// One sub-frame = the tiles [tileFirst, tileFirst + tileCount) of the shard with their own streams and counts, on one HIP stream.  Which
// launches a call makes for it, and in what order, is wf_schedule.h's to say: the functions below make one launch (or one round) each.
static unsigned pixelBlocks(const TraceParams& P) { return (P.tileCount * 64u + WF_BLOCK - 1) / WF_BLOCK; }
// begin: counts cleared and, with `init`, one closest-ray record per pixel (raytrace.rgen:27-60; a degenerate frame, no samples or no
// depth, has no rounds: k_wf_init stores its pixels).  A frame of camera rounds starts from the pixel grid instead: no init.
static hipError_t subframeBegin(const TraceParams& P, const WfBuffers& B, bool init, hipStream_t stream)
{
  const hipError_t e = hipMemsetAsync(B.ctrl, 0, 64, stream);
  if(e == hipSuccess && init)
    hipLaunchKernelGGL(k_wf_init, dim3(pixelBlocks(P)), dim3(WF_BLOCK), 0, stream, P, B);
  return e;
}
// One traversal launch on the records of round r, its geometry for a sub-frame's tiles: workgroups of travBlock threads (64 unless 128
// or 256 is asked for).  Every path holds one record and a record at most two rays; +4 blocks for the partial tails of the four ray
// kinds.  One wavefront per workgroup by default: a finished wave frees its slot and LDS without waiting for three others.
static void launchTraverse(const TraceParams& P, const WfBuffers& B, int r, unsigned travBlock, bool count, hipStream_t stream)
{
  const unsigned work = P.tileCount * 64u, tb = (travBlock == 256u || travBlock == 128u) ? travBlock : 64u;
  vkrt_wf_launch_traverse(P, B, r, tb, count, dim3(2 * ((work + tb - 1) / tb) + 4), (size_t)P.sc.stackCap * tb * sizeof(int), stream);
}
// round r: traverse the rays of the records, shade the results into the next round's records.  cameraSample >= 0: r is the first
// round of that sample in a frame of camera rounds -- its rays and their state come from the pixel grid, not from records.
static void subframeRound(const TraceParams& P, const WfBuffers& B, int r, int cameraSample, unsigned travBlock, bool count, hipStream_t stream, WfTiming* timing)
{
  const bool timed = timing && timing->events && 2 * (timing->used + 1) <= timing->capacity;
  if(timed)
    (void)hipEventRecord(timing->events[2 * timing->used], stream);
  if(cameraSample >= 0)
    vkrt_wf_launch_traverse_camera(P, B, r, cameraSample, count, (size_t)P.sc.stackCap * 64u * sizeof(int), stream);
  else
    launchTraverse(P, B, r, travBlock, count, stream);
  if(timed)
  {
    (void)hipEventRecord(timing->events[2 * timing->used + 1], stream);
    timing->used++;
  }
  if(cameraSample >= 0)
    hipLaunchKernelGGL(k_wf_shade_camera, dim3(pixelBlocks(P)), dim3(WF_BLOCK), 0, stream, P, B, r, cameraSample);
  else
    hipLaunchKernelGGL(k_wf_shade, dim3(pixelBlocks(P) + 3), dim3(WF_BLOCK), 0, stream, P, B, r);
}

hipError_t vkrt_launch_wavefront(const TraceParams& P, const WfBuffers& B, const WfOptions& opt, int frames, uint32_t seedStep, bool count,
                                 hipStream_t stream, WfTiming* timing, const WfAsync* async)
{
  const WfCall call{P.pc.samples, P.pc.depth, (P.flags & VKRT_FLAG_SAMPLE_SYNC) != 0u, (P.flags & VKRT_FLAG_CAMERA_ROUNDS) != 0u, P.tileCount, frames,
                    opt.inFlight, opt.subframes, (int)B.groups, async ? async->count : 0, timing != nullptr};
  const WfLanes lanes = wfLanes(call);
  const int L = lanes.F * lanes.S;
  const bool staged = lanes.F > 1;
  if(staged && wfPoolEvents(lanes.frames) > async->poolSize)
    return hipErrorInvalidValue;  // (api_frames.cpp sizes the pool with the same function)
  // a single lane is the caller's stream and B itself; several have internal streams and their slices of B
  hipStream_t laneStream[VKRT_WF_MAX_LANES];
  WfBuffers Bq[VKRT_WF_MAX_LANES];
  laneStream[0] = stream;
  Bq[0] = B;
  const size_t groupQuads = (size_t)2 * WF_SLOTS * B.capacity;
  for(int q = 0; L > 1 && q < L; q++)
  {
    const int g = q / lanes.S, j = q % lanes.S;
    const uint32_t tile0 = lanes.tileFirst(j);
    Bq[q].ctrl = B.ctrl + 64 * q;
    Bq[q].planes = B.planes + (size_t)g * groupQuads + (size_t)2 * WF_SLOTS * ((size_t)tile0 * 64u);
    Bq[q].stage = staged ? B.stage + (size_t)g * B.capacity : nullptr;
    Bq[q].sampleState = B.sampleState + (size_t)g * B.capacity;  // indexed by the pixel's tile in the shard: no offset per tile range
    Bq[q].capacity = (lanes.tileFirst(j + 1) - tile0) * 64u;
    Bq[q].groups = 1;
    laneStream[q] = async->streams[q];
  }
  // fork: every lane starts behind what the caller enqueued before this call; whatever happens afterwards, the lanes that were
  // started are joined to the caller's stream again before the function returns (nothing of a failed call runs on unordered)
  int forked = 0;
  auto joinLanes = [&]() {
    hipError_t first = hipSuccess;
    for(int q = 0; q < forked; q++)
    {
      hipError_t x = hipEventRecord(async->join[q], laneStream[q]);
      if(x == hipSuccess) x = hipStreamWaitEvent(stream, async->join[q], 0);
      if(x != hipSuccess)
      {
        (void)hipStreamSynchronize(laneStream[q]);
        if(first == hipSuccess) first = x;
      }
    }
    return first;
  };
  hipError_t e = hipSuccess;
  if(L > 1 && (e = hipEventRecord(async->fork, stream)) != hipSuccess) return e;
  for(int q = 0; L > 1 && q < L; q++)
  {
    if((e = hipStreamWaitEvent(laneStream[q], async->fork, 0)) != hipSuccess)
    {
      (void)joinLanes();
      return e;
    }
    forked = q + 1;
  }
  const bool init = !wfCameraRounds(call);
  const bool all = wfForEachItem(call, lanes, [&](const WfItem& it) {
    const WfBuffers& Bl = Bq[it.lane];
    hipStream_t st = laneStream[it.lane];
    TraceParams Q = wfFrameParams(P, (uint32_t)it.frame, seedStep);
    Q.tileFirst = lanes.tileFirst(it.range);
    Q.tileCount = lanes.tileFirst(it.range + 1) - Q.tileFirst;
    if(staged)
    {
      Q.image = (float*)Bl.stage;
      Q.flags |= VKRT_FLAG_STORE_STAGED;
    }
    switch(it.kind)
    {
    case WfItem::BEGIN:
      e = subframeBegin(Q, Bl, init, st);
      break;
    case WfItem::STEP:
    {
      const WfStep s = wfStep(call, it.step);
      if(s.kind == WfStep::SAMPLE_INIT)
        hipLaunchKernelGGL(k_wf_sample_init, dim3(pixelBlocks(Q)), dim3(WF_BLOCK), 0, st, Q, Bl, s.round, s.sample);
      else
        subframeRound(Q, Bl, s.round, s.sample, (unsigned)opt.travBlock, count, st, timing);
      break;
    }
    case WfItem::BLEND:  // the frame's pixels are staged: blend them into the image behind the blend of the frame before
      if(it.wait >= 0 && (e = hipStreamWaitEvent(st, async->pool[it.wait], 0)) != hipSuccess)
        break;
      Q.image = P.image;
      hipLaunchKernelGGL(k_wf_blend, dim3(pixelBlocks(Q)), dim3(WF_BLOCK), 0, st, Q, (const float4*)Bl.stage);
      if(it.record >= 0)
        e = hipEventRecord(async->pool[it.record], st);
      break;
    }
    return e == hipSuccess;
  });
  if(e == hipSuccess && !all)
    e = hipErrorUnknown;  // (a lane held for ever: tests/test_wf_schedule.py shows there is no such call)
  const hipError_t ej = joinLanes();
  if(e == hipSuccess) e = ej;
  if(e == hipSuccess) e = hipGetLastError();
  return e;
}

// ---- hybrid GI -------------------------------------------------------------------------------------------------------
uint2* vkrt_wf_hybrid_tmp(const WfBuffers& B)
{
  // the streams of parity 1 are first written by the shade step of round 0: until then their first plane is free
  return (uint2*)(B.planes + (size_t)(1 * WF_SLOTS + 0) * B.capacity);
}

hipError_t vkrt_launch_hybrid_gi(const TraceParams& P, const WfBuffers& B, const HybridGi& G, unsigned travBlock, hipStream_t stream)
{
  const unsigned work = P.tileCount * 64u;
  hipError_t e = hipMemsetAsync(B.ctrl, 0, 64, stream);
  if(e != hipSuccess)
    return e;
  const unsigned blocks = (work + WF_BLOCK - 1) / WF_BLOCK;
  hipLaunchKernelGGL(k_hy_gi_init, dim3(blocks), dim3(WF_BLOCK), 0, stream, P, B, G, (const uint2*)vkrt_wf_hybrid_tmp(B));
  // the GI path is one sample that starts at depth 1: at most pc.depth - 1 segments, i.e. pc.depth rounds of the paired pipeline
  const int rounds = P.pc.depth;
  for(int r = 0; r < rounds; r++)
  {
    launchTraverse(P, B, r, travBlock, false, stream);
    hipLaunchKernelGGL(k_wf_shade_hybrid, dim3(blocks + 3), dim3(WF_BLOCK), 0, stream, P, B, G, r);
  }
  return hipGetLastError();
}
