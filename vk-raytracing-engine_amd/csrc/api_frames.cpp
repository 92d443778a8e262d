// api_frames.cpp -- rendered frames (include/vkrt.h): vkrt_pathtrace*, vkrt_gbuffer_raycast*, vkrt_hybrid_trace*, and vkrt_reserve* for
// their working set.  The three families check their arguments in orders of their own; the rules themselves are entry_checks.h's.
#include "scene_state.h"

using namespace vkrt;

namespace {

// Working set of the wavefront pipeline for `paths` path records (whole 8x8 tiles of the shard) in each of `groups` frame groups
// (frames in flight) + the internal streams of the lanes.  Growing it is the only place a trace call may synchronise with the
// host (vkrt_reserve).
int ensureWorkingSet(vkrt_scene* s, uint32_t paths, int groups, hipStream_t stream)
{
  groups = std::max(1, std::min(VKRT_WF_MAX_LANES, groups));
  // wf_streams.h rec(): a record's byte offset inside a plane is a 32-bit lane offset (16 B x slot); 2^28 path records and more
  // (16384 x 16384 pixels in one shard, ~146 GB of streams) would wrap it silently
  if(paths >= (1u << 28))
    return fail(VKRT_ERR_UNSUPPORTED, "wavefront mode: %u path records in one shard (limit 2^28 - 1: split the launch into shards)", paths);
  if(!s->wfMem.get() || s->wf.capacity < paths || (int)s->wf.groups < groups)
  {
    HIP_TRY(hipStreamSynchronize(stream));  // an earlier frame may still be using the smaller buffer
    paths = std::max(paths, s->wf.capacity);
    groups = std::max(groups, (int)s->wf.groups);
    s->wf = WfBuffers{};
    HIP_TRY(s->wfMem.alloc(vkrt_wf_state_bytes(paths, groups)));
    vkrt_wf_carve(s->wfMem.get(), paths, groups, &s->wf);
  }
  if(s->wfAsync.count == 0)
  {  // (a call that fails half-way keeps what it created; the next one creates the rest)
    if(!s->wfFork.get())
      HIP_TRY(s->wfFork.create(hipEventDisableTiming));
    for(int j = 0; j < VKRT_WF_MAX_LANES; j++)
    {
      if(!s->wfStreams[j].get())
        HIP_TRY(s->wfStreams[j].create(hipStreamNonBlocking));
      if(!s->wfJoin[j].get())
        HIP_TRY(s->wfJoin[j].create(hipEventDisableTiming));
      s->wfAsync.streams[j] = s->wfStreams[j].get();
      s->wfAsync.join[j] = s->wfJoin[j].get();
    }
    s->wfAsync.fork = s->wfFork.get();
    s->wfAsync.count = VKRT_WF_MAX_LANES;
  }
  return VKRT_OK;
}

// at least `want` events with `flags` in an owner list and in the raw array a launcher takes
int growEvents(std::vector<DevEvent>& owners, std::vector<hipEvent_t>& raw, size_t want, unsigned flags)
{
  while(raw.size() < want)
  {
    DevEvent e;
    HIP_TRY(e.create(flags));
    raw.push_back(e.get());
    owners.push_back(std::move(e));
  }
  return VKRT_OK;
}

// the working set and the event pool (the events that order the lanes of a call; created once, kept; no device synchronisation) of a
// wavefront call of `frames` frames, which the launcher sees as batches, on `tiles` 8x8 tiles: wf_schedule.h says how much of each
int ensureFrameCall(vkrt_scene* s, uint32_t tiles, uint32_t frames, hipStream_t stream)
{
  RC_TRY(ensureWorkingSet(s, tiles * 64u, wfGroupsWanted(s->opt[VKRT_OPT_WF_FRAMES_IN_FLIGHT], frames), stream));
  RC_TRY(growEvents(s->wfPoolOwners, s->wfPool, (size_t)wfPoolEvents((int)std::min<uint32_t>(frames, VKRT_FRAMES_PER_BATCH)), hipEventDisableTiming));
  s->wfAsync.pool = s->wfPool.data();
  s->wfAsync.poolSize = (int)s->wfPool.size();
  return VKRT_OK;
}

// The alpha-test stage of a frame call (VKRT_OPT_ALPHA_TEST): active when the option is on and some material is MASK right now -- read
// per call, so nothing of it is a property of the tree.  The call's copy of the scene carries the flag to the launchers
// (frame_tri_mode); its walks exist for 64-thread traversal workgroups only, like those of the other non-default triangle modes.
int frameAlphaStage(const vkrt_scene* s, const char* who, TraceParams& P)
{
  if(s->opt[VKRT_OPT_ALPHA_TEST] == 0 || s->alphaMasks == 0u)
    return VKRT_OK;
  if(s->wavefront && travBlock(s) != 64)
    return fail(VKRT_ERR_UNSUPPORTED, "%s: VKRT_OPT_ALPHA_TEST with a VKRT_ALPHA_MASK material is built for the default 64-thread traversal workgroups "
                "(VKRT_OPT_WF_TRAV_BLOCK = %d)", who, travBlock(s));
  P.sc.alphaTest = 1u;
  return VKRT_OK;
}

// The TraceParams every trace entry point shares: tree, camera, seed, public flags, the shard's rows and its 8x8 tiles, counters.
// Callers check the tree (checkBuilt) and the shard (check_shard) first and add what is their own.
int launchParams(const vkrt_scene* s, const PushConstantRay* pc, const GlobalUniforms* cam, const vkrt_trace_opts* opts, const vkrt_shard* shard,
                 TraceParams& P)
{
  memset(&P, 0, sizeof P);
  P.sc = s->dev;
  if(pc) P.pc = *pc;
  memcpy(P.viewInverse, cam->viewInverse.m, sizeof P.viewInverse);
  memcpy(P.projInverse, cam->projInverse.m, sizeof P.projInverse);
  P.seed = opts ? opts->seed : 0u;
  P.flags = (opts ? opts->flags : 0u) & VKRT_TRACE_PUBLIC_FLAGS;  // (the hybrid passes never skip shadow rays: hitDists needs their result)
  P.fullW = shard->full_width;
  P.fullH = shard->full_height;
  const bool sharded = shard->shard_count > 1;
  P.stripRows = sharded ? shard->strip_rows : 0u;
  P.shardCount = sharded ? shard->shard_count : 1u;
  P.shardIndex = sharded ? shard->shard_index : 0u;
  P.localRows = vkrt_shard_rows(shard);
  P.counters = s->counters;
  P.tilesX = (P.fullW + 7) / 8;
  P.tileFirst = 0;
  CHECK_TRY(shard_tiles(shard, P.tileCount, err));
  return VKRT_OK;
}

int gbufferImpl(vkrt_scene* s, const float clearColor[4], int lightsCount, const GlobalUniforms* cam, const float* viewMatrix, const vkrt_shard* shard,
                const vkrt_gbuffer* out, const vkrt_nrd_planes* nrd, vkrt_hit* hits, void* hip_stream)
{
  if(s && clearColor && cam && shard && out && vkrt_shard_rows(shard) == 0u)
    return VKRT_OK;  // a shard without rows: nothing to write, no planes to pass
  if(!s || !clearColor || !cam || !shard || !out || !out->color || !out->position || !out->normal || !out->roughMetal)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  CHECK_TRY(check_lights_count("lightsCount", lightsCount, s->lightCount, err));
  RC_TRY(enter(s));
  TraceParams P;
  RC_TRY(checkBuilt(s, "vkrt_gbuffer_raycast"));
  CHECK_TRY(check_shard(shard, err));
  RC_TRY(launchParams(s, nullptr, cam, nullptr, shard, P));
  if(P.localRows == 0)
    return VKRT_OK;
  RC_TRY(frameAlphaStage(s, "vkrt_gbuffer_raycast", P));
  P.sc.gbufferMips = (uint32_t)s->opt[VKRT_OPT_GBUFFER_MIPS];
  const HybridGi G{(float4*)out->color, (float4*)out->position, (float4*)out->normal, (float2*)out->roughMetal, nullptr,
                   nrd ? (float4*)nrd->diffRadianceHitDist : nullptr, nrd ? nrd->viewZ : nullptr};
  HIP_TRY(vkrt_launch_gbuffer(P, clearColor, lightsCount, G, nrd ? nrd->normalRoughness : nullptr, viewMatrix, (float4*)hits, (hipStream_t)hip_stream));
  return VKRT_OK;
}

int hybridImpl(vkrt_scene* s, const PushConstantRay* pc, const GlobalUniforms* cam, const vkrt_trace_opts* opts, const vkrt_shard* shard,
               const vkrt_gbuffer* g, const vkrt_nrd_planes* nrd, float* accum, void* hip_stream)
{
  if(s && pc && cam && shard && g && vkrt_shard_rows(shard) == 0u)
    return VKRT_OK;
  if(!s || !pc || !cam || !shard || !g || !accum || !g->color || !g->position || !g->normal || !g->roughMetal)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  CHECK_TRY(check_lights_count("PushConstantRay.lightsCount", pc->lightsCount, s->lightCount, err));
  CHECK_TRY(check_samples_depth("depth", 0, pc->depth, err));
  RC_TRY(enter(s));
  TraceParams P;
  RC_TRY(checkBuilt(s, "vkrt_hybrid_trace"));
  CHECK_TRY(check_shard(shard, err));
  RC_TRY(launchParams(s, pc, cam, opts, shard, P));
  if(P.localRows == 0)
    return VKRT_OK;
  RC_TRY(frameAlphaStage(s, "vkrt_hybrid_trace", P));
  hipStream_t stream = (hipStream_t)hip_stream;
  HIP_TRY(hipEventRecord(s->evStart.get(), stream));
  const HybridGi G{(float4*)g->color, (float4*)g->position, (float4*)g->normal, (float2*)g->roughMetal, (float4*)accum,
                   nrd ? (float4*)nrd->diffRadianceHitDist : nullptr, nrd ? nrd->viewZ : nullptr};
  // The GI paths (raytraceHybrid.rgen:172-282) run on the path tracer's wavefront streams when the scene was built for them:
  // k_hybrid does the shadow and AO rays and leaves the per-pixel state for k_hy_gi_init (wavefront.hip).  The megakernel mode
  // keeps the whole rgen in k_hybrid.
  const bool giOnStreams = s->wavefront && pc->useGI == 1 && P.fullW <= 65535u && P.localRows <= 65535u;
  if(giOnStreams)
  {
    RC_TRY(ensureWorkingSet(s, P.tileCount * 64u, 1, stream));
    P.tileFirst = 0;
    HIP_TRY(vkrt_launch_hybrid(P, G, vkrt_wf_hybrid_tmp(s->wf), stream));
    HIP_TRY(vkrt_launch_hybrid_gi(P, s->wf, G, (unsigned)travBlock(s), stream));
  }
  else
    HIP_TRY(vkrt_launch_hybrid(P, G, nullptr, stream));
  HIP_TRY(hipEventRecord(s->evStop.get(), stream));
  s->timed = true;
  s->wfTimed = false;
  return VKRT_OK;
}

}  // namespace

extern "C" {

int vkrt_reserve(vkrt_scene* s, const vkrt_shard* shard, void* hip_stream)
{
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  // frame groups: what a vkrt_pathtrace_frames call would keep in flight under the current options
  return vkrt_reserve_frames(s, shard, (uint32_t)std::max(1, s->opt[VKRT_OPT_WF_FRAMES_IN_FLIGHT]), hip_stream);
}

int vkrt_reserve_frames(vkrt_scene* s, const vkrt_shard* shard, uint32_t frames_per_call, void* hip_stream)
{
  if(!s || !shard)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  if(frames_per_call == 0)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "frames_per_call is 0");
  CHECK_TRY(check_shard(shard, err));
  RC_TRY(enter(s));
  uint32_t tiles = 0;
  CHECK_TRY(shard_tiles(shard, tiles, err));
  // the mode that counts is the one the acceleration structure was built for (vkrt_pathtrace and vkrt_hybrid_trace look at
  // s->wavefront, not at an option that may have changed since); before a build, the option is the best guess there is
  const bool wavefront = s->built ? s->wavefront : useWavefront(s);
  if(tiles == 0 || !wavefront)
    return VKRT_OK;  // the megakernel keeps its state in registers / LDS
  return ensureFrameCall(s, tiles, frames_per_call, (hipStream_t)hip_stream);
}

int vkrt_pathtrace(vkrt_scene* s, const PushConstantRay* pc, const GlobalUniforms* cam, const vkrt_trace_opts* opts,
                   const vkrt_shard* shard, float* image, void* hip_stream)
{
  return vkrt_pathtrace_frames(s, pc, cam, opts, shard, image, 1u, hip_stream);
}

int vkrt_pathtrace_frames(vkrt_scene* s, const PushConstantRay* pc, const GlobalUniforms* cam, const vkrt_trace_opts* opts,
                          const vkrt_shard* shard, float* image, uint32_t n_frames, void* hip_stream)
{
  if(!s || !pc || !cam || !shard)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  if(n_frames == 0u)
    return VKRT_OK;
  CHECK_TRY(check_frame_count(n_frames, pc->frame, err));
  if(!image && vkrt_shard_rows(shard) != 0u)  // (a shard without rows -- more ranks than strips -- has no image to pass)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL image");
  RC_TRY(checkBuilt(s, "vkrt_pathtrace"));
  CHECK_TRY(check_shard(shard, err));
  CHECK_TRY(check_lights_count("PushConstantRay.lightsCount", pc->lightsCount, s->lightCount, err));
  CHECK_TRY(check_samples_depth("samples/depth", pc->samples, pc->depth, err));
  RC_TRY(enter(s));
  hipStream_t stream = (hipStream_t)hip_stream;
  TraceParams P;
  RC_TRY(launchParams(s, pc, cam, opts, shard, P));
  if(P.localRows == 0)
    return VKRT_OK;
  RC_TRY(frameAlphaStage(s, "vkrt_pathtrace", P));
  if(s->opt[VKRT_OPT_SKIP_DEAD_SHADOW_RAYS])
    P.flags |= VKRT_FLAG_SKIP_DEAD_SHADOW;  // internal bit (device_scene.h)
  P.image = image;
  P.workCounter = s->workCounter;

  const bool count = (P.flags & VKRT_TRACE_COUNT_TRAVERSAL) != 0;
  const uint32_t seedStep = (P.flags & VKRT_TRACE_SAME_SEED_EVERY_FRAME) ? 0u : 1u;
  if(s->wavefront)
  {
    if(P.fullW > 65535u || P.localRows > 65535u || pc->samples > 65535)
      return fail(VKRT_ERR_UNSUPPORTED, "wavefront mode packs pixel coordinates / sample index in 16 bits");
    if(s->opt[VKRT_OPT_WF_SAMPLE_SYNC])
      P.flags |= VKRT_FLAG_SAMPLE_SYNC;  // internal bit (device_scene.h)
    // camera rounds: only in that schedule, and only where the sharing wave of k_wf_traverse_camera runs (wide8 tree, one-wave traversal
    // workgroups, sharing on); anywhere else the option resolves to the record path
    if(s->opt[VKRT_OPT_WF_CAMERA_ROUNDS] && (P.flags & VKRT_FLAG_SAMPLE_SYNC) && s->dev.layout == 1u && travBlock(s) == 64 && s->dev.shareMinIdle != 0u &&
       s->dev.triThreshold != 0u)
      P.flags |= VKRT_FLAG_CAMERA_ROUNDS;
    RC_TRY(ensureFrameCall(s, P.tileCount, n_frames, stream));
    WfTiming* timing = nullptr;
    if(P.flags & VKRT_TRACE_TIME_KERNELS)
    {
      RC_TRY(growEvents(s->wfEventOwners, s->wfEvents, wfTimingEvents(pc->samples, pc->depth, n_frames), hipEventDefault));
      s->wfTiming.events = s->wfEvents.data();
      s->wfTiming.capacity = (int)s->wfEvents.size();
      timing = &s->wfTiming;
    }
    s->wfTimed = timing != nullptr;
    s->wfTimingRounds = wfRounds(pc->samples, pc->depth);
    HIP_TRY(hipEventRecord(s->evStart.get(), stream));
    const WfOptions wo{s->opt[VKRT_OPT_WF_SUBFRAMES], travBlock(s), s->opt[VKRT_OPT_WF_FRAMES_IN_FLIGHT]};
    if(timing)
      timing->used = 0;  // one timing record per call: the batches of a long call append to it
    for(uint32_t first = 0; first < n_frames; first += VKRT_FRAMES_PER_BATCH)
    {
      const TraceParams Pb = wfFrameParams(P, first, seedStep);
      HIP_TRY(vkrt_launch_wavefront(Pb, s->wf, wo, (int)std::min<uint32_t>(VKRT_FRAMES_PER_BATCH, n_frames - first), seedStep, count, stream, timing, &s->wfAsync));
    }
    HIP_TRY(hipEventRecord(s->evStop.get(), stream));
    s->timed = true;
    return VKRT_OK;
  }
  const size_t lds = (size_t)P.sc.stackCap * 256 * sizeof(int);
  int perCU = 0;
  HIP_TRY(vkrt_pathtrace_occupancy(lds, &perCU));
  if(perCU < 1)
    return fail(VKRT_ERR_UNSUPPORTED, "path-trace kernel does not fit a CU with %zu B of LDS", lds);
  const uint64_t wantBlocks = ((uint64_t)P.tileCount * 64 + 255) / 256;
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(wantBlocks, (uint64_t)s->cuCount * perCU));

  HIP_TRY(hipEventRecord(s->evStart.get(), stream));
  for(uint32_t k = 0; k < n_frames; k++)  // the megakernel renders the frames of a call one after another
  {
    const TraceParams Pk = wfFrameParams(P, k, seedStep);
    HIP_TRY(hipMemsetAsync(s->workCounter, 0, sizeof(unsigned int), stream));
    HIP_TRY(vkrt_launch_pathtrace(Pk, grid, count, stream));
  }
  HIP_TRY(hipEventRecord(s->evStop.get(), stream));
  s->timed = true;
  s->wfTimed = false;
  return VKRT_OK;
}

int vkrt_gbuffer_raycast(vkrt_scene* s, const float clearColor[4], int lightsCount, const GlobalUniforms* cam, const vkrt_shard* shard,
                         const vkrt_gbuffer* out, void* hip_stream)
{
  return gbufferImpl(s, clearColor, lightsCount, cam, nullptr, shard, out, nullptr, nullptr, hip_stream);
}

int vkrt_gbuffer_raycast_nrd(vkrt_scene* s, const float clearColor[4], int lightsCount, const GlobalUniforms* cam, const float viewMatrix[16],
                             const vkrt_shard* shard, const vkrt_gbuffer* out, const vkrt_nrd_planes* nrd, void* hip_stream)
{
  if(s && clearColor && cam && shard && out && nrd && vkrt_shard_rows(shard) == 0u)
    return VKRT_OK;  // a shard without rows
  if(!nrd || !viewMatrix || !nrd->normalRoughness || !nrd->viewZ || !nrd->diffRadianceHitDist)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL NRD plane / view matrix");
  return gbufferImpl(s, clearColor, lightsCount, cam, viewMatrix, shard, out, nrd, nullptr, hip_stream);
}

int vkrt_gbuffer_raycast_hits(vkrt_scene* s, const float clearColor[4], int lightsCount, const GlobalUniforms* cam, const float viewMatrix[16],
                              const vkrt_shard* shard, const vkrt_gbuffer* out, const vkrt_nrd_planes* nrd, vkrt_hit* hits, void* hip_stream)
{
  if(s && clearColor && cam && shard && out && hits && (!nrd) == (!viewMatrix) && vkrt_shard_rows(shard) == 0u)
    return VKRT_OK;  // a shard without rows
  if((!nrd) != (!viewMatrix))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_gbuffer_raycast_hits: view_matrix and nrd go together (both NULL or both given)");
  if(nrd && (!nrd->normalRoughness || !nrd->viewZ || !nrd->diffRadianceHitDist))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL NRD plane");
  if(!hits)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_gbuffer_raycast_hits: hits is NULL");
  if(((uintptr_t)hits & 15u) != 0u)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_gbuffer_raycast_hits: hits is not 16-byte aligned");
  return gbufferImpl(s, clearColor, lightsCount, cam, viewMatrix, shard, out, nrd, hits, hip_stream);
}

int vkrt_hybrid_trace(vkrt_scene* s, const PushConstantRay* pc, const GlobalUniforms* cam, const vkrt_trace_opts* opts, const vkrt_shard* shard,
                      const vkrt_gbuffer* g, float* accum, void* hip_stream)
{
  return hybridImpl(s, pc, cam, opts, shard, g, nullptr, accum, hip_stream);
}

int vkrt_hybrid_trace_nrd(vkrt_scene* s, const PushConstantRay* pc, const GlobalUniforms* cam, const vkrt_trace_opts* opts, const vkrt_shard* shard,
                          const vkrt_gbuffer* g, const vkrt_nrd_planes* nrd, float* accum, void* hip_stream)
{
  if(s && pc && cam && shard && g && nrd && vkrt_shard_rows(shard) == 0u)
    return VKRT_OK;  // a shard without rows
  if(!nrd || !nrd->viewZ || !nrd->diffRadianceHitDist)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL NRD plane");
  return hybridImpl(s, pc, cam, opts, shard, g, nrd, accum, hip_stream);
}

}  // extern "C"
