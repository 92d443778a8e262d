// vkrt_api.cpp -- implementation of the C ABI declared in include/vkrt.h (compiled as HIP).
//
// Scene upload mirrors HelloVulkan::loadGltfScene's device-local buffers (hello_vulkan.cpp:353-381);
// vkrt_accel_build stands in for createBottomLevelASGltf/createTopLevelAsGltf (:1001-1047);
// vkrt_pathtrace stands in for HelloVulkan::pathtrace (:1423-1448).  There is no CPU fallback:
// without a HIP device the compute entry points fail with VKRT_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/vkrt.h"
#include "bvh_host.h"
#include "dev_buffer.h"
#include "device_scene.h"
#include "kernels.h"
#include "scene_options.h"
#include "scene_pack.h"
#include "trav_lds.h"
#include "wide_node.h"

#include "lbvh.h"
#include "morph.h"
#include "node_update.h"
#include "refit.h"
#include "skin.h"
#include "vertex_anim.h"
#include "vertex_update.h"

namespace {

thread_local std::string g_lastError;

int fail(int code, const char* fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_lastError = buf;
  return code;
}

#define HIP_TRY(expr)                                                      \
  do                                                                       \
  {                                                                        \
    std::string m_;                                                        \
    if(const int rc_ = vkrt::hip_status((expr), #expr, m_); rc_ != VKRT_OK) \
      return fail(rc_, "%s", m_.c_str());                                  \
  } while(0)

}  // namespace

struct vkrt_scene
{
  int device = 0;
  int cuCount = 256;
  // host copies (kept like m_gltfScene keeps its vectors)
  std::vector<float> positions;  // (after a device-sourced vkrt_scene_update_vertices: behind the device's until the next build, positionsOnDevice)
  std::vector<uint32_t> indices;
  std::vector<vkrt_prim_mesh> primMeshes;
  std::vector<vkrt_node> nodes;  // (after a device-sourced vkrt_scene_update_node_transforms: matrices behind the device's, nodesOnDevice)
  uint32_t lightCount = 0, materialCount = 0;
  std::vector<float> materialAlpha;  // pbrBaseColorFactor.a per material (the any-hit stage's dissolve), host copy for the host builder
  // device allocations
  vkrt::DevArena tables;  // what vkrt_scene_create uploads, and the counters
  DevScene dev{};
  vkrt::TreeBuffers accel;  // the built tree (dev.nodes / tris / triShade point into it)
  bool built = false;
  vkrt_accel_info info{};
  unsigned int* workCounter = nullptr;
  DevCounters* counters = nullptr;
  vkrt::DevEvent evStart, evStop;
  bool timed = false;
  // wavefront mode working set; WfAsync and WfTiming are the raw views the launchers take, filled from the owners beside them
  vkrt::DevBuf wfMem;
  WfBuffers wf{};
  vkrt::DevStream wfStreams[VKRT_WF_MAX_LANES];
  vkrt::DevEvent wfFork, wfJoin[VKRT_WF_MAX_LANES];
  WfAsync wfAsync{};
  std::vector<vkrt::DevEvent> wfEventOwners;
  std::vector<hipEvent_t> wfEvents;
  WfTiming wfTiming{};
  bool wfTimed = false;
  int splitResolved = 0;  // the budget the last vkrt_accel_build used (VKRT_INFO_SPLIT_BUDGET): what -1 resolved to
  int wfTimingRounds = 0;  // rounds per frame of the last timed call (vkrt_last_trace_timing: which gaps are shade launches)
  std::vector<vkrt::DevEvent> wfPoolOwners;  // events ordering the lanes of one call (kernels.h WfAsync::pool)
  std::vector<hipEvent_t> wfPool;
  int opt[vkrt::kOptionLast + 1];  // execution options (include/vkrt.h vkrt_option); index = option id, values from scene_options.h
  bool hasLargeTriangles = false;  // some instanced triangle covers more than 1 % of the largest face of the scene's box (any-hit order heuristic)
  bool wavefront = true;  // execution mode the acceleration structure was built for (opt[VKRT_OPT_MODE] at vkrt_accel_build)
  // moving instances (vkrt_scene_update_nodes / vkrt_accel_refit)
  bool stale = false;      // node transforms or vertex positions changed since the tree was built or refitted: no trace until the next refit or build
  bool refitted = false;   // the tree has been refitted since its build: vkrt_accel_get_info reads the refit's SAH cost from the device
  vkrt::RefitScratch refit;  // level lists + exact node boxes of the current build (allocated at its first refit)
  bool nodesOnDevice = false;  // a device-sourced vkrt_scene_update_node_transforms moved nodes whose matrices `nodes` has not seen: whoever
                               // reads matrices from `nodes` (the builders, scene_bounds, the split hook) downloads the records first
  // deforming meshes (vkrt_scene_update_vertices)
  bool positionsOnDevice = false;  // a device-sourced update moved vertices the host copy has not seen: the next build downloads them first
  vkrt::StageBuf vertexStage;      // staging of host-sourced updates, joint matrices and morph weights
  // skinned meshes (vkrt_scene_add_skin): per skin one allocation holding the captured bind pose and the influences of its vertex range;
  // the ranges are disjoint, the index in the list is the skin's number
  struct Skin
  {
    vkrt::DevBuf mem;
    vkrt::SkinArrays arrays;
    uint32_t jointCount = 0;
  };
  std::vector<Skin> skins;
  // morph targets (vkrt_scene_add_morph): per morph one allocation holding the captured base shape and the deltas of its vertex range;
  // the ranges are disjoint, the index in the list is the morph's number.  skin >= 0: the range lies inside that skin's, and the morph
  // writes the skin's bind pose instead of the live arrays
  struct Morph
  {
    vkrt::DevBuf mem;
    vkrt::MorphArrays arrays;
    int skin = -1;
  };
  std::vector<Morph> morphs;
  // ray-query visibility (vkrt_scene_set_instance_visibility): host copy per node, and which masks occur (bit m of masksPresent[m >> 6])
  std::vector<vkrt_instance_visibility> vis;
  uint64_t masksPresent[4] = {0, 0, 0, 0};
  vkrt::DevBuf nodeMasks;  // wide8: the node-mask table of the current tree (8 B per node), allocated and computed with it
  // alpha-tested materials (vkrt_scene_set_material_alpha): host copy per material, and how many are VKRT_ALPHA_MASK right now (> 0: the
  // ray queries walk with the alpha-test stage, and so do the frames with VKRT_OPT_ALPHA_TEST)
  std::vector<vkrt_material_alpha> alpha;
  uint32_t alphaMasks = 0;
  // vkrt_hit_surface: 16 B per primitive-mesh (device_scene.h DevSurfaceScene), uploaded at vkrt_scene_create, released with `tables`
  const uint4* surfacePrimMeshes = nullptr;
  // vkrt_scene_motion_mark: the instance records (96 B per node) and vertex positions (12 B per vertex) as they were at the last mark, one
  // allocation made by the first mark and kept until the scene goes; before any mark the previous state is the live arrays
  vkrt::DevBuf motion;
  const DevInstance* prevInstances() const { return motion.get() ? motion.get<const DevInstance>() : dev.instances; }
  const float* prevPositions() const { return motion.get() ? (const float*)(motion.get<const char>() + motionPositionsAt()) : dev.positions; }
  size_t motionPositionsAt() const { return std::max<size_t>(nodes.size() * sizeof(DevInstance), 16); }
};

namespace {

template <typename T>
int upload(vkrt_scene* s, const T* src, size_t count, const T** dst)
{
  T* p = nullptr;
  HIP_TRY(s->tables.alloc(&p, count));
  if(count)
    HIP_TRY(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
  *dst = p;
  return VKRT_OK;
}

// a refusal of scene_pack.h's or vertex_anim.h's checks, whose reason is in err
int failWith(int code, const std::string& err) { return fail(code, "%s", err.c_str()); }

// return such a refusal from the enclosing function: CHECK_TRY(check_x(..., err)), a function of namespace vkrt given the macro's own err
#define CHECK_TRY(call)                                    \
  do                                                       \
  {                                                        \
    std::string err;                                       \
    if(const int rc_ = vkrt::call; rc_ != VKRT_OK)         \
      return failWith(rc_, err);                           \
  } while(0)

// the vertex ranges of the scene's skins or morphs, where they are kept
template <typename T>
vkrt::RangeSet rangesOf(const std::vector<T>& v)
{
  return vkrt::RangeSet{v.empty() ? nullptr : &v[0].arrays, v.size(), sizeof(T)};
}

// Live positions moved on the device: the tree is stale until the next refit or build, and -- unless the host copy got the same values --
// the next build downloads them first.
void positionsMoved(vkrt_scene* s, bool hostCopyFollowed = false)
{
  if(!hostCopyFollowed)
    s->positionsOnDevice = true;
  if(s->built)
    s->stale = true;
}

// execution mode: wavefront pipeline (default) or the single persistent megakernel
bool useWavefront(const vkrt_scene* s) { return s->opt[VKRT_OPT_MODE] == 1; }

void freeAccel(vkrt_scene* s)
{
  s->accel = vkrt::TreeBuffers{};
  s->nodeMasks = vkrt::DevBuf{};
  s->built = false;
  s->refit = vkrt::RefitScratch{};
  s->refitted = false;
  s->stale = false;
}

void noteMasks(vkrt_scene* s)
{
  memset(s->masksPresent, 0, sizeof s->masksPresent);
  for(const vkrt_instance_visibility& v : s->vis)
    s->masksPresent[v.mask >> 6] |= 1ull << (v.mask & 63u);
}

// does every node's mask meet cullMask?  (then a query with that mask and no facing flag walks exactly what vkrt_intersect walks)
bool everyMaskMeets(const vkrt_scene* s, uint32_t cullMask)
{
  for(uint32_t m = 0; m < 256; m++)
    if(((s->masksPresent[m >> 6] >> (m & 63u)) & 1ull) && (m & cullMask) == 0u)
      return false;
  return true;
}

// the node-mask table of the installed wide8 tree from the current instance records, enqueued on `stream` (levels + 1 passes: no read-back)
int computeNodeMasks(vkrt_scene* s, hipStream_t stream)
{
  if(s->dev.layout != 1u || !s->nodeMasks.get())
    return VKRT_OK;
  const uint32_t nodes = (uint32_t)(s->info.node_bytes / VKRT_WNODE_BYTES);
  HIP_TRY(vkrt_launch_node_masks(s->dev, nodes, (uint32_t)s->nodes.size(), s->info.max_depth + 1u, s->nodeMasks.get<uint2>(), stream));
  return VKRT_OK;
}

int setDevice(const vkrt_scene* s)
{
  HIP_TRY(hipSetDevice(s->device));
  return VKRT_OK;
}

// Nodes moved by a device-sourced vkrt_scene_update_node_transforms: bring the matrices of the host copy up to date from the instance
// records (o2w = rows 0-2; the bottom row, which nothing reads, becomes 0 0 0 1).  Synchronises the device.  A matrix that is not finite
// -- the device path does not inspect its values -- is refused like one given to vkrt_scene_create, and the host copy stays as it was.
int downloadNodeTransforms(vkrt_scene* s, const char* who)
{
  if(!s->nodesOnDevice)
    return VKRT_OK;
  const int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  std::vector<DevInstance> inst(s->nodes.size());
  if(!inst.empty())
    HIP_TRY(hipMemcpy(inst.data(), s->dev.instances, inst.size() * sizeof(DevInstance), hipMemcpyDeviceToHost));
  std::vector<vkrt_node> fresh = s->nodes;
  for(size_t i = 0; i < fresh.size(); i++)
  {
    float* M = fresh[i].worldMatrix;
    for(int r = 0; r < 3; r++)
      for(int c = 0; c < 4; c++)
        M[c * 4 + r] = inst[i].o2w[r * 4 + c];
    M[3] = M[7] = M[11] = 0.0f;
    M[15] = 1.0f;
    if(std::string err; vkrt::check_transform(fresh[i], (uint32_t)i, err) != VKRT_OK)
      return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: after a device-sourced vkrt_scene_update_node_transforms: %s", who, err.c_str());
  }
  s->nodes.swap(fresh);
  s->nodesOnDevice = false;
  return VKRT_OK;
}

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
int growEvents(std::vector<vkrt::DevEvent>& owners, std::vector<hipEvent_t>& raw, size_t want, unsigned flags)
{
  while(raw.size() < want)
  {
    vkrt::DevEvent e;
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
  const int rc = ensureWorkingSet(s, tiles * 64u, wfGroupsWanted(s->opt[VKRT_OPT_WF_FRAMES_IN_FLIGHT], frames), stream);
  if(rc != VKRT_OK)
    return rc;
  if(const int rc = growEvents(s->wfPoolOwners, s->wfPool, (size_t)wfPoolEvents((int)std::min<uint32_t>(frames, VKRT_FRAMES_PER_BATCH)), hipEventDisableTiming); rc != VKRT_OK)
    return rc;
  s->wfAsync.pool = s->wfPool.data();
  s->wfAsync.poolSize = (int)s->wfPool.size();
  return VKRT_OK;
}

// traversal workgroup size (the non-default triangle modes exist for the default 64-thread workgroup only)
int travBlock(const vkrt_scene* s) { return (s->dev.watertight || s->dev.dissolve) ? 64 : s->opt[VKRT_OPT_WF_TRAV_BLOCK]; }

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

// the tree can be traced: built, and not moved since (`who` names the caller in the refusal)
int checkBuilt(const vkrt_scene* s, const char* who)
{
  if(!s->built)
    return fail(VKRT_ERR_NOT_BUILT, "%s before vkrt_accel_build", who);
  if(s->stale)
    return fail(VKRT_ERR_NOT_BUILT, "%s after vkrt_scene_update_nodes / vkrt_scene_update_vertices: vkrt_accel_refit or vkrt_accel_build first", who);
  return VKRT_OK;
}

int checkShard(const vkrt_shard* shard)
{
  if(shard->full_width == 0 || shard->full_height == 0)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "empty launch size");
  if(shard->shard_count > 1 && (shard->strip_rows == 0 || shard->shard_index >= shard->shard_count))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "bad shard (strip_rows %u, %u of %u)", shard->strip_rows, shard->shard_index,
                shard->shard_count);
  return VKRT_OK;
}

// 8x8 tiles that cover a shard's rows
int shardTiles(const vkrt_shard* shard, uint32_t& tileCount)
{
  const uint64_t tiles = (uint64_t)((shard->full_width + 7) / 8) * ((vkrt_shard_rows(shard) + 7) / 8);
  if(tiles * 64 >= 0xFFFFFFFFull)
    return fail(VKRT_ERR_UNSUPPORTED, "launch too large");
  tileCount = (uint32_t)tiles;
  return VKRT_OK;
}

// The TraceParams every trace entry point shares: tree, camera, seed, public flags, the shard's rows and its 8x8 tiles, counters.
// Callers check the tree (checkBuilt) and the shard (checkShard) first and add what is their own.
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
  return shardTiles(shard, P.tileCount);
}

// The trace set-up every query entry point shares once its own arguments are checked and n > 0: the tree can be traced, the scene's
// device is current, and the walk's scene carries the call's options.  filter: the filtering walk is needed -- only where it can change
// a result: a facing flag, or a cull mask that some node's mask misses.
int querySetup(vkrt_scene* s, const vkrt_query_opts& q, const char* who, DevQueryScene& qs, bool& filter)
{
  int rc = checkBuilt(s, who);
  if(rc != VKRT_OK)
    return rc;
  if((rc = setDevice(s)) != VKRT_OK)
    return rc;
  static_cast<DevScene&>(qs) = s->dev;
  qs.nodeMasks = s->nodeMasks.get<const uint2>();
  qs.cullMask = q.cull_mask;
  qs.rayFlags = q.ray_flags & (VKRT_RAY_CULL_BACK_FACING | VKRT_RAY_CULL_FRONT_FACING);
  filter = qs.rayFlags != 0u || !everyMaskMeets(s, q.cull_mask);
  return VKRT_OK;
}

static_assert(sizeof(vkrt_ray) == 32 && sizeof(vkrt_hit) == 32, "k_query reads and writes 2 x 16 B per ray");
static_assert(sizeof(vkrt_surface) == 128, "k_hit_surface writes 8 x 16 B per record");
static_assert(sizeof(vkrt_instance_visibility) == 4 && sizeof(vkrt_query_opts) == 16, "include/vkrt.h");
static_assert(sizeof(vkrt_material_alpha) == 8 && sizeof(vkrt_material_alpha) == sizeof(uint2), "k_material_alpha takes (mode, cutoff bits) pairs");
// The argument checks every query entry point starts with, in this order: the scene, then (n > 0) an array that is NULL, then an array
// that is misaligned.  alignText: the call's list of alignments as its message shows it.
struct QueryArray
{
  const void* p;
  unsigned align;  // bytes, a power of two
  bool mayBeNull;
};
int checkQueryArrays(const vkrt_scene* s, const char* who, uint32_t n, std::initializer_list<QueryArray> arrays, const char* alignText)
{
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  if(n == 0)
    return VKRT_OK;
  for(const QueryArray& a : arrays)
    if(!a.p && !a.mayBeNull)
      return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: NULL array", who);
  for(const QueryArray& a : arrays)
    if(((uintptr_t)a.p & (a.align - 1u)) != 0u)
      return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: misaligned array %s", who, alignText);
  return VKRT_OK;
}

// vkrt_intersect / vkrt_occluded (and the _ex pair, whose options are checked by the caller): one k_query launch per 2^30 rays on the
// caller's stream (query.hip); out = hits or occluded flags
int rayQuery(vkrt_scene* s, const vkrt_ray* rays, uint32_t n, const vkrt_query_opts& q, void* out, bool anyHit, void* hip_stream, const char* who)
{
  int rc = checkQueryArrays(s, who, n, {{rays, 16u, false}, {out, anyHit ? 4u : 16u, false}}, "(rays and hits: 16 bytes, occluded: 4)");
  if(rc != VKRT_OK || n == 0)
    return rc;
  DevQueryScene qs;
  bool filter;
  if((rc = querySetup(s, q, who, qs, filter)) != VKRT_OK)
    return rc;
  const bool opaque = (q.ray_flags & VKRT_RAY_OPAQUE) != 0u;
  HIP_TRY(vkrt_launch_query(qs, (const float4*)rays, n, q.anyhit_seed, filter, opaque, s->alphaMasks != 0u, anyHit ? nullptr : (float4*)out, anyHit ? (int*)out : nullptr,
                            (hipStream_t)hip_stream));
  return VKRT_OK;
}

// the options of vkrt_intersect_ex / vkrt_occluded_ex (include/vkrt.h)
int checkQueryOpts(const vkrt_query_opts* q, const char* who)
{
  if(!q)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: opts is NULL", who);
  if(q->struct_size < sizeof(vkrt_query_opts))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: vkrt_query_opts.struct_size %u < %zu (ABI mismatch)", who, q->struct_size, sizeof(vkrt_query_opts));
  const uint32_t known = VKRT_RAY_OPAQUE | VKRT_RAY_CULL_BACK_FACING | VKRT_RAY_CULL_FRONT_FACING;
  if(q->ray_flags & ~known)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: ray_flags 0x%x has bits outside OPAQUE | CULL_BACK_FACING | CULL_FRONT_FACING", who, q->ray_flags);
  if((q->ray_flags & VKRT_RAY_CULL_BACK_FACING) && (q->ray_flags & VKRT_RAY_CULL_FRONT_FACING))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: ray_flags: CULL_BACK_FACING and CULL_FRONT_FACING together", who);
  if(q->cull_mask > 0xFFu)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: cull_mask 0x%x > 0xFF", who, q->cull_mask);
  return VKRT_OK;
}

// vkrt_intersect_multi after its options and max_hits are checked: one k_query_multi launch per 2^30 rays on the caller's stream
// (multihit.hip)
int rayQueryMulti(vkrt_scene* s, const vkrt_ray* rays, uint32_t n, const vkrt_query_opts& q, uint32_t maxHits, vkrt_hit* hits, int32_t* counts,
                  void* hip_stream, const char* who)
{
  int rc = checkQueryArrays(s, who, n, {{rays, 16u, false}, {hits, 16u, false}, {counts, 4u, true}}, "(rays and hits: 16 bytes, counts: 4)");
  if(rc != VKRT_OK || n == 0)
    return rc;
  DevQueryScene qs;
  bool filter;
  if((rc = querySetup(s, q, who, qs, filter)) != VKRT_OK)
    return rc;
  const bool opaque = (q.ray_flags & VKRT_RAY_OPAQUE) != 0u;
  HIP_TRY(vkrt_launch_query_multi(qs, (const float4*)rays, n, q.anyhit_seed, filter, opaque, s->alphaMasks != 0u, maxHits, (float4*)hits, counts, (hipStream_t)hip_stream));
  return VKRT_OK;
}

static_assert(sizeof(vkrt_point_query) == 16, "k_closest_point reads 16 B per query");
// the options of vkrt_closest_point: those of vkrt_intersect_ex (NULL = the defaults), and no ray flag -- a point has no facing and no
// any-hit stage
int checkPointOpts(const vkrt_query_opts* opts, const char* who, vkrt_query_opts& q)
{
  q = vkrt_query_opts{sizeof(vkrt_query_opts), 0u, 0xFFu, 0u};
  if(!opts)
    return VKRT_OK;
  const int rc = checkQueryOpts(opts, who);
  if(rc != VKRT_OK)
    return rc;
  if(opts->ray_flags != 0u)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: ray_flags 0x%x: a point query takes no ray flag", who, opts->ray_flags);
  q = *opts;
  return VKRT_OK;
}

// vkrt_closest_point after its options are checked: one k_closest_point launch per 2^30 queries on the caller's stream (closest.hip)
int pointQuery(vkrt_scene* s, const vkrt_point_query* queries, uint32_t n, const vkrt_query_opts& q, vkrt_hit* hits, void* hip_stream, const char* who)
{
  int rc = checkQueryArrays(s, who, n, {{queries, 16u, false}, {hits, 16u, false}}, "(queries and hits: 16 bytes)");
  if(rc != VKRT_OK || n == 0)
    return rc;
  DevQueryScene qs;
  bool filter;
  if((rc = querySetup(s, q, who, qs, filter)) != VKRT_OK)
    return rc;
  HIP_TRY(vkrt_launch_closest_point(qs, (const float4*)queries, n, filter, (float4*)hits, nullptr, (hipStream_t)hip_stream));
  return VKRT_OK;
}

// a node range [first, first + count) with its array: the checks vkrt_scene_set/get_instance_visibility share after their own
int checkVisibilityRange(const vkrt_scene* s, uint32_t first, uint32_t count, const char* who)
{
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  if((uint64_t)first + count > s->nodes.size())
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: nodes [%u, %llu) outside the scene's %zu nodes", who, first, (unsigned long long)first + count,
                s->nodes.size());
  return VKRT_OK;
}

// the same for a material range of vkrt_scene_set/get_material_alpha
int checkMaterialRange(const vkrt_scene* s, uint32_t first, uint32_t count, const char* who)
{
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  if((uint64_t)first + count > s->materialCount)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: materials [%u, %llu) outside the scene's %u materials", who, first, (unsigned long long)first + count,
                s->materialCount);
  return VKRT_OK;
}

}  // namespace

extern "C" {

int vkrt_abi_version(void) { return VKRT_ABI_VERSION; }
const char* vkrt_last_error(void) { return g_lastError.c_str(); }

int vkrt_device_count(void)
{
  int n = 0;
  if(hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

int vkrt_scene_create(const vkrt_scene_desc* d, int device, vkrt_scene** out)
{
  if(!out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  std::string err;
  int rc = vkrt::validate_scene(d, err);
  if(rc != VKRT_OK)
    return failWith(rc, err);
  const int ndev = vkrt_device_count();
  if(ndev <= 0)
    return fail(VKRT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
  if(device < 0 || device >= ndev)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "device %d out of range [0,%d)", device, ndev);
  vkrt_scene* s = new vkrt_scene();
  s->device = device;
  vkrt::initial_options(s->opt);
  auto bail = [&](int code) {
    vkrt_scene_destroy(s);
    return code;
  };
  if((rc = setDevice(s)) != VKRT_OK)
    return bail(rc);
  hipDeviceProp_t prop;
  if(hipGetDeviceProperties(&prop, device) == hipSuccess)
    s->cuCount = prop.multiProcessorCount;

  s->positions.assign(d->positions, d->positions + 3 * (size_t)d->vertex_count);
  s->indices.assign(d->indices, d->indices + d->index_count);
  s->primMeshes.assign(d->prim_meshes, d->prim_meshes + d->prim_mesh_count);
  s->nodes.assign(d->nodes, d->nodes + d->node_count);
  s->lightCount = d->light_count;
  s->materialCount = d->material_count;
  s->alpha.assign(d->material_count, vkrt::kDefaultAlpha);
  for(uint32_t i = 0; i < d->material_count; i++)
    s->materialAlpha.push_back(d->materials[i].pbrBaseColorFactor[3]);
  s->vis.assign(d->node_count, vkrt::kDefaultVisibility);
  noteMasks(s);

  // VKRT_TEX_QUADS=0 (test hook): no footprint pool
  const char* quadEnv = getenv("VKRT_TEX_QUADS");
  vkrt::PackedScene packed;
  if((rc = vkrt::pack_scene(d, !(quadEnv && atoi(quadEnv) == 0), packed, err)) != VKRT_OK)
    return bail(failWith(rc, err));
  DevScene& D = s->dev;
  const float *pn = nullptr, *lut = nullptr;
  const uint32_t *pm = nullptr, *quads = nullptr;
  if((rc = upload(s, d->positions, 3 * (size_t)d->vertex_count, &D.positions)) != VKRT_OK) return bail(rc);
  if((rc = upload(s, d->indices, (size_t)d->index_count, &D.indices)) != VKRT_OK) return bail(rc);
  if((rc = upload(s, packed.vertexPN.data(), packed.vertexPN.size(), &pn)) != VKRT_OK) return bail(rc);
  if((rc = upload(s, d->lights, (size_t)d->light_count, &D.lights)) != VKRT_OK) return bail(rc);
  if((rc = upload(s, packed.primMeshes.data(), packed.primMeshes.size(), &pm)) != VKRT_OK) return bail(rc);
  if((rc = upload(s, packed.instances.data(), packed.instances.size(), &D.instances)) != VKRT_OK) return bail(rc);
  if((rc = upload(s, packed.materials.data(), packed.materials.size(), &D.materials)) != VKRT_OK) return bail(rc);
  if((rc = upload(s, packed.shadeMaterials.data(), packed.shadeMaterials.size(), &D.shadeMaterials)) != VKRT_OK) return bail(rc);
  if((rc = upload(s, packed.textures.data(), packed.textures.size(), &D.textures)) != VKRT_OK) return bail(rc);
  if((rc = upload(s, packed.texMips.data(), packed.texMips.size(), &D.texMips)) != VKRT_OK) return bail(rc);
  if((rc = upload(s, packed.texels.data(), packed.texels.size(), &D.texels)) != VKRT_OK) return bail(rc);
  if(!packed.texQuads.empty() && (rc = upload(s, packed.texQuads.data(), packed.texQuads.size(), &quads)) != VKRT_OK) return bail(rc);
  if((rc = upload(s, packed.srgbLut, 512, &lut)) != VKRT_OK) return bail(rc);
  D.vertexPN = (const float4*)pn;
  s->surfacePrimMeshes = (const uint4*)pm;
  D.texQuads = (const uint4*)quads;
  D.srgbLut = lut;
  D.textureCount = d->texture_count;
  D.rootRef = VKRT_TRAV_DONE;
  D.stackCap = 1;
  D.layout = 0;
  D.stepLimit = 64;
  D.triThreshold = 0;
  D.shareMinIdle = 0;
  D.sharePeriodMask = 0;
  D.shareFlags = 0;
  D.gbufferMips = 1;

  if(s->tables.alloc(&s->workCounter, 16) != hipSuccess) return bail(fail(VKRT_ERR_OUT_OF_MEMORY, "hipMalloc(work counter)"));
  if(s->tables.alloc(&s->counters, 1) != hipSuccess) return bail(fail(VKRT_ERR_OUT_OF_MEMORY, "hipMalloc(counters)"));
  D.faults = &s->counters->v[0][10];
  if(hipMemset(s->counters, 0, sizeof(DevCounters)) != hipSuccess) return bail(fail(VKRT_ERR_HIP, "hipMemset(counters)"));
  if(s->evStart.create() != hipSuccess || s->evStop.create() != hipSuccess)
    return bail(fail(VKRT_ERR_HIP, "hipEventCreate"));
  *out = s;
  return VKRT_OK;
}

void vkrt_scene_destroy(vkrt_scene* s)
{
  if(!s)
    return;
  (void)hipSetDevice(s->device);
  delete s;
}

int vkrt_scene_set_option(vkrt_scene* s, int option, int value)
{
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "scene is NULL");
  if(option < VKRT_OPT_MODE || option > VKRT_OPT_ALPHA_TEST)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "unknown option %d", option);
  if(vkrt::clamp_option(option, value) != value)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "option %d: value %d out of range", option, value);
  s->opt[option] = value;
  if(option == VKRT_OPT_WF_TRI_LEND && s->built && s->dev.layout == 1u)  // a launch-uniform word of the walk, not a property of the tree: no rebuild needed
    s->dev.shareFlags = (s->dev.shareFlags & ~VKRT_SHARE_TRI_LEND) | (value ? VKRT_SHARE_TRI_LEND : 0u);
  return VKRT_OK;
}

int vkrt_scene_get_option(const vkrt_scene* s, int option, int* value)
{
  if(!s || !value)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  if(option == VKRT_INFO_ANYHIT_ORDER)
  {
    *value = s->built ? (int)(s->dev.shareFlags & 6u) : 0;
    return VKRT_OK;
  }
  if(option == VKRT_INFO_SPLIT_BUDGET)
  {
    *value = s->built ? s->splitResolved : 0;
    return VKRT_OK;
  }
  if(option < VKRT_OPT_MODE || option > VKRT_OPT_ALPHA_TEST)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "unknown option %d", option);
  *value = s->opt[option];
  return VKRT_OK;
}

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
  int rc = checkShard(shard);
  if(rc == VKRT_OK)
    rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  uint32_t tiles = 0;
  if((rc = shardTiles(shard, tiles)) != VKRT_OK)
    return rc;
  // the mode that counts is the one the acceleration structure was built for (vkrt_pathtrace and vkrt_hybrid_trace look at
  // s->wavefront, not at an option that may have changed since); before a build, the option is the best guess there is
  const bool wavefront = s->built ? s->wavefront : useWavefront(s);
  if(tiles == 0 || !wavefront)
    return VKRT_OK;  // the megakernel keeps its state in registers / LDS
  return ensureFrameCall(s, tiles, frames_per_call, (hipStream_t)hip_stream);
}

namespace {

// Moves a builder's record into the scene.
void installTree(vkrt_scene* s, vkrt::BuiltTree& t)
{
  s->accel = std::move(t.buf);
  s->dev.nodes = s->accel.nodes.get<const float4>();
  s->dev.tris = s->accel.tris.get<const float4>();
  s->dev.triShade = s->accel.triShade.get<const uint4>();
  s->dev.layout = t.layout;
  s->dev.rootRef = t.rootRef;
  // (trav_lds.h; traversalSettings adds the room for parked triangle groups)
  s->dev.stackCap = travStackCap(t.layout, t.maxDepth, false, 0u);
  s->info.node_count = t.nodeCount;
  s->info.max_depth = t.maxDepth;
  s->info.sah_cost = t.sahCost;
  s->info.node_bytes = t.nodeBytes;
  s->info.triangle_bytes = t.triangleBytes;
}

// A tree built on the host -- a BVH2 (bvh) or a wide8 tree (w8), exactly one of them -- over `tris`: packs the triangle and shading
// records in its slot order and uploads them with the nodes.  The host SAH builder and the host collapse of a device-built binary tree
// both end here.
int uploadHostTree(vkrt_scene* s, const std::vector<vkrt::FlatTri>& tris, const vkrt::BuiltBvh* bvh, const vkrt::BuiltWide8* w8,
                   const std::vector<uint8_t>* instDissolves, hipStream_t stream, vkrt::BuiltTree& t)
{
  const std::vector<uint32_t>& order = w8 ? w8->triOrder : bvh->triOrder;
  std::vector<float> packed;
  std::vector<uint32_t> shadeRec;
  vkrt::pack_triangles(tris, order, packed, s->dev.watertight != 0, instDissolves);
  vkrt::pack_tri_shade(tris, order, s->indices.data(), s->primMeshes.data(), s->nodes.data(), shadeRec);
  const void* nodeData = w8 ? (const void*)w8->nodes.data() : (const void*)bvh->nodes.data();
  t = w8 ? vkrt::BuiltTree{1, tris.empty() ? VKRT_TRAV_DONE : 0, w8->maxDepth, w8->nodeCount, w8->sahCost, w8->nodes.size() * 4, packed.size() * 4}
         : vkrt::BuiltTree{0, bvh->rootRef, bvh->maxDepth, (uint32_t)(bvh->nodes.size() / 16), bvh->sahCost, bvh->nodes.size() * 4, packed.size() * 4};
  hipError_t e = hipSuccess;
  auto tryHip = [&](hipError_t x) { if(e == hipSuccess) e = x; };
  tryHip(t.buf.nodes.alloc(std::max<size_t>(t.nodeBytes, VKRT_WNODE_MIN_ALLOC)));
  tryHip(t.buf.tris.alloc(std::max<size_t>(t.triangleBytes, 48)));
  tryHip(t.buf.triShade.alloc(std::max<size_t>(shadeRec.size() * 4, 16)));
  if(e == hipSuccess && t.nodeBytes) tryHip(hipMemcpyAsync(t.buf.nodes.get(), nodeData, t.nodeBytes, hipMemcpyHostToDevice, stream));
  if(e == hipSuccess && !packed.empty()) tryHip(hipMemcpyAsync(t.buf.tris.get(), packed.data(), t.triangleBytes, hipMemcpyHostToDevice, stream));
  if(e == hipSuccess && !shadeRec.empty()) tryHip(hipMemcpyAsync(t.buf.triShade.get(), shadeRec.data(), shadeRec.size() * 4, hipMemcpyHostToDevice, stream));
  if(e == hipSuccess) tryHip(hipStreamSynchronize(stream));  // (the host arrays end with this call)
  std::string m;
  const int rc = vkrt::hip_status(e, "uploading the acceleration structure", m);
  return rc == VKRT_OK ? VKRT_OK : fail(rc, "%s", m.c_str());
}

// The traversal settings of the installed tree: step bound, any-hit order, triangle postponing and work sharing (from the options),
// and the LDS stack they need.
int traversalSettings(vkrt_scene* s)
{
  s->info.reference_count = s->dev.triCount;
  s->dev.stepLimit = 4u * (s->info.node_count + s->dev.triCount) + 64u;
  s->dev.triThreshold = 0;
  s->dev.shareMinIdle = 0;
  s->dev.sharePeriodMask = 0;
  // order of any-hit walks (bits 1, 2: every layout and mode; traverse.h anyhit_far_first).  Bit 3 = automatic: far-first for rays that
  // end outside the scene bounds unless the scene has LARGE triangles -- room-sized polygons sit in the leaves of the top nodes and
  // stop such rays within a step or two of a front-to-back walk, which the far-first order then only delays (measured on the two
  // tessellations of the atrium, profiles/r03_experiments.md #94: +3.3 % on the uniform one, -2 % on the Sponza-like one).  Round 5: that
  // holds while the large triangles enter the tree WHOLE; pre-split into references (VKRT_OPT_SPLIT_BUDGET) they are spread over the
  // tree like any other geometry and far-first wins again -- the Sponza-like building rotated 20 / 45 / 35+20 degrees with the automatic
  // budget: -2.2 % / -2.9 % / -2.0 % traversal time, the rotated uniform one -2.5 % ... -3.1 % (profiles/r05_experiments.md #144)
  s->dev.shareFlags = (uint32_t)s->opt[VKRT_OPT_WF_SHARE_FLAGS] & 6u;
  const bool largeWhole = s->hasLargeTriangles && s->info.reference_count == s->info.triangle_count;
  if((s->opt[VKRT_OPT_WF_SHARE_FLAGS] & 8) && !largeWhole)
    s->dev.shareFlags |= 4u;
  if(s->dev.layout == 1)
  {
    // triangle postponing (traverse_wide.h): lanes with pending triangles before a wave tests them; 0 = immediate
    s->dev.triThreshold = (uint32_t)s->opt[VKRT_OPT_TRI_THRESHOLD];
    // room for parked triangle groups (uint2 entries).  The stack is what decides how many traversal waves a CU holds: six per SIMD
    // up to wide depth 9, five beyond (travLdsPlan, trav_lds.h)
    s->dev.stackCap = travStackCap(1u, s->info.max_depth, s->dev.triThreshold != 0u, VKRT_W8_POSTPONE_ROOM);
    // work sharing inside a traversal wave (traverse_share.h): minimum number of idle lanes before they take over subtrees
    s->dev.shareMinIdle = (uint32_t)s->opt[VKRT_OPT_WF_SHARE];
    s->dev.sharePeriodMask = (uint32_t)s->opt[VKRT_OPT_WF_SHARE_PERIOD];
    s->dev.shareFlags |= (uint32_t)s->opt[VKRT_OPT_WF_SHARE_FLAGS] & 17u;  // bit 0: child donation, bit 4: triangle-group donation
    if(s->opt[VKRT_OPT_WF_TRI_LEND])
      s->dev.shareFlags |= VKRT_SHARE_TRI_LEND;
  }
  // LDS budget: stackCap * 256 lanes * 4 B must fit a workgroup (160 KiB per CU on gfx950)
  if((size_t)s->dev.stackCap * 256 * 4 > 64 * 1024)
    return fail(VKRT_ERR_UNSUPPORTED, "BVH depth %u needs a %zu-byte LDS stack per workgroup (limit 64 KiB)", s->info.max_depth,
                (size_t)s->dev.stackCap * 256 * 4);
  return VKRT_OK;
}

// One build with a given pre-split budget (read by the device builders only): validate flags -> free the old tree -> build (host or
// device) -> install -> scene bounds -> traversal settings.
int accelBuildOnce(vkrt_scene* s, uint32_t flags, int splitBudget, hipStream_t stream)
{
  if(flags == 0)
    flags = VKRT_BUILD_DEFAULT;
  const bool wantPloc = (flags & VKRT_BUILD_PLOC_GPU) != 0;
  const bool wantLbvh = (flags & VKRT_BUILD_LBVH_GPU) != 0 || wantPloc, wantSah = (flags & VKRT_BUILD_SAH_HOST) != 0;
  if(wantLbvh == wantSah || (wantPloc && (flags & VKRT_BUILD_LBVH_GPU) != 0) || (flags & ~7u) != 0)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "build_flags must select exactly one of VKRT_BUILD_LBVH_GPU / VKRT_BUILD_PLOC_GPU / VKRT_BUILD_SAH_HOST");
  int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  HIP_TRY(hipStreamSynchronize(stream));  // no trace may be reading the old tree
  freeAccel(s);
  const auto t0 = std::chrono::steady_clock::now();
  s->info = vkrt_accel_info{};
  s->info.build_flags = wantPloc ? VKRT_BUILD_PLOC_GPU : wantLbvh ? VKRT_BUILD_LBVH_GPU : VKRT_BUILD_SAH_HOST;
  s->wavefront = useWavefront(s);
  const bool watertight = s->opt[VKRT_OPT_WATERTIGHT] != 0;
  if((watertight || s->opt[VKRT_OPT_ANYHIT_DISSOLVE] != 0) && useWavefront(s) && s->opt[VKRT_OPT_WF_TRAV_BLOCK] != 64)
    return fail(VKRT_ERR_UNSUPPORTED, "VKRT_OPT_WATERTIGHT / VKRT_OPT_ANYHIT_DISSOLVE are built for the default 64-thread traversal workgroups "
                "(VKRT_OPT_WF_TRAV_BLOCK = %d)", s->opt[VKRT_OPT_WF_TRAV_BLOCK]);
  // per instance: is its material non-opaque (dissolve = pbrBaseColorFactor.a < 1)?  The stage is compiled into the traversal only when
  // the scene has such an instance: without one no record carries the flag, the stage could never ignore a hit, and the flag test
  // and seed load per ray would cost 3.8 % for nothing (profiles/r03_options/ANYHIT_DISSOLVE.json)
  std::vector<uint8_t> instDissolves;
  bool dissolve = false;
  if(s->opt[VKRT_OPT_ANYHIT_DISSOLVE] != 0)
    for(const vkrt_node& n : s->nodes)
    {
      const int32_t m = std::max(0, s->primMeshes[(size_t)n.primMesh].materialIndex);
      const bool nonOpaque = s->materialAlpha[(size_t)m] < 1.0f && s->primMeshes[(size_t)n.primMesh].indexCount >= 3u;
      instDissolves.push_back(nonOpaque ? 1 : 0);
      dissolve = dissolve || nonOpaque;
    }
  s->dev.watertight = watertight ? 1u : 0u;
  s->dev.dissolve = dissolve ? 1u : 0u;
  const std::vector<uint8_t>* dissolvePtr = dissolve ? &instDissolves : nullptr;
  // wide8 (compressed 8-wide) is the trace-optimised layout; the megakernel and VKRT_OPT_BVH_LAYOUT = 0 keep BVH2
  const bool wide = useWavefront(s) && s->opt[VKRT_OPT_BVH_LAYOUT] == 1;

  vkrt::BuiltTree tree;
  if(wantSah)
  {
    std::vector<vkrt::FlatTri> tris;
    vkrt::flatten_instances(s->positions.data(), s->indices.data(), s->primMeshes.data(), s->nodes.data(),
                            (uint32_t)s->nodes.size(), tris);
    vkrt::BuiltBvh bvh;
    vkrt::BuiltWide8 w8;
    if(wide)
      vkrt::build_wide8_host(tris, w8, watertight);
    else
      vkrt::build_sah_host(tris, 4, bvh, watertight);
    if((rc = uploadHostTree(s, tris, wide ? nullptr : &bvh, wide ? &w8 : nullptr, dissolvePtr, stream, tree)) != VKRT_OK)
      return rc;
    s->dev.triCount = (uint32_t)tris.size();
    s->info.triangle_count = (uint32_t)tris.size();
  }
  else
  {
    // GPU radix-tree build (Morton codes, sort, Karras hierarchy, bottom-up fit).  For the trace-optimised layout the
    // binary tree keeps one triangle per leaf and is collapsed into wide8 nodes by the same SAH-optimal DP as the SAH
    // path -- on the device too (wide_collapse.hip); nothing but four statistics words comes back to the host.
    // VKRT_BUILD_PLOC_GPU: same pipeline with the radix tree replaced by locally-ordered clustering (ploc.hip)
    vkrt::LbvhParams p;
    p.wide = wide;
    p.ploc = wantPloc;
    p.splitPercent = (unsigned)splitBudget;
    vkrt::LbvhResult r;
    rc = vkrt::build_lbvh_device(s->dev, (uint32_t)s->nodes.size(), s->primMeshes, s->nodes, p, stream, r);
    if(rc != VKRT_OK)
      return fail(rc, "%s build failed: %s", wantPloc ? "PLOC" : "LBVH", r.error.c_str());
    s->info.triangle_count = r.uniqueTris;
    s->dev.triCount = r.triCount;  // slots: a pre-split triangle occupies one per reference
    if(r.wide.buf.nodes.get())
      tree = std::move(r.wide);
    else if(wide && r.triCount > 0)
    {
      // fallback (a single triangle, or a radix tree too deep for the device collapse's level budget): download the binary
      // tree (device layout == host layout of BuiltBvh) and the sorted triangle records, collapse on the host
      vkrt::BuiltBvh b2;
      b2.nodes.resize((size_t)r.tree.nodeCount * 16);
      std::vector<float> records((size_t)r.triCount * 12);
      hipError_t e = hipSuccess;
      if(r.tree.nodeCount) e = hipMemcpy(b2.nodes.data(), r.tree.buf.nodes.get(), b2.nodes.size() * 4, hipMemcpyDeviceToHost);
      if(e == hipSuccess) e = hipMemcpy(records.data(), r.tree.buf.tris.get(), records.size() * 4, hipMemcpyDeviceToHost);
      r.tree.buf = vkrt::TreeBuffers{};  // (freed before the wide tree is uploaded)
      if(e != hipSuccess)
        return fail(VKRT_ERR_HIP, "LBVH download: %s", hipGetErrorString(e));
      b2.rootRef = r.tree.rootRef;
      b2.maxDepth = r.tree.maxDepth;
      b2.triOrder.resize(r.triCount);
      // (decoded p1 = v0 + e1 is not the exact vertex, but the boxes of the collapse only grow by it; pack_triangles sets the any-hit
      // flag that decoding clears again)
      std::vector<vkrt::FlatTri> tris(r.triCount);
      for(uint32_t k = 0; k < r.triCount; k++)
      {
        b2.triOrder[k] = k;
        tris[k] = vkrt::unpack_triangle(&records[(size_t)k * 12], watertight);
      }
      vkrt::BuiltWide8 w8;
      vkrt::collapse_wide8(b2, tris, w8, watertight);
      if((rc = uploadHostTree(s, tris, nullptr, &w8, dissolvePtr, stream, tree)) != VKRT_OK)
        return rc;
    }
    else
      tree = std::move(r.tree);
  }
  installTree(s, tree);
  vkrt::scene_bounds(s->positions, s->indices, s->primMeshes, s->nodes, s->dev.sceneLo, s->dev.sceneHi, s->hasLargeTriangles);
  if((rc = traversalSettings(s)) != VKRT_OK)
    return rc;
  if(s->dev.layout == 1u)
  {  // the node-mask table of the ray-query filter lives and dies with the tree
    HIP_TRY(s->nodeMasks.alloc(std::max<size_t>(s->info.node_bytes / VKRT_WNODE_BYTES * 8, 16)));
    if((rc = computeNodeMasks(s, stream)) != VKRT_OK)
      return rc;
  }
  s->info.build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  s->built = true;
  return VKRT_OK;
}

}  // namespace

// VKRT_OPT_SPLIT_BUDGET = -1: the library decides.  Triangle pre-splitting pays where large triangles are not aligned with the axes
// (+14 % ... +97 % on a rotated building) and costs 1-8 % elsewhere (profiles/r05_split_rotated.jsonl), and the SAH cost of the finished
// tree tells the two apart: a 30 % budget lowers it by 18-30 % in the first case and by at most 5 % -- or raises it -- in the second.
// So: build with a 30 % budget, build without, keep the split tree only when its cost is below 0.9 of the unsplit one (one more build
// in that case; device builds are ~13 ms each for 262 k triangles).  Pixels do not depend on the outcome.
int vkrt_accel_build(vkrt_scene* s, uint32_t flags, void* hip_stream)
{
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "scene is NULL");
  hipStream_t stream = (hipStream_t)hip_stream;
  if(s->positionsOnDevice)
  {  // vertices moved by a device-sourced vkrt_scene_update_vertices: the host builder and scene_bounds read the host copy
    int rc = setDevice(s);
    if(rc != VKRT_OK)
      return rc;
    HIP_TRY(hipDeviceSynchronize());
    if(!s->positions.empty())
      HIP_TRY(hipMemcpy(s->positions.data(), s->dev.positions, s->positions.size() * sizeof(float), hipMemcpyDeviceToHost));
    s->positionsOnDevice = false;
  }
  // nodes moved by a device-sourced vkrt_scene_update_node_transforms: every builder and scene_bounds read the matrices of the host copy
  if(const int rc = downloadNodeTransforms(s, "vkrt_accel_build"); rc != VKRT_OK)
    return rc;
  const bool deviceBuild = flags == 0 || (flags & (VKRT_BUILD_LBVH_GPU | VKRT_BUILD_PLOC_GPU)) != 0;
  if(s->opt[VKRT_OPT_SPLIT_BUDGET] >= 0 || !deviceBuild)
  {
    s->splitResolved = std::max(0, s->opt[VKRT_OPT_SPLIT_BUDGET]);  // (the host builder does not split)
    return accelBuildOnce(s, flags, s->splitResolved, stream);
  }
  const auto t0 = std::chrono::steady_clock::now();
  float sahSplit = 0.0f;
  int rc = accelBuildOnce(s, flags, 30, stream);
  if(rc == VKRT_OK)
  {
    sahSplit = s->info.sah_cost;
    rc = accelBuildOnce(s, flags, 0, stream);
  }
  s->splitResolved = 0;
  if(rc == VKRT_OK && sahSplit < 0.9f * s->info.sah_cost)
  {
    rc = accelBuildOnce(s, flags, 30, stream);
    s->splitResolved = 30;
  }
  if(rc == VKRT_OK)
    s->info.build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();  // all the builds it took
  return rc;
}

int vkrt_accel_get_info(const vkrt_scene* s, vkrt_accel_info* out)
{
  if(!s || !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  if(!s->built)
    return fail(VKRT_ERR_NOT_BUILT, "vkrt_accel_build has not been called");
  *out = s->info;
  if(s->refitted && s->refit.levelStart.size() > 1)
  {  // the refitted tree's SAH cost (k_rf_finish), same formula as the builders'; reading it waits for the refit
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&out->sah_cost, &s->refit.words[2], 4, hipMemcpyDeviceToHost));
  }
  return VKRT_OK;
}

int vkrt_scene_update_nodes(vkrt_scene* s, uint32_t first, uint32_t count, const vkrt_node* nodes, void* hip_stream)
{
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "scene is NULL");
  if(count && !nodes)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "nodes is NULL");
  if((uint64_t)first + count > s->nodes.size())
    return fail(VKRT_ERR_INVALID_ARGUMENT, "nodes [%u, %llu) outside the scene's %zu nodes", first, (unsigned long long)first + count, s->nodes.size());
  // the rules of vkrt_scene_create, checked for the whole range before anything changes (a refused call leaves the scene as it was)
  for(uint32_t i = 0; i < count; i++)
  {
    if(nodes[i].primMesh != s->nodes[(size_t)first + i].primMesh)
      return fail(VKRT_ERR_INVALID_ARGUMENT, "node %u: primMesh %d != %d (an update moves instances, it does not change their geometry)", first + i,
                  nodes[i].primMesh, s->nodes[(size_t)first + i].primMesh);
    if(std::string err; vkrt::check_transform(nodes[i], first + i, err) != VKRT_OK)
      return failWith(VKRT_ERR_INVALID_ARGUMENT, err);
  }
  if(count == 0)
    return VKRT_OK;
  int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  std::vector<DevInstance> inst(count);
  for(uint32_t i = 0; i < count; i++)
    vkrt::make_instance(nodes[i], s->vis[(size_t)first + i], inst[i]);  // (the visibility word stays; the mirrored bit follows the new matrix)
  // Stream-ordered: the records travel as kernel arguments of launches on hip_stream, after whatever the caller enqueued there before
  // (a trace that still reads the old transforms) and before whatever comes after (the refit, the next trace).  The trace entry points'
  // internal lane streams fork from and join to the caller's stream, so ordering on it is all that is needed.
  HIP_TRY(vkrt::upload_instances(const_cast<DevInstance*>(s->dev.instances), first, count, inst.data(), (hipStream_t)hip_stream));
  std::copy(nodes, nodes + count, s->nodes.begin() + first);
  // (the any-hit stage's per-instance dissolve flags -- bit 31 of the records' id words -- follow from primMesh, which an update keeps)
  if(s->built)
    s->stale = true;
  return VKRT_OK;
}

int vkrt_accel_refit(vkrt_scene* s, void* hip_stream)
{
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "scene is NULL");
  if(!s->built)
    return fail(VKRT_ERR_NOT_BUILT, "vkrt_accel_refit before vkrt_accel_build");
  int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  std::string err;
  if(!s->refit.mem.get())
  {  // first refit of this build: scratch + level lists (the one place a refit allocates and synchronises)
    const uint32_t nodeCap = (uint32_t)(s->info.node_bytes / (s->dev.layout == 1u ? VKRT_WNODE_BYTES : 64u));
    if((rc = vkrt::refit_prepare(s->dev, nodeCap, stream, s->refit, err)) != VKRT_OK)
    {
      s->refit = vkrt::RefitScratch{};
      return fail(rc, "vkrt_accel_refit: %s", err.c_str());
    }
  }
  // Everything the build decided stays: layout, record format, split references, dissolve flags, any-hit order, stackCap, step bound.
  // sceneLo / sceneHi (read only by the any-hit order heuristic, which cannot change a pixel) also stay as built: updating them would
  // need the new bounds on the host, i.e. a synchronisation.
  if((rc = vkrt::refit_enqueue(s->dev, (uint32_t)s->nodes.size(), s->refit, stream, err)) != VKRT_OK)
    return fail(rc, "vkrt_accel_refit: %s", err.c_str());
  s->refitted = true;
  s->stale = false;
  return VKRT_OK;
}

int vkrt_scene_update_node_transforms(vkrt_scene* s, const vkrt_node_update* u, void* hip_stream)
{
  const char* who = "vkrt_scene_update_node_transforms";
  const int bad = VKRT_ERR_INVALID_ARGUMENT;
  if(!u)
    return fail(bad, "%s: update is NULL", who);
  if(u->struct_size < sizeof(vkrt_node_update))
    return fail(bad, "%s: vkrt_node_update.struct_size %u < %zu (ABI mismatch)", who, u->struct_size, sizeof(vkrt_node_update));
  if(u->memory != VKRT_MEMORY_HOST && u->memory != VKRT_MEMORY_DEVICE)
    return fail(bad, "%s: memory %u is neither VKRT_MEMORY_HOST nor VKRT_MEMORY_DEVICE", who, u->memory);
  if(u->node_indices && u->first != 0)
    return fail(bad, "%s: first is %u with node_indices given (a sparse update takes first = 0)", who, u->first);
  if(!s)
    return fail(bad, "%s: scene is NULL", who);
  const size_t nodeCount = s->nodes.size(), n = u->count;
  if(!u->node_indices && (uint64_t)u->first + u->count > nodeCount)
    return fail(bad, "%s: nodes [%u, %llu) outside the scene's %zu nodes", who, u->first, (unsigned long long)u->first + u->count, nodeCount);
  if(n && !u->world_matrices)
    return fail(bad, "%s: world_matrices is NULL", who);
  const bool host = u->memory == VKRT_MEMORY_HOST;
  if(!host)
  {
    if(((uintptr_t)u->world_matrices & 15u) != 0)
      return fail(bad, "%s: world_matrices %p is not 16-byte aligned", who, (const void*)u->world_matrices);
    if(((uintptr_t)u->node_indices & 3u) != 0)
      return fail(bad, "%s: node_indices %p is not 4-byte aligned", who, (const void*)u->node_indices);
  }
  else
  {  // the rules of vkrt_scene_update_nodes, checked for every entry before anything changes
    if(u->node_indices)
      for(size_t k = 0; k < n; k++)
        if(u->node_indices[k] >= nodeCount)
          return fail(bad, "%s: node_indices[%zu] is %u, outside the scene's %zu nodes", who, k, u->node_indices[k], nodeCount);
    for(size_t k = 0; k < 16 * n; k++)
      if(!std::isfinite(u->world_matrices[k]))
        return fail(bad, "%s: world_matrices[%zu] (entry %zu, node %u) is not finite", who, k, k / 16,
                    u->node_indices ? u->node_indices[k / 16] : u->first + (uint32_t)(k / 16));
  }
  if(n == 0)
    return VKRT_OK;
  if(!host)
  {
    const int rc = setDevice(s);
    if(rc != VKRT_OK)
      return rc;
    // One launch on hip_stream, stream-ordered like vkrt_scene_update_nodes; no allocation, no copy, no wait.  The host copy of the
    // matrices falls behind: its readers download the records first (downloadNodeTransforms).
    HIP_TRY(vkrt::launch_node_transforms(const_cast<DevInstance*>(s->dev.instances), (uint32_t)nodeCount, u->first, u->count, u->world_matrices,
                                         u->node_indices, (hipStream_t)hip_stream));
    s->nodesOnDevice = true;
    if(s->built)
      s->stale = true;
    return VKRT_OK;
  }
  // host memory: vkrt_scene_update_nodes itself -- the dense form in one call, the sparse form run by run of consecutive indices, in the
  // order given (so the last of several entries for one node wins)
  std::vector<vkrt_node> nodes(n);
  for(size_t k = 0; k < n; k++)
  {
    std::copy(u->world_matrices + 16 * k, u->world_matrices + 16 * k + 16, nodes[k].worldMatrix);
    nodes[k].primMesh = s->nodes[u->node_indices ? u->node_indices[k] : (size_t)u->first + k].primMesh;
  }
  if(!u->node_indices)
    return vkrt_scene_update_nodes(s, u->first, u->count, nodes.data(), hip_stream);
  for(size_t k = 0; k < n;)
  {
    size_t end = k + 1;
    while(end < n && u->node_indices[end] == u->node_indices[end - 1] + 1u)
      end++;
    if(const int rc = vkrt_scene_update_nodes(s, u->node_indices[k], (uint32_t)(end - k), &nodes[k], hip_stream); rc != VKRT_OK)
      return rc;
    k = end;
  }
  return VKRT_OK;
}

int vkrt_debug_read_instances(vkrt_scene* s, uint32_t first, uint32_t count, void* out, uint64_t bytes)
{
  const char* who = "vkrt_debug_read_instances";
  if(!s || !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
  if((uint64_t)first + count > s->nodes.size())
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: nodes [%u, %llu) outside the scene's %zu nodes", who, first, (unsigned long long)first + count,
                s->nodes.size());
  if(bytes != (uint64_t)count * sizeof(DevInstance))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: bytes %llu != %zu x %u records", who, (unsigned long long)bytes, sizeof(DevInstance), count);
  const int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  if(count)
    HIP_TRY(hipMemcpy(out, s->dev.instances + first, (size_t)count * sizeof(DevInstance), hipMemcpyDeviceToHost));
  return VKRT_OK;
}

int vkrt_scene_update_vertices(vkrt_scene* s, const vkrt_vertex_update* u, void* hip_stream)
{
  CHECK_TRY(check_update_desc(u, err));
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_scene_update_vertices: scene is NULL");
  CHECK_TRY(check_update_range(*u, s->positions.size() / 3, err));
  const bool host = u->memory == VKRT_MEMORY_HOST;
  const size_t n = u->count;
  if(n == 0 || (!u->positions && !u->normals && !u->tangents && !u->texcoords0))
    return VKRT_OK;
  int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  vkrt::VertexUpdate d;
  d.first = u->first;
  d.count = u->count;
  d.positions = u->positions; d.normals = u->normals; d.tangents = u->tangents; d.texcoords0 = u->texcoords0;
  if(host)  // the given arrays through the staging buffer, 16-byte elements first, so every part starts aligned for its loads
    HIP_TRY(s->vertexStage.put({{u->tangents, 4 * n, &d.tangents}, {u->texcoords0, 2 * n, &d.texcoords0}, {u->positions, 3 * n, &d.positions},
                                {u->normals, 3 * n, &d.normals}}, stream));
  // Stream-ordered like vkrt_scene_update_nodes: one launch on hip_stream, after whatever still reads the old vertices and before the
  // refit and the next trace (whose internal lane streams fork from and join to the caller's stream).
  HIP_TRY(vkrt::launch_vertex_update(const_cast<float*>(s->dev.positions), const_cast<float4*>(s->dev.vertexPN), d, stream));
  if(host)
  {
    HIP_TRY(hipStreamSynchronize(stream));  // the caller's arrays and the staging buffer are free again
    if(u->positions)
      std::copy(u->positions, u->positions + 3 * n, s->positions.begin() + 3 * (size_t)u->first);
  }
  if(u->positions)
    positionsMoved(s, host);
  return VKRT_OK;
}

int vkrt_scene_add_skin(vkrt_scene* s, const vkrt_skin_desc* k, void* hip_stream, uint32_t* out_skin)
{
  const char* who = "vkrt_scene_add_skin";
  CHECK_TRY(check_skin_desc(k, err));
  if(!out_skin)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: out_skin is NULL", who);
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  CHECK_TRY(check_skin_range(*k, s->positions.size() / 3, rangesOf(s->skins), rangesOf(s->morphs), err));
  int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  const size_t n = k->count;
  vkrt_scene::Skin skin;
  skin.jointCount = k->joint_count;
  HIP_TRY(skin.mem.alloc(vkrt::skin_bytes(k->count)));
  vkrt::skin_carve(skin.mem.get(), k->first, k->count, skin.arrays);
  HIP_TRY(hipMemcpy(skin.arrays.joints, k->joints, n * 4 * sizeof(uint16_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(skin.arrays.weights, k->weights, n * 4 * sizeof(float), hipMemcpyHostToDevice));
  // stream-ordered like the update calls: the bind pose is what the updates enqueued before this call on hip_stream left
  HIP_TRY(vkrt::launch_pose_capture(s->dev.positions, s->dev.vertexPN, k->first, k->count, skin.arrays.bind, (hipStream_t)hip_stream));
  *out_skin = (uint32_t)s->skins.size();
  s->skins.push_back(std::move(skin));
  return VKRT_OK;
}

int vkrt_scene_skin_vertices(vkrt_scene* s, uint32_t skin, const float* joint_matrices, uint32_t memory, void* hip_stream)
{
  const char* who = "vkrt_scene_skin_vertices";
  CHECK_TRY(check_memory(who, memory, err));
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  CHECK_TRY(check_skin_index(skin, s->skins.size(), err));
  const vkrt_scene::Skin& k = s->skins[skin];
  CHECK_TRY(check_joint_matrices(joint_matrices, memory, k.jointCount, err));
  const bool host = memory == VKRT_MEMORY_HOST;
  int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  const float* palette = joint_matrices;
  if(host)
    HIP_TRY(s->vertexStage.put({{joint_matrices, (size_t)k.jointCount * 16, &palette}}, stream));
  HIP_TRY(vkrt::launch_skin(const_cast<float*>(s->dev.positions), const_cast<float4*>(s->dev.vertexPN), k.arrays, (const float4*)palette, stream));
  if(host)
    HIP_TRY(hipStreamSynchronize(stream));  // the caller's matrices and the staging buffer are free again
  positionsMoved(s);  // (host matrices too: the posed positions exist on the device only)
  return VKRT_OK;
}

int vkrt_scene_add_morph(vkrt_scene* s, const vkrt_morph_desc* m, void* hip_stream, uint32_t* out_morph)
{
  const char* who = "vkrt_scene_add_morph";
  CHECK_TRY(check_morph_desc(m, err));
  if(!out_morph)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: out_morph is NULL", who);
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  int inSkin = -1;
  CHECK_TRY(check_morph_range(*m, s->positions.size() / 3, rangesOf(s->skins), rangesOf(s->morphs), inSkin, err));
  int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  const size_t n = m->count, floats = (size_t)m->target_count * n * 3;
  const float* const deltas[3] = {m->position_deltas, m->normal_deltas, m->tangent_deltas};
  vkrt_scene::Morph morph;
  morph.skin = inSkin;
  const bool has[3] = {deltas[0] != nullptr, deltas[1] != nullptr, deltas[2] != nullptr};
  if(morph.mem.alloc(vkrt::morph_bytes(m->count, m->target_count, has[0], has[1], has[2])) != hipSuccess)
  {
    (void)hipGetLastError();
    return fail(VKRT_ERR_OUT_OF_MEMORY, "%s: no device memory for %u targets of %u vertices", who, m->target_count, m->count);
  }
  vkrt::MorphArrays& a = morph.arrays;
  vkrt::morph_carve(morph.mem.get(), m->first, m->count, m->target_count, has[0], has[1], has[2], a);
  float* const dst[3] = {a.dPos, a.dNrm, a.dTan};
  for(int i = 0; i < 3; i++)
    if(deltas[i])
      HIP_TRY(hipMemcpy(dst[i], deltas[i], floats * sizeof(float), hipMemcpyHostToDevice));
  // stream-ordered like the update calls: the base is what the calls enqueued before this one on hip_stream left
  hipStream_t stream = (hipStream_t)hip_stream;
  if(inSkin < 0)
    HIP_TRY(vkrt::launch_pose_capture(s->dev.positions, s->dev.vertexPN, a.first, a.count, a.base, stream));
  else
  {
    const vkrt::SkinArrays& k = s->skins[inSkin].arrays;
    const vkrt::Pose bind = k.bind.at(m->first - k.first);
    HIP_TRY(hipMemcpyAsync(a.base.pn, bind.pn, n * sizeof(float4), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(a.base.nyz, bind.nyz, n * sizeof(float2), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(a.base.tan, bind.tan, n * sizeof(float4), hipMemcpyDeviceToDevice, stream));
  }
  *out_morph = (uint32_t)s->morphs.size();
  s->morphs.push_back(std::move(morph));
  return VKRT_OK;
}

int vkrt_scene_morph_vertices(vkrt_scene* s, uint32_t morph, const float* weights, uint32_t memory, void* hip_stream)
{
  const char* who = "vkrt_scene_morph_vertices";
  CHECK_TRY(check_memory(who, memory, err));
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  CHECK_TRY(check_morph_index(morph, s->morphs.size(), err));
  const vkrt_scene::Morph& m = s->morphs[morph];
  CHECK_TRY(check_morph_weights(weights, memory, m.arrays.targetCount, err));
  const bool host = memory == VKRT_MEMORY_HOST;
  int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  const float* w = weights;
  if(host)
    HIP_TRY(s->vertexStage.put({{weights, m.arrays.targetCount, &w}}, stream));
  if(m.skin >= 0)
  {  // morph, then skin: the skin's next pose reads the morphed bind pose; the live arrays and the tree are as they were
    const vkrt::SkinArrays& k = s->skins[m.skin].arrays;
    HIP_TRY(vkrt::launch_morph_bind(k.bind.at(m.arrays.first - k.first), m.arrays, w, stream));
  }
  else
    HIP_TRY(vkrt::launch_morph_live(const_cast<float*>(s->dev.positions), const_cast<float4*>(s->dev.vertexPN), m.arrays, w, stream));
  if(host)
    HIP_TRY(hipStreamSynchronize(stream));  // the caller's weights and the staging buffer are free again
  if(m.skin < 0)
    positionsMoved(s);  // (host weights too: the morphed positions exist on the device only; inside a skin no live vertex moved)
  return VKRT_OK;
}

int vkrt_debug_read_vertices(vkrt_scene* s, uint32_t first, uint32_t count, float* positions, float* normals, float* tangents, float* texcoords0)
{
  const char* who = "vkrt_debug_read_vertices";
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  CHECK_TRY(check_vertex_range(who, first, count, s->positions.size() / 3, err));
  if(!positions && !normals && !tangents && !texcoords0)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: positions, normals, tangents and texcoords0 are all NULL", who);
  const int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  if(count == 0)
    return VKRT_OK;
  const size_t n = count;
  if(positions)
    HIP_TRY(hipMemcpy(positions, s->dev.positions + 3 * (size_t)first, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if(normals || tangents || texcoords0)
  {  // quad 0 = position.xyz, normal.x; quad 1 = normal.yz, uv; quad 2 = tangent
    std::vector<float> rec(n * 4 * VKRT_VERTEX_QUADS);
    HIP_TRY(hipMemcpy(rec.data(), s->dev.vertexPN + VKRT_VERTEX_QUADS * (size_t)first, rec.size() * sizeof(float), hipMemcpyDeviceToHost));
    for(size_t i = 0; i < n; i++)
    {
      const float* r = &rec[i * 4 * VKRT_VERTEX_QUADS];
      if(normals)
        normals[3 * i] = r[3], normals[3 * i + 1] = r[4], normals[3 * i + 2] = r[5];
      if(texcoords0)
        texcoords0[2 * i] = r[6], texcoords0[2 * i + 1] = r[7];
      if(tangents)
        std::copy(r + 8, r + 12, tangents + 4 * i);
    }
  }
  return VKRT_OK;
}

int vkrt_intersect(vkrt_scene* s, const vkrt_ray* rays, uint32_t n, uint32_t anyhit_seed, vkrt_hit* hits, void* hip_stream)
{
  const vkrt_query_opts q = {sizeof(vkrt_query_opts), 0u, 0xFFu, anyhit_seed};
  return rayQuery(s, rays, n, q, hits, false, hip_stream, "vkrt_intersect");
}

int vkrt_occluded(vkrt_scene* s, const vkrt_ray* rays, uint32_t n, uint32_t anyhit_seed, int32_t* occluded, void* hip_stream)
{
  const vkrt_query_opts q = {sizeof(vkrt_query_opts), 0u, 0xFFu, anyhit_seed};
  return rayQuery(s, rays, n, q, occluded, true, hip_stream, "vkrt_occluded");
}

int vkrt_hit_surface(vkrt_scene* s, const vkrt_hit* hits, uint32_t n, uint32_t fields, vkrt_surface* out, void* hip_stream)
{
  int rc = checkQueryArrays(s, "vkrt_hit_surface", n, {{hits, 16u, false}, {out, 16u, false}}, "(hits and out: 16 bytes)");
  if(rc != VKRT_OK)
    return rc;
  if(fields != VKRT_SURFACE_GEOMETRY && fields != (VKRT_SURFACE_GEOMETRY | VKRT_SURFACE_MATERIAL))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_hit_surface: fields 0x%x is neither VKRT_SURFACE_GEOMETRY nor VKRT_SURFACE_GEOMETRY | VKRT_SURFACE_MATERIAL", fields);
  if(n == 0)
    return VKRT_OK;
  // (no checkBuilt: everything read here is kept current by vkrt_scene_update_nodes / vkrt_scene_update_vertices, the tree is not read)
  if((rc = setDevice(s)) != VKRT_OK)
    return rc;
  DevSurfaceScene ss;
  static_cast<DevScene&>(ss) = s->dev;
  ss.primMeshes = s->surfacePrimMeshes;
  ss.instanceCount = (uint32_t)s->nodes.size();
  HIP_TRY(vkrt_launch_hit_surface(ss, (const float4*)hits, n, (fields & VKRT_SURFACE_MATERIAL) != 0u, (float4*)out, (hipStream_t)hip_stream));
  return VKRT_OK;
}

int vkrt_scene_motion_mark(vkrt_scene* s, void* hip_stream)
{
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_scene_motion_mark: scene is NULL");
  int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  const size_t instBytes = s->nodes.size() * sizeof(DevInstance), posBytes = s->positions.size() * sizeof(float);
  if(!s->motion.get())
  {  // first mark: the one place a mark allocates (and, through hipMalloc, may synchronise)
    const hipError_t e = s->motion.alloc(s->motionPositionsAt() + std::max<size_t>(posBytes, 16));
    if(e != hipSuccess)
      return fail(e == hipErrorOutOfMemory ? VKRT_ERR_OUT_OF_MEMORY : VKRT_ERR_HIP, "vkrt_scene_motion_mark: hipMalloc: %s", hipGetErrorString(e));
  }
  // Stream-ordered like the two update calls: the copies read what the updates enqueued before them on hip_stream wrote, and are read
  // by what comes after (vkrt_hit_motion).  Nothing here depends on the tree, so a build or a refit leaves the snapshot alone.
  hipStream_t stream = (hipStream_t)hip_stream;
  if(instBytes)
    HIP_TRY(hipMemcpyAsync(const_cast<DevInstance*>(s->prevInstances()), s->dev.instances, instBytes, hipMemcpyDeviceToDevice, stream));
  if(posBytes)
    HIP_TRY(hipMemcpyAsync(const_cast<float*>(s->prevPositions()), s->dev.positions, posBytes, hipMemcpyDeviceToDevice, stream));
  return VKRT_OK;
}

int vkrt_hit_motion(vkrt_scene* s, const vkrt_hit* hits, uint32_t n, float* current, float* previous, void* hip_stream)
{
  int rc = checkQueryArrays(s, "vkrt_hit_motion", n, {{hits, 16u, false}, {current, 16u, true}, {previous, 16u, true}},
                            "(hits, current and previous: 16 bytes)");
  if(rc != VKRT_OK)
    return rc;
  if(!current && !previous)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_hit_motion: current and previous are both NULL");
  if(n == 0)
    return VKRT_OK;
  // (no checkBuilt: like vkrt_hit_surface, nothing read here belongs to the tree)
  if((rc = setDevice(s)) != VKRT_OK)
    return rc;
  DevMotionScene ms;
  static_cast<DevScene&>(ms) = s->dev;
  ms.primMeshes = s->surfacePrimMeshes;
  ms.instanceCount = (uint32_t)s->nodes.size();
  ms.prevInstances = s->prevInstances();
  ms.prevPositions = s->prevPositions();
  HIP_TRY(vkrt_launch_hit_motion(ms, (const float4*)hits, n, (float4*)current, (float4*)previous, (hipStream_t)hip_stream));
  return VKRT_OK;
}

int vkrt_intersect_ex(vkrt_scene* s, const vkrt_ray* rays, uint32_t n, const vkrt_query_opts* opts, vkrt_hit* hits, void* hip_stream)
{
  const int rc = checkQueryOpts(opts, "vkrt_intersect_ex");
  return rc != VKRT_OK ? rc : rayQuery(s, rays, n, *opts, hits, false, hip_stream, "vkrt_intersect_ex");
}

int vkrt_occluded_ex(vkrt_scene* s, const vkrt_ray* rays, uint32_t n, const vkrt_query_opts* opts, int32_t* occluded, void* hip_stream)
{
  const int rc = checkQueryOpts(opts, "vkrt_occluded_ex");
  return rc != VKRT_OK ? rc : rayQuery(s, rays, n, *opts, occluded, true, hip_stream, "vkrt_occluded_ex");
}

int vkrt_intersect_multi(vkrt_scene* s, const vkrt_ray* rays, uint32_t n, const vkrt_query_opts* opts, uint32_t max_hits, vkrt_hit* hits,
                         int32_t* counts, void* hip_stream)
{
  const int rc = checkQueryOpts(opts, "vkrt_intersect_multi");
  if(rc != VKRT_OK)
    return rc;
  if(max_hits == 0u || max_hits > VKRT_MULTIHIT_MAX)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_intersect_multi: max_hits %u outside 1..%d (VKRT_MULTIHIT_MAX)", max_hits, VKRT_MULTIHIT_MAX);
  return rayQueryMulti(s, rays, n, *opts, max_hits, hits, counts, hip_stream, "vkrt_intersect_multi");
}

int vkrt_closest_point(vkrt_scene* s, const vkrt_point_query* queries, uint32_t n, const vkrt_query_opts* opts, vkrt_hit* hits, void* hip_stream)
{
  vkrt_query_opts q;
  const int rc = checkPointOpts(opts, "vkrt_closest_point", q);
  return rc != VKRT_OK ? rc : pointQuery(s, queries, n, q, hits, hip_stream, "vkrt_closest_point");
}

int vkrt_scene_set_instance_visibility(vkrt_scene* s, uint32_t first, uint32_t count, const vkrt_instance_visibility* vis, void* hip_stream)
{
  const char* who = "vkrt_scene_set_instance_visibility";
  if(count && !vis)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: vis is NULL", who);
  for(uint32_t i = 0; i < count; i++)
  {
    if(vis[i].mask == 0)
      return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: entry %u: mask 0 (hide an instance from every ray with a zero-scale transform)", who, i);
    if(vis[i].flags & ~(VKRT_INSTANCE_FACING_CULL_DISABLE | VKRT_INSTANCE_FLIP_FACING))
      return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: entry %u: unknown flag bits 0x%x", who, i, (unsigned)vis[i].flags);
    if(vis[i].reserved != 0)
      return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: entry %u: reserved is not 0", who, i);
  }
  int rc = checkVisibilityRange(s, first, count, who);
  if(rc != VKRT_OK || count == 0)
    return rc;
  if((rc = setDevice(s)) != VKRT_OK)
    return rc;
  // the visibility words alone, sent as kernel arguments on hip_stream like vkrt_scene_update_nodes sends its records: stream-ordered,
  // nothing staged, no synchronisation.  The kernel keeps each record's mirrored bit and does not touch its transform, so a transform
  // that came from device memory (vkrt_scene_update_node_transforms) stays; with the host copy current the records are bit for bit
  // what make_instance gives for the node and the new visibility
  std::vector<uint32_t> words(count);
  for(uint32_t i = 0; i < count; i++)
    words[i] = (uint32_t)vis[i].mask | ((uint32_t)vis[i].flags << 8);
  hipStream_t stream = (hipStream_t)hip_stream;
  HIP_TRY(vkrt::launch_instance_visibility(const_cast<DevInstance*>(s->dev.instances), first, count, words.data(), stream));
  std::copy(vis, vis + count, s->vis.begin() + first);
  noteMasks(s);
  // the table follows the masks on the same stream (a stale tree too: records and topology are those of its build or last refit)
  return s->built ? computeNodeMasks(s, stream) : VKRT_OK;
}

int vkrt_scene_get_instance_visibility(const vkrt_scene* s, uint32_t first, uint32_t count, vkrt_instance_visibility* out)
{
  const char* who = "vkrt_scene_get_instance_visibility";
  if(count && !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: out is NULL", who);
  const int rc = checkVisibilityRange(s, first, count, who);
  if(rc != VKRT_OK)
    return rc;
  std::copy(s->vis.begin() + first, s->vis.begin() + first + count, out);
  return VKRT_OK;
}

int vkrt_scene_set_material_alpha(vkrt_scene* s, uint32_t first, uint32_t count, const vkrt_material_alpha* alpha, void* hip_stream)
{
  const char* who = "vkrt_scene_set_material_alpha";
  if(count && !alpha)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: alpha is NULL", who);
  for(uint32_t i = 0; i < count; i++)
  {
    if(alpha[i].mode != VKRT_ALPHA_OPAQUE && alpha[i].mode != VKRT_ALPHA_MASK)
      return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: entry %u: mode %u is neither VKRT_ALPHA_OPAQUE nor VKRT_ALPHA_MASK", who, i, alpha[i].mode);
    if(!std::isfinite(alpha[i].cutoff) || alpha[i].cutoff < 0.0f)
      return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: entry %u: cutoff %g is not a finite number >= 0", who, i, (double)alpha[i].cutoff);
  }
  int rc = checkMaterialRange(s, first, count, who);
  if(rc != VKRT_OK || count == 0)
    return rc;
  if((rc = setDevice(s)) != VKRT_OK)
    return rc;
  // the pairs travel as kernel arguments on hip_stream like the records of vkrt_scene_set_instance_visibility: stream-ordered, nothing
  // staged, no synchronisation.  (vkrt_material_alpha is the (mode, cutoff bits) pair the kernel writes.)
  HIP_TRY(vkrt_launch_material_alpha(const_cast<DevMaterial*>(s->dev.materials), first, count, (const uint2*)alpha, (hipStream_t)hip_stream));
  std::copy(alpha, alpha + count, s->alpha.begin() + first);
  s->alphaMasks = 0u;
  for(const vkrt_material_alpha& a : s->alpha)
    s->alphaMasks += a.mode == VKRT_ALPHA_MASK ? 1u : 0u;
  return VKRT_OK;
}

int vkrt_scene_get_material_alpha(const vkrt_scene* s, uint32_t first, uint32_t count, vkrt_material_alpha* out)
{
  const char* who = "vkrt_scene_get_material_alpha";
  if(count && !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: out is NULL", who);
  const int rc = checkMaterialRange(s, first, count, who);
  if(rc != VKRT_OK)
    return rc;
  std::copy(s->alpha.begin() + first, s->alpha.begin() + first + count, out);
  return VKRT_OK;
}

uint32_t vkrt_shard_rows(const vkrt_shard* sh)
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
  if(n_frames > 65536u || (int64_t)pc->frame + (int64_t)n_frames > 0x7fffffffll)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "n_frames %u out of range", n_frames);
  if(!image && vkrt_shard_rows(shard) != 0u)  // (a shard without rows -- more ranks than strips -- has no image to pass)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL image");
  int rc = checkBuilt(s, "vkrt_pathtrace");
  if(rc == VKRT_OK)
    rc = checkShard(shard);
  if(rc != VKRT_OK)
    return rc;
  if(pc->lightsCount < 0 || (uint32_t)pc->lightsCount > s->lightCount)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "PushConstantRay.lightsCount %d outside [0,%u]", pc->lightsCount, s->lightCount);
  if(pc->samples < 0 || pc->depth < 0 || pc->depth > 99)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "samples/depth out of range");
  if((rc = setDevice(s)) != VKRT_OK)
    return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  TraceParams P;
  if((rc = launchParams(s, pc, cam, opts, shard, P)) != VKRT_OK)
    return rc;
  if(P.localRows == 0)
    return VKRT_OK;
  if((rc = frameAlphaStage(s, "vkrt_pathtrace", P)) != VKRT_OK)
    return rc;
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
    if((rc = ensureFrameCall(s, P.tileCount, n_frames, stream)) != VKRT_OK)
      return rc;
    WfTiming* timing = nullptr;
    if(P.flags & VKRT_TRACE_TIME_KERNELS)
    {
      if((rc = growEvents(s->wfEventOwners, s->wfEvents, wfTimingEvents(pc->samples, pc->depth, n_frames), hipEventDefault)) != VKRT_OK)
        return rc;
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

namespace {
int gbufferImpl(vkrt_scene* s, const float clearColor[4], int lightsCount, const GlobalUniforms* cam, const float* viewMatrix, const vkrt_shard* shard,
                const vkrt_gbuffer* out, const vkrt_nrd_planes* nrd, vkrt_hit* hits, void* hip_stream);
int hybridImpl(vkrt_scene* s, const PushConstantRay* pc, const GlobalUniforms* cam, const vkrt_trace_opts* opts, const vkrt_shard* shard,
               const vkrt_gbuffer* g, const vkrt_nrd_planes* nrd, float* accum, void* hip_stream);
}  // namespace

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

namespace {
int gbufferImpl(vkrt_scene* s, const float clearColor[4], int lightsCount, const GlobalUniforms* cam, const float* viewMatrix, const vkrt_shard* shard,
                const vkrt_gbuffer* out, const vkrt_nrd_planes* nrd, vkrt_hit* hits, void* hip_stream)
{
  if(s && clearColor && cam && shard && out && vkrt_shard_rows(shard) == 0u)
    return VKRT_OK;  // a shard without rows: nothing to write, no planes to pass
  if(!s || !clearColor || !cam || !shard || !out || !out->color || !out->position || !out->normal || !out->roughMetal)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  if(lightsCount < 0 || (uint32_t)lightsCount > s->lightCount)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "lightsCount %d outside [0,%u]", lightsCount, s->lightCount);
  int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  TraceParams P;
  if((rc = checkBuilt(s, "vkrt_gbuffer_raycast")) != VKRT_OK || (rc = checkShard(shard)) != VKRT_OK ||
     (rc = launchParams(s, nullptr, cam, nullptr, shard, P)) != VKRT_OK)
    return rc;
  if(P.localRows == 0)
    return VKRT_OK;
  if((rc = frameAlphaStage(s, "vkrt_gbuffer_raycast", P)) != VKRT_OK)
    return rc;
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
  if(pc->lightsCount < 0 || (uint32_t)pc->lightsCount > s->lightCount)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "PushConstantRay.lightsCount %d outside [0,%u]", pc->lightsCount, s->lightCount);
  if(pc->depth < 0 || pc->depth > 99)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "depth out of range");
  int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  TraceParams P;
  if((rc = checkBuilt(s, "vkrt_hybrid_trace")) != VKRT_OK || (rc = checkShard(shard)) != VKRT_OK ||
     (rc = launchParams(s, pc, cam, opts, shard, P)) != VKRT_OK)
    return rc;
  if(P.localRows == 0)
    return VKRT_OK;
  if((rc = frameAlphaStage(s, "vkrt_hybrid_trace", P)) != VKRT_OK)
    return rc;
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
    if((rc = ensureWorkingSet(s, P.tileCount * 64u, 1, stream)) != VKRT_OK)
      return rc;
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

int vkrt_post(int device, const PushConstantPost* pc, uint32_t n, const float* mainImg, const float* rtImg, float* out, void* hip_stream)
{
  if(!pc || !mainImg || !out || (pc->rtMode == 0 && !rtImg))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  if(vkrt_device_count() <= 0)
    return fail(VKRT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
  HIP_TRY(hipSetDevice(device));
  if(n == 0)
    return VKRT_OK;
  HIP_TRY(vkrt_launch_post(pc->rtMode, pc->viewAccumulated, pc->useGI, n, mainImg, rtImg, out, (hipStream_t)hip_stream));
  return VKRT_OK;
}

int vkrt_counters_reset(vkrt_scene* s, void* hip_stream)
{
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "scene is NULL");
  int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  HIP_TRY(hipMemsetAsync(s->counters, 0, sizeof(DevCounters), (hipStream_t)hip_stream));
  return VKRT_OK;
}

int vkrt_counters_read(vkrt_scene* s, vkrt_counters* out)
{
  if(!s || !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  DevCounters h;
  HIP_TRY(hipMemcpy(&h, s->counters, sizeof h, hipMemcpyDeviceToHost));
  unsigned long long t[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for(int sl = 0; sl < VKRT_COUNTER_SLOTS; sl++)
    for(int k = 0; k < 12; k++) t[k] += h.v[sl][k];
  out->rays_closest = t[0]; out->rays_shadow = t[1]; out->hits = t[2]; out->diffuse_hits = t[3];
  out->tex_taps = t[4]; out->pixels = t[5]; out->nodes_visited = t[6]; out->tris_tested = t[7];
  out->wave_node_steps = t[8]; out->wave_tri_steps = t[9]; out->traversal_faults = t[10]; out->pair_records = t[11];
  return VKRT_OK;
}

int vkrt_last_trace_ms(vkrt_scene* s, float* ms)
{
  if(!s || !ms)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  if(!s->timed)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "no trace has been launched on this scene");
  HIP_TRY(hipEventSynchronize(s->evStop.get()));
  HIP_TRY(hipEventElapsedTime(ms, s->evStart.get(), s->evStop.get()));
  return VKRT_OK;
}

int vkrt_last_trace_timing(vkrt_scene* s, vkrt_trace_timing* out)
{
  if(!s || !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  if(!s->timed)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "no trace has been launched on this scene");
  memset(out, 0, sizeof *out);
  HIP_TRY(hipEventSynchronize(s->evStop.get()));
  HIP_TRY(hipEventElapsedTime(&out->total_ms, s->evStart.get(), s->evStop.get()));
  out->mode = s->wavefront ? 1u : 0u;
  if(s->wfTimed)
  {
    for(int k = 0; k < s->wfTiming.used; k++)
    {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, s->wfEvents[2 * k], s->wfEvents[2 * k + 1]));
      out->traverse_ms += ms;
    }
    out->traverse_launches = (uint32_t)s->wfTiming.used;
    // the shade launch of round r sits between the traversal launches of rounds r and r + 1 on the same stream
    const int rounds = s->wfTimingRounds;
    for(int k = 0; k + 1 < s->wfTiming.used; k++)
    {
      if(rounds > 0 && (k + 1) % rounds == 0)
        continue;  // a frame ends here: its last shade launch is followed by the next frame's begin
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, s->wfEvents[2 * k + 1], s->wfEvents[2 * k + 2]));
      out->shade_ms += ms;
      out->shade_launches++;
    }
  }
  else if(!s->wavefront)
  {
    out->traverse_ms = out->total_ms;
    out->traverse_launches = 1;
  }
  return VKRT_OK;
}

int vkrt_debug_trace_rays(vkrt_scene* s, uint32_t n, const float* origins, const float* directions, float tmin, float tmax,
                          int any_hit, float* t, float* u, float* v, int32_t* gid)
{
  if(!s || (n && (!origins || !directions || !t || !u || !v || !gid)))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  int rc = checkBuilt(s, "vkrt_debug_trace_rays");
  if(rc != VKRT_OK || n == 0)
    return rc;
  if((rc = setDevice(s)) != VKRT_OK)
    return rc;
  vkrt::DevBuf dO, dD, dT, dU, dV, dG;
  const size_t b3 = (size_t)n * 3 * sizeof(float), b1 = (size_t)n * sizeof(float);
  hipError_t e = hipSuccess;
  auto tryHip = [&](hipError_t x) { if(e == hipSuccess) e = x; };
  tryHip(dO.alloc(b3)); tryHip(dD.alloc(b3)); tryHip(dT.alloc(b1));
  tryHip(dU.alloc(b1)); tryHip(dV.alloc(b1)); tryHip(dG.alloc(b1));
  if(e == hipSuccess) tryHip(hipMemcpy(dO.get(), origins, b3, hipMemcpyHostToDevice));
  if(e == hipSuccess) tryHip(hipMemcpy(dD.get(), directions, b3, hipMemcpyHostToDevice));
  if(e == hipSuccess) tryHip(vkrt_launch_trace_rays(s->dev, n, dO.get<float>(), dD.get<float>(), tmin, tmax, any_hit, dT.get<float>(), dU.get<float>(),
                                                    dV.get<float>(), dG.get<int>(), nullptr));
  if(e == hipSuccess) tryHip(hipDeviceSynchronize());
  if(e == hipSuccess) tryHip(hipMemcpy(t, dT.get(), b1, hipMemcpyDeviceToHost));
  if(e == hipSuccess) tryHip(hipMemcpy(u, dU.get(), b1, hipMemcpyDeviceToHost));
  if(e == hipSuccess) tryHip(hipMemcpy(v, dV.get(), b1, hipMemcpyDeviceToHost));
  if(e == hipSuccess) tryHip(hipMemcpy(gid, dG.get(), b1, hipMemcpyDeviceToHost));
  if(e != hipSuccess)
    return fail(VKRT_ERR_HIP, "vkrt_debug_trace_rays: %s", hipGetErrorString(e));
  return VKRT_OK;
}

int vkrt_debug_closest_point_work(vkrt_scene* s, const vkrt_point_query* host_queries, uint32_t n, const vkrt_query_opts* opts, uint64_t out[2])
{
  const char* who = "vkrt_debug_closest_point_work";
  vkrt_query_opts q;
  int rc = checkPointOpts(opts, who, q);
  if(rc != VKRT_OK)
    return rc;
  if(!s || !out || (n && !host_queries))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  out[0] = out[1] = 0;
  if(n == 0)
    return VKRT_OK;
  DevQueryScene qs;
  bool filter;
  if((rc = querySetup(s, q, who, qs, filter)) != VKRT_OK)
    return rc;
  vkrt::DevBuf dQ, dH, dW;
  hipError_t e = hipSuccess;
  auto tryHip = [&](hipError_t x) { if(e == hipSuccess) e = x; };
  tryHip(dQ.alloc((size_t)n * sizeof(vkrt_point_query))); tryHip(dH.alloc((size_t)n * sizeof(vkrt_hit))); tryHip(dW.alloc(2 * sizeof(uint64_t)));
  if(e == hipSuccess) tryHip(hipMemcpy(dQ.get(), host_queries, (size_t)n * sizeof(vkrt_point_query), hipMemcpyHostToDevice));
  if(e == hipSuccess) tryHip(hipMemset(dW.get(), 0, 2 * sizeof(uint64_t)));
  if(e == hipSuccess) tryHip(vkrt_launch_closest_point(qs, dQ.get<const float4>(), n, true, dH.get<float4>(), dW.get<unsigned long long>(), nullptr));
  if(e == hipSuccess) tryHip(hipDeviceSynchronize());
  if(e == hipSuccess) tryHip(hipMemcpy(out, dW.get(), 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if(e != hipSuccess)
    return fail(VKRT_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  return VKRT_OK;
}

int vkrt_debug_read_accel(vkrt_scene* s, void* nodes, uint64_t nodes_bytes, void* tris, uint64_t tris_bytes, int32_t* root_ref)
{
  if(!s || !root_ref || (nodes_bytes && !nodes) || (tris_bytes && !tris))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  int rc = checkBuilt(s, "vkrt_debug_read_accel");
  if(rc == VKRT_OK)
    rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  if(nodes_bytes != s->info.node_bytes || tris_bytes != s->info.triangle_bytes)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_debug_read_accel: buffers of %llu / %llu bytes for a tree of %llu / %llu",
                (unsigned long long)nodes_bytes, (unsigned long long)tris_bytes, (unsigned long long)s->info.node_bytes,
                (unsigned long long)s->info.triangle_bytes);
  HIP_TRY(hipDeviceSynchronize());
  if(nodes_bytes)
    HIP_TRY(hipMemcpy(nodes, s->dev.nodes, nodes_bytes, hipMemcpyDeviceToHost));
  if(tris_bytes)
    HIP_TRY(hipMemcpy(tris, s->dev.tris, tris_bytes, hipMemcpyDeviceToHost));
  *root_ref = s->dev.rootRef;
  return VKRT_OK;
}

int vkrt_debug_read_node_masks(vkrt_scene* s, void* out, uint64_t bytes)
{
  if(!s || !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  if(!s->built)
    return fail(VKRT_ERR_NOT_BUILT, "vkrt_debug_read_node_masks before vkrt_accel_build");
  if(s->dev.layout != 1u)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_debug_read_node_masks: a BVH2 tree has no node-mask table");
  const uint64_t want = s->info.node_bytes / VKRT_WNODE_BYTES * 8;
  if(bytes != want)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_debug_read_node_masks: a buffer of %llu bytes for a table of %llu", (unsigned long long)bytes,
                (unsigned long long)want);
  const int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  if(bytes)
    HIP_TRY(hipMemcpy(out, s->nodeMasks.get(), bytes, hipMemcpyDeviceToHost));
  return VKRT_OK;
}

int vkrt_debug_read_triangle_ids(vkrt_scene* s, uint32_t* out, uint64_t bytes)
{
  if(!s || !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  int rc = checkBuilt(s, "vkrt_debug_read_triangle_ids");
  if(rc == VKRT_OK)
    rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  const uint64_t slots = s->info.triangle_bytes / 48, want = slots * 4;
  if(bytes != want)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_debug_read_triangle_ids: a buffer of %llu bytes for %llu slots (%llu bytes)",
                (unsigned long long)bytes, (unsigned long long)slots, (unsigned long long)want);
  HIP_TRY(hipDeviceSynchronize());
  if(slots)
  {
    // word 9 of every 48-B record: the flattened triangle id (bit 31: the non-opaque flag of the any-hit stage)
    std::vector<uint32_t> rec((size_t)slots * 12);
    HIP_TRY(hipMemcpy(rec.data(), s->dev.tris, (size_t)slots * 48, hipMemcpyDeviceToHost));
    for(uint64_t k = 0; k < slots; k++) out[k] = rec[(size_t)k * 12 + 9] & 0x7fffffffu;
  }
  return VKRT_OK;
}

int vkrt_debug_split_references(vkrt_scene* s, uint32_t split_percent, float* prio, float* scale, uint32_t* ref_tri, float* ref_box, uint64_t capacity,
                                uint32_t* ref_count)
{
  if(!s || !ref_tri || !ref_box || !ref_count)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  if(split_percent < 1u || split_percent > 100u)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_debug_split_references: a budget of %u %% (1..100)", split_percent);
  if(vkrt_device_count() <= 0)
    return fail(VKRT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
  int rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  if((rc = downloadNodeTransforms(s, "vkrt_debug_split_references")) != VKRT_OK)
    return rc;
  // the builders' view of the scene with the option as it stands now; the installed tree keeps the setting it was built with
  DevScene sc = s->dev;
  sc.watertight = s->opt[VKRT_OPT_WATERTIGHT] != 0 ? 1u : 0u;
  std::string err;
  rc = vkrt::split_references_device(sc, (uint32_t)s->nodes.size(), s->primMeshes, s->nodes, split_percent, nullptr, prio, scale, ref_tri, ref_box,
                                     capacity, ref_count, err);
  if(rc != VKRT_OK)
    return fail(rc, "vkrt_debug_split_references: %s", err.c_str());
  return VKRT_OK;
}

int vkrt_debug_check_accel(vkrt_scene* s, vkrt_accel_check* out)
{
  if(!s || !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  int rc = checkBuilt(s, "vkrt_debug_check_accel");
  if(rc == VKRT_OK)
    rc = setDevice(s);
  if(rc != VKRT_OK)
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  const uint32_t T = s->dev.triCount, N = s->info.node_count;
  std::vector<float> tris((size_t)T * 12);
  std::vector<uint32_t> nodes((size_t)N * (s->dev.layout == 1u ? 20 : 16));
  if(T)
    HIP_TRY(hipMemcpy(tris.data(), s->dev.tris, tris.size() * 4, hipMemcpyDeviceToHost));
  if(N)
    HIP_TRY(hipMemcpy(nodes.data(), s->dev.nodes, nodes.size() * 4, hipMemcpyDeviceToHost));
  vkrt::check_tree(s->dev.layout, s->dev.rootRef, nodes.data(), N, tris.data(), T, s->info.triangle_count, s->dev.watertight != 0, *out);
  return VKRT_OK;
}

// ---- diffuse denoiser (denoise.hip) ---------------------------------------------------------------------------------------
struct vkrt_denoiser
{
  int device = 0;
  uint32_t width = 0, height = 0;
  vkrt::DevBuf mem;             // one allocation: 8 planes of float4 per pixel
  float4* colour[3] = {};       // colour history / temporal result / ping-pong of the a-trous passes (roles rotate per call)
  float4* geom[2] = {};         // (position.xyz, oct normal) of the current and the previous call
  float4* mom[2] = {};          // (m1, m2, history length, 0)
  float4* rec = nullptr;        // guide record of the current call
  int hist = 0;                 // colour[hist] holds the colour history
  int cur = 0;                  // geom[cur] / mom[cur] are written by the next call
  bool hasHistory = false;
  float prevViewProj[16] = {};
};

int vkrt_denoiser_create(int device, uint32_t width, uint32_t height, vkrt_denoiser** out)
{
  if(!out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  *out = nullptr;
  if(width == 0 || height == 0 || (uint64_t)width * height > 0x7FFFFFFFull / 4u)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "denoiser size %ux%u out of range", width, height);
  const int ndev = vkrt_device_count();
  if(ndev <= 0)
    return fail(VKRT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
  if(device < 0 || device >= ndev)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "device %d outside [0,%d)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  vkrt_denoiser* dn = new vkrt_denoiser();
  dn->device = device;
  dn->width = width;
  dn->height = height;
  const size_t plane = (size_t)width * height * sizeof(float4);
  const hipError_t e = dn->mem.alloc(8 * plane);
  if(e != hipSuccess)
  {
    delete dn;
    return fail(e == hipErrorOutOfMemory ? VKRT_ERR_OUT_OF_MEMORY : VKRT_ERR_HIP, "vkrt_denoiser_create: hipMalloc: %s", hipGetErrorString(e));
  }
  float4* base = dn->mem.get<float4>();
  const size_t n = (size_t)width * height;
  for(int k = 0; k < 3; k++) dn->colour[k] = base + k * n;
  dn->geom[0] = base + 3 * n; dn->geom[1] = base + 4 * n;
  dn->mom[0] = base + 5 * n; dn->mom[1] = base + 6 * n;
  dn->rec = base + 7 * n;
  *out = dn;
  return VKRT_OK;
}

void vkrt_denoiser_destroy(vkrt_denoiser* dn)
{
  if(!dn)
    return;
  (void)hipSetDevice(dn->device);
  delete dn;
}

int vkrt_denoiser_reset(vkrt_denoiser* dn)
{
  if(!dn)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL denoiser");
  dn->hasHistory = false;
  return VKRT_OK;
}

namespace {
// vkrt_denoise_diffuse (prevPosition NULL) and vkrt_denoise_diffuse_motion: one call sequence, the temporal kernel differs
int denoiseImpl(vkrt_denoiser* dn, const vkrt_denoise_settings* settings, const GlobalUniforms* cam, const vkrt_gbuffer* g, const vkrt_nrd_planes* nrd,
                const float* prevPosition, float* out, void* hip_stream)
{
  vkrt_denoise_settings st{sizeof(vkrt_denoise_settings), 5, 32};
  if(settings)
  {
    if(settings->struct_size < sizeof(vkrt_denoise_settings))
      return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_denoise_settings.struct_size %u < %zu", settings->struct_size, sizeof(vkrt_denoise_settings));
    st = *settings;
    if(st.atrous_iterations < 0 || st.atrous_iterations > 5)
      return fail(VKRT_ERR_INVALID_ARGUMENT, "atrous_iterations %d outside [0,5]", st.atrous_iterations);
    if(st.max_history < 1 || st.max_history > 255)
      return fail(VKRT_ERR_INVALID_ARGUMENT, "max_history %d outside [1,255]", st.max_history);
  }
  if(!cam || !g || !nrd || !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  if(!g->color || !g->position || !g->normal || !g->roughMetal)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL G-buffer plane");
  if(!nrd->viewZ || !nrd->diffRadianceHitDist)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL NRD plane (viewZ / diffRadianceHitDist)");
  if(!dn)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL denoiser");
  HIP_TRY(hipSetDevice(dn->device));
  hipStream_t stream = (hipStream_t)hip_stream;
  const int K = st.atrous_iterations;
  // colour roles: h = history (read by the temporal taps), a = temporal result, b = variance output; a-trous iteration 0 writes the
  // new history over the old one (read only by the temporal stage), then the passes alternate between the two others
  const int h = dn->hist, a = (h + 1) % 3, b = (h + 2) % 3;
  DenoiseParams D;
  memset(&D, 0, sizeof D);
  D.W = dn->width; D.H = dn->height;
  D.color = (const float4*)g->color; D.position = (const float4*)g->position; D.normal = (const float4*)g->normal;
  D.rough = (const float2*)g->roughMetal; D.viewZ = nrd->viewZ; D.radHitD = (const float4*)nrd->diffRadianceHitDist;
  D.histColor = dn->colour[h];
  D.geomPrev = dn->geom[dn->cur ^ 1]; D.geomCur = dn->geom[dn->cur];
  D.momPrev = dn->mom[dn->cur ^ 1]; D.momCur = dn->mom[dn->cur];
  D.rec = dn->rec;
  D.colorOut = dn->colour[a]; D.colorVar = dn->colour[b];
  D.out = K == 0 ? out : nullptr;
  memcpy(D.curViewProj, cam->viewProj.m, sizeof D.curViewProj);
  memcpy(D.prevViewProj, dn->prevViewProj, sizeof D.prevViewProj);
  D.useHistory = dn->hasHistory ? 1 : 0;
  D.maxHistory = st.max_history;
  D.prevPosition = (const float4*)prevPosition;
  HIP_TRY(vkrt_launch_denoise_temporal(D, K > 0, stream));
  int in = b;
  for(int i = 0; i < K; i++)
  {
    const int dst = i == 0 ? h : (in == h ? a : (in == a ? b : a));
    DenoiseAtrous A;
    A.W = dn->width; A.H = dn->height; A.step = 1 << i;
    A.rec = dn->rec; A.in = dn->colour[in]; A.outBuf = dn->colour[dst];
    A.out = i == K - 1 ? out : nullptr;
    A.color = D.color; A.position = D.position; A.normal = D.normal; A.rough = D.rough;
    HIP_TRY(vkrt_launch_denoise_atrous(A, stream));
    in = dst;
  }
  if(K == 0)
    dn->hist = a;  // the temporal result is the history
  memcpy(dn->prevViewProj, cam->viewProj.m, sizeof dn->prevViewProj);
  dn->cur ^= 1;
  dn->hasHistory = true;
  return VKRT_OK;
}
}  // namespace

int vkrt_denoise_diffuse(vkrt_denoiser* dn, const vkrt_denoise_settings* settings, const GlobalUniforms* cam, const vkrt_gbuffer* g,
                         const vkrt_nrd_planes* nrd, float* out, void* hip_stream)
{
  return denoiseImpl(dn, settings, cam, g, nrd, nullptr, out, hip_stream);
}

int vkrt_denoise_diffuse_motion(vkrt_denoiser* dn, const vkrt_denoise_settings* settings, const GlobalUniforms* cam, const vkrt_gbuffer* g,
                                const vkrt_nrd_planes* nrd, const float* prevPosition, float* out, void* hip_stream)
{
  if(!prevPosition)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_denoise_diffuse_motion: prev_position_rgba32f is NULL");
  if(((uintptr_t)prevPosition & 15u) != 0u)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_denoise_diffuse_motion: prev_position_rgba32f is not 16-byte aligned");
  return denoiseImpl(dn, settings, cam, g, nrd, prevPosition, out, hip_stream);
}

int vkrt_debug_eval_math(int device, int op, uint32_t n, const float* a, const float* b, float* out)
{
  if(n && (!a || !b || !out))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  if(vkrt_device_count() <= 0)
    return fail(VKRT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
  if(n == 0)
    return VKRT_OK;
  HIP_TRY(hipSetDevice(device));
  vkrt::DevBuf dA, dB, dC;
  const size_t bytes = (size_t)n * sizeof(float);
  hipError_t e = hipSuccess;
  auto tryHip = [&](hipError_t x) { if(e == hipSuccess) e = x; };
  tryHip(dA.alloc(bytes)); tryHip(dB.alloc(bytes)); tryHip(dC.alloc(bytes));
  if(e == hipSuccess) tryHip(hipMemcpy(dA.get(), a, bytes, hipMemcpyHostToDevice));
  if(e == hipSuccess) tryHip(hipMemcpy(dB.get(), b, bytes, hipMemcpyHostToDevice));
  if(e == hipSuccess) tryHip(vkrt_launch_eval_math(op, n, dA.get<float>(), dB.get<float>(), dC.get<float>(), nullptr));
  if(e == hipSuccess) tryHip(hipDeviceSynchronize());
  if(e == hipSuccess) tryHip(hipMemcpy(out, dC.get(), bytes, hipMemcpyDeviceToHost));
  if(e != hipSuccess)
    return fail(VKRT_ERR_HIP, "vkrt_debug_eval_math: %s", hipGetErrorString(e));
  return VKRT_OK;
}

int vkrt_debug_eval_shade(int device, uint32_t n, const float* in, float* out)
{
  if(n && (!in || !out))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  if(vkrt_device_count() <= 0)
    return fail(VKRT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
  if(n == 0)
    return VKRT_OK;
  for(uint32_t i = 0; i < n; i++)
  {
    int32_t lightsCount;
    memcpy(&lightsCount, in + 40 * (size_t)i + 35, sizeof lightsCount);
    if(lightsCount < 1 || lightsCount > VKRT_EVAL_SHADE_MAX_LIGHTS)
      return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_debug_eval_shade: record %u has lightsCount %d (1 to %d)", i, lightsCount, VKRT_EVAL_SHADE_MAX_LIGHTS);
  }
  HIP_TRY(hipSetDevice(device));
  vkrt::DevBuf dIn, dLights, dOut;
  const size_t inBytes = (size_t)n * 40 * sizeof(float), outBytes = (size_t)n * 20 * sizeof(float);
  hipError_t e = hipSuccess;
  auto tryHip = [&](hipError_t x) { if(e == hipSuccess) e = x; };
  tryHip(dIn.alloc(inBytes)); tryHip(dOut.alloc(outBytes));
  tryHip(dLights.alloc((size_t)n * VKRT_EVAL_SHADE_MAX_LIGHTS * sizeof(GltfLight)));
  if(e == hipSuccess) tryHip(hipMemcpy(dIn.get(), in, inBytes, hipMemcpyHostToDevice));
  if(e == hipSuccess) tryHip(vkrt_launch_eval_shade(n, dIn.get<float>(), dLights.get<float4>(), dOut.get<float>(), nullptr));
  if(e == hipSuccess) tryHip(hipDeviceSynchronize());
  if(e == hipSuccess) tryHip(hipMemcpy(out, dOut.get(), outBytes, hipMemcpyDeviceToHost));
  if(e != hipSuccess)
    return fail(VKRT_ERR_HIP, "vkrt_debug_eval_shade: %s", hipGetErrorString(e));
  return VKRT_OK;
}

}  // extern "C"
