// scene_state.h -- private to the units that implement the C ABI of include/vkrt.h (api_*.cpp, compiled as HIP): the scene record, the
// one error path, and the few helpers more than one area uses.  Nothing here is installed or seen by a caller of the library.
// Scene upload mirrors HelloVulkan::loadGltfScene's device-local buffers (hello_vulkan.cpp:353-381); vkrt_accel_build stands in for
// createBottomLevelASGltf/createTopLevelAsGltf (:1001-1047); vkrt_pathtrace stands in for HelloVulkan::pathtrace (:1423-1448).  There
// is no CPU fallback: without a HIP device the compute entry points fail with VKRT_ERR_NO_DEVICE.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vkrt.h"
#include "dev_buffer.h"
#include "device_scene.h"
#include "entry_checks.h"
#include "kernels.h"
#include "morph.h"
#include "refit.h"
#include "scene_options.h"
#include "skin.h"
#include "vertex_anim.h"
#include "wide_node.h"

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
  // editing the live scene (api_edit.cpp).  The texture tables as vkrt_scene_create packed them, which are fixed: the DevTexture records,
  // the level offsets ([texture][VKRT_MAX_MIPS]) and each texture's first footprint record (read when dev.texQuads exists); the
  // thresholds of the sRGB encode on the device (released with `tables`)
  std::vector<DevTexture> textures;
  std::vector<uint32_t> texMips, texQuadFirst;
  const float* srgbEncode = nullptr;
  // the dissolve rule of vkrt_scene_update_materials: per material, had it alpha < 1 at the last vkrt_accel_build (empty: that build ran
  // with VKRT_OPT_ANYHIT_DISSOLVE = 0, or there is no tree); and whether an update since has made the tree's triangle flags insufficient
  std::vector<uint8_t> builtNonOpaque;
  bool dissolveRebuild = false;
};

namespace vkrt {

// The one error path: the message becomes vkrt_last_error's (one thread-local, in api_scene.cpp), the code is returned.  failWith: a
// refusal of scene_pack.h's, vertex_anim.h's or entry_checks.h's checks, whose reason is in err.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline int failWith(int code, const std::string& err) { return fail(code, "%s", err.c_str()); }

// Each returns from the enclosing function with the code of what failed.  HIP_TRY: a HIP call, described as its own text (HIP_TRY_AS: as
// `what`).  CHECK_TRY(check_x(..., err)): a refusal of a function of namespace vkrt, given the macro's own err.  RC_TRY: a call that has
// already said why (fail).
#define HIP_TRY_AS(expr, what) do { std::string m_; if(const int rc_ = vkrt::hip_status((expr), what, m_); rc_ != VKRT_OK) return vkrt::failWith(rc_, m_); } while(0)
#define HIP_TRY(expr) HIP_TRY_AS(expr, #expr)
#define CHECK_TRY(call) do { std::string err; if(const int rc_ = vkrt::call; rc_ != VKRT_OK) return vkrt::failWith(rc_, err); } while(0)
#define RC_TRY(call) do { if(const int rc_ = (call); rc_ != VKRT_OK) return rc_; } while(0)

// the tree can be traced: built, and not moved since (`who` names the caller in the refusal)
inline int checkBuilt(const vkrt_scene* s, const char* who)
{
  if(!s->built)
    return fail(VKRT_ERR_NOT_BUILT, "%s before vkrt_accel_build", who);
  if(s->dissolveRebuild)
    return fail(VKRT_ERR_NOT_BUILT, "%s after vkrt_scene_update_materials gave a material alpha < 1 that was opaque when the tree was built with "
                "VKRT_OPT_ANYHIT_DISSOLVE: vkrt_accel_build first", who);
  if(s->stale)
    return fail(VKRT_ERR_NOT_BUILT, "%s after vkrt_scene_update_nodes / vkrt_scene_update_vertices: vkrt_accel_refit or vkrt_accel_build first", who);
  return VKRT_OK;
}

// The prologue of an entry point once its arguments are accepted: (tracedBy = the caller's name: the tree can be traced, then) the scene's
// device is current.
inline int enter(const vkrt_scene* s, const char* tracedBy = nullptr)
{
  if(tracedBy)
    RC_TRY(checkBuilt(s, tracedBy));
  HIP_TRY(hipSetDevice(s->device));
  return VKRT_OK;
}

// The read-back of the debug readers and the host mirror: wait for everything enqueued on the device, then copy `bytes` from it (if any).
inline hipError_t readBack(void* dst, const void* src, size_t bytes)
{
  if(const hipError_t e = hipDeviceSynchronize(); e != hipSuccess)
    return e;
  return bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
}

// the vertex ranges of the scene's skins or morphs, where they are kept
template <typename T>
RangeSet rangesOf(const std::vector<T>& v)
{
  return RangeSet{v.empty() ? nullptr : &v[0].arrays, v.size(), sizeof(T)};
}

// Live positions moved on the device: the tree is stale until the next refit or build, and -- unless the host copy got the same values --
// the next build downloads them first.
inline void positionsMoved(vkrt_scene* s, bool hostCopyFollowed = false)
{
  if(!hostCopyFollowed)
    s->positionsOnDevice = true;
  if(s->built)
    s->stale = true;
}

// execution mode: wavefront pipeline (default) or the single persistent megakernel
inline bool useWavefront(const vkrt_scene* s) { return s->opt[VKRT_OPT_MODE] == 1; }

// traversal workgroup size (the non-default triangle modes exist for the default 64-thread workgroup only)
inline int travBlock(const vkrt_scene* s) { return (s->dev.watertight || s->dev.dissolve) ? 64 : s->opt[VKRT_OPT_WF_TRAV_BLOCK]; }

inline void freeAccel(vkrt_scene* s)
{
  s->accel = TreeBuffers{};
  s->nodeMasks = DevBuf{};
  s->built = false;
  s->refit = RefitScratch{};
  s->refitted = false;
  s->stale = false;
  s->builtNonOpaque.clear();
  s->dissolveRebuild = false;
}

inline void noteMasks(vkrt_scene* s)
{
  memset(s->masksPresent, 0, sizeof s->masksPresent);
  for(const vkrt_instance_visibility& v : s->vis)
    s->masksPresent[v.mask >> 6] |= 1ull << (v.mask & 63u);
}

// does every node's mask meet cullMask?  (then a query with that mask and no facing flag walks exactly what vkrt_intersect walks)
inline bool everyMaskMeets(const vkrt_scene* s, uint32_t cullMask)
{
  for(uint32_t m = 0; m < 256; m++)
    if(((s->masksPresent[m >> 6] >> (m & 63u)) & 1ull) && (m & cullMask) == 0u)
      return false;
  return true;
}

// the node-mask table of the installed wide8 tree from the current instance records, enqueued on `stream` (levels + 1 passes: no read-back)
inline int computeNodeMasks(vkrt_scene* s, hipStream_t stream)
{
  if(s->dev.layout != 1u || !s->nodeMasks.get())
    return VKRT_OK;
  const uint32_t nodes = (uint32_t)(s->info.node_bytes / VKRT_WNODE_BYTES);
  HIP_TRY(vkrt_launch_node_masks(s->dev, nodes, (uint32_t)s->nodes.size(), s->info.max_depth + 1u, s->nodeMasks.get<uint2>(), stream));
  return VKRT_OK;
}

// Bring the host copies up to date with what device-sourced updates moved (api_accel.cpp): the positions when `positions` asks for them,
// and the node matrices.  `who` names the caller in the refusal of a matrix that is not finite.
int syncHostMirror(vkrt_scene* s, bool positions, const char* who);

}  // namespace vkrt
