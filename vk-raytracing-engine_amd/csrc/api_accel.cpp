// api_accel.cpp -- the acceleration structure (include/vkrt.h): build, info, refit, and the node updates that make a tree stale, with
// the host mirror the builders read (syncHostMirror).
#include <chrono>

#include "bvh_host.h"
#include "lbvh.h"
#include "node_update.h"
#include "scene_pack.h"
#include "scene_state.h"
#include "trav_lds.h"
#include "wide_node.h"

using namespace vkrt;

// Nodes moved by a device-sourced vkrt_scene_update_node_transforms, vertices moved by a device-sourced vkrt_scene_update_vertices: the
// host builder, scene_bounds and the split hook read the host copies.  The matrices come from the instance records (o2w = rows 0-2; the
// bottom row, which nothing reads, becomes 0 0 0 1).  Synchronises the device when there is something to bring.  A matrix that is not
// finite -- the device path does not inspect its values -- is refused like one given to vkrt_scene_create, and the host copy of the
// nodes stays as it was.
int vkrt::syncHostMirror(vkrt_scene* s, bool positions, const char* who)
{
  positions = positions && s->positionsOnDevice;
  if(!positions && !s->nodesOnDevice)
    return VKRT_OK;
  RC_TRY(enter(s));
  if(positions)
  {
    HIP_TRY(readBack(s->positions.data(), s->dev.positions, s->positions.size() * sizeof(float)));
    s->positionsOnDevice = false;
  }
  if(!s->nodesOnDevice)
    return VKRT_OK;
  std::vector<DevInstance> inst(s->nodes.size());
  HIP_TRY(readBack(inst.data(), s->dev.instances, inst.size() * sizeof(DevInstance)));
  std::vector<vkrt_node> fresh = s->nodes;
  for(size_t i = 0; i < fresh.size(); i++)
  {
    float* M = fresh[i].worldMatrix;
    for(int r = 0; r < 3; r++)
      for(int c = 0; c < 4; c++)
        M[c * 4 + r] = inst[i].o2w[r * 4 + c];
    M[3] = M[7] = M[11] = 0.0f;
    M[15] = 1.0f;
    if(std::string err; check_transform(fresh[i], (uint32_t)i, err) != VKRT_OK)
      return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: after a device-sourced vkrt_scene_update_node_transforms: %s", who, err.c_str());
  }
  s->nodes.swap(fresh);
  s->nodesOnDevice = false;
  return VKRT_OK;
}

namespace {

// Moves a builder's record into the scene.
void installTree(vkrt_scene* s, BuiltTree& t)
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
int uploadHostTree(vkrt_scene* s, const std::vector<FlatTri>& tris, const BuiltBvh* bvh, const BuiltWide8* w8, const std::vector<uint8_t>* instDissolves,
                   hipStream_t stream, BuiltTree& t)
{
  const std::vector<uint32_t>& order = w8 ? w8->triOrder : bvh->triOrder;
  std::vector<float> packed;
  std::vector<uint32_t> shadeRec;
  pack_triangles(tris, order, packed, s->dev.watertight != 0, instDissolves);
  pack_tri_shade(tris, order, s->indices.data(), s->primMeshes.data(), s->nodes.data(), shadeRec);
  const void* nodeData = w8 ? (const void*)w8->nodes.data() : (const void*)bvh->nodes.data();
  t = w8 ? BuiltTree{1, tris.empty() ? VKRT_TRAV_DONE : 0, w8->maxDepth, w8->nodeCount, w8->sahCost, w8->nodes.size() * 4, packed.size() * 4}
         : BuiltTree{0, bvh->rootRef, bvh->maxDepth, (uint32_t)(bvh->nodes.size() / 16), bvh->sahCost, bvh->nodes.size() * 4, packed.size() * 4};
  const char* what = "uploading the acceleration structure";
  HIP_TRY_AS(t.buf.nodes.alloc(std::max<size_t>(t.nodeBytes, VKRT_WNODE_MIN_ALLOC)), what);
  HIP_TRY_AS(t.buf.tris.alloc(std::max<size_t>(t.triangleBytes, 48)), what);
  HIP_TRY_AS(t.buf.triShade.alloc(std::max<size_t>(shadeRec.size() * 4, 16)), what);
  hipError_t e = t.nodeBytes ? hipMemcpyAsync(t.buf.nodes.get(), nodeData, t.nodeBytes, hipMemcpyHostToDevice, stream) : hipSuccess;
  if(e == hipSuccess && !packed.empty())
    e = hipMemcpyAsync(t.buf.tris.get(), packed.data(), t.triangleBytes, hipMemcpyHostToDevice, stream);
  if(e == hipSuccess && !shadeRec.empty())
    e = hipMemcpyAsync(t.buf.triShade.get(), shadeRec.data(), shadeRec.size() * 4, hipMemcpyHostToDevice, stream);
  // the host arrays end with this call: whatever was enqueued is waited for, on the failing paths too
  const hipError_t waited = hipStreamSynchronize(stream);
  HIP_TRY_AS(e != hipSuccess ? e : waited, what);
  return VKRT_OK;
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
  RC_TRY(enter(s));
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

  BuiltTree tree;
  if(wantSah)
  {
    std::vector<FlatTri> tris;
    flatten_instances(s->positions.data(), s->indices.data(), s->primMeshes.data(), s->nodes.data(), (uint32_t)s->nodes.size(), tris);
    BuiltBvh bvh;
    BuiltWide8 w8;
    if(wide)
      build_wide8_host(tris, w8, watertight);
    else
      build_sah_host(tris, 4, bvh, watertight);
    RC_TRY(uploadHostTree(s, tris, wide ? nullptr : &bvh, wide ? &w8 : nullptr, dissolvePtr, stream, tree));
    s->dev.triCount = (uint32_t)tris.size();
    s->info.triangle_count = (uint32_t)tris.size();
  }
  else
  {
    // GPU radix-tree build (Morton codes, sort, Karras hierarchy, bottom-up fit).  For the trace-optimised layout the
    // binary tree keeps one triangle per leaf and is collapsed into wide8 nodes by the same SAH-optimal DP as the SAH
    // path -- on the device too (wide_collapse.hip); nothing but four statistics words comes back to the host.
    // VKRT_BUILD_PLOC_GPU: same pipeline with the radix tree replaced by locally-ordered clustering (ploc.hip)
    LbvhParams p;
    p.wide = wide;
    p.ploc = wantPloc;
    p.splitPercent = (unsigned)splitBudget;
    LbvhResult r;
    if(const int rc = build_lbvh_device(s->dev, (uint32_t)s->nodes.size(), s->primMeshes, s->nodes, p, stream, r); rc != VKRT_OK)
      return fail(rc, "%s build failed: %s", wantPloc ? "PLOC" : "LBVH", r.error.c_str());
    s->info.triangle_count = r.uniqueTris;
    s->dev.triCount = r.triCount;  // slots: a pre-split triangle occupies one per reference
    if(r.wide.buf.nodes.get())
      tree = std::move(r.wide);
    else if(wide && r.triCount > 0)
    {
      // fallback (a single triangle, or a radix tree too deep for the device collapse's level budget): download the binary
      // tree (device layout == host layout of BuiltBvh) and the sorted triangle records, collapse on the host
      BuiltBvh b2;
      b2.nodes.resize((size_t)r.tree.nodeCount * 16);
      std::vector<float> records((size_t)r.triCount * 12);
      hipError_t e = hipSuccess;
      if(r.tree.nodeCount) e = hipMemcpy(b2.nodes.data(), r.tree.buf.nodes.get(), b2.nodes.size() * 4, hipMemcpyDeviceToHost);
      if(e == hipSuccess) e = hipMemcpy(records.data(), r.tree.buf.tris.get(), records.size() * 4, hipMemcpyDeviceToHost);
      r.tree.buf = TreeBuffers{};  // (freed before the wide tree is uploaded)
      if(e != hipSuccess)
        return fail(VKRT_ERR_HIP, "LBVH download: %s", hipGetErrorString(e));
      b2.rootRef = r.tree.rootRef;
      b2.maxDepth = r.tree.maxDepth;
      b2.triOrder.resize(r.triCount);
      // (decoded p1 = v0 + e1 is not the exact vertex, but the boxes of the collapse only grow by it; pack_triangles sets the any-hit
      // flag that decoding clears again)
      std::vector<FlatTri> tris(r.triCount);
      for(uint32_t k = 0; k < r.triCount; k++)
      {
        b2.triOrder[k] = k;
        tris[k] = unpack_triangle(&records[(size_t)k * 12], watertight);
      }
      BuiltWide8 w8;
      collapse_wide8(b2, tris, w8, watertight);
      RC_TRY(uploadHostTree(s, tris, nullptr, &w8, dissolvePtr, stream, tree));
    }
    else
      tree = std::move(r.tree);
  }
  installTree(s, tree);
  scene_bounds(s->positions, s->indices, s->primMeshes, s->nodes, s->dev.sceneLo, s->dev.sceneHi, s->hasLargeTriangles);
  RC_TRY(traversalSettings(s));
  if(s->dev.layout == 1u)
  {  // the node-mask table of the ray-query filter lives and dies with the tree
    HIP_TRY(s->nodeMasks.alloc(std::max<size_t>(s->info.node_bytes / VKRT_WNODE_BYTES * 8, 16)));
    RC_TRY(computeNodeMasks(s, stream));
  }
  s->info.build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  s->built = true;
  if(s->opt[VKRT_OPT_ANYHIT_DISSOLVE] != 0)  // what the triangle flags of this tree cover (vkrt_scene_update_materials' dissolve rule)
    for(const float a : s->materialAlpha)
      s->builtNonOpaque.push_back(a < 1.0f ? 1 : 0);
  return VKRT_OK;
}

}  // namespace

extern "C" {

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
  RC_TRY(syncHostMirror(s, true, "vkrt_accel_build"));
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
    RC_TRY(enter(s));
    HIP_TRY(readBack(&out->sah_cost, &s->refit.words[2], 4));
  }
  return VKRT_OK;
}

int vkrt_scene_update_nodes(vkrt_scene* s, uint32_t first, uint32_t count, const vkrt_node* nodes, void* hip_stream)
{
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "scene is NULL");
  if(count && !nodes)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "nodes is NULL");
  CHECK_TRY(check_node_range(nullptr, first, count, s->nodes.size(), err));
  // the rules of vkrt_scene_create, checked for the whole range before anything changes (a refused call leaves the scene as it was)
  for(uint32_t i = 0; i < count; i++)
  {
    CHECK_TRY(check_prim_mesh_kept(first + i, nodes[i].primMesh, s->nodes[(size_t)first + i].primMesh, err));
    CHECK_TRY(check_transform(nodes[i], first + i, err));
  }
  if(count == 0)
    return VKRT_OK;
  RC_TRY(enter(s));
  std::vector<DevInstance> inst(count);
  for(uint32_t i = 0; i < count; i++)
    make_instance(nodes[i], s->vis[(size_t)first + i], inst[i]);  // (the visibility word stays; the mirrored bit follows the new matrix)
  // Stream-ordered: the records travel as kernel arguments of launches on hip_stream, after whatever the caller enqueued there before
  // (a trace that still reads the old transforms) and before whatever comes after (the refit, the next trace).  The trace entry points'
  // internal lane streams fork from and join to the caller's stream, so ordering on it is all that is needed.
  HIP_TRY(upload_instances(const_cast<DevInstance*>(s->dev.instances), first, count, inst.data(), (hipStream_t)hip_stream));
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
  if(s->dissolveRebuild)
    return fail(VKRT_ERR_NOT_BUILT, "vkrt_accel_refit after vkrt_scene_update_materials gave a material alpha < 1 that was opaque when the tree was built "
                "with VKRT_OPT_ANYHIT_DISSOLVE: a refit keeps the triangle flags, vkrt_accel_build first");
  RC_TRY(enter(s));
  hipStream_t stream = (hipStream_t)hip_stream;
  std::string err;
  if(!s->refit.mem.get())
  {  // first refit of this build: scratch + level lists (the one place a refit allocates and synchronises)
    const uint32_t nodeCap = (uint32_t)(s->info.node_bytes / (s->dev.layout == 1u ? VKRT_WNODE_BYTES : 64u));
    if(const int rc = refit_prepare(s->dev, nodeCap, stream, s->refit, err); rc != VKRT_OK)
    {
      s->refit = RefitScratch{};
      return fail(rc, "vkrt_accel_refit: %s", err.c_str());
    }
  }
  // Everything the build decided stays: layout, record format, split references, dissolve flags, any-hit order, stackCap, step bound.
  // sceneLo / sceneHi (read only by the any-hit order heuristic, which cannot change a pixel) also stay as built: updating them would
  // need the new bounds on the host, i.e. a synchronisation.
  if(const int rc = refit_enqueue(s->dev, (uint32_t)s->nodes.size(), s->refit, stream, err); rc != VKRT_OK)
    return fail(rc, "vkrt_accel_refit: %s", err.c_str());
  s->refitted = true;
  s->stale = false;
  return VKRT_OK;
}

int vkrt_scene_update_node_transforms(vkrt_scene* s, const vkrt_node_update* u, void* hip_stream)
{
  CHECK_TRY(check_node_update_desc(u, err));
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_scene_update_node_transforms: scene is NULL");
  const size_t nodeCount = s->nodes.size(), n = u->count;
  CHECK_TRY(check_node_update_range(*u, nodeCount, err));
  if(n == 0)
    return VKRT_OK;
  if(u->memory != VKRT_MEMORY_HOST)
  {
    RC_TRY(enter(s));
    // One launch on hip_stream, stream-ordered like vkrt_scene_update_nodes; no allocation, no copy, no wait.  The host copy of the
    // matrices falls behind: its readers download the records first (syncHostMirror).
    HIP_TRY(launch_node_transforms(const_cast<DevInstance*>(s->dev.instances), (uint32_t)nodeCount, u->first, u->count, u->world_matrices,
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
    RC_TRY(vkrt_scene_update_nodes(s, u->node_indices[k], (uint32_t)(end - k), &nodes[k], hip_stream));
    k = end;
  }
  return VKRT_OK;
}

int vkrt_debug_read_instances(vkrt_scene* s, uint32_t first, uint32_t count, void* out, uint64_t bytes)
{
  const char* who = "vkrt_debug_read_instances";
  if(!s || !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
  CHECK_TRY(check_node_range(who, first, count, s->nodes.size(), err));
  if(bytes != (uint64_t)count * sizeof(DevInstance))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: bytes %llu != %zu x %u records", who, (unsigned long long)bytes, sizeof(DevInstance), count);
  RC_TRY(enter(s));
  HIP_TRY(readBack(out, s->dev.instances + first, (size_t)count * sizeof(DevInstance)));
  return VKRT_OK;
}

}  // extern "C"
