// api_scene.cpp -- the scene's life and its settings (include/vkrt.h): version, devices, create / destroy, options, instance visibility,
// material alpha, counters, the timing of the last trace, and the last error, whose thread-local lives here (scene_state.h fail).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "scene_pack.h"
#include "node_update.h"
#include "scene_state.h"

using namespace vkrt;

namespace {
thread_local std::string g_lastError;
}

int vkrt::fail(int code, const char* fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_lastError = buf;
  return code;
}

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

static_assert(sizeof(vkrt_instance_visibility) == 4, "include/vkrt.h");
static_assert(sizeof(vkrt_material_alpha) == 8 && sizeof(vkrt_material_alpha) == sizeof(uint2), "k_material_alpha takes (mode, cutoff bits) pairs");

}  // namespace

extern "C" {

int vkrt_abi_version(void) { return VKRT_ABI_VERSION; }
const char* vkrt_last_error(void) { return g_lastError.c_str(); }

int vkrt_device_count(void)
{
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int vkrt_scene_create(const vkrt_scene_desc* d, int device, vkrt_scene** out)
{
  if(!out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  std::string err;
  int rc = validate_scene(d, err);
  if(rc != VKRT_OK)
    return failWith(rc, err);
  const int ndev = vkrt_device_count();
  if(ndev <= 0)
    return fail(VKRT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
  if(device < 0 || device >= ndev)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "device %d out of range [0,%d)", device, ndev);
  std::unique_ptr<vkrt_scene, void (*)(vkrt_scene*)> owner(new vkrt_scene(), vkrt_scene_destroy);  // destroyed by every early return
  vkrt_scene* s = owner.get();
  s->device = device;
  initial_options(s->opt);
  RC_TRY(enter(s));
  hipDeviceProp_t prop;
  if(hipGetDeviceProperties(&prop, device) == hipSuccess)
    s->cuCount = prop.multiProcessorCount;

  s->positions.assign(d->positions, d->positions + 3 * (size_t)d->vertex_count);
  s->indices.assign(d->indices, d->indices + d->index_count);
  s->primMeshes.assign(d->prim_meshes, d->prim_meshes + d->prim_mesh_count);
  s->nodes.assign(d->nodes, d->nodes + d->node_count);
  s->lightCount = d->light_count;
  s->materialCount = d->material_count;
  s->alpha.assign(d->material_count, kDefaultAlpha);
  for(uint32_t i = 0; i < d->material_count; i++)
    s->materialAlpha.push_back(d->materials[i].pbrBaseColorFactor[3]);
  s->vis.assign(d->node_count, kDefaultVisibility);
  noteMasks(s);

  // VKRT_TEX_QUADS=0 (test hook): no footprint pool
  const char* quadEnv = getenv("VKRT_TEX_QUADS");
  PackedScene packed;
  if((rc = pack_scene(d, !(quadEnv && atoi(quadEnv) == 0), packed, err)) != VKRT_OK)
    return failWith(rc, err);
  DevScene& D = s->dev;
  const float *pn = nullptr, *lut = nullptr;
  const uint32_t *pm = nullptr, *quads = nullptr;
  RC_TRY(upload(s, d->positions, 3 * (size_t)d->vertex_count, &D.positions));
  RC_TRY(upload(s, d->indices, (size_t)d->index_count, &D.indices));
  RC_TRY(upload(s, packed.vertexPN.data(), packed.vertexPN.size(), &pn));
  RC_TRY(upload(s, d->lights, (size_t)d->light_count, &D.lights));
  RC_TRY(upload(s, packed.primMeshes.data(), packed.primMeshes.size(), &pm));
  RC_TRY(upload(s, packed.instances.data(), packed.instances.size(), &D.instances));
  RC_TRY(upload(s, packed.materials.data(), packed.materials.size(), &D.materials));
  RC_TRY(upload(s, packed.shadeMaterials.data(), packed.shadeMaterials.size(), &D.shadeMaterials));
  RC_TRY(upload(s, packed.textures.data(), packed.textures.size(), &D.textures));
  RC_TRY(upload(s, packed.texMips.data(), packed.texMips.size(), &D.texMips));
  RC_TRY(upload(s, packed.texels.data(), packed.texels.size(), &D.texels));
  if(!packed.texQuads.empty())
    RC_TRY(upload(s, packed.texQuads.data(), packed.texQuads.size(), &quads));
  RC_TRY(upload(s, packed.srgbLut, 512, &lut));
  RC_TRY(upload(s, packed.srgbEncode, (size_t)VKRT_SRGB_THRESHOLDS, &s->srgbEncode));
  s->textures = packed.textures;
  s->texMips = packed.texMips;
  s->texQuadFirst = packed.texQuadFirst;
  D.vertexPN = (const float4*)pn;
  s->surfacePrimMeshes = (const uint4*)pm;
  D.texQuads = (const uint4*)quads;
  D.srgbLut = lut;
  D.textureCount = d->texture_count;
  D.rootRef = VKRT_TRAV_DONE;  // no tree yet: BVH2 layout, nothing postponed or shared (the zeroes of `dev`)
  D.stackCap = 1;
  D.stepLimit = 64;
  D.gbufferMips = 1;

  if(s->tables.alloc(&s->workCounter, 16) != hipSuccess) return fail(VKRT_ERR_OUT_OF_MEMORY, "hipMalloc(work counter)");
  if(s->tables.alloc(&s->counters, 1) != hipSuccess) return fail(VKRT_ERR_OUT_OF_MEMORY, "hipMalloc(counters)");
  D.faults = &s->counters->v[0][10];
  if(hipMemset(s->counters, 0, sizeof(DevCounters)) != hipSuccess) return fail(VKRT_ERR_HIP, "hipMemset(counters)");
  if(s->evStart.create() != hipSuccess || s->evStop.create() != hipSuccess)
    return fail(VKRT_ERR_HIP, "hipEventCreate");
  *out = owner.release();
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
  if(clamp_option(option, value) != value)
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
  if(option == VKRT_INFO_ANYHIT_ORDER || option == VKRT_INFO_SPLIT_BUDGET)
  {
    *value = !s->built ? 0 : option == VKRT_INFO_ANYHIT_ORDER ? (int)(s->dev.shareFlags & 6u) : s->splitResolved;
    return VKRT_OK;
  }
  if(option < VKRT_OPT_MODE || option > VKRT_OPT_ALPHA_TEST)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "unknown option %d", option);
  *value = s->opt[option];
  return VKRT_OK;
}

int vkrt_scene_set_instance_visibility(vkrt_scene* s, uint32_t first, uint32_t count, const vkrt_instance_visibility* vis, void* hip_stream)
{
  const char* who = "vkrt_scene_set_instance_visibility";
  CHECK_TRY(check_visibility_values(who, count, vis, err));
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  CHECK_TRY(check_node_range(who, first, count, s->nodes.size(), err));
  if(count == 0)
    return VKRT_OK;
  RC_TRY(enter(s));
  // the visibility words alone, sent as kernel arguments on hip_stream like vkrt_scene_update_nodes sends its records: stream-ordered,
  // nothing staged, no synchronisation.  The kernel keeps each record's mirrored bit and does not touch its transform, so a transform
  // that came from device memory (vkrt_scene_update_node_transforms) stays; with the host copy current the records are bit for bit
  // what make_instance gives for the node and the new visibility
  std::vector<uint32_t> words(count);
  for(uint32_t i = 0; i < count; i++)
    words[i] = (uint32_t)vis[i].mask | ((uint32_t)vis[i].flags << 8);
  hipStream_t stream = (hipStream_t)hip_stream;
  HIP_TRY(launch_instance_visibility(const_cast<DevInstance*>(s->dev.instances), first, count, words.data(), stream));
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
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  CHECK_TRY(check_node_range(who, first, count, s->nodes.size(), err));
  std::copy(s->vis.begin() + first, s->vis.begin() + first + count, out);
  return VKRT_OK;
}

int vkrt_scene_set_material_alpha(vkrt_scene* s, uint32_t first, uint32_t count, const vkrt_material_alpha* alpha, void* hip_stream)
{
  const char* who = "vkrt_scene_set_material_alpha";
  CHECK_TRY(check_alpha_values(who, count, alpha, err));
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  CHECK_TRY(check_material_range(who, first, count, s->materialCount, err));
  if(count == 0)
    return VKRT_OK;
  RC_TRY(enter(s));
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
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  CHECK_TRY(check_material_range(who, first, count, s->materialCount, err));
  std::copy(s->alpha.begin() + first, s->alpha.begin() + first + count, out);
  return VKRT_OK;
}

int vkrt_counters_reset(vkrt_scene* s, void* hip_stream)
{
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "scene is NULL");
  RC_TRY(enter(s));
  HIP_TRY(hipMemsetAsync(s->counters, 0, sizeof(DevCounters), (hipStream_t)hip_stream));
  return VKRT_OK;
}

int vkrt_counters_read(vkrt_scene* s, vkrt_counters* out)
{
  if(!s || !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  RC_TRY(enter(s));
  DevCounters h;
  HIP_TRY(readBack(&h, s->counters, sizeof h));
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

}  // extern "C"
