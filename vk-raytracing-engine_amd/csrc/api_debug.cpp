// api_debug.cpp -- the test hooks of include/vkrt.h that belong to no other area: rays from host arrays, the readers and the checker of the
// installed tree, the builders' split references, the device's arithmetic and shading on host records.  Each reads through readBack.
#include "bvh_host.h"
#include "lbvh.h"
#include "scene_state.h"

using namespace vkrt;

extern "C" {

int vkrt_debug_trace_rays(vkrt_scene* s, uint32_t n, const float* origins, const float* directions, float tmin, float tmax,
                          int any_hit, float* t, float* u, float* v, int32_t* gid)
{
  if(!s || (n && (!origins || !directions || !t || !u || !v || !gid)))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  RC_TRY(checkBuilt(s, "vkrt_debug_trace_rays"));
  if(n == 0)
    return VKRT_OK;
  RC_TRY(enter(s));
  DevBuf dO, dD, dT, dU, dV, dG;
  const size_t b3 = (size_t)n * 3 * sizeof(float), b1 = (size_t)n * sizeof(float);
  HIP_TRY(dO.alloc(b3)); HIP_TRY(dD.alloc(b3)); HIP_TRY(dT.alloc(b1));
  HIP_TRY(dU.alloc(b1)); HIP_TRY(dV.alloc(b1)); HIP_TRY(dG.alloc(b1));
  HIP_TRY(hipMemcpy(dO.get(), origins, b3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dD.get(), directions, b3, hipMemcpyHostToDevice));
  HIP_TRY(vkrt_launch_trace_rays(s->dev, n, dO.get<float>(), dD.get<float>(), tmin, tmax, any_hit, dT.get<float>(), dU.get<float>(), dV.get<float>(),
                                 dG.get<int>(), nullptr));
  HIP_TRY(readBack(t, dT.get(), b1));
  HIP_TRY(hipMemcpy(u, dU.get(), b1, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(v, dV.get(), b1, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(gid, dG.get(), b1, hipMemcpyDeviceToHost));
  return VKRT_OK;
}

int vkrt_debug_read_accel(vkrt_scene* s, void* nodes, uint64_t nodes_bytes, void* tris, uint64_t tris_bytes, int32_t* root_ref)
{
  if(!s || !root_ref || (nodes_bytes && !nodes) || (tris_bytes && !tris))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  RC_TRY(enter(s, "vkrt_debug_read_accel"));
  if(nodes_bytes != s->info.node_bytes || tris_bytes != s->info.triangle_bytes)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_debug_read_accel: buffers of %llu / %llu bytes for a tree of %llu / %llu",
                (unsigned long long)nodes_bytes, (unsigned long long)tris_bytes, (unsigned long long)s->info.node_bytes,
                (unsigned long long)s->info.triangle_bytes);
  HIP_TRY(readBack(nodes, s->dev.nodes, nodes_bytes));
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
  RC_TRY(enter(s));
  HIP_TRY(readBack(out, s->nodeMasks.get(), bytes));
  return VKRT_OK;
}

int vkrt_debug_read_triangle_ids(vkrt_scene* s, uint32_t* out, uint64_t bytes)
{
  if(!s || !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  RC_TRY(enter(s, "vkrt_debug_read_triangle_ids"));
  const uint64_t slots = s->info.triangle_bytes / 48, want = slots * 4;
  if(bytes != want)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_debug_read_triangle_ids: a buffer of %llu bytes for %llu slots (%llu bytes)",
                (unsigned long long)bytes, (unsigned long long)slots, (unsigned long long)want);
  // word 9 of every 48-B record: the flattened triangle id (bit 31: the non-opaque flag of the any-hit stage)
  std::vector<uint32_t> rec((size_t)slots * 12);
  HIP_TRY(readBack(rec.data(), s->dev.tris, (size_t)slots * 48));
  for(uint64_t k = 0; k < slots; k++) out[k] = rec[(size_t)k * 12 + 9] & 0x7fffffffu;
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
  RC_TRY(enter(s));
  HIP_TRY(hipDeviceSynchronize());
  // the kernels read the device's positions and the host's matrices: the mirror brings the nodes alone
  RC_TRY(syncHostMirror(s, false, "vkrt_debug_split_references"));
  // the builders' view of the scene with the option as it stands now; the installed tree keeps the setting it was built with
  DevScene sc = s->dev;
  sc.watertight = s->opt[VKRT_OPT_WATERTIGHT] != 0 ? 1u : 0u;
  std::string err;
  if(const int rc = split_references_device(sc, (uint32_t)s->nodes.size(), s->primMeshes, s->nodes, split_percent, nullptr, prio, scale, ref_tri, ref_box,
                                            capacity, ref_count, err); rc != VKRT_OK)
    return fail(rc, "vkrt_debug_split_references: %s", err.c_str());
  return VKRT_OK;
}

int vkrt_debug_check_accel(vkrt_scene* s, vkrt_accel_check* out)
{
  if(!s || !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  RC_TRY(enter(s, "vkrt_debug_check_accel"));
  const uint32_t T = s->dev.triCount, N = s->info.node_count;
  std::vector<float> tris((size_t)T * 12);
  std::vector<uint32_t> nodes((size_t)N * (s->dev.layout == 1u ? 20 : 16));
  HIP_TRY(readBack(tris.data(), s->dev.tris, tris.size() * 4));
  if(N)
    HIP_TRY(hipMemcpy(nodes.data(), s->dev.nodes, nodes.size() * 4, hipMemcpyDeviceToHost));
  check_tree(s->dev.layout, s->dev.rootRef, nodes.data(), N, tris.data(), T, s->info.triangle_count, s->dev.watertight != 0, *out);
  return VKRT_OK;
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
  DevBuf dA, dB, dC;
  const size_t bytes = (size_t)n * sizeof(float);
  HIP_TRY(dA.alloc(bytes)); HIP_TRY(dB.alloc(bytes)); HIP_TRY(dC.alloc(bytes));
  HIP_TRY(hipMemcpy(dA.get(), a, bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dB.get(), b, bytes, hipMemcpyHostToDevice));
  HIP_TRY(vkrt_launch_eval_math(op, n, dA.get<float>(), dB.get<float>(), dC.get<float>(), nullptr));
  HIP_TRY(readBack(out, dC.get(), bytes));
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
  DevBuf dIn, dLights, dOut;
  const size_t inBytes = (size_t)n * 40 * sizeof(float), outBytes = (size_t)n * 20 * sizeof(float);
  HIP_TRY(dIn.alloc(inBytes)); HIP_TRY(dOut.alloc(outBytes));
  HIP_TRY(dLights.alloc((size_t)n * VKRT_EVAL_SHADE_MAX_LIGHTS * sizeof(GltfLight)));
  HIP_TRY(hipMemcpy(dIn.get(), in, inBytes, hipMemcpyHostToDevice));
  HIP_TRY(vkrt_launch_eval_shade(n, dIn.get<float>(), dLights.get<float4>(), dOut.get<float>(), nullptr));
  HIP_TRY(readBack(out, dOut.get(), outBytes));
  return VKRT_OK;
}

}  // extern "C"
