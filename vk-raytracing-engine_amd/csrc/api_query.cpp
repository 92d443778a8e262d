// api_query.cpp -- queries on caller rays, points and hits (include/vkrt.h): vkrt_intersect*, vkrt_occluded*, vkrt_closest_point (with
// its work-counting debug twin), vkrt_hit_surface, vkrt_hit_motion.  What the calls refuse of their arguments is entry_checks.h's.
#include "scene_state.h"

using namespace vkrt;

namespace {

static_assert(sizeof(vkrt_ray) == 32 && sizeof(vkrt_hit) == 32, "k_query reads and writes 2 x 16 B per ray");
static_assert(sizeof(vkrt_surface) == 128, "k_hit_surface writes 8 x 16 B per record");
static_assert(sizeof(vkrt_query_opts) == 16, "include/vkrt.h");
static_assert(sizeof(vkrt_point_query) == 16, "k_closest_point reads 16 B per query");

// The argument checks every query entry point starts with, in this order: the scene, then (n > 0) an array that is NULL, then an array
// that is misaligned (check_query_arrays).
#define QUERY_ARRAYS_TRY(s, who, n, alignText, ...)                                          \
  do { if(!(s)) return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);            \
       CHECK_TRY(check_query_arrays(who, n, {__VA_ARGS__}, alignText, err)); } while(0)

// The trace set-up every query entry point shares once its own arguments are checked and n > 0: the tree can be traced, the scene's
// device is current, and the walk's scene carries the call's options.  filter: the filtering walk is needed -- only where it can change
// a result: a facing flag, or a cull mask that some node's mask misses.
int querySetup(vkrt_scene* s, const vkrt_query_opts& q, const char* who, DevQueryScene& qs, bool& filter)
{
  RC_TRY(enter(s, who));
  static_cast<DevScene&>(qs) = s->dev;
  qs.nodeMasks = s->nodeMasks.get<const uint2>();
  qs.cullMask = q.cull_mask;
  qs.rayFlags = q.ray_flags & (VKRT_RAY_CULL_BACK_FACING | VKRT_RAY_CULL_FRONT_FACING);
  filter = qs.rayFlags != 0u || !everyMaskMeets(s, q.cull_mask);
  return VKRT_OK;
}

// vkrt_intersect / vkrt_occluded (and the _ex pair, whose options are checked by the caller): one k_query launch per 2^30 rays on the
// caller's stream (query.hip); out = hits or occluded flags
int rayQuery(vkrt_scene* s, const vkrt_ray* rays, uint32_t n, const vkrt_query_opts& q, void* out, bool anyHit, void* hip_stream, const char* who)
{
  QUERY_ARRAYS_TRY(s, who, n, "(rays and hits: 16 bytes, occluded: 4)", {rays, 16u, false}, {out, anyHit ? 4u : 16u, false});
  if(n == 0)
    return VKRT_OK;
  DevQueryScene qs;
  bool filter;
  RC_TRY(querySetup(s, q, who, qs, filter));
  const bool opaque = (q.ray_flags & VKRT_RAY_OPAQUE) != 0u;
  HIP_TRY(vkrt_launch_query(qs, (const float4*)rays, n, q.anyhit_seed, filter, opaque, s->alphaMasks != 0u, anyHit ? nullptr : (float4*)out, anyHit ? (int*)out : nullptr,
                            (hipStream_t)hip_stream));
  return VKRT_OK;
}

}  // namespace

extern "C" {

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

int vkrt_intersect_ex(vkrt_scene* s, const vkrt_ray* rays, uint32_t n, const vkrt_query_opts* opts, vkrt_hit* hits, void* hip_stream)
{
  CHECK_TRY(check_query_opts(opts, "vkrt_intersect_ex", err));
  return rayQuery(s, rays, n, *opts, hits, false, hip_stream, "vkrt_intersect_ex");
}

int vkrt_occluded_ex(vkrt_scene* s, const vkrt_ray* rays, uint32_t n, const vkrt_query_opts* opts, int32_t* occluded, void* hip_stream)
{
  CHECK_TRY(check_query_opts(opts, "vkrt_occluded_ex", err));
  return rayQuery(s, rays, n, *opts, occluded, true, hip_stream, "vkrt_occluded_ex");
}

// one k_query_multi launch per 2^30 rays on the caller's stream (multihit.hip)
int vkrt_intersect_multi(vkrt_scene* s, const vkrt_ray* rays, uint32_t n, const vkrt_query_opts* opts, uint32_t max_hits, vkrt_hit* hits,
                         int32_t* counts, void* hip_stream)
{
  const char* who = "vkrt_intersect_multi";
  CHECK_TRY(check_query_opts(opts, who, err));
  CHECK_TRY(check_max_hits(max_hits, err));
  QUERY_ARRAYS_TRY(s, who, n, "(rays and hits: 16 bytes, counts: 4)", {rays, 16u, false}, {hits, 16u, false}, {counts, 4u, true});
  if(n == 0)
    return VKRT_OK;
  DevQueryScene qs;
  bool filter;
  RC_TRY(querySetup(s, *opts, who, qs, filter));
  const bool opaque = (opts->ray_flags & VKRT_RAY_OPAQUE) != 0u;
  HIP_TRY(vkrt_launch_query_multi(qs, (const float4*)rays, n, opts->anyhit_seed, filter, opaque, s->alphaMasks != 0u, max_hits, (float4*)hits, counts,
                                  (hipStream_t)hip_stream));
  return VKRT_OK;
}

// one k_closest_point launch per 2^30 queries on the caller's stream (closest.hip)
int vkrt_closest_point(vkrt_scene* s, const vkrt_point_query* queries, uint32_t n, const vkrt_query_opts* opts, vkrt_hit* hits, void* hip_stream)
{
  const char* who = "vkrt_closest_point";
  vkrt_query_opts q;
  CHECK_TRY(check_point_opts(opts, who, q, err));
  QUERY_ARRAYS_TRY(s, who, n, "(queries and hits: 16 bytes)", {queries, 16u, false}, {hits, 16u, false});
  if(n == 0)
    return VKRT_OK;
  DevQueryScene qs;
  bool filter;
  RC_TRY(querySetup(s, q, who, qs, filter));
  HIP_TRY(vkrt_launch_closest_point(qs, (const float4*)queries, n, filter, (float4*)hits, nullptr, (hipStream_t)hip_stream));
  return VKRT_OK;
}

int vkrt_debug_closest_point_work(vkrt_scene* s, const vkrt_point_query* host_queries, uint32_t n, const vkrt_query_opts* opts, uint64_t out[2])
{
  const char* who = "vkrt_debug_closest_point_work";
  vkrt_query_opts q;
  CHECK_TRY(check_point_opts(opts, who, q, err));
  if(!s || !out || (n && !host_queries))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  out[0] = out[1] = 0;
  if(n == 0)
    return VKRT_OK;
  DevQueryScene qs;
  bool filter;
  RC_TRY(querySetup(s, q, who, qs, filter));
  DevBuf dQ, dH, dW;
  HIP_TRY(dQ.alloc((size_t)n * sizeof(vkrt_point_query))); HIP_TRY(dH.alloc((size_t)n * sizeof(vkrt_hit))); HIP_TRY(dW.alloc(2 * sizeof(uint64_t)));
  HIP_TRY(hipMemcpy(dQ.get(), host_queries, (size_t)n * sizeof(vkrt_point_query), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(dW.get(), 0, 2 * sizeof(uint64_t)));
  HIP_TRY(vkrt_launch_closest_point(qs, dQ.get<const float4>(), n, true, dH.get<float4>(), dW.get<unsigned long long>(), nullptr));
  HIP_TRY(readBack(out, dW.get(), 2 * sizeof(uint64_t)));
  return VKRT_OK;
}

int vkrt_hit_surface(vkrt_scene* s, const vkrt_hit* hits, uint32_t n, uint32_t fields, vkrt_surface* out, void* hip_stream)
{
  QUERY_ARRAYS_TRY(s, "vkrt_hit_surface", n, "(hits and out: 16 bytes)", {hits, 16u, false}, {out, 16u, false});
  if(fields != VKRT_SURFACE_GEOMETRY && fields != (VKRT_SURFACE_GEOMETRY | VKRT_SURFACE_MATERIAL))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_hit_surface: fields 0x%x is neither VKRT_SURFACE_GEOMETRY nor VKRT_SURFACE_GEOMETRY | VKRT_SURFACE_MATERIAL", fields);
  if(n == 0)
    return VKRT_OK;
  // (no checkBuilt: everything read here is kept current by vkrt_scene_update_nodes / vkrt_scene_update_vertices, the tree is not read)
  RC_TRY(enter(s));
  DevSurfaceScene ss;
  static_cast<DevScene&>(ss) = s->dev;
  ss.primMeshes = s->surfacePrimMeshes;
  ss.instanceCount = (uint32_t)s->nodes.size();
  HIP_TRY(vkrt_launch_hit_surface(ss, (const float4*)hits, n, (fields & VKRT_SURFACE_MATERIAL) != 0u, (float4*)out, (hipStream_t)hip_stream));
  return VKRT_OK;
}

int vkrt_hit_motion(vkrt_scene* s, const vkrt_hit* hits, uint32_t n, float* current, float* previous, void* hip_stream)
{
  QUERY_ARRAYS_TRY(s, "vkrt_hit_motion", n, "(hits, current and previous: 16 bytes)", {hits, 16u, false}, {current, 16u, true}, {previous, 16u, true});
  if(!current && !previous)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_hit_motion: current and previous are both NULL");
  if(n == 0)
    return VKRT_OK;
  // (no checkBuilt: like vkrt_hit_surface, nothing read here belongs to the tree)
  RC_TRY(enter(s));
  DevMotionScene ms;
  static_cast<DevScene&>(ms) = s->dev;
  ms.primMeshes = s->surfacePrimMeshes;
  ms.instanceCount = (uint32_t)s->nodes.size();
  ms.prevInstances = s->prevInstances();
  ms.prevPositions = s->prevPositions();
  HIP_TRY(vkrt_launch_hit_motion(ms, (const float4*)hits, n, (float4*)current, (float4*)previous, (hipStream_t)hip_stream));
  return VKRT_OK;
}

}  // extern "C"
