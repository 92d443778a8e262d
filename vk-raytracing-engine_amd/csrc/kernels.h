// kernels.h -- host-callable launch wrappers implemented in the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include "device_scene.h"
#include "wf_schedule.h"

hipError_t vkrt_launch_pathtrace(const TraceParams& P, unsigned gridBlocks, bool count, hipStream_t stream);
int        vkrt_pathtrace_block_size();
hipError_t vkrt_pathtrace_occupancy(size_t ldsBytes, int* blocksPerCU);
hipError_t vkrt_launch_trace_rays(const DevScene& sc, unsigned n, const float* o, const float* d, float tmin, float tmax, int anyHit,
                                  float* t, float* u, float* v, int* gid, hipStream_t stream);
hipError_t vkrt_launch_eval_math(int op, unsigned n, const float* a, const float* b, float* out, hipStream_t stream);
// vkrt_debug_eval_shade: n records of 40 floats -> 20 floats each, one per thread of 256-thread blocks; lights = scratch of
// VKRT_EVAL_SHADE_MAX_LIGHTS 32-byte light records (2 float4) per record, written and read by the record's own thread
#define VKRT_EVAL_SHADE_MAX_LIGHTS 16
hipError_t vkrt_launch_eval_shade(unsigned n, const float* in, float4* lights, float* out, hipStream_t stream);

// The three query launches below run one thread per item in chunks of at most 2^30 items (query_common.h query_launch_chunks) and return
// the first launch error; the ray queries pick their triangle mode there too (query_tri_mode, VKRT_QUERY_TM_SWITCH).
// ray queries (query.hip): n caller rays (2 float4 each: origin + tmin, direction + tmax) -> closest hits (2 float4 each, vkrt_hit) when
// hits != NULL, otherwise occluded flags (one int each) into occ.  seed = the any-hit stage's payload seed.  filter: walk with the
// ray-query filter (sc.cullMask / rayFlags / nodeMasks, VKRT_TM_FILTER); opaque: VKRT_RAY_OPAQUE (no any-hit stage); alpha: some
// material of the scene is VKRT_ALPHA_MASK (the alpha-test stage, VKRT_TM_ALPHA, unless opaque).
hipError_t vkrt_launch_query(const DevQueryScene& sc, const float4* rays, uint64_t n, uint32_t seed, bool filter, bool opaque, bool alpha, float4* hits,
                             int* occ, hipStream_t stream);
// multi-hit ray queries (multihit.hip): the first maxHits (1..VKRT_MULTIHIT_MAX) candidates of every ray in the order (t, triangle id) into
// hits (maxHits records of 2 float4 per ray, ray-major, miss records behind the count), their number into counts (may be NULL).  seed,
// filter, opaque, alpha: as vkrt_launch_query.  Walks lane by lane; LDS per wave: the stack columns + 5 x maxHits x 64 words.
hipError_t vkrt_launch_query_multi(const DevQueryScene& sc, const float4* rays, uint64_t n, uint32_t seed, bool filter, bool opaque, bool alpha,
                                   uint32_t maxHits, float4* hits, int* counts, hipStream_t stream);
// closest-point queries (closest.hip): n queries (one float4 each: point + radius) -> the nearest surface point within the radius as a
// vkrt_hit (2 float4 each; t = the distance).  filter: walk with sc.cullMask / sc.nodeMasks.  work != NULL: the instrumented kernel adds
// (nodes visited, triangle records tested) to work[0..1].  Walks lane by lane; LDS per wave: the stack columns.
hipError_t vkrt_launch_closest_point(const DevQueryScene& sc, const float4* queries, uint64_t n, bool filter, float4* hits, unsigned long long* work,
                                     hipStream_t stream);
// The node-mask table of a wide8 tree (query.hip): `sweeps` passes over all nodes, each node ORing its leaves' instance masks and its
// child nodes' bytes; a node of height h is exact after h passes, so sweeps >= the tree's levels gives the table without reading
// anything back.  instCount bounds the instance ids of the records.
hipError_t vkrt_launch_node_masks(const DevScene& sc, uint32_t nodeCount, uint32_t instCount, uint32_t sweeps, uint2* masks, hipStream_t stream);
// (mode, cutoff bits) of materials [first, first + count) into their DevMaterial records: the pairs travel as kernel arguments of launches
// on `stream` (stream-ordered, nothing staged, no synchronisation), like the instance records of refit.hip upload_instances
hipError_t vkrt_launch_material_alpha(DevMaterial* table, uint32_t first, uint32_t count, const uint2* src, hipStream_t stream);
// shading inputs at hit records (surface.hip): n vkrt_hit records (2 float4 each) -> n vkrt_surface records (8 float4 each).  material:
// the four texture taps and the material fields too, else the geometry alone.  Reads no tree.
hipError_t vkrt_launch_hit_surface(const DevSurfaceScene& sc, const float4* hits, uint32_t n, bool material, float4* out, hipStream_t stream);
// surface points at hit records, now and at the scene's last vkrt_scene_motion_mark (motion.hip): n vkrt_hit records -> (xyz, 1) per
// record into cur (from sc.instances / sc.vertexPN) and / or prev (from prevInstances / prevPositions); either may be NULL.  A record
// that is not a hit of the scene gives (0, 0, 0, 0).  Reads no tree.
struct DevMotionScene : DevSurfaceScene
{
  const DevInstance* prevInstances;  // the snapshot, or sc.instances / sc.positions before any mark
  const float* prevPositions;        // vec3[]
};
hipError_t vkrt_launch_hit_motion(const DevMotionScene& sc, const float4* hits, uint32_t n, float4* cur, float4* prev, hipStream_t stream);

// wavefront mode (wavefront.hip)
struct WfTiming
{
  hipEvent_t* events;   // optional pool of 2*rounds+2 events (NULL = no per-kernel timing)
  int capacity;
  int used;             // pairs recorded around k_wf_traverse launches
};
// Lanes: a call's work is dealt to up to VKRT_WF_MAX_LANES lanes, each with its own record streams and its own HIP stream; which lanes,
// which launches and in what order is wf_schedule.h's to say.
struct WfAsync
{
  hipStream_t streams[VKRT_WF_MAX_LANES];  // internal streams (created by the caller of vkrt_launch_wavefront)
  hipEvent_t fork, join[VKRT_WF_MAX_LANES];
  int count;                                // usable entries (0/1 = everything on the caller's stream)
  hipEvent_t* pool;                         // events for the blend order of the frames of one call, no timing
  int poolSize;                             // >= wfPoolEvents(frames) of every call
};
size_t     vkrt_wf_state_bytes(uint32_t pathCapacity, int groups);
void       vkrt_wf_carve(void* base, uint32_t pathCapacity, int groups, WfBuffers* B);
struct WfOptions
{
  int subframes;   // VKRT_OPT_WF_SUBFRAMES
  int travBlock;   // VKRT_OPT_WF_TRAV_BLOCK (64 / 128 / 256)
  int inFlight;    // VKRT_OPT_WF_FRAMES_IN_FLIGHT
};
// frames >= 1: frame k uses wfFrameParams(P, k, seedStep)
hipError_t vkrt_launch_wavefront(const TraceParams& P, const WfBuffers& B, const WfOptions& opt, int frames, uint32_t seedStep, bool count,
                                 hipStream_t stream, WfTiming* timing, const WfAsync* async);
// one launch of k_wf_traverse on the records of round r (wf_traverse.hip): travBlock 64 / 128 / 256 threads per workgroup, tg = grid,
// tlds = LDS bytes of the per-lane stacks; count = the instrumented instantiation.  Launch errors surface through hipGetLastError.
void       vkrt_wf_launch_traverse(const TraceParams& P, const WfBuffers& B, int r, unsigned travBlock, bool count, dim3 tg, size_t tlds,
                                   hipStream_t stream);
// one launch of k_wf_traverse_camera (wf_traverse.hip) for round r, the first round of sample smpl (VKRT_FLAG_CAMERA_ROUNDS): one wave per
// tile of the sub-frame; tlds = LDS bytes of 64 per-lane stacks
void       vkrt_wf_launch_traverse_camera(const TraceParams& P, const WfBuffers& B, int r, int smpl, bool count, size_t tlds, hipStream_t stream);

// hybrid mode (hybrid.hip, wavefront.hip)
struct HybridGi  // the planes of the hybrid passes: one struct for the three launches below
{
  float4* color;           // G-buffer planes: k_gbuffer writes them, the trace reads them
  float4* position;
  float4* normal;
  float2* rough;
  float4* accum;           // rgba32f accumulation image (read-modify-write; unused by k_gbuffer)
  float4* nrdRadHitD;      // optional NRD / REBLUR front-end attachments (include/vkrt.h vkrt_nrd_planes; NULL = not requested):
  float* nrdViewZ;         // k_gbuffer clears radHitD and writes viewZ, the GI path reads viewZ and writes radHitD
};
// nrdNormRough != NULL: the NRD attachments are wanted: that plane and G.nrdViewZ are filled too, with viewMatrix = the raster pass's
// view matrix (column-major)
// hits != NULL: one vkrt_hit (2 float4) per pixel too, rows stacked like the planes (vkrt_gbuffer_raycast_hits)
hipError_t vkrt_launch_gbuffer(const TraceParams& P, const float clearColor[4], int lightsCount, const HybridGi& G, float* nrdNormRough,
                               const float* viewMatrix, float4* hits, hipStream_t stream);
// giLater: non-NULL = the GI part follows on the wavefront streams (vkrt_launch_hybrid_gi): the kernel does shadows + AO only and
// leaves (seed, visibility) per pixel there instead of writing the accumulation image
hipError_t vkrt_launch_hybrid(const TraceParams& P, const HybridGi& G, uint2* giLater, hipStream_t stream);
// GI of the hybrid mode on the path tracer's wavefront streams (wavefront.hip): k_hybrid (direct part, tmp = per-pixel seed and
// visibility) -> k_hy_gi_init (first GI ray of every shaded pixel) -> pc.depth rounds of traverse / shade -> accumulation image.
hipError_t vkrt_launch_hybrid_gi(const TraceParams& P, const WfBuffers& B, const HybridGi& G, unsigned travBlock, hipStream_t stream);
// the scratch plane k_hybrid leaves the per-pixel (seed, visibility) in for vkrt_launch_hybrid_gi
uint2* vkrt_wf_hybrid_tmp(const WfBuffers& B);
hipError_t vkrt_launch_post(int rtMode, int viewAccumulated, int useGI, unsigned n, const float* mainImg, const float* rtImg, float* out,
                            hipStream_t stream);

// denoise.hip: the SVGF stages of vkrt_denoise_diffuse.  Whole-frame W x H planes, rows tightly packed.
struct DenoiseParams
{
  uint32_t W, H;
  const float4* color;     // G-buffer planes (albedo in the three .w channels)
  const float4* position;
  const float4* normal;
  const float2* rough;     // roughness, metalness
  const float* viewZ;      // nrd->viewZ
  const float4* radHitD;   // nrd->diffRadianceHitDist (YCoCg)
  const float4* histColor; // colour history (rgb demodulated), read at the reprojected taps
  const float4* geomPrev;  // previous call's (position.xyz, oct normal); normal word 0x80008000 = no geometry
  float4* geomCur;
  const float4* momPrev;   // (m1, m2, history length, 0)
  float4* momCur;
  float4* rec;             // guide record (viewZ, dz/dx, dz/dy, oct normal)
  float4* colorOut;        // temporal result (rgb, 0)
  float4* colorVar;        // k_dn_variance output (rgb, variance)
  float* out;              // non-NULL: temporal stage only, remodulated rgb written here
  float curViewProj[16];
  float prevViewProj[16];
  int useHistory;
  int maxHistory;
  const float4* prevPosition;  // vkrt_denoise_diffuse_motion: where each pixel's surface point was at the previous call (.w == 0: nowhere);
                               // NULL = the plain call (k_dn_temporal; last member: the fields above keep their kernel-argument offsets)
};
struct DenoiseAtrous
{
  uint32_t W, H;
  int step;
  const float4* rec;
  const float4* in;        // (rgb, variance)
  float4* outBuf;
  float* out;              // non-NULL on the last iteration
  const float4* color;     // albedo for the remodulation of the last iteration
  const float4* position;
  const float4* normal;
  const float2* rough;
};
hipError_t vkrt_launch_denoise_temporal(const DenoiseParams& D, bool variance, hipStream_t stream);
hipError_t vkrt_launch_denoise_atrous(const DenoiseAtrous& A, hipStream_t stream);
