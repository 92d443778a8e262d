// device_scene.h -- HBM-resident scene + acceleration structure as the kernels see it.
//
// Flat geometry buffers are the reference's own (hello_vulkan.cpp:353-379, read by
// raytrace.rchit:41-66): SoA positions/normals/tangents/uv + u32 indices + PrimMeshInfo.
// The acceleration structure replaces VK_KHR_acceleration_structure (hello_vulkan.cpp:955-1047):
// all TLAS instances are flattened to ONE world-space BVH.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/vkrt_host_device.h"
#include "device_math.h"
#include "scene_records.h"  // DevInstance, DevMaterial, DevShadeMaterial, DevTexture: the records packed on the host

// BVH2 node, 64 bytes = 4 x float4 (one 64-B line, four dwordx4 loads):
//   q0 = (lo0.x, lo0.y, lo0.z, hi0.x)  q1 = (hi0.y, hi0.z, lo1.x, lo1.y)
//   q2 = (lo1.z, hi1.x, hi1.y, hi1.z)  q3 = (child0, child1, 0, 0) as int bits
// child >= 0: internal node index; child < 0: leaf, ~child = (firstTri << 3) | (count-1).
#define VKRT_NODE_QUADS 4
#define VKRT_LEAF_MAX 8
#define VKRT_TRAV_DONE ((int)0x80000000)
#define VKRT_SHARE_TRI_LEND 0x20u  // DevScene::shareFlags, set by vkrt_accel_build (the public option 8 holds bits 0-4)

// Triangle record, 48 bytes = 3 x float4, in leaf order:
//   a = (v0.x, v0.y, v0.z, e1.x)  b = (e1.y, e1.z, e2.x, e2.y)  c = (e2.z, gid, inst, prim) (ints as bits)
#define VKRT_TRI_QUADS 3

struct DevScene
{
  const float* positions;     // vec3[]
  const uint32_t* indices;
  const float4* vertexPN;     // VKRT_VERTEX_QUADS float4 per vertex (see above)
  const DevMaterial* materials;
  const DevShadeMaterial* shadeMaterials;  // the same materials as the path tracer's hit shader reads them
  const GltfLight* lights;
  const DevInstance* instances;
  const DevTexture* textures;
  const uint32_t* texMips;    // [textureCount][VKRT_MAX_MIPS]: first texel of every mip level (hello_vulkan.cpp:496 cmdGenerateMipmaps)
  const uint32_t* texels;     // RGBA8 pool (all levels)
  const uint4* texQuads;      // footprint pool of every texture's level 0, or NULL: record (x, y) = the texels (x, y) (x+1, y) (x, y+1) (x+1, y+1) with REPEAT
                              // wrap -- the 2x2 footprint of a bilinear tap as ONE 16-byte lane-load instead of four 4-byte ones (the hit shader is
                              // bound by the L1's lane-load rate, not by bytes: profiles/r04_experiments.md #115)
  const float* srgbLut;       // 512 floats: [0,256) sRGB decode of i/255, [256,512) i/255 (UNORM decode)
  const float4* nodes;
  const float4* tris;
  const uint4* triShade;      // per triangle slot: absolute vertex indices i0,i1,i2 and max(0, materialIndex)
  uint32_t textureCount;
  uint32_t triCount;
  int32_t rootRef;            // 0 (internal root) or a leaf ref for tiny scenes
  uint32_t stackCap;          // traversal stack: 4-byte LDS words per lane
  uint32_t layout;            // 0 = BVH2 (64-B nodes), 1 = wide8 (80-B compressed nodes)
  uint32_t stepLimit;         // traversal step bound (termination safety net)
  uint32_t triThreshold;      // wide8: lanes with pending triangles needed before a wave tests them (0 = test at once)
  uint32_t sharePeriodMask;   // work sharing is attempted on steps with (step & mask) == mask (0 = every step)
  uint32_t shareMinIdle;      // wide8, wavefront mode: idle lanes of a wave take over pending subtrees of busy lanes once this many are idle (0 = off)
  uint32_t gbufferMips;       // hybrid G-buffer: 1 = implicit-LOD texture() as in a fragment shader (trilinear + 4x anisotropy), 0 = LOD 0
  uint32_t shareFlags;        // bit 0: lanes whose stack is empty also donate the farthest pending child of their current group; bits 1, 2: order of
                              // any-hit walks (traverse.h); bit 4: lanes with nothing else to give donate half of their pending triangles
                              // VKRT_SHARE_TRI_LEND (internal, VKRT_OPT_WF_TRI_LEND): triangle steps lend pending triangles to free lanes
  uint32_t watertight;        // 1: triangle records hold (p0, p1, p2) and the kernels run the watertight test (VKRT_OPT_WATERTIGHT)
  float sceneLo[3], sceneHi[3];  // world-space bounds of the instanced geometry (conservative; read by the any-hit order heuristic only)
  uint32_t dissolve;          // 1: any-hit alpha / dissolve stage (VKRT_OPT_ANYHIT_DISSOLVE): bit 31 of a record's id word flags a non-opaque triangle
  uint32_t alphaTest;         // 1: alpha-test stage of the frame kernels (VKRT_OPT_ALPHA_TEST and a MASK material): set per call in the call's copy, 0 in
                              // the scene's own; sits in what was padding, so every other member keeps its kernel-argument offset
  unsigned long long* faults; // sticky tally of dropped stack pushes + step-limit exits (a walk that was cut short); must stay 0
};
static_assert(offsetof(DevScene, alphaTest) == 196 && offsetof(DevScene, faults) == 200 && sizeof(DevScene) == 208, "DevScene");
// The scene of a ray query with options (k_query, query.hip): the walks receive it as their DevScene and read the fields below only in
// the triangle modes with VKRT_TM_FILTER (traverse.h query_rejects), so every other walk compiles as it did.
struct DevQueryScene : DevScene
{
  const uint2* nodeMasks;  // wide8: per node, byte s = OR of the instance masks under child slot s (vkrt_launch_node_masks)
  uint32_t cullMask;       // 0..0xFF, launch-uniform
  uint32_t rayFlags;       // VKRT_RAY_CULL_BACK_FACING / VKRT_RAY_CULL_FRONT_FACING or 0
};
// The scene of vkrt_hit_surface (k_hit_surface, surface.hip): a hit record names (instance, primitive), not a tree slot, so the kernel
// resolves it as raytrace.rchit:34-50 does.  The table lives here, not in DevScene, whose layout every other kernel's arguments share.
struct DevSurfaceScene : DevScene
{
  const uint4* primMeshes;  // per primitive-mesh: (firstIndex, vertexOffset, indexCount / 3, max(0, materialIndex)); fixed at vkrt_scene_create
  uint32_t instanceCount;   // nodes of the scene: the bound of a record's instance
};

// a traversal could not keep a pending subtree (stack full) or ran into the step bound: the result may be wrong -> make it visible
#define VKRT_TRAV_FAULT(sc) atomicAdd((sc).faults, 1ull)

#ifndef VKRT_W8_MAX_POSTPONED
#define VKRT_W8_MAX_POSTPONED 8  // parked triangle groups per lane (traverse_wide.h, traverse_share.h), held in the free top end of its stack column
#endif
#ifndef VKRT_W8_POSTPONE_ROOM
#define VKRT_W8_POSTPONE_ROOM 0  // entries of the column reserved for them on top of the node stack's own depth (api_accel.cpp); groups parked beyond
                                 // these are tested out when a node push needs the slot (profiles/r04_experiments.md #117)
#endif

// Counter storage: 64 slots of 10 counters (padded to two 64-byte lines, order of vkrt_counters).  A workgroup
// adds its block-reduced totals to slot (blockIdx % 64), so same-address atomic serialisation is
// 64x lower than with one set of counters; vkrt_counters_read sums the slots.
#define VKRT_COUNTER_SLOTS 64
struct DevCounters
{
  unsigned long long v[VKRT_COUNTER_SLOTS][VKRT_COUNTER_STRIDE];
};

// TraceParams.flags: the public vkrt_trace_flags (include/vkrt.h) in the low bits + internal launch-uniform switches
#define VKRT_TRACE_PUBLIC_FLAGS 0xFu
#define VKRT_FLAG_SKIP_DEAD_SHADOW 0x100u  // VKRT_OPT_SKIP_DEAD_SHADOW_RAYS: a diffuse hit whose contribution is exactly zero emits no shadow ray
#define VKRT_FLAG_STORE_STAGED 0x200u      // frames in flight: `image` is the frame's staging plane; storePixel writes the pixel value unblended
#define VKRT_FLAG_SAMPLE_SYNC 0x400u       // VKRT_OPT_WF_SAMPLE_SYNC: all pixels of a frame trace sample s before any starts sample s + 1 (wavefront.hip)
#define VKRT_FLAG_CAMERA_ROUNDS 0x800u     // VKRT_OPT_WF_CAMERA_ROUNDS (with VKRT_FLAG_SAMPLE_SYNC): the first round of a sample traces and shades its camera
                                           // rays straight from the pixel grid, without path records (k_wf_traverse_camera, k_wf_shade_camera)

struct TraceParams
{
  DevScene sc;
  PushConstantRay pc;
  float viewInverse[16];
  float projInverse[16];
  uint32_t seed;
  uint32_t flags;
  uint32_t fullW, fullH;
  uint32_t stripRows, shardCount, shardIndex;
  uint32_t localRows;       // rows in this shard's buffer
  uint32_t tilesX, tileCount;
  uint32_t tileFirst;       // wavefront mode: first 8x8 tile of this launch's sub-frame (0 elsewhere)
  float* image;             // rgba32f, localRows x fullW
  unsigned int* workCounter;
  DevCounters* counters;
};

// Wavefront-mode working set (wavefront.hip): six record streams [parity][type] of SoA float4 planes + their counts, once per
// frame group (frames in flight), the staging plane of each group and the per-pixel sample state of each group.
struct WfBuffers
{
  unsigned* ctrl;       // stream counts [parity * 4 + type]; 64 words per lane
  float4* planes;       // [group][parity][17 planes: 8 shared by the C and S streams, 9 of the pair stream][capacity] (wavefront.hip plane())
  float4* stage;        // [group][capacity]: pixel values of a frame in flight, shard-local image layout (groups > 1 only)
  uint32_t capacity;    // paths (pixels of the shard, rounded up to whole 8x8 tiles)
  uint32_t groups;      // frame groups the allocation holds
  float4* sampleState;  // [group][capacity]: (hitValues.xyz, seed) of a pixel between two of its samples, tile-major pixel index of the
                        // shard (VKRT_FLAG_SAMPLE_SYNC; last member: the fields above keep their kernel-argument offsets)
};
