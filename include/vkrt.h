/*
 * vkrt.h -- C ABI of the MI355X-native ray-tracing path.
 *
 * This is the drop-in boundary for the path-tracing path of vk-raytracing-engine.
 * The reference has no plugin ABI; its ray-tracing path is entered through member
 * functions of `HelloVulkan` plus the data contract of shaders/host_device.h.  Each
 * entry point below names the reference interface it replaces (file:line relative to
 * the reference tree).  Plain pointers and sizes only; no C++ or torch types.
 *
 *   reference call (main.cpp)                      this ABI
 *   ---------------------------------------------  -------------------------------
 *   loadGltfScene()        hello_vulkan.cpp:327     vkrt_scene_create (flat arrays)
 *   createBottomLevelASGltf()  :1001                vkrt_accel_build
 *   createTopLevelAsGltf()     :1031                vkrt_accel_build (same call)
 *   updateUniformBuffer()      :61                  GlobalUniforms* argument
 *   pathtrace()                :1423                vkrt_pathtrace
 *   the frame loop at rest     main.cpp:503-508     vkrt_pathtrace_frames (n progressive frames per call)
 *   resetFrame()/updateFrame() :1501-1521           caller-owned PushConstantRay.frame
 *   destroyResources()         :518                 vkrt_scene_destroy
 *
 * Ownership: every input array is copied at vkrt_scene_create (the caller may free
 * it on return, like the reference's staging upload, hello_vulkan.cpp:353-357).  The
 * radiance image is caller-owned device memory (rgba32f, tightly packed rows); it is
 * read-modify-written when PushConstantRay.frame > 0 (raytrace.rgen:136-141).
 * Errors: int return codes, 0 = VKRT_OK; text via vkrt_last_error(); nothing throws
 * across the ABI.  Threading: one host thread per scene handle at a time; work is
 * enqueued on the caller's HIP stream (hipStream_t passed as void*; NULL = default).
 * The library never falls back to a CPU path: without a HIP device every compute
 * entry point returns VKRT_ERR_NO_DEVICE.
 */
#ifndef VKRT_H
#define VKRT_H

#include <stdint.h>
#include "vkrt_host_device.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VKRT_ABI_VERSION 4 /* 4: vkrt_reserve_frames; vkrt_counters.pair_records, vkrt_trace_timing.shade_ms / shade_launches (appended).
                              2: vkrt_scene_set_option / vkrt_reserve, vkrt_counters.traversal_faults.
                              3: vkrt_pathtrace_frames, VKRT_TRACE_SAME_SEED_EVERY_FRAME, options 10-14, vkrt_accel_info.reference_count,
                                 vkrt_accel_check.triangles_uncovered, VKRT_INFO_ANYHIT_ORDER (the options and the query
                                 that round 3 had added under version 2 are part of 3: a client that needs them asks for >= 3) */

enum vkrt_status {
  VKRT_OK = 0,
  VKRT_ERR_INVALID_ARGUMENT = 1,
  VKRT_ERR_NO_DEVICE = 2,
  VKRT_ERR_HIP = 3,
  VKRT_ERR_OUT_OF_MEMORY = 4,
  VKRT_ERR_NOT_BUILT = 5,     /* vkrt_pathtrace before vkrt_accel_build */
  VKRT_ERR_UNSUPPORTED = 6
};

typedef struct vkrt_scene vkrt_scene; /* opaque; one per GPU */

/* One glTF primitive-mesh, as nvh::GltfPrimMesh is consumed by the reference
 * (hello_vulkan.cpp:363-368 for the shader lookup, :955-987 for the BLAS ranges:
 * primitiveCount = indexCount/3, firstVertex = vertexOffset, maxVertex = vertexCount). */
typedef struct vkrt_prim_mesh {
  uint32_t firstIndex;    /* into indices[] */
  uint32_t indexCount;    /* multiple of 3 */
  uint32_t vertexOffset;  /* added to every index value */
  uint32_t vertexCount;
  int32_t  materialIndex; /* may be -1; the shader clamps with max(0, .) (raytrace.rchit:38) */
} vkrt_prim_mesh;

/* One drawable node = one TLAS instance (hello_vulkan.cpp:1035-1043):
 * transform = worldMatrix, instanceCustomIndex = primMesh, mask 0xFF, cull disabled (the initial visibility of every node;
 * vkrt_scene_set_instance_visibility changes mask and flags for the ray-query entry points). */
typedef struct vkrt_node {
  float   worldMatrix[16]; /* column-major object->world */
  int32_t primMesh;
} vkrt_node;

/* One sampled image: 8-bit RGBA, row-major, top row first (what tinygltf/stb hand the
 * reference, hello_vulkan.cpp:482-499).  is_srgb follows getImageFormat
 * (hello_vulkan.cpp:417-443).  Sampler (:448-454 and SURVEY Appendix A 27-29): linear, REPEAT;
 * the ray tracing stages read LOD 0 (no derivatives there), the hybrid mode's G-buffer pass samples
 * like the fragment shader it stands for -- implicit LOD over the mip chain the library generates at
 * vkrt_scene_create (:499), anisotropy 4.  textures[i] here is glTF texture i (already resolved to
 * its source image, :505-509). */
typedef struct vkrt_texture {
  uint32_t       width;
  uint32_t       height;
  const uint8_t* rgba8;
  int32_t        is_srgb;
} vkrt_texture;

/* Flat scene arrays exactly as the reference uploads them (hello_vulkan.cpp:353-379):
 * SoA vertex attributes shared by all primitive-meshes, one u32 index buffer. */
typedef struct vkrt_scene_desc {
  uint32_t struct_size;        /* = sizeof(vkrt_scene_desc), ABI check */
  uint32_t vertex_count;
  const float*    positions;   /* vec3[vertex_count]  (m_gltfScene.m_positions)  */
  const float*    normals;     /* vec3[vertex_count]  (m_normals)                */
  const float*    tangents;    /* vec4[vertex_count]  (m_tangents, w=handedness) */
  const float*    texcoords0;  /* vec2[vertex_count]  (m_texcoords0)             */
  const uint32_t* indices;     /* u32[index_count]    (m_indices)                */
  uint32_t index_count;
  uint32_t prim_mesh_count;
  const vkrt_prim_mesh*  prim_meshes;
  const GltfPBRMaterial* materials;
  uint32_t material_count;
  uint32_t light_count;
  const GltfLight*       lights;
  const vkrt_node*       nodes;
  uint32_t node_count;
  uint32_t texture_count;      /* 0 => a 1x1 white dummy is bound (hello_vulkan.cpp:468-472) */
  const vkrt_texture*    textures;
} vkrt_scene_desc;

/* Acceleration-structure build selection (replaces
 * VK_BUILD_ACCELERATION_STRUCTURE_PREFER_FAST_TRACE_BIT_KHR, hello_vulkan.cpp:1010,1046). */
enum vkrt_build_flags {
  VKRT_BUILD_LBVH_GPU = 0x1,  /* Morton-code radix tree built by HIP kernels on the device (fastest build)  */
  VKRT_BUILD_SAH_HOST = 0x2,  /* binned-SAH BVH built by the C++ host, then uploaded (best tree, ~15x the build time)  */
  VKRT_BUILD_PLOC_GPU = 0x4,  /* device build for trace speed: locally-ordered clustering over the Morton order (ploc.hip), upper
                                 levels re-built with a full-sweep SAH over the clustered subtrees (lbvh.hip)  */
  VKRT_BUILD_DEFAULT  = 0x4   /* the reference builds on the device with PREFER_FAST_TRACE: so does the default  */
};

/* Image-space sharding (replaces the single vkCmdTraceRaysKHR(W,H,1) grid,
 * hello_vulkan.cpp:1446).  The full launch size stays gl_LaunchSizeEXT for every
 * shard so seeds and camera rays depend on global pixel coordinates only.
 * Rows are dealt in strips: strip s = rows [s*strip_rows, (s+1)*strip_rows) belongs to
 * shard (s % shard_count).  The shard's output buffer holds its strips stacked in
 * increasing s, full_width pixels per row.  strip_rows = 0 means "the whole image". */
typedef struct vkrt_shard {
  uint32_t full_width;
  uint32_t full_height;
  uint32_t strip_rows;
  uint32_t shard_count;
  uint32_t shard_index;
} vkrt_shard;

enum vkrt_trace_flags {
  /* Default reproduces raytrace.rgen:27: seed index = y*x + x.  This flag selects the
   * collision-free y*full_width + x instead (not parity). */
  VKRT_TRACE_SEED_INDEX_ROW_MAJOR = 0x1,
  /* Instrumented launch (slower): also count BVH nodes visited / triangles tested / wavefront steps and, in the default
   * wavefront pipeline, the hit / diffuse-lobe / texture-tap tallies of the shading stage.  Rays and pixels are always counted. */
  VKRT_TRACE_COUNT_TRAVERSAL = 0x2,
  /* Record HIP events around every traversal-kernel launch of the frame (vkrt_last_trace_timing). */
  VKRT_TRACE_TIME_KERNELS = 0x4,
  /* vkrt_pathtrace_frames: every frame of the call uses opts->seed instead of opts->seed + i (a host that does not advance its seed) */
  VKRT_TRACE_SAME_SEED_EVERY_FRAME = 0x8
};

typedef struct vkrt_trace_opts {
  uint32_t seed;   /* replaces int(clockARB()) in raytrace.rgen:27 */
  uint32_t flags;  /* vkrt_trace_flags */
} vkrt_trace_opts;

/* Totals accumulated by device atomics since the last vkrt_counters_reset. */
typedef struct vkrt_counters {
  uint64_t rays_closest;   /* traceRayEXT calls of raytrace.rgen:64-75          */
  uint64_t rays_shadow;    /* traceRayEXT calls of raytrace.rgen:85-97          */
  uint64_t hits;           /* raytrace.rchit invocations                 (wavefront pipeline: with COUNT_TRAVERSAL) */
  uint64_t diffuse_hits;   /* rchit invocations that took the diffuse lobe           (same)                    */
  uint64_t tex_taps;       /* texture() calls                                         (same)                    */
  uint64_t pixels;         /* rgen invocations                                  */
  uint64_t nodes_visited;  /* only with VKRT_TRACE_COUNT_TRAVERSAL              */
  uint64_t tris_tested;    /* only with VKRT_TRACE_COUNT_TRAVERSAL              */
  uint64_t wave_node_steps; /* COUNT_TRAVERSAL, wide8 layout: node steps per wavefront (one per 64 lanes);
                              nodes_visited / (64 * wave_node_steps) = lane efficiency of the node phase */
  uint64_t wave_tri_steps;  /* same for the triangle phase                        */
  uint64_t traversal_faults; /* always counted: stack pushes dropped (stack sized from the builder's depth) + walks cut by the step
                               bound.  Non-zero means a builder / traversal mismatch and possibly wrong pixels; tests assert 0. */
  uint64_t pair_records;   /* ABI 4, wavefront pipeline: path records that carried TWO rays through a round (the shadow ray of a segment and
                              the closest-hit ray of the next one): records moved = rays_closest + rays_shadow - pair_records */
} vkrt_counters;

typedef struct vkrt_accel_info {
  uint32_t triangle_count;   /* instanced (flattened) triangles */
  uint32_t node_count;       /* BVH nodes in the traversal layout */
  uint32_t max_depth;
  uint32_t build_flags;      /* which builder produced it */
  float    sah_cost;         /* SAH cost of the tree in its traversal layout, traversal 1 / intersect 1, every builder and the refit alike:
                                [sum over nodes of A(node) + sum over leaf children of A(child) x triangle count] / A(root), where A is
                                the surface area of the float (unquantised) box -- a wide8 child's or a BVH2 child's box, a node's box =
                                the union of its children's -- and the sums run over the nodes a walk from the root reaches.  A BVH2
                                whose root is a leaf costs its triangle count; otherwise a root box of zero area costs 0. */
  float    build_ms;         /* wall time of the last build */
  uint64_t node_bytes;
  uint64_t triangle_bytes;
  uint32_t reference_count;  /* triangle slots of the tree = leaves' references; > triangle_count when VKRT_OPT_SPLIT_BUDGET split triangles */
  uint32_t reserved;
} vkrt_accel_info;

/* ---- library ---------------------------------------------------------------------- */
int         vkrt_abi_version(void);
const char* vkrt_last_error(void);       /* thread-local, never NULL */
int         vkrt_device_count(void);     /* 0 without a HIP device */

/* ---- scene (replaces loadGltfScene's uploads, hello_vulkan.cpp:353-381) ----------- */
int  vkrt_scene_create(const vkrt_scene_desc* desc, int device, vkrt_scene** out);
void vkrt_scene_destroy(vkrt_scene* scene);

/* ---- per-scene execution options ------------------------------------------------------
 * Scheduling knobs of the HIP path; none of them changes a pixel (tests/test_gpu_parity.py hashes every
 * combination).  They are fields of the scene handle, not process globals.  Their INITIAL values are read once, at
 * vkrt_scene_create, from the environment variables named below -- process-wide test hooks kept for A/B runs of
 * unmodified binaries (bench.py, vkrt_render); vkrt_scene_set_option overrides them per handle.
 * Options marked [build] are consumed by the next vkrt_accel_build, the others by the next vkrt_pathtrace. */
enum vkrt_option {
  VKRT_OPT_MODE            = 1, /* 1 = wavefront pipeline (default), 0 = one persistent megakernel (BVH2 only) [build]; env VKRT_MODE=mega */
  VKRT_OPT_BVH_LAYOUT      = 2, /* 1 = 8-wide compressed nodes (default with the wavefront pipeline), 0 = BVH2 [build]; env VKRT_BVH=bvh2 */
  VKRT_OPT_WF_SUBFRAMES    = 3, /* independent sub-frames of a launch on internal streams, 1..8 (default 3); env VKRT_WF_SUBFRAMES */
  VKRT_OPT_WF_TRAV_BLOCK   = 4, /* threads per traversal workgroup: 64 (default), 128, 256; env VKRT_WF_TRAV_BLOCK */
  VKRT_OPT_WF_SHARE        = 5, /* idle lanes of a traversal wave needed before they adopt subtrees, 0 = off (default 16) [build]; env VKRT_WF_SHARE */
  VKRT_OPT_TRI_THRESHOLD   = 6, /* lanes with pending triangles, per 64 lanes still walking, before a wave tests them; 1 = every step, 0 = test at once,
                                   no parking (default 32) [build]; env VKRT_TRI_THRESHOLD */
  VKRT_OPT_WF_SHARE_PERIOD = 7, /* sharing attempted on steps with (step & mask) == mask (default 0 = every step) [build]; env VKRT_WF_SHARE_PERIOD */
  VKRT_OPT_WF_SHARE_FLAGS  = 8, /* bit 0: lanes with an empty stack also donate a pending child of their current group.  Bits 1-3: child order of
                                   any-hit (shadow / AO) walks -- "is anything in the way" has the same answer in any order, so this is a cost
                                   heuristic only: bit 1 = always the FARTHEST pending child first; bit 2 = farthest first for rays that end outside
                                   the bounds of the scene (a shadow ray towards a light outside the building is stopped by the building's shell,
                                   the last thing a front-to-back walk reaches), front to back otherwise; bit 3 = automatic: like bit 2 unless the
                                   scene has room-sized triangles, which a front-to-back walk meets at once.  Bit 4 (round 4): lanes that have no node
                                   work to give but hold two or more pending triangles (a ray grazing a plane of thin strips leaves a node test
                                   with up to 24) give half of them to an idle lane.  Default 25 = bits 0, 3 and 4 [build];
                                   env VKRT_WF_SHARE_FLAGS */
  VKRT_OPT_GBUFFER_MIPS    = 9, /* NOT a scheduling knob: 1 (default) = vkrt_gbuffer_raycast samples textures like the fragment shader it replaces
                                   (implicit LOD over the mip chain, anisotropy 4; hello_vulkan.cpp:448-454, :499), 0 = LOD 0; env VKRT_GBUFFER_MIPS */
  VKRT_OPT_WATERTIGHT      = 10, /* NOT a scheduling knob [build]: 0 (default) = Moeller-Trumbore on pre-subtracted (v0, e1, e2) records in binary32
                                   (what BASELINE.json's north star names); 1 = the watertight ray/triangle test of Woop, Benthin, Wald 2013 on the exact
                                   vertices (p0, p1, p2): edge functions in ray space with a double-precision fallback on exact zeros, so a ray through a
                                   shared edge or vertex hits one of the triangles -- what the Vulkan specification demands of traceRayEXT
                                   (raytrace.rgen:64-75).  Hits differ from the default in the last bits of (t, u, v), and in the rare pixels where the
                                   default leaks through an edge; the oracle implements both (orc_set_watertight).  env VKRT_WATERTIGHT */
  VKRT_OPT_SKIP_DEAD_SHADOW_RAYS = 11, /* 0 (default) = every diffuse hit traces its shadow ray, as raytrace.rgen:79-97 does; 1 = a diffuse hit whose
                                   contribution min(prd.hitValue * curWeight, 10) is exactly zero (light behind the surface, no emission) traces none:
                                   raytrace.rgen:99-102 adds that zero whether or not the ray is occluded, so every pixel is bit-identical, only
                                   vkrt_counters.rays_shadow drops.  Path-tracing mode of the wavefront pipeline only.  env VKRT_SKIP_DEAD_SHADOW_RAYS */
  VKRT_OPT_ANYHIT_DISSOLVE = 12, /* [build] the any-hit alpha / dissolve stage of raytrace_rahit_todo.glsl:23-37 (hello_vulkan.cpp:1185-1191 keeps its
                                   registration commented out; every ray of the reference is gl_RayFlagsOpaqueEXT): 0 (default) = all geometry opaque,
                                   as the reference runs; 1 = a candidate hit on a triangle whose material has dissolve < 1 is ignored when dissolve == 0
                                   and otherwise with probability 1 - dissolve, for closest-hit and shadow rays of both modes (not for the ray-cast
                                   G-buffer: a raster pass has no any-hit stage).  The shader is written against the dead OBJ pipeline's WaveFrontMaterial;
                                   on the glTF material the live pipeline has, dissolve = pbrBaseColorFactor.a and "illum == 4" = dissolve < 1.  The GLSL
                                   draws rnd(prd.seed) per invocation, but Vulkan defines neither the order nor the number of any-hit invocations, so the
                                   decision here is a pure function of the ray and the triangle: rnd(tea(triangle id, prd.seed when the ray is traced)) >
                                   dissolve; prd.seed itself is not advanced.  The result stays a property of the triangle set (any tree, any schedule);
                                   the oracle implements the same rule (orc_set_dissolve).  env VKRT_ANYHIT_DISSOLVE */
  VKRT_OPT_WF_FRAMES_IN_FLIGHT = 13, /* vkrt_pathtrace_frames: consecutive frames of a call rendered at the same time, 1..8 (default 3), each on
                                   record streams of its own (544 B per pixel and frame in flight); their pixel values meet in the ordered blend at
                                   the end of a frame, so the image is bit-identical for every value.  A call with frames in flight does not split
                                   its frames into sub-frames (option 3): few, large launches overlap best.  env VKRT_WF_FRAMES_IN_FLIGHT */
  VKRT_OPT_SPLIT_BUDGET    = 14, /* [build] NOT a pixel-changing knob: triangle pre-splitting in the device builders (VKRT_BUILD_PLOC_GPU /
                                   VKRT_BUILD_LBVH_GPU), the part of PREFER_FAST_TRACE (hello_vulkan.cpp:1010, :1046) that matters on artist-made
                                   geometry.  Value = budget of EXTRA triangle references in percent of the triangle count, 0..100 (0 = off), or -1 = automatic (the default since ABI 4): triangles
                                   that are large against the scene grid enter the tree as several references, each with the box of one piece of
                                   the triangle.  Only references multiply (a copy of the 48-byte record per reference): the hit test, the triangle id
                                   of the tie rule and every pixel are unchanged.  vkrt_accel_info.reference_count reports the result.
                                   WHEN TO SET IT (measured, profiles/r05_split_rotated.jsonl): 10-30 for scenes whose large triangles are
                                   not aligned with the coordinate axes -- a building rotated 45 degrees about y traces +14 % faster, one
                                   rotated 35 / 20 degrees about y / x +97 % (the box of a room-sized diagonal triangle is mostly empty:
                                   61 -> 30 triangles tested per ray); 0 for axis-aligned architecture and for finely tessellated meshes,
                                   where the extra references cost 1-8 %.  -1 (ABI 4) = automatic: the device builders build with a 30 %
                                   budget and without, and keep the split tree only when its SAH cost is below 0.9 of the unsplit one
                                   (rotated buildings: 0.70-0.82; axis-aligned and finely tessellated scenes: 0.95-1.08) -- two or three
                                   builds of ~13 ms instead of one; VKRT_INFO_SPLIT_BUDGET reports the outcome.  env VKRT_SPLIT_BUDGET */
  VKRT_OPT_LAST            = 14,
  VKRT_OPT_WF_SAMPLE_SYNC  = 15, /* (appended within ABI 4; VKRT_OPT_LAST keeps naming the last option every ABI-4 library has)  1 (default) = the wavefront
                                   path tracer keeps all pixels of a frame on the same sample: a path whose sample ends waits, 16 B of state per
                                   pixel and frame in flight, until a kernel of its own starts the next sample of every pixel in 8x8-tile order,
                                   so camera rays are traced and their hits shaded as whole tiles; 0 = a pixel starts its next sample in the
                                   round its sample ends.  Same paths, draws and float operations: no pixel and no counter changes; a timed
                                   call's shade_ms includes the sample starts.  env VKRT_WF_SAMPLE_SYNC */
  VKRT_OPT_WF_CAMERA_ROUNDS = 16, /* (appended within ABI 4 like option 15)  1 (default) = in the schedule of option 15 the first round of every sample
                                   traces and shades its camera rays straight from the pixel grid: one wave per 8x8 tile makes the rays from the
                                   16-B sample state, and the shade step makes the same state again, so the frame has no init kernels and the camera
                                   rays no path records (96 instead of 256 B moved per pixel and sample in that round); 0 = init kernels write a
                                   record per camera ray.  Takes effect in path-tracing mode with option 15 = 1, the wide8 layout, 64-thread traversal
                                   workgroups and work sharing on; anywhere else it resolves to 0 silently.  Same paths, draws and float operations: no
                                   pixel and no counter changes.  env VKRT_WF_CAMERA_ROUNDS */
  VKRT_OPT_WF_TRI_LEND = 17, /* (appended within ABI 4 like options 15 and 16)  1 (default) = in a triangle step of the sharing traversal wave (wide8
                                   layout, work sharing on) a lane with two or more pending triangles lends its last one to a walking lane that
                                   holds none; the borrower tests it in the same step with the lender's ray and publishes to that ray's result.
                                   Lanes of the wave that have no work walk along to borrow.  0 = every lane tests its own triangles, one per step.  Closest hit is the minimum over (t, triangle id)
                                   and any-hit is "exists", whoever runs a test: no pixel, hit record or ray counter changes; tris_tested per
                                   wave_tri_steps rises, nodes_visited may move with the bound.  Read at vkrt_accel_build, and taken over at once when set on a
                                   built scene; not built for option 10 and option 12 together, where it resolves to 0 silently.  env VKRT_WF_TRI_LEND */
  VKRT_OPT_ALPHA_TEST = 18, /* (appended within ABI 4 like options 15 to 17)  NOT a scheduling knob: 0 (default) = the frame entry points treat every
                                   material as opaque, as the reference does; 1 = vkrt_pathtrace*, vkrt_gbuffer_raycast* and vkrt_hybrid_trace* run
                                   the alpha test of VKRT_ALPHA_MASK materials ("alpha-tested materials" below) on every ray they trace: camera,
                                   bounce, shadow, AO and GI rays and the G-buffer's primary ray, which passes where a raster pass would discard
                                   the fragment.  Read by each frame call, not by the builders: it survives builds and refits, and the stage is
                                   active in a call when the option is 1 and some material is MASK at that moment; otherwise the call launches
                                   the kernels it launched before.  While active, a wavefront-mode scene with VKRT_OPT_WF_TRAV_BLOCK other than
                                   64 gets VKRT_ERR_UNSUPPORTED from the frame call, which enqueues nothing.  Options 15 to 17 keep their
                                   effect (17 resolves to 0 with option 12, as with options 10 + 12).  env VKRT_ALPHA_TEST */
  VKRT_INFO_ANYHIT_ORDER   = 100, /* read-only (vkrt_scene_get_option; set is refused): the child-order bits (2 | 4) that the last vkrt_accel_build
                                   resolved VKRT_OPT_WF_SHARE_FLAGS to, i.e. what bit 3 ("automatic") decided for this scene; 0 before a build */
  VKRT_INFO_SPLIT_BUDGET   = 101  /* read-only (ABI 4): the pre-splitting budget the last vkrt_accel_build used -- what VKRT_OPT_SPLIT_BUDGET = -1
                                   ("automatic") resolved to: 30 or 0 */
};
int vkrt_scene_set_option(vkrt_scene* scene, int option, int value);
int vkrt_scene_get_option(const vkrt_scene* scene, int option, int* value);

/* ---- acceleration structure (replaces createBottomLevelASGltf :1001-1011 and
 *      createTopLevelAsGltf :1031-1047) ------------------------------------------- */
int vkrt_accel_build(vkrt_scene* scene, uint32_t build_flags, void* hip_stream);
/* After a vkrt_accel_refit: sah_cost is the refitted tree's (same formula as the builders'; reading it synchronises the device), the
 * number a caller weighs to decide when a full rebuild pays; build_ms stays that of the build. */
int vkrt_accel_get_info(const vkrt_scene* scene, vkrt_accel_info* out);

/* ---- moving instances (replaces the update path of the TLAS build: VK_BUILD_ACCELERATION_STRUCTURE_ALLOW_UPDATE_BIT_KHR at
 *      createTopLevelAsGltf :1031-1047, then vkCmdBuildAccelerationStructuresKHR with VK_BUILD_ACCELERATION_STRUCTURE_MODE_UPDATE_KHR).
 *      Rigid motion of whole instances here, vertex deformation below (vkrt_scene_update_vertices); no topology change.  These entry
 *      points came after ABI version 4 without changing it or any struct: detect them by symbol. -------------------------------- */
/* Replace the transforms of nodes [first, first+count) (vkrt_node as at vkrt_scene_create; primMesh must equal the node's
 * existing primMesh).  Enqueued on hip_stream; the array is copied before return.  After this call the scene's tree is stale:
 * trace / G-buffer / hybrid entry points (and the vkrt_debug_* tree hooks) return VKRT_ERR_NOT_BUILT until vkrt_accel_refit or
 * vkrt_accel_build.  Same rules as vkrt_scene_create: a non-finite matrix, a range outside the scene's nodes, a changed primMesh or a
 * NULL scene give VKRT_ERR_INVALID_ARGUMENT and change nothing; what vkrt_scene_create accepts (a zero scale that hides an
 * instance, a mirroring matrix) is accepted.  A later vkrt_accel_build builds the moved scene. */
int vkrt_scene_update_nodes(vkrt_scene* scene, uint32_t first, uint32_t count, const vkrt_node* nodes, void* hip_stream);
/* Refit the built tree to the scene's current node transforms and vertices: same topology, same slots, new boxes and triangle records.
 * Enqueued on hip_stream.  No host synchronisation and no allocation, except on the first refit of a build.  Everything the build
 * decided stays (layout, record format, split references, any-hit order, traversal stack); options changed since the build take effect
 * at the next vkrt_accel_build.  The image stays a property of the triangle set: a refitted tree traces exactly the pixels and ray
 * counts of a fresh build of the moved scene; only its speed depends on how far the instances moved (vkrt_accel_info.sah_cost).
 * VKRT_ERR_NOT_BUILT before any vkrt_accel_build. */
int vkrt_accel_refit(vkrt_scene* scene, void* hip_stream);

/* ---- deforming meshes (replaces the update path of the BLAS build: VK_BUILD_ACCELERATION_STRUCTURE_ALLOW_UPDATE_BIT_KHR at
 *      createBottomLevelASGltf :1001-1011, then vkCmdBuildAccelerationStructuresKHR with VK_BUILD_ACCELERATION_STRUCTURE_MODE_UPDATE_KHR
 *      on a new vertex buffer -- a skinned character, a cloth, a simulated surface).  This entry point came after ABI version 4 without
 *      changing it or any existing struct: detect it by symbol. ----------------------------------------------------------------------
 * New attributes for vertices [first, first+count) of the scene's shared vertex arrays (vkrt_scene_desc: an absolute vertex index, i.e.
 * a primitive-mesh's vertexOffset already added).  Each of the four arrays is laid out as at vkrt_scene_create with element 0 = vertex
 * `first`; a NULL array keeps that attribute of every vertex as it is.  Deformation only: index buffers, primitive-meshes, nodes and
 * materials are untouched, so a mesh that several nodes instance deforms in all of them.
 * Ordering: enqueued on hip_stream (NULL = default stream) like vkrt_scene_update_nodes -- after what was enqueued there before (a trace
 * that still reads the old vertices), before what comes after (the refit, the next trace).
 * VKRT_MEMORY_DEVICE: the arrays are device memory on the scene's device (what the caller's skinning or simulation kernel has just
 *   written on that stream), float-aligned.  The call neither allocates nor synchronises with the host and returns after the enqueue;
 *   the arrays must stay valid until the stream has passed the call.  The values are not inspected: a non-finite position is the
 *   caller's error.  It cannot make any kernel read or write out of bounds (indices do not change), and a later correct update + refit
 *   repairs the scene completely; what rays return in between is unspecified.
 * VKRT_MEMORY_HOST: the arrays may be freed or reused on return, as at vkrt_scene_create.  Positions are checked as there (finite)
 *   before anything changes.  The arrays are staged through a device buffer the scene owns -- allocated (hipMalloc) by the first host
 *   update and again by one larger than every earlier one, released by vkrt_scene_destroy -- and the call waits for hip_stream before
 *   it returns.  A caller that must not wait uses VKRT_MEMORY_DEVICE.
 * Stale tree: with positions given and a built tree, the tree is stale exactly as after vkrt_scene_update_nodes -- trace, G-buffer,
 *   hybrid, ray-query and vkrt_debug_* tree hooks return VKRT_ERR_NOT_BUILT until vkrt_accel_refit or vkrt_accel_build; one refit serves
 *   any number of vertex and node updates before it.  An update of normals, tangents or texture coordinates alone does not make the
 *   tree stale: the next trace shades with them.
 * vkrt_accel_refit after it: same topology, slots, split references, node-mask table and dissolve flags; new records and boxes;
 *   vkrt_accel_info.sah_cost is the deformed tree's.  The refitted tree gives bit for bit the pixels, ray counts and hits of a fresh
 *   scene created from the deformed arrays and built with the same options.  The scene bounds and the large-triangle flag of the
 *   any-hit order heuristic stay as built (they cannot change a pixel).
 * vkrt_accel_build after it builds the deformed scene with every builder.  The library keeps a host copy of the positions for the host
 *   builder and the scene bounds: a host update keeps it current, and after a device update the next vkrt_accel_build downloads the
 *   positions first (a build synchronises anyway).
 * Refused with VKRT_ERR_INVALID_ARGUMENT, changing nothing, in this order: a NULL update; struct_size < sizeof(vkrt_vertex_update); a
 * memory value that is neither of the two; a NULL scene; a range outside the scene's vertices; (host memory) a non-finite position.
 * Then count == 0 or all four arrays NULL: VKRT_OK, nothing is enqueued, the tree does not become stale.  Then, without a device:
 * VKRT_ERR_NO_DEVICE. */
enum vkrt_memory { VKRT_MEMORY_HOST = 0, VKRT_MEMORY_DEVICE = 1 };
typedef struct vkrt_vertex_update {
  uint32_t struct_size;     /* sizeof(vkrt_vertex_update) */
  uint32_t first, count;    /* vertices [first, first+count) */
  uint32_t memory;          /* vkrt_memory: where the four arrays below live */
  const float* positions;   /* vec3[count] or NULL = keep */
  const float* normals;     /* vec3[count] or NULL = keep */
  const float* tangents;    /* vec4[count] or NULL = keep */
  const float* texcoords0;  /* vec2[count] or NULL = keep */
} vkrt_vertex_update;
int vkrt_scene_update_vertices(vkrt_scene* scene, const vkrt_vertex_update* update, void* hip_stream);

/* ---- moving instances from device memory (the instance buffer of a TLAS update that a compute pass has just written: a rigid-body
 *      simulation, a particle or crowd system, a learned policy driving thousands of instances).  With it a frame of a moving scene --
 *      vkrt_scene_motion_mark, update, vkrt_accel_refit, trace -- has no host round trip left.  These entry points came after ABI
 *      version 4 without changing it or any existing struct: detect them by symbol. ---------------------------------------------------
 * New transforms for count nodes: the dense form (node_indices == NULL) moves nodes [first, first+count), entry k being node first + k;
 * the sparse form moves node node_indices[k] with entry k, and first must be 0.  world_matrices holds 16 floats per entry, column-major
 * object->world like vkrt_node.worldMatrix; only rows 0..2 are read (elements 3, 7, 11 and 15 of an entry are ignored).
 * Scope: the call changes transforms only.  Every node keeps its primMesh, its visibility (vkrt_scene_set_instance_visibility), its
 *   dissolve flag and its slot.  Stream ordering and the stale tree are those of vkrt_scene_update_nodes: enqueued on hip_stream
 *   (NULL = default stream) after what was enqueued there before and before what comes after; with a built tree, trace, G-buffer,
 *   hybrid, ray-query and vkrt_debug_* tree hooks return VKRT_ERR_NOT_BUILT until vkrt_accel_refit or vkrt_accel_build.  One
 *   vkrt_accel_refit serves any number of node, vertex, skin and morph updates before it.  vkrt_hit_surface and vkrt_hit_motion read
 *   the live records and see the new transforms without a refit; the motion snapshot (vkrt_scene_motion_mark) is untouched.
 * The record (96 B per node, what vkrt_debug_read_instances returns) is the one vkrt_scene_create and vkrt_scene_update_nodes write:
 *   o2w[4 r + c] = M[4 c + r]; w2o = the cofactor inverse of o2w's 3x3 in binary64, in a fixed operation order with inv = 1.0 / det,
 *   each entry rounded to binary32; the mirrored bit of the visibility word = (binary64 determinant < 0).  One set of functions makes it
 *   on the host and on the device: a device update is bit for bit a host update of the same matrices, a singular one (a zero scale:
 *   infinities and NaNs in w2o) included.  One corner is open: an inverse entry so small that its binary32 value is subnormal (matrix
 *   entries near 1e38) may differ between the two.
 * VKRT_MEMORY_DEVICE: the arrays are device memory on the scene's device, world_matrices 16-byte and node_indices 4-byte aligned, valid
 *   until the stream has passed the call.  The call is one kernel launch on hip_stream: nothing is allocated, nothing synchronises,
 *   and the values are not inspected.  A non-finite or singular matrix is the caller's matter, exactly as a non-finite position of a
 *   device vertex update: it cannot make any kernel read or write out of bounds, and a later correct update + refit repairs the scene
 *   completely; what rays return in between is unspecified.  An index >= node_count skips its entry.  With duplicate indices, which
 *   entry wins is unspecified.  The library's host copy of the matrices falls behind the device: vkrt_accel_build (every builder and
 *   the scene bounds read that copy) and vkrt_debug_split_references download the records first -- they synchronise anyway -- and
 *   refuse a scene that holds a non-finite matrix with VKRT_ERR_INVALID_ARGUMENT, building nothing.  A host vkrt_scene_update_nodes
 *   in between is fine: it still checks primMesh, which no device update changes.
 * VKRT_MEMORY_HOST: the contract of vkrt_scene_update_nodes, for the sparse form too.  Every matrix element is checked finite and
 *   every index < node_count before anything changes; the arrays are copied before return; the records travel as kernel arguments,
 *   so nothing is staged and the call does not wait for the stream (unlike a host vertex update); the host copy follows.  Duplicate
 *   indices are applied in order: the last entry wins.
 * Refused with VKRT_ERR_INVALID_ARGUMENT, changing nothing, in this order: a NULL update; struct_size < sizeof(vkrt_node_update); a
 * memory value that is neither of the two; first != 0 together with node_indices; a NULL scene; a dense range outside the scene's
 * nodes; (count > 0) NULL world_matrices; (device memory) a misaligned array; (host memory) an index out of range; (host memory) a
 * non-finite element.  Then count == 0: VKRT_OK, nothing is enqueued, the tree does not become stale.  Then, without a device:
 * VKRT_ERR_NO_DEVICE. */
typedef struct vkrt_node_update {
  uint32_t struct_size;           /* sizeof(vkrt_node_update) */
  uint32_t first, count;          /* node_indices == NULL: nodes [first, first+count); else count entries and first must be 0 */
  uint32_t memory;                /* vkrt_memory: where the two arrays live */
  const float*    world_matrices; /* [count][16], column-major object->world like vkrt_node.worldMatrix; only rows 0..2 are read */
  const uint32_t* node_indices;   /* NULL, or [count]: entry k moves node node_indices[k] (sparse update) */
} vkrt_node_update;
int vkrt_scene_update_node_transforms(vkrt_scene* scene, const vkrt_node_update* update, void* hip_stream);

/* ---- skinned meshes (glTF skins: JOINTS_0 / WEIGHTS_0 per vertex, a palette of joint matrices per frame): linear-blend skinning inside
 *      the library, straight into the scene's live vertex arrays.  These entry points came after ABI version 4 without changing it or
 *      any existing struct: detect them by symbol. ------------------------------------------------------------------------------------
 * vkrt_scene_add_skin binds four influences per vertex to the range [first, first+count) (absolute vertex indices, as in
 * vkrt_vertex_update) and captures the range's bind pose: positions, normals and tangents as the scene holds them at this point of
 * hip_stream.  joints and weights are host arrays, copied to the device before return; the call may allocate and synchronise, like the
 * first refit and the first mark.  *out_skin is the skin's number: 0, 1, ... in creation order.  Skins live until vkrt_scene_destroy
 * and survive builds, refits and node updates; their ranges do not overlap.  A later vkrt_scene_update_vertices on a skinned range is
 * allowed: the next vkrt_scene_skin_vertices overwrites positions, normals and tangents from the captured bind pose (not from the
 * update).  Texture coordinates are never touched by skinning, so an update of them stays.
 * Refused with VKRT_ERR_INVALID_ARGUMENT, changing nothing, in this order: a NULL desc; struct_size < sizeof(vkrt_skin_desc);
 * joint_count 0 or above 65536; NULL joints or weights with count > 0; a joint index >= joint_count; a non-finite weight; a NULL
 * out_skin; a NULL scene; a range outside the scene's vertices; count == 0; a range that overlaps an existing skin's; a range that
 * overlaps an existing morph's (vkrt_scene_add_morph: skins are added before the morphs inside them).  Then, without a device:
 * VKRT_ERR_NO_DEVICE.
 *
 * vkrt_scene_skin_vertices poses skin `skin` from joint_matrices ([joint_count][16], column-major like vkrt_node.worldMatrix: glTF's
 * jointMatrix = inverse(meshGlobal) * jointGlobal * inverseBind, in the space the scene's vertices live in): one kernel launch on
 * hip_stream (ordering as vkrt_scene_update_vertices) that writes the positions, normals and tangents of the skin's range.
 * VKRT_MEMORY_DEVICE: the matrices are device memory on the scene's device, 16-byte aligned, valid until the stream has passed the
 *   call.  Nothing is allocated, nothing synchronises, the values are not inspected (as for a device vertex update).
 * VKRT_MEMORY_HOST: every element is checked finite before anything changes; the matrices are staged through the scene's staging
 *   buffer (the one of host vertex updates) and the call waits for hip_stream before it returns.
 * In both cases the library's host copy of the positions falls behind the device's: the next vkrt_accel_build downloads them first.
 * Stale tree: with a built tree, the tree is stale exactly as after a vertex update with positions; one vkrt_accel_refit serves any
 *   number of skin, vertex and node updates before it.  vkrt_hit_surface and vkrt_hit_motion see the new pose without a refit.  The
 *   motion snapshot is untouched: mark -> skin -> vkrt_hit_motion gives the pose before the skin call as `previous`.
 * Refused with VKRT_ERR_INVALID_ARGUMENT, changing nothing, in this order: a memory value that is neither of the two; a NULL scene; a
 * skin index out of range; NULL or (device memory) misaligned joint_matrices; (host memory) a non-finite element.  Then, without a
 * device: VKRT_ERR_NO_DEVICE.
 *
 * Arithmetic: binary32, in source order, no contraction.  Element (r, c) of joint k is m[16k + 4c + r]; only rows 0 to 2 are read.  For
 * a vertex with joints j0..j3, weights w0..w3 (used as given: not renormalised, all four always multiply -- glTF pads unused
 * influences with weight 0), bind position p, normal n and tangent (t, tw):
 *     M[r][c] = ((w0*J[j0][r][c] + w1*J[j1][r][c]) + w2*J[j2][r][c]) + w3*J[j3][r][c]        r = 0..2, c = 0..3
 *     p'[r]   = ((M[r][0]*p.x + M[r][1]*p.y) + M[r][2]*p.z) + M[r][3]
 *     N[r]    = (M[r][0]*n.x + M[r][1]*n.y) + M[r][2]*n.z ;  d = (N.x*N.x + N.y*N.y) + N.z*N.z
 *     n'      = (d > 0 && d < inf) ? N * (1.0f / sqrtf(d)) : N
 *     t'.xyz  = the same from t ;  t'.w = tw
 * Normals go through the blended 3x3 as glTF viewers do, not through its inverse transpose: exact for rigid joints and uniform scale,
 * tilted towards the stretched axis under non-uniform scale. */
typedef struct vkrt_skin_desc {
  uint32_t struct_size;      /* sizeof(vkrt_skin_desc) */
  uint32_t first, count;     /* vertices [first, first+count), absolute indices as in vkrt_vertex_update */
  uint32_t joint_count;      /* 1..65536 */
  const uint16_t* joints;    /* host, u16[count][4]: glTF JOINTS_0 */
  const float*    weights;   /* host, f32[count][4]: glTF WEIGHTS_0, used as given (not renormalised) */
} vkrt_skin_desc;
int vkrt_scene_add_skin(vkrt_scene* scene, const vkrt_skin_desc* desc, void* hip_stream, uint32_t* out_skin);
int vkrt_scene_skin_vertices(vkrt_scene* scene, uint32_t skin, const float* joint_matrices, uint32_t memory /* vkrt_memory */, void* hip_stream);

/* ---- morph targets (glTF primitives[].targets, blend shapes: a displacement of POSITION, NORMAL and TANGENT per target and vertex, a
 *      vector of weights per frame): base + sum(w * delta) inside the library.  These entry points came after ABI version 4 without
 *      changing it or any existing struct: detect them by symbol. ---------------------------------------------------------------------
 * vkrt_scene_add_morph binds target_count targets to the range [first, first+count) (absolute vertex indices, as in
 * vkrt_vertex_update) and captures the range's base shape: positions, normals and tangents as they stand at this point of hip_stream.
 * The delta arrays are host arrays, vec3[target_count][count] (target-major: all vertices of target 0, then of target 1, ...), copied
 * to the device before return; an attribute whose array is NULL is not morphed.  Tangent deltas are xyz only, as in glTF: the
 * handedness w is kept.  The call may allocate and synchronise.  *out_morph is the morph's number: 0, 1, ... in creation order.
 * Morphs live until vkrt_scene_destroy and survive builds, refits and node updates; their ranges do not overlap each other.
 * Where a morph writes (glTF 3.7.2.2: morph, then skin):
 *   a range that overlaps no skin: the live arrays, like a skin: positions, normals and tangents; texture coordinates are never
 *     touched.  A later vkrt_scene_update_vertices on the range is allowed: the next vkrt_scene_morph_vertices overwrites positions,
 *     normals and tangents from the captured base (not from the update).
 *   a range that lies wholly inside one skin's range: the base is captured from that skin's bind pose, and vkrt_scene_morph_vertices
 *     writes that bind pose and nothing else -- the live arrays and the tree stay as they are.  The next vkrt_scene_skin_vertices of
 *     that skin, later on the same stream, carries the morphed shape into the scene.  Add skins before morphs.
 * Refused with VKRT_ERR_INVALID_ARGUMENT, changing nothing, in this order: a NULL desc; struct_size < sizeof(vkrt_morph_desc);
 * target_count 0 or above VKRT_MORPH_TARGETS_MAX; all three delta arrays NULL; a non-finite delta (positions, then normals, then
 * tangents); a NULL out_morph; a NULL scene; a range outside the scene's vertices; count == 0; a range that overlaps an existing
 * morph's; a range that straddles a skin's boundary or touches two skins.  Then, without a device: VKRT_ERR_NO_DEVICE; if the device
 * has no memory for the deltas: VKRT_ERR_OUT_OF_MEMORY, and nothing has been added.
 *
 * vkrt_scene_morph_vertices poses morph `morph` from weights[target_count]: one kernel launch on hip_stream (ordering as
 * vkrt_scene_update_vertices).
 * VKRT_MEMORY_DEVICE: the weights are device memory on the scene's device, 4-byte aligned, valid until the stream has passed the
 *   call.  Nothing is allocated, nothing synchronises, the values are not inspected.
 * VKRT_MEMORY_HOST: every weight is checked finite before anything changes; the weights are staged through the scene's staging buffer
 *   (the one of host vertex updates) and the call waits for hip_stream before it returns.
 * A morph outside every skin leaves the library's host copy of the positions behind the device's (the next vkrt_accel_build downloads
 * them first) and, with a built tree, the tree stale exactly as after vkrt_scene_skin_vertices; one vkrt_accel_refit serves any number
 * of morph, skin, vertex and node updates before it.  vkrt_hit_surface and vkrt_hit_motion see the new shape without a refit.  The
 * motion snapshot is untouched: mark -> morph -> vkrt_hit_motion gives the shape before the morph call as `previous`.
 * Refused with VKRT_ERR_INVALID_ARGUMENT, changing nothing, in this order: a memory value that is neither of the two; a NULL scene; a
 * morph index out of range; NULL or (device memory) misaligned weights; (host memory) a non-finite weight.  Then, without a device:
 * VKRT_ERR_NO_DEVICE.
 *
 * Arithmetic: binary32, in source order, no contraction.  For a vertex with captured base position p, normal n and tangent (t, tw),
 * deltas dP[k], dN[k], dT[k] of target k and weights w[0..T-1], per component:
 *     P = p;  for k = 0..T-1 in index order:  if (w[k] != 0)  P = P + w[k] * dP[k]         (the product rounded, then the sum)
 *     N, Tn likewise from n, t with dN, dT -- only if the morph has that delta array
 *     p'      = P
 *     n'      = (the morph has normal deltas and some w[k] != 0) ? normalizeGuarded(N) : n
 *     t'.xyz  = (the morph has tangent deltas and some w[k] != 0) ? normalizeGuarded(Tn) : t ;  t'.w = tw
 *     normalizeGuarded(a): d = (a.x*a.x + a.y*a.y) + a.z*a.z ;  (d > 0 && d < inf) ? a * (1.0f / sqrtf(d)) : a     (the skin's rule)
 * A weight of exactly zero, of either sign, skips its target: all-zero weights give back the captured base in every bit (a component
 * that is -0 stays -0, which -0 + 0 * d would not), and the kernel reads only the targets that are in use.  An attribute without deltas
 * is written from the captured base. */
#define VKRT_MORPH_TARGETS_MAX 256
typedef struct vkrt_morph_desc {
  uint32_t struct_size;            /* sizeof(vkrt_morph_desc) */
  uint32_t first, count;           /* vertices [first, first+count), absolute indices as in vkrt_vertex_update */
  uint32_t target_count;           /* 1..VKRT_MORPH_TARGETS_MAX */
  const float* position_deltas;    /* host, vec3[target_count][count] (target-major) or NULL */
  const float* normal_deltas;      /* host, vec3[target_count][count] or NULL */
  const float* tangent_deltas;     /* host, vec3[target_count][count] or NULL (glTF: xyz only, w is kept) */
} vkrt_morph_desc;
int vkrt_scene_add_morph(vkrt_scene* scene, const vkrt_morph_desc* desc, void* hip_stream, uint32_t* out_morph);
int vkrt_scene_morph_vertices(vkrt_scene* scene, uint32_t morph, const float* weights /* [target_count] */, uint32_t memory /* vkrt_memory */,
                              void* hip_stream);

/* ---- ray queries (replaces traceRayEXT on rays of the caller's own, raytrace.rgen:64-97 / VK_KHR_ray_query: a closest-hit and an
 *      occlusion query per ray of a device array).  These entry points came after ABI version 4 without changing it or any
 *      existing struct: detect them by symbol. ---------------------------------------------------------------------------------------
 * Memory and ordering: `rays`, `hits` and `occluded` are device memory on the scene's device; `rays` and `hits` are 16-byte aligned.
 * The call is enqueued on hip_stream (NULL = default stream), after what was enqueued there before it; it allocates nothing, does not
 * synchronise with the host and returns after the enqueue.  n may be any uint32_t.
 * Closest hit: the hit the library's walks compute everywhere else -- the smallest t in the open interval (tmin, tmax), ties to the
 * smallest flattened triangle id.  Miss: t = tmax, u = v = 0, and all five integer fields -1.
 * Occlusion: occluded[i] = 1 when some hit exists in (tmin, tmax), else 0.
 * Rays that miss without a walk: tmin < 0, tmin >= tmax (a NaN bound included), a zero direction, a NaN or infinite component of the
 * origin or the direction.  tmax = +inf is accepted.  The direction need not be normalised (t is in units of its length).
 * Scene options: the triangle options of the build apply -- VKRT_OPT_WATERTIGHT, and VKRT_OPT_ANYHIT_DISSOLVE with anyhit_seed as the
 * payload seed of every ray (0 = what vkrt_debug_trace_rays and the oracle use).  The scheduling options (VKRT_OPT_WF_SHARE,
 * VKRT_OPT_WF_SHARE_FLAGS, VKRT_OPT_TRI_THRESHOLD) apply too; none of them changes a result.
 * Errors, in this order: a NULL scene, or (n > 0) a NULL or misaligned pointer: VKRT_ERR_INVALID_ARGUMENT; n == 0: VKRT_OK, nothing is
 * enqueued; no tree, or a stale one after vkrt_scene_update_nodes / vkrt_scene_update_vertices: VKRT_ERR_NOT_BUILT; without a device: VKRT_ERR_NO_DEVICE.
 * Counters: a walk cut short adds to vkrt_counters.traversal_faults, like every other walk; no other counter moves. */
typedef struct vkrt_ray {        /* 32 B */
  float origin[3];    float tmin;
  float direction[3]; float tmax;
} vkrt_ray;
typedef struct vkrt_hit {        /* 32 B */
  float   t, u, v;    /* u, v: barycentric weights of vertices 1 and 2, as the hit shader receives them (raytrace.rchit:68) */
  int32_t instance;   /* node index (the reference's TLAS instance); -1 = miss */
  int32_t primitive;  /* triangle index within its primitive-mesh (gl_PrimitiveID) */
  int32_t prim_mesh;  /* the node's primMesh (gl_InstanceCustomIndexEXT, hello_vulkan.cpp:1039) */
  int32_t triangle;   /* flattened triangle id: the gid of vkrt_debug_trace_rays and of the oracle */
  int32_t material;   /* max(0, materialIndex) of the primitive-mesh: the material the hit shader reads */
} vkrt_hit;
int vkrt_intersect(vkrt_scene* scene, const vkrt_ray* rays, uint32_t n, uint32_t anyhit_seed, vkrt_hit* hits, void* hip_stream);
int vkrt_occluded(vkrt_scene* scene, const vkrt_ray* rays, uint32_t n, uint32_t anyhit_seed, int32_t* occluded, void* hip_stream);

/* ---- instance visibility and ray flags (traceRayEXT's cullMask and rayFlags, raytrace.rgen:64-66 / :86-87, acting on
 *      VkAccelerationStructureInstanceKHR::mask and ::flags, hello_vulkan.cpp:1040-1041).  These entry points came after ABI version 4
 *      without changing it or any existing struct: detect them by symbol. ------------------------------------------------------------
 * They act on the ray-query entry points only: vkrt_pathtrace*, vkrt_gbuffer_raycast*, vkrt_hybrid_trace* and vkrt_debug_trace_rays
 * trace as the reference does (cull mask 0xFF, no culling), and since a mask is never 0 their pixels and counters do not depend on
 * any visibility setting.
 * Candidates: a triangle of instance I is a candidate for a ray of a call with options (ray_flags, cull_mask) when
 *   1. (I.mask & cull_mask) != 0,
 *   2. it is not culled by facing: with VKRT_RAY_CULL_BACK_FACING (VKRT_RAY_CULL_FRONT_FACING) back-facing (front-facing) triangles are
 *      not candidates, unless I has VKRT_INSTANCE_FACING_CULL_DISABLE,
 *   3. the any-hit dissolve stage does not ignore it (VKRT_OPT_ANYHIT_DISSOLVE; never with VKRT_RAY_OPAQUE), nor does the alpha test
 *      of a VKRT_ALPHA_MASK material ("alpha-tested materials" below; never with VKRT_RAY_OPAQUE).
 * Closest hit and occlusion follow the rules above over the candidates; the filter is a pure function of (ray, triangle), so a result
 * stays a property of the triangle set, independent of builder, layout, split and schedule.
 * Facing is decided in object space: a triangle is FRONT-facing when its object-space vertices p0, p1, p2 (index order) appear
 * counter-clockwise seen from the ray's origin, i.e. when (p1 - p0) x (p2 - p0) points against the object-space direction (glTF's
 * front face); VKRT_INSTANCE_FLIP_FACING swaps front and back.  (On world-space vertices: front <=> (Moeller-Trumbore's
 * det = e1 . (d x e2) > 0) XOR (the node's 3x3 has a negative determinant) XOR FLIP_FACING.) */
enum vkrt_instance_flags {
  VKRT_INSTANCE_FACING_CULL_DISABLE = 0x1, /* the ray's facing-cull flags do not apply to this instance */
  VKRT_INSTANCE_FLIP_FACING = 0x2          /* front and back are swapped */
};
typedef struct vkrt_instance_visibility { /* 4 B; every node starts as {0xFF, VKRT_INSTANCE_FACING_CULL_DISABLE}, the reference's TLAS */
  uint8_t  mask;     /* 1..255 (to hide an instance from every ray give it a zero-scale transform) */
  uint8_t  flags;    /* vkrt_instance_flags */
  uint16_t reserved; /* 0 */
} vkrt_instance_visibility;
/* Set the visibility of nodes [first, first+count).  Same rules as vkrt_scene_update_nodes: the array is copied before return, the work
 * is enqueued on hip_stream with no host synchronisation and no allocation, and ray queries enqueued on that stream after it see the new
 * values.  It does not make the tree stale and works on a stale one.  Refused with VKRT_ERR_INVALID_ARGUMENT, changing nothing, in this
 * order: a NULL array with count > 0; an entry with mask 0, unknown flag bits or reserved != 0; a NULL scene; a range outside the
 * scene's nodes.  Then, without a device: VKRT_ERR_NO_DEVICE.  The visibility of a node survives vkrt_scene_update_nodes,
 * vkrt_scene_update_node_transforms, vkrt_accel_refit and vkrt_accel_build.  The call writes the visibility word of each record and
 * nothing else of it: a transform that came from device memory stays in place. */
int vkrt_scene_set_instance_visibility(vkrt_scene* scene, uint32_t first, uint32_t count, const vkrt_instance_visibility* vis, void* hip_stream);
/* Reads the host copy (no synchronisation).  VKRT_ERR_INVALID_ARGUMENT: a NULL array with count > 0, a NULL scene, a range outside. */
int vkrt_scene_get_instance_visibility(const vkrt_scene* scene, uint32_t first, uint32_t count, vkrt_instance_visibility* out);

enum vkrt_ray_flags {                 /* the gl_RayFlags*EXT values; no other bit is accepted */
  VKRT_RAY_OPAQUE = 0x1,              /* skip the any-hit stages: dissolve (VKRT_OPT_ANYHIT_DISSOLVE) and the alpha test of MASK materials */
  VKRT_RAY_CULL_BACK_FACING = 0x10,   /* back-facing triangles are not candidates (instances with FACING_CULL_DISABLE excepted) */
  VKRT_RAY_CULL_FRONT_FACING = 0x20   /* front-facing triangles are not candidates (the same) -- not together with CULL_BACK_FACING */
};
typedef struct vkrt_query_opts {
  uint32_t struct_size; /* sizeof(vkrt_query_opts) */
  uint32_t ray_flags;   /* vkrt_ray_flags */
  uint32_t cull_mask;   /* 0..0xFF; 0 = every ray misses (results are written, nothing is walked) */
  uint32_t anyhit_seed; /* as in vkrt_intersect */
} vkrt_query_opts;
/* vkrt_intersect / vkrt_occluded with options for the whole call (a caller with two kinds of rays makes two calls); same memory,
 * ordering, miss and error rules.  vkrt_intersect(..., seed, ...) is vkrt_intersect_ex with {sizeof, 0, 0xFF, seed}, and
 * vkrt_occluded likewise.  Refused with VKRT_ERR_INVALID_ARGUMENT before the checks of vkrt_intersect (NULL scene, arrays; then n == 0,
 * NOT_BUILT, NO_DEVICE): a NULL opts, struct_size < sizeof(vkrt_query_opts), a ray flag outside the three above, both cull flags,
 * cull_mask > 0xFF.
 * Cost: with no cull flag and a cull mask that meets every node's mask the call runs the kernel of vkrt_intersect / vkrt_occluded.
 * Otherwise the walk filters candidates; on the 8-wide layout it also skips the children whose subtree holds no instance the mask
 * admits (a table of one byte per child slot, kept with the tree); the BVH2 layout filters at the triangles only. */
int vkrt_intersect_ex(vkrt_scene* scene, const vkrt_ray* rays, uint32_t n, const vkrt_query_opts* opts, vkrt_hit* hits, void* hip_stream);
int vkrt_occluded_ex(vkrt_scene* scene, const vkrt_ray* rays, uint32_t n, const vkrt_query_opts* opts, int32_t* occluded, void* hip_stream);

/* ---- multi-hit queries (the any-hit stage of traceRayEXT for a caller without callbacks: Embree's rtcIntersect with a collecting filter,
 *      OptiX any-hit, trimesh's multiple_hits): the first max_hits candidates along each ray, in order.  Alpha cut-outs and ordered
 *      blending from vkrt_surface.alpha, lidar multi-return, thickness sums and inside/outside parity need the hits behind the closest
 *      one; re-tracing with tmin = t of the last hit skips a second surface at exactly that t (the interval is open).  This entry point
 *      came after ABI version 4 without changing it or any existing struct: detect it by symbol. ------------------------------------
 * Result: sort the candidates of ray i (the section above: cull mask, facing flags, the dissolve stage with opts->anyhit_seed unless
 * VKRT_RAY_OPAQUE; the build's VKRT_OPT_WATERTIGHT applies) with t in the open interval (tmin, tmax) by the key (t, flattened triangle
 * id).  counts[i] = min(max_hits, their number); hits[i * max_hits + j] for j < counts[i] is the j-th of them, with the eight fields
 * vkrt_intersect writes; for j >= counts[i] it is the miss record of vkrt_intersect (t = tmax, u = v = 0, the five integers -1), so
 * the whole buffer is defined.  A triangle appears at most once per ray, whatever VKRT_OPT_SPLIT_BUDGET made of it; two triangles at
 * the same t (coincident faces, decals, doubled instances) both appear, the smaller id first.
 * Consequences: with max_hits = 1 the call writes bit for bit what vkrt_intersect_ex writes.  The list is a property of the triangle
 * set: the same under every builder, layout, split budget and scheduling option, and after a refit.  Rays that miss without a walk
 * (tmin < 0, tmin >= tmax, a zero direction, a non-finite component) and every ray of a call with cull_mask = 0 have count 0.
 * tmax = +inf is accepted.
 * Memory and ordering are those of vkrt_intersect: `hits` is device memory, 16-byte aligned, n * max_hits records, ray-major (the
 * product may pass 2^32: index it with 64 bits); `counts` is NULL or device memory, 4-byte aligned, n words.  The call is enqueued on
 * hip_stream, allocates nothing, does not synchronise with the host; n may be any uint32_t; only vkrt_counters.traversal_faults may move.
 * Errors, in this order: what vkrt_intersect_ex refuses of opts; max_hits == 0 or max_hits > VKRT_MULTIHIT_MAX:
 * VKRT_ERR_INVALID_ARGUMENT; then the checks of vkrt_intersect in their order (a NULL scene; for n > 0 a NULL or misaligned rays or
 * hits, a misaligned counts; n == 0: VKRT_OK, nothing is enqueued; VKRT_ERR_NOT_BUILT; VKRT_ERR_NO_DEVICE).
 * Cost: every ray is walked on its own (no shared walk), once, as far as the t of its max_hits-th candidate -- or to tmax when it has
 * fewer; the list lives in on-chip memory, 20 B x max_hits per ray in flight. */
#define VKRT_MULTIHIT_MAX 16
int vkrt_intersect_multi(vkrt_scene* scene, const vkrt_ray* rays, uint32_t n, const vkrt_query_opts* opts, uint32_t max_hits, vkrt_hit* hits,
                         int32_t* counts, void* hip_stream);

/* ---- closest-point queries (Embree's rtcPointQuery, trimesh's nearest.on_surface, the distance query of collision and
 *      signed-distance pipelines): per query the nearest point of the scene's surface to a point, within a radius.  Rays cannot
 *      emulate it.  The result is a vkrt_hit, so vkrt_hit_surface turns it into position, normal and material with nothing in between
 *      (signed distance: t with the sign of (point - position) . geometric_normal).  This entry point came after ABI version 4 without
 *      changing it or any existing struct: detect it by symbol. -------------------------------------------------------------------
 * The triangle: the one the ray tests see, (p0, p0 + e1, p0 + e2) with p0, e1, e2 the binary32 values of its record (vkrt_debug_read_accel:
 * floats 0-2, 3-5, 6-8 of the 48-B record).  With VKRT_OPT_WATERTIGHT the record holds (p0, p1, p2), and e1 = p1 - p0, e2 = p2 - p0 are
 * formed in binary32: the bits the default record stores, so a result does not depend on that option.
 * The point/triangle function (Ericson, Real-Time Collision Detection 5.1.5) runs in binary64 on those binary32 inputs and the
 * binary32 query point q: no contraction, source order, a dot product a . b = (ax * bx + ay * by) + az * bz.
 *   ap = q - p0                d1 = e1 . ap    d2 = e2 . ap
 *   bp = ap - e1               d3 = e1 . bp    d4 = e2 . bp
 *   cp = ap - e2               d5 = e1 . cp    d6 = e2 . cp
 *   vc = d1 * d4 - d3 * d2     vb = d5 * d2 - d1 * d6     va = d3 * d6 - d5 * d4
 * The first of these rows whose condition holds gives the weights (u, v) of vertices 1 and 2:
 *   1. d1 <= 0 && d2 <= 0                             (0, 0)
 *   2. d3 >= 0 && d4 <= d3                            (1, 0)
 *   3. vc <= 0 && d1 >= 0 && d3 <= 0                  (d1 / (d1 - d3), 0)
 *   4. d6 >= 0 && d5 <= d6                            (0, 1)
 *   5. vb <= 0 && d2 >= 0 && d6 <= 0                  (0, d2 / (d2 - d6))
 *   6. va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0    w = (d4 - d3) / ((d4 - d3) + (d5 - d6));  (1 - w, w)
 *   7. otherwise                                      den = 1 / ((va + vb) + vc);  (vb * den, vc * den)
 * Then diff = (ap - u * e1) - v * e2 per component and dist2 = diff . diff.  A triangle whose dist2 is NaN is no candidate (a
 * collinear triangle whose point falls through to row 7).  (Binary32 is not enough: on needle triangles it is wrong by 1e-2 of the
 * scene's size; binary64 agrees with an 80-bit evaluation to 2e-11.)
 * Result of query i: among the candidates -- triangles of instances with (mask & cull_mask) != 0 and dist2 < (double)radius * radius,
 * the comparison strict -- the one with the smallest key (dist2, flattened triangle id).  Its record: t = sqrtf((float)dist2), the
 * distance; u, v = (float)u, (float)v, as in every other vkrt_hit; the five integers as vkrt_intersect writes them.  Without a
 * candidate: t = radius, u = v = 0, the five integers -1.  A query misses without a walk when a component of `point` is NaN or
 * infinite, when radius is NaN, negative or 0, and when cull_mask is 0.  radius = +inf is accepted.
 * The result is a property of the triangle set: the same under every builder, layout, split budget and scheduling option, and
 * after a refit.  The walk prunes with a lower bound of the squared point/box distance that carries margins for the binary32
 * rounding of the boxes, and keeps a box whose bound equals the best dist2, so an equally near triangle with a smaller id is found.
 * Options: opts may be NULL = {sizeof(vkrt_query_opts), 0, 0xFF, 0}.  ray_flags must be 0 -- a point has no facing and no any-hit
 * stage, so VKRT_OPT_ANYHIT_DISSOLVE never applies; anyhit_seed is ignored; cull_mask works as in vkrt_intersect_ex.
 * Memory and ordering are those of vkrt_intersect: `queries` and `hits` are device memory on the scene's device, 16-byte aligned; the
 * call is enqueued on hip_stream, allocates nothing, does not synchronise with the host; n may be any uint32_t; only
 * vkrt_counters.traversal_faults may move.
 * Errors, in this order: what vkrt_intersect_ex refuses of a non-NULL opts, and ray_flags != 0: VKRT_ERR_INVALID_ARGUMENT; then the
 * checks of vkrt_intersect in their order (a NULL scene; for n > 0 a NULL or misaligned queries or hits; n == 0: VKRT_OK, nothing is
 * enqueued; VKRT_ERR_NOT_BUILT, also on a stale tree; VKRT_ERR_NO_DEVICE).
 * Cost: every query walks on its own, nearest box first; the triangle step is binary64. */
typedef struct vkrt_point_query { /* 16 B */
  float point[3];
  float radius;       /* > 0, +inf allowed: only surface points nearer than this are found */
} vkrt_point_query;
int vkrt_closest_point(vkrt_scene* scene, const vkrt_point_query* queries, uint32_t n, const vkrt_query_opts* opts, vkrt_hit* hits,
                       void* hip_stream);

/* ---- shading inputs at the hits of ray queries (what raytrace.rchit:34-113 computes before its BRDF: attribute fetch, world
 *      transforms, tangent frame, the four texture() taps, normal mapping; Vulkan's hit attributes + buffer references, Embree's
 *      rtcInterpolate).  With vkrt_intersect and vkrt_occluded it is enough to write a path tracer outside the library.  This entry
 *      point came after ABI version 4 without changing it or any existing struct: detect it by symbol. ------------------------------
 * Memory and ordering are those of vkrt_intersect: `hits` and `out` are device memory on the scene's device, 16-byte aligned; the call
 * is enqueued on hip_stream, allocates nothing, does not synchronise with the host and returns after the enqueue; n may be any
 * uint32_t.  A vkrt_intersect and a vkrt_hit_surface enqueued on one stream need nothing between them.
 * A record is a function of (instance, primitive, u, v) of the hit and of the scene's current arrays; t, prim_mesh, triangle and
 * material of the input are not read.  All arithmetic is that of the path tracer's hit shader: binary32, no contraction, LOD 0.
 *   position          gl_ObjectToWorldEXT * interpolated position (rchit:70-72): bit for bit the origin the path tracer gives the next ray
 *   normal            the interpolated vertex normal, normalised, * gl_WorldToObjectEXT, normalised (rchit:74-75)
 *                     (gl_WorldToObjectEXT: the cofactor inverse of the node's 3x3 in binary64, rounded to binary32, as everywhere in the
 *                     library; its zero entries carry the signs that form gives them, and a normal component of -0 is a zero)
 *   texcoord_u/v      the interpolated TEXCOORD_0 (rchit:79)
 *   shading_normal, tangent, binormal   the frame the shader hands the BRDF.  Without a normal texture, or with VKRT_SURFACE_GEOMETRY
 *                     alone: `normal`, the Gram-Schmidt tangent and tangent.w * cross(N, T) (rchit:77-78).  With VKRT_SURFACE_MATERIAL and
 *                     a normal texture: the tap * 2 - 1 carried into that frame, then createCoordinateSystem (rchit:100-106)
 *   base_color, metallic, roughness     pbrGetBaseColor / pbrGetMetallicRoughness (gltf.glsl:26-45), unclamped as fetched
 *   emission          emissiveFactor * texture(emissiveTexture), always (the depth / isSpecular rule of rchit:83 is the integrator's)
 *   alpha             pbrBaseColorFactor.a, times the .a of the base colour tap where the material has that texture (glTF's alpha)
 *   geometric_normal  normalize(cross(p1 - p0, p2 - p0) * gl_WorldToObjectEXT) on the object-space vertices in index order: the
 *                     counter-clockwise front face of the visibility section above, carried to world space by the inverse transpose
 *                     like a vertex normal, so it stays on the front side under mirroring and non-uniform scale.  It is not turned
 *                     towards any ray: the caller has the direction and takes the sign of the dot product
 *   material          max(0, materialIndex) of the instance's primitive-mesh;  valid = 1;  reserved = 0
 * With VKRT_SURFACE_GEOMETRY alone alpha, metallic, roughness, base_color and emission are 0 and no texel is read.
 * Records that are not hits of this scene have a defined result and read nothing out of bounds: instance < 0 (a miss as
 * vkrt_intersect writes it), instance >= node_count, primitive outside [0, indexCount / 3) of the instance's primitive-mesh, or a
 * non-finite u or v give an all-zero record with material = -1 and valid = 0.  Finite u, v outside the triangle are used as given.
 * No tree is needed: everything read is uploaded at vkrt_scene_create and kept current, in stream order, by vkrt_scene_update_nodes
 * and vkrt_scene_update_vertices.  The call works before vkrt_accel_build and on a stale tree and never returns VKRT_ERR_NOT_BUILT, so
 * a caller can follow surface points (instance, primitive, u, v) through motion and deformation.
 * Errors, in this order, the first four before anything of the scene is read: a NULL scene, or (n > 0) a NULL or misaligned pointer,
 * or a `fields` value other than the two below: VKRT_ERR_INVALID_ARGUMENT; n == 0: VKRT_OK, nothing is enqueued; without a device:
 * VKRT_ERR_NO_DEVICE.  No counter moves. */
enum vkrt_surface_fields {
  VKRT_SURFACE_GEOMETRY = 0x1,   /* position, geometric and interpolated normal, vertex tangent frame, texture coordinate */
  VKRT_SURFACE_MATERIAL = 0x2    /* + the four texture() taps: normal mapping, base colour, alpha, metallic, roughness, emission */
};
typedef struct vkrt_surface {            /* 128 B, 16-byte aligned, eight float4 */
  float position[3];         float texcoord_u;
  float geometric_normal[3]; float texcoord_v;
  float normal[3];           float alpha;
  float shading_normal[3];   float metallic;
  float tangent[3];          float roughness;
  float binormal[3];         int32_t material;
  float base_color[3];       int32_t valid;
  float emission[3];         uint32_t reserved;   /* 0 */
} vkrt_surface;
int vkrt_hit_surface(vkrt_scene* scene, const vkrt_hit* hits, uint32_t n, uint32_t fields, vkrt_surface* out, void* hip_stream);

/* ---- motion: where a visible surface point was one frame ago (what NRD takes as IN_MV, as world positions), for scenes that
 *      vkrt_scene_update_nodes and vkrt_scene_update_vertices move and deform.  These entry points came after ABI version 4 without
 *      changing it or any existing struct: detect them by symbol. ----------------------------------------------------------------
 * The scene keeps a *previous state*: the node transforms and vertex positions as they were at the last mark.  A frame loop marks,
 * then updates, then refits, then renders:
 *     mark -> update nodes / vertices -> refit -> vkrt_gbuffer_raycast_hits -> vkrt_hit_motion -> trace -> vkrt_denoise_diffuse_motion
 *
 * vkrt_scene_motion_mark: the node transforms and vertex positions, as they are at this point of hip_stream, become the previous
 * state: two stream-ordered device-to-device copies (the instance records and the positions).  The first call allocates 96 bytes
 * per node + 12 bytes per vertex and may synchronise, like the first refit; later calls neither allocate nor synchronise.  Before
 * any mark the previous state is the current state (the live arrays, nothing allocated).  The snapshot is not part of the tree: it
 * survives vkrt_accel_build, vkrt_accel_refit and updates of normals, tangents and texture coordinates, and goes with the scene.  A
 * mark copies all nodes and all positions (no partial snapshots).  Refused with VKRT_ERR_INVALID_ARGUMENT: a NULL scene. */
int vkrt_scene_motion_mark(vkrt_scene* scene, void* hip_stream);
/* The surface point of n hit records now (current_rgba32f) and in the previous state (previous_rgba32f): device arrays of n x 4
 * floats, 16-byte aligned like hits; either may be NULL, not both.  Records are resolved and validated as vkrt_hit_surface does --
 * (instance, primitive, u, v) are read, t and the other ids are not -- and like it the call needs no tree (it works on a stale one).
 * A miss, an id outside the scene or a non-finite u or v gives (0, 0, 0, 0); a valid record gives (x, y, z, 1) with, in binary32
 * without contraction, bw = ((1 - u) - v, u, v), Pk = objectToWorld * (position of vertex k, 1) and
 *     xyz = ((0 + P0 * bw0) + P1 * bw1) + P2 * bw2
 * -- current from the live transforms and vertices, previous from the snapshot.  That is the raster stand-in's order (transform the
 * corners, then interpolate), not raytrace.rchit's: for a record written by vkrt_gbuffer_raycast_hits, current.xyz equals the
 * G-buffer's position.xyz in every bit, and while nothing moved previous equals current in every bit, which keeps a still frame's
 * reprojection exactly on the pixel.  One thread per record, on hip_stream, no allocation and no synchronisation. */
int vkrt_hit_motion(vkrt_scene* scene, const vkrt_hit* hits, uint32_t n, float* current_rgba32f, float* previous_rgba32f, void* hip_stream);

/* ---- alpha-tested materials (glTF's alphaMode MASK; Vulkan's any-hit shader for cut-out geometry: foliage, fences, fabric edges):
 *      the texture decides inside the walk whether a candidate counts.  These entry points came after ABI version 4 without changing
 *      it or any existing struct: detect them by symbol. ------------------------------------------------------------------------
 * A candidate hit on a triangle whose material is VKRT_ALPHA_MASK is ignored when !(alpha >= cutoff).  alpha is, bit for bit, the
 * value vkrt_hit_surface(..., VKRT_SURFACE_GEOMETRY | VKRT_SURFACE_MATERIAL) writes into vkrt_surface.alpha for the candidate's
 * (instance, primitive, u, v), with u, v the floats the walk would put into the vkrt_hit: in binary32 without contraction
 * b = (1 - u - v, u, v), tu = (uv0.x * b.x + uv1.x * b.y) + uv2.x * b.z and tv likewise, the bilinear LOD-0 REPEAT tap of the base
 * colour texture, its .a decoded as UNORM (never through the sRGB curve), times pbrBaseColorFactor[3]; a material without a base
 * colour texture has alpha = pbrBaseColorFactor[3].  A cutoff of 0 admits every candidate; a NaN alpha admits none.
 * The stage acts in vkrt_intersect, vkrt_occluded, their _ex forms and vkrt_intersect_multi (whose lists then hold admitted candidates
 * only), as the third filter after the cull mask and the facing flags and beside the dissolve stage of VKRT_OPT_ANYHIT_DISSOLVE: both
 * may be active, and a candidate is ignored if either says so.  VKRT_RAY_OPAQUE skips both, as gl_RayFlagsOpaqueEXT does.  With
 * VKRT_OPT_ALPHA_TEST = 1 the same rule, with the payload's seed for the dissolve stage, acts on every ray of vkrt_pathtrace*,
 * vkrt_gbuffer_raycast* (always the LOD-0 tap, whatever VKRT_OPT_GBUFFER_MIPS says) and vkrt_hybrid_trace*; the shading of an admitted
 * hit is unchanged.  With the option 0 (the default) those results do not depend on any alpha mode.  It never acts in
 * vkrt_closest_point, vkrt_hit_surface or vkrt_debug_trace_rays.
 * The decision is a pure function of (ray, triangle), so a result stays a property of the triangle set: the same under every builder,
 * layout, split budget and scheduling option, and after a refit; vkrt_intersect_multi with max_hits = 1 still writes what
 * vkrt_intersect_ex writes.  The stage reads the live vertex array: a texture-coordinate update (vkrt_scene_update_vertices with
 * texcoords0 only) takes effect in the next query, without a refit.
 * Cost: while no material of the scene is MASK, and for every VKRT_RAY_OPAQUE call, a query launches the kernel it launched before.
 * Otherwise the walk looks up the material of each candidate that passed the distance test and the other filters (two dependent
 * loads); a MASK material adds three vertex loads, the material's texture reference and the tap. */
enum vkrt_alpha_mode { VKRT_ALPHA_OPAQUE = 0, VKRT_ALPHA_MASK = 1 };
typedef struct vkrt_material_alpha { /* 8 B; every material starts as {VKRT_ALPHA_OPAQUE, 0.5}: the reference's behaviour */
  uint32_t mode;   /* vkrt_alpha_mode */
  float    cutoff; /* finite, >= 0 (glTF's alphaCutoff, default 0.5); read for VKRT_ALPHA_MASK only */
} vkrt_material_alpha;
/* Set the alpha mode of materials [first, first+count).  The rules of vkrt_scene_set_instance_visibility: the array is copied before
 * return, the work is enqueued on hip_stream with no host synchronisation and no allocation, and ray queries enqueued on that stream
 * after it see the new values, and so do frames (VKRT_OPT_ALPHA_TEST).  It does not make the tree stale and works on a stale one, and
 * before vkrt_accel_build.  Refused with VKRT_ERR_INVALID_ARGUMENT, changing nothing, in this order: a NULL array with count > 0; an
 * entry with a mode other than the two or a
 * cutoff that is NaN, infinite or negative; a NULL scene; a range outside the scene's materials.  Then, without a device:
 * VKRT_ERR_NO_DEVICE.  The values survive vkrt_accel_build, vkrt_accel_refit, vkrt_scene_update_nodes and vkrt_scene_update_vertices. */
int vkrt_scene_set_material_alpha(vkrt_scene* scene, uint32_t first, uint32_t count, const vkrt_material_alpha* alpha, void* hip_stream);
/* Reads the host copy (no synchronisation).  VKRT_ERR_INVALID_ARGUMENT: a NULL array with count > 0, a NULL scene, a range outside. */
int vkrt_scene_get_material_alpha(const vkrt_scene* scene, uint32_t first, uint32_t count, vkrt_material_alpha* out);

/* ---- editing a live scene's lights, materials and textures (a moved light, a changed colour or texture binding, a video texture or
 *      the result of a render-to-texture pass: what a Vulkan application does with vkCmdUpdateBuffer and vkCmdCopyBufferToImage +
 *      vkCmdBlitImage between frames).  These entry points came after ABI version 4 without changing it or any existing struct: detect
 *      them by symbol. -------------------------------------------------------------------------------------------------------------
 * Ordering: each of the three calls is enqueued on hip_stream (NULL = the default stream), ordered after what was enqueued there before
 * (a frame that still reads the old values) and before what comes after (the next query or frame, which sees the new values).
 * Not stale: none of them makes the tree stale; all of them work on a stale tree and before vkrt_accel_build; like
 * vkrt_scene_set_material_alpha the next query or frame on that stream sees the new values without a refit.  The one exception is the
 * dissolve rule of vkrt_scene_update_materials below.  A refused call changes nothing; the first failing check of a call's list wins.
 * Tables, sizes and counts are those of vkrt_scene_create: the number of lights, materials and textures, every texture's size, is_srgb
 * and place in the pools are fixed.  While none of these entry points is called the library launches what it launched before.
 *
 * vkrt_scene_update_lights: new records for lights [first, first+count), taken as given exactly as at vkrt_scene_create, which does not
 * inspect them; lightsCount of the frame calls stays the caller's, within [0, light_count].
 *   VKRT_MEMORY_HOST    the array is copied before return: the 32-B records travel as kernel arguments; nothing is staged and the call
 *                       does not wait for the stream.
 *   VKRT_MEMORY_DEVICE  the array is device memory on the scene's device, 16-byte aligned, valid until the stream has passed the call;
 *                       the call is one stream-ordered device copy, with no allocation and no host synchronisation.
 * Refused with VKRT_ERR_INVALID_ARGUMENT, in this order: a NULL update; struct_size < sizeof(vkrt_light_update); a memory value that is
 * neither VKRT_MEMORY_HOST nor VKRT_MEMORY_DEVICE; a NULL scene; a range outside the scene's lights; (count > 0) NULL lights; (device
 * memory) lights that is not 16-byte aligned.  Then count == 0: VKRT_OK with nothing enqueued.  Then, without a device:
 * VKRT_ERR_NO_DEVICE. */
typedef struct vkrt_light_update {
  uint32_t struct_size;     /* sizeof(vkrt_light_update) */
  uint32_t first, count;
  uint32_t memory;          /* vkrt_memory */
  const GltfLight* lights;  /* [count], entry k = light first + k */
} vkrt_light_update;
int vkrt_scene_update_lights(vkrt_scene* scene, const vkrt_light_update* update, void* hip_stream);
/* vkrt_scene_update_materials: new materials [first, first+count) from a host array, which may be reused on return: both device records
 * of each material are re-made by the code that makes them at vkrt_scene_create and travel as kernel arguments (192 B per material,
 * chunked); nothing is staged and the call does not wait for the stream.  The records are bit for bit what vkrt_scene_create packs for a
 * scene created with these materials.  The alpha mode and cutoff of a material are kept: they belong to
 * vkrt_scene_set_material_alpha.  Texture indices may change freely among the scene's textures.
 * Refused, in this order: VKRT_ERR_INVALID_ARGUMENT for a NULL array with count > 0; for a texture index >= texture_count in a scene
 * that has textures (the rule of vkrt_scene_create); for a NULL scene; for a range outside the scene's materials; VKRT_ERR_UNSUPPORTED
 * for a reference to a texture with a side above 32768.  Then count == 0: VKRT_OK.  Then, without a device: VKRT_ERR_NO_DEVICE.
 * Dissolve: the any-hit dissolve stage (VKRT_OPT_ANYHIT_DISSOLVE) reads pbrBaseColorFactor[3] from the live record, so changing it among
 * values < 1 needs nothing; but the builders flag the triangles of a material with alpha < 1 at build time.  When the scene's last
 * vkrt_accel_build ran with VKRT_OPT_ANYHIT_DISSOLVE = 1 and after the update some material has alpha < 1 that did not have alpha < 1 at
 * that build, the tree needs a rebuild, not only a refit: until the next vkrt_accel_build every call that needs a built tree, and
 * vkrt_accel_refit, return VKRT_ERR_NOT_BUILT with a message naming vkrt_scene_update_materials.  The opposite direction (< 1 becoming
 * >= 1) needs nothing: a flagged triangle with alpha >= 1 is never ignored. */
int vkrt_scene_update_materials(vkrt_scene* scene, uint32_t first, uint32_t count, const GltfPBRMaterial* materials, void* hip_stream);
/* vkrt_scene_update_texture: replaces the whole image of one texture; width and height must equal the texture's (sub-rectangles,
 * resizing and adding textures are out of scope).  After the call, in stream order, level 0 in the RGBA8 pool, the texture's footprint
 * records (when the scene has that pool) and every mip level behind level 0 hold bit for bit what vkrt_scene_create packs from the new
 * texels: the scene renders, samples (vkrt_hit_surface, the alpha test, the G-buffer's implicit-LOD taps) and reads back exactly like a
 * scene created with that image.  The mip levels are vkCmdBlitImage's with VK_FILTER_LINEAR, level by level, as at vkrt_scene_create; the
 * 8-bit sRGB codes come from a table of thresholds the host derived from its own encode function at vkrt_scene_create, so that the device
 * never evaluates a curve whose last bit could differ.
 *   VKRT_MEMORY_DEVICE  rgba8 is device memory on the scene's device, 16-byte aligned, valid until the stream has passed the call; no
 *                       allocation, no host synchronisation, at most 1 + VKRT_MAX_MIPS (16) kernel launches.
 *   VKRT_MEMORY_HOST    the texels are staged through the scene's staging buffer, the same kernels run, and the call waits for the
 *                       stream before it returns, like a host-sourced vkrt_scene_update_vertices.
 * Refused with VKRT_ERR_INVALID_ARGUMENT, in this order: a NULL update; struct_size < sizeof(vkrt_texture_update); a memory value that
 * is neither of the two; a NULL scene; a texture index out of range (always, in a scene without textures); a width or height that is
 * not the texture's; NULL rgba8; (device memory) rgba8 that is not 16-byte aligned.  Then, without a device: VKRT_ERR_NO_DEVICE. */
typedef struct vkrt_texture_update {
  uint32_t struct_size;  /* sizeof(vkrt_texture_update) */
  uint32_t texture;
  uint32_t width, height;
  uint32_t memory;       /* vkrt_memory */
  const uint8_t* rgba8;  /* width*height RGBA8 texels, row-major, top row first */
} vkrt_texture_update;
int vkrt_scene_update_texture(vkrt_scene* scene, const vkrt_texture_update* update, void* hip_stream);

/* ---- path trace (replaces HelloVulkan::pathtrace :1423-1448 = one
 *      vkCmdTraceRaysKHR over raytrace.rgen/.rchit/.rmiss/raytraceShadow.rmiss) ---- */
uint32_t vkrt_shard_rows(const vkrt_shard* shard); /* rows of the shard's buffer */
/* Sizes the per-scene working set (path-record streams of the wavefront pipeline, internal streams and events) for
 * launches of this shard geometry, like the reference allocates its offscreen images at start-up and on resize
 * (createOffscreenRender, hello_vulkan.cpp:637-665).  After vkrt_reserve a vkrt_pathtrace of the same or a smaller
 * shard never allocates and never synchronises with the host.  Without it the first launch (and any launch larger
 * than every earlier one) grows the working set lazily: one hipStreamSynchronize + hipMalloc inside that call. */
int vkrt_reserve(vkrt_scene* scene, const vkrt_shard* shard, void* hip_stream);
/* The same for a caller that knows how many frames it hands to one vkrt_pathtrace_frames call (ABI 4).  The working set holds one
 * set of path-record streams (544 B per pixel of the shard) and a 16-B sample-state record per pixel (VKRT_OPT_WF_SAMPLE_SYNC) per frame
 * the library keeps in flight inside a call, plus a 16-B staging plane per pixel and frame in flight: frames_per_call = 1 (a client of vkrt_pathtrace only) sizes it for ONE set -- 1.1 GB at
 * 1920x1080, 4.5 GB at 3840x2160 --, frames_per_call >= VKRT_OPT_WF_FRAMES_IN_FLIGHT (default 3) for that many: 3.5 GB / 14 GB.
 * vkrt_reserve is vkrt_reserve_frames with frames_per_call = VKRT_OPT_WF_FRAMES_IN_FLIGHT, i.e. the larger figure whatever the
 * client goes on to call.  The working set only grows (a later, larger call or reservation re-allocates it once); it is released by
 * vkrt_scene_destroy.  Texture memory, for the record: vkrt_scene_create keeps, beside the RGBA8 pool with its mip chain (4/3 of the
 * texel bytes), a footprint pool of 16 B per level-0 texel -- 4x the level-0 texel bytes -- so that a bilinear tap of the path tracer
 * is one load; it is built while it stays under 2 GiB (above that, and with the test hook VKRT_TEX_QUADS=0 in the environment, taps
 * gather their four texels from the RGBA8 pool: same values, ~9 % slower hit shading). */
int vkrt_reserve_frames(vkrt_scene* scene, const vkrt_shard* shard, uint32_t frames_per_call, void* hip_stream);
/* Asynchronous like the command-buffer recording it replaces: returns after enqueueing.  All work is ordered after what
 * was enqueued on `hip_stream` before the call and complete before anything enqueued on it afterwards (the library may
 * run parts of a frame on internal streams that fork from and join `hip_stream` through events).  No host
 * synchronisation happens inside the call once the working set is large enough (vkrt_reserve above).  pc->frame > 0 blends into the image the caller kept from the previous
 * frame (raytrace.rgen:136-145), so the image buffer is caller-owned and persistent.  Calls on one scene handle must
 * be serialised by the caller.  A shard without rows (more shards than strips) is a no-op and may pass NULL buffers. */
int vkrt_pathtrace(vkrt_scene* scene, const PushConstantRay* pc, const GlobalUniforms* cam,
                   const vkrt_trace_opts* opts, const vkrt_shard* shard,
                   float* rgba32f_device, void* hip_stream);

/* n_frames progressive frames of an unchanged camera in one call: the reference's render loop with the camera at rest
 * (main.cpp:503-508: updateFrame() -> pathtrace(), frame after frame; hello_vulkan.cpp:1501-1521 advances pcRay.frame, raytrace.rgen:136-145
 * blends frame f into the image with weight 1 / (f + 1)).  Frame i of the call (0 <= i < n_frames) is traced with pc->frame + i and
 * opts->seed + i (opts->seed with VKRT_TRACE_SAME_SEED_EVERY_FRAME); the image afterwards is bit for bit what n_frames vkrt_pathtrace calls
 * with those values would have left.  Inside the call consecutive frames run at the same time (VKRT_OPT_WF_FRAMES_IN_FLIGHT): the
 * launches of one frame fill the tails of the other's, which a sequence of single-frame calls -- each complete before the next
 * begins -- cannot do.  Same asynchrony, ordering and
 * shard rules as vkrt_pathtrace (which is this call with n_frames = 1); vkrt_counters and vkrt_last_trace_ms cover the whole call.
 * Working set: vkrt_reserve_frames(scene, shard, n_frames, stream) sizes it for such calls (vkrt_reserve: for whatever the current
 * options keep in flight). */
int vkrt_pathtrace_frames(vkrt_scene* scene, const PushConstantRay* pc, const GlobalUniforms* cam,
                          const vkrt_trace_opts* opts, const vkrt_shard* shard,
                          float* rgba32f_device, uint32_t n_frames, void* hip_stream);

/* ---- hybrid mode (reference rtMode == 0; SURVEY.md 8f row 1, BASELINE config 5) --------------------- */
/* The four raster planes that raytraceHybrid.rgen reads (RtxBindings 1,3,4,6; host_device.h:51-63,
 * attachments hello_vulkan.cpp:690-734).  Caller-owned device memory, rows of the shard stacked like the
 * path-trace image. */
typedef struct vkrt_gbuffer {
  float* color;      /* rgba32f eOutImage : rgb = emission + un-shadowed direct light (frag_shader.frag:190-214), a = albedo.r */
  float* position;   /* rgba32f ePosMap   : xyz = world position, w = albedo.g; cleared to (0,0,0,1)                    */
  float* normal;     /* rgba32f eNormMap  : xyz = shading normal, w = albedo.b; cleared to (0,0,0,1)                     */
  float* roughMetal; /* 2 floats/pixel eRoughMap: roughness, metalness after the rg16f round trip                        */
} vkrt_gbuffer;
/* Replaces the raster pass HelloVulkan::rasterizeGltf (hello_vulkan.cpp:583-615, vert_shader.vert,
 * frag_shader.frag) by a primary ray cast per pixel centre evaluating the same shader math.  texture() takes
 * its LOD as in a fragment shader: dFdx / dFdy of the texture coordinate inside the pixel's 2x2 quad (the quad
 * partner evaluated on the same triangle's plane), then the Vulkan scale-factor / LOD / anisotropy formulas
 * with the reference's sampler (trilinear, maxAnisotropy 4); VKRT_OPT_GBUFFER_MIPS = 0 reads LOD 0 instead.
 * lightsCount = PushConstantRaster.lightsCount. */
int vkrt_gbuffer_raycast(vkrt_scene* scene, const float clearColor[4], int lightsCount, const GlobalUniforms* cam,
                         const vkrt_shard* shard, const vkrt_gbuffer* out, void* hip_stream);
/* Replaces HelloVulkan::raytraceRasterizedScene (hello_vulkan.cpp:1450-1473 = vkCmdTraceRaysKHR over
 * raytraceHybrid.rgen): shadow / AO / GI per PushConstantRay.useShadows/useAO/useGI, accumulated into
 * accum_rgba32f (eAccumMap; rgb = indirect light, a = visibility * (1 - ao)). */
int vkrt_hybrid_trace(vkrt_scene* scene, const PushConstantRay* pc, const GlobalUniforms* cam, const vkrt_trace_opts* opts,
                      const vkrt_shard* shard, const vkrt_gbuffer* gbuffer, float* accum_rgba32f_device, void* hip_stream);
/* ---- NRD / REBLUR front-end planes ----------------------------------------------------------
 * The raster pass also writes the denoiser's inputs (frag_shader.frag:133-136, attachments hello_vulkan.cpp:690-741) and
 * raytraceHybrid.rgen:273-281 packs the GI radiance + normalised hit distance for REBLUR (gltf.glsl:156-273, hitDistParams
 * (3, 1, 20, -25)).  The reference's NRD.Denoise call is commented out (main.cpp:566-602), so these planes have no consumer
 * there; they are offered as optional outputs so a host that enables NRD finds its inputs.  All three are plain float planes
 * holding the values the Vulkan attachments would store (rgb10_a2 UNORM / r16f / rgba16f quantisation applied). */
typedef struct vkrt_nrd_planes {
  float* normalRoughness;     /* rgba32f eInNormRough: oct-encoded normal .xy, roughness, clamp(materialId / 3, 0, 1); cleared to 0   */
  float* viewZ;               /* 1 float/pixel eInViewZ: (pcRaster.viewMatrix * worldPos).z; cleared to 0                             */
  float* diffRadianceHitDist; /* rgba32f eInRadHitD: YCoCg radiance of the GI path + normalised hit distance; 0 where GI did not run */
} vkrt_nrd_planes;
/* vkrt_gbuffer_raycast that also fills nrd->normalRoughness / viewZ and clears nrd->diffRadianceHitDist.
 * view_matrix = PushConstantRaster.viewMatrix (hello_vulkan.cpp:600), column-major 4x4. */
int vkrt_gbuffer_raycast_nrd(vkrt_scene* scene, const float clearColor[4], int lightsCount, const GlobalUniforms* cam, const float view_matrix[16],
                             const vkrt_shard* shard, const vkrt_gbuffer* out, const vkrt_nrd_planes* nrd, void* hip_stream);
/* vkrt_gbuffer_raycast (view_matrix and nrd both NULL) or vkrt_gbuffer_raycast_nrd (both given) that also writes one vkrt_hit per
 * pixel into hits, a 16-byte aligned device array of rows x full_width records stacked like the planes: a visibility buffer (picking,
 * vkrt_hit_surface on pixels) and the input of vkrt_hit_motion.  At a pixel with geometry the record is what vkrt_intersect writes for
 * the primary hit: t of the G-buffer's own ray (origin = the camera, tmin 0.001, tmax 10000), u, v, and the ids, `triangle` without
 * the dissolve stage's flag; at a background pixel it is the miss record with t = 10000.  The planes are, bit for bit, those of the
 * call without hits.  Refused with VKRT_ERR_INVALID_ARGUMENT besides what those calls refuse: only one of view_matrix and nrd, hits
 * NULL or misaligned.  Came after ABI version 4 without changing it: detect it by symbol. */
int vkrt_gbuffer_raycast_hits(vkrt_scene* scene, const float clearColor[4], int lightsCount, const GlobalUniforms* cam, const float view_matrix[16],
                              const vkrt_shard* shard, const vkrt_gbuffer* out, const vkrt_nrd_planes* nrd, vkrt_hit* hits, void* hip_stream);
/* vkrt_hybrid_trace that also writes nrd->diffRadianceHitDist where PushConstantRay.useGI ran (reads nrd->viewZ). */
int vkrt_hybrid_trace_nrd(vkrt_scene* scene, const PushConstantRay* pc, const GlobalUniforms* cam, const vkrt_trace_opts* opts,
                          const vkrt_shard* shard, const vkrt_gbuffer* gbuffer, const vkrt_nrd_planes* nrd, float* accum_rgba32f_device,
                          void* hip_stream);
/* Replaces drawPost's fragment stage (post.frag:36-58): hybrid composite main.rgb * rt.a + rt.rgb (rtMode 0) or
 * pass-through (rtMode 1), then gamma 1/2.2 on all four channels.  n_pixels rgba32f device buffers.
 * NaN texels are part of the result, as in the reference: post.frag:57 applies pow(x, 1/2.2) to whatever the composite holds
 * and pow of a negative base is undefined in GLSL (NaN here, on the oracle and on the GPUs the reference targets).  The
 * hybrid accumulation plane does go negative -- raytrace.rchit's specular branch returns negative weights when
 * dot(N, L) < 0 and raytraceHybrid.rgen adds the GI radiance unclamped -- so a hybrid frame shows them:
 * 898 of the 46,080 texels sampled by the BASELINE config-5 test (1920x1080 atrium, shadows + AO + GI depth 8, two frames),
 * at the same texels on both sides (tests/test_gpu_configs.py asserts the coincidence).  The path-tracing mode's image
 * (rtMode 1) is not affected in practice: raytrace.rgen clamps every contribution with min(., 10) but sums can still be
 * negative; callers that display the plane should treat NaN as black, like a UNORM swapchain write does. */
int vkrt_post(int device, const PushConstantPost* pc, uint32_t n_pixels, const float* main_rgba32f, const float* rt_rgba32f,
              float* out_rgba32f, void* hip_stream);

/* ---- diffuse denoiser (stands where the reference's commented-out NRD.Denoise sits, main.cpp:565-602) ---------------------
 * A spatio-temporal variance-guided filter (SVGF, Schied et al. 2017) of the hybrid GI term: it reads the planes that
 * vkrt_gbuffer_raycast_nrd and vkrt_hybrid_trace_nrd write (nrd->viewZ, nrd->diffRadianceHitDist) and the G-buffer, and writes
 * the filtered GI radiance.  Three stages on the caller's stream -- temporal reprojection + moments, variance, `atrous_iterations`
 * edge-avoiding a-trous passes -- with no host synchronisation and no allocation inside the call; the history lives in the handle.
 * Whole-frame planes only (no vkrt_shard): a host that renders strips denoises the gathered frame.  Same inputs and history give
 * bitwise the same output (no atomics).  These entry points came after ABI version 4 without changing it: detect them by symbol.
 * The handle is bound to one device and one width x height; every plane passed to it has exactly that many pixels. */
typedef struct vkrt_denoiser vkrt_denoiser;
typedef struct vkrt_denoise_settings {
  uint32_t struct_size;       /* sizeof(vkrt_denoise_settings) */
  int32_t  atrous_iterations; /* 0..5, default 5 (0 = temporal stage only) */
  int32_t  max_history;       /* 1..255, default 32 (1 = no temporal reuse) */
} vkrt_denoise_settings;
/* Allocates everything the filter keeps (128 B per pixel); VKRT_ERR_NO_DEVICE without a HIP device. */
int  vkrt_denoiser_create(int device, uint32_t width, uint32_t height, vkrt_denoiser** out);
void vkrt_denoiser_destroy(vkrt_denoiser* dn);
/* Drops the history: the next call behaves like the first (a camera cut; the reference's resetFrame). */
int  vkrt_denoiser_reset(vkrt_denoiser* dn);
/* cam = the camera the G-buffer was cast with (its viewProj is kept for the next call's reprojection); settings NULL = defaults.
 * out_rgba32f: W*H rgba32f; .xyz is written at pixels with geometry (G-buffer position or normal non-zero), everything else --
 * .w and the background -- is left untouched, so a host can denoise into a copy of the accumulation plane and hand it to vkrt_post
 * unchanged.  Refused with VKRT_ERR_INVALID_ARGUMENT: struct_size too small, settings out of range, a NULL handle, camera,
 * G-buffer plane, nrd->viewZ, nrd->diffRadianceHitDist or output.  A NaN radiance sample counts as black (the decode clamps with
 * fmaxf(., 0)) and never reaches the history; an infinite one is the caller's error. */
int  vkrt_denoise_diffuse(vkrt_denoiser* dn, const vkrt_denoise_settings* settings, const GlobalUniforms* cam, const vkrt_gbuffer* gbuffer,
                          const vkrt_nrd_planes* nrd, float* out_rgba32f, void* hip_stream);
/* vkrt_denoise_diffuse for moving and deforming geometry: one more W*H rgba32f plane, prev_position_rgba32f (16-byte aligned), says
 * where each pixel's surface point was at the previous call -- what vkrt_hit_motion writes as `previous` for the records of
 * vkrt_gbuffer_raycast_hits.  In the temporal stage Xp = prev.xyz takes the place of the pixel's position in two places: the
 * projection under the previous call's viewProj, and the plane test d = (previous position plane)[tap] - Xp.  The projection under the
 * current viewProj, the normal test (the current normal against the stored previous one), the tolerance, the bilinear weights and
 * everything after the taps are those of the plain call; with prev == position at every pixel (w = 1) the two calls agree bit for bit.
 * A pixel with geometry whose prev.w == 0 takes no history (a surface that did not exist); a non-finite Xp takes none either.  At
 * pixels without geometry the plane is not read.  The two calls may be mixed freely on one handle.  Known limit: the normal test
 * admits about 25 degrees of rotation per frame (N . N_prev >= 0.9); there is no previous-normal plane.  Refused as the plain call,
 * and a NULL or misaligned prev_position_rgba32f.  Came after ABI version 4 without changing it: detect it by symbol. */
int  vkrt_denoise_diffuse_motion(vkrt_denoiser* dn, const vkrt_denoise_settings* settings, const GlobalUniforms* cam, const vkrt_gbuffer* gbuffer,
                                 const vkrt_nrd_planes* nrd, const float* prev_position_rgba32f, float* out_rgba32f, void* hip_stream);

/* ---- counters / timing ------------------------------------------------------------ */
int vkrt_counters_reset(vkrt_scene* scene, void* hip_stream);
int vkrt_counters_read(vkrt_scene* scene, vkrt_counters* out); /* synchronises the device */
/* Device time of the most recent vkrt_pathtrace kernel on this scene in milliseconds,
 * from HIP events recorded on the launch stream (synchronises on the stop event). */
int vkrt_last_trace_ms(vkrt_scene* scene, float* ms);
/* Breakdown of the most recent vkrt_pathtrace: whole frame, and (with VKRT_TRACE_TIME_KERNELS, or always
 * in megakernel mode) the summed duration and number of launches of the traversal kernel -- the dominant
 * kernel of the path (k_wf_traverse / k_pathtrace). */
typedef struct vkrt_trace_timing {
  float    total_ms;
  float    traverse_ms;
  uint32_t traverse_launches;
  uint32_t mode;            /* 1 wavefront pipeline, 0 megakernel (VKRT_MODE=mega) */
  float    shade_ms;        /* ABI 4, with VKRT_TRACE_TIME_KERNELS: summed time between the end of a traversal launch and the start of the
                               next one of the same frame = the k_wf_shade launch between them (and the launch gap on either side) */
  uint32_t shade_launches;  /* the shade launches shade_ms covers (the last one of each frame is not bracketed and not counted) */
} vkrt_trace_timing;
int vkrt_last_trace_timing(vkrt_scene* scene, vkrt_trace_timing* out);

/* ---- test hooks (used by tests/ to compare single pieces with the oracle) ---------- */
/* Structural check of the built acceleration structure (downloads it; host walk).  A tree is sound when every triangle slot
 * is referenced by exactly one leaf, every node is reached exactly once from the root, every instanced triangle owns at least one
 * slot, and every triangle is covered by the boxes above its slots: with one slot, its three vertices lie inside the decoded box
 * of each of that slot's ancestors (the quantised boxes are conservative); with several (VKRT_OPT_SPLIT_BUDGET), every point of a
 * 45-point barycentric lattice on the triangle (vertices, edges, interior) lies inside ALL ancestor boxes of at least one of its
 * slots -- the slots together must leave no part of the triangle unreachable.  Any builder, both layouts. */
typedef struct vkrt_accel_check {
  uint64_t nodes_reached;        /* == vkrt_accel_info.node_count */
  uint64_t triangles_referenced; /* leaf references in total */
  uint64_t triangles_missing;    /* slots no leaf references */
  uint64_t triangles_repeated;   /* references beyond the first of a slot */
  uint64_t box_violations;       /* single-slot triangles: (triangle, ancestor slot) pairs with a vertex outside the slot's box */
  uint64_t bad_references;       /* child / triangle indices out of range, nodes reached twice */
  uint32_t max_depth;            /* nodes on the longest root-to-leaf path */
  uint32_t layout;               /* 1 = 8-wide compressed, 0 = BVH2 */
  uint64_t triangles_uncovered;  /* multi-slot triangles with a lattice point that no slot's chain of boxes contains; triangles without any slot */
  uint64_t triangles_split;      /* triangles that own more than one slot */
} vkrt_accel_check;
int vkrt_debug_check_accel(vkrt_scene* scene, vkrt_accel_check* out);
/* The installed tree exactly as the kernels read it (synchronises the device; a test hook like the other vkrt_debug_* calls, added
 * without a struct change, so VKRT_ABI_VERSION stays 4): the node array (nodes_bytes == vkrt_accel_info.node_bytes; wide8: 80-B nodes,
 * bvh_host.h; BVH2: 64-B nodes, device_scene.h -- a device-built BVH2 array also holds radix nodes no walk from the root reaches), the
 * 48-B triangle records in slot order (tris_bytes == triangle_bytes) and the BVH2 root reference (wide8: 0, the root node; a leaf
 * reference for a BVH2 whose root is a leaf; VKRT_TRAV_DONE for an empty scene).  Other byte counts or a NULL pointer:
 * VKRT_ERR_INVALID_ARGUMENT; no tree, or a stale one: VKRT_ERR_NOT_BUILT. */
int vkrt_debug_read_accel(vkrt_scene* scene, void* nodes, uint64_t nodes_bytes, void* tris, uint64_t tris_bytes, int32_t* root_ref);
/* The 8-wide tree's node-mask table as the query kernels read it (synchronises the device): 8 B per node of the node array
 * (bytes == vkrt_accel_info.node_bytes / 80 * 8), byte s of node k = the OR of the instance masks of every triangle reference under
 * child slot s (0 for an empty slot).  Other byte counts, a NULL pointer or a BVH2 tree: VKRT_ERR_INVALID_ARGUMENT; no tree:
 * VKRT_ERR_NOT_BUILT (a stale tree is read as it stands: a refit leaves the table valid). */
int vkrt_debug_read_node_masks(vkrt_scene* scene, void* out, uint64_t bytes);
/* Which triangle sits in every slot of the installed tree (synchronises the device; a test hook like the other vkrt_debug_* calls, no
 * kernel of its own): out[k] = the flattened triangle id of slot k -- instances in node order, each instance's triangles in index
 * order; the id word of the slot's 48-B record without its non-opaque flag -- for the slots of vkrt_debug_read_accel's triangle
 * records, in that order, either layout, any builder (bytes == vkrt_accel_info.triangle_bytes / 48 * 4).  A triangle with several
 * references (VKRT_OPT_SPLIT_BUDGET) appears once per slot it owns.  Other byte counts or a NULL pointer:
 * VKRT_ERR_INVALID_ARGUMENT; no tree, or a stale one: VKRT_ERR_NOT_BUILT. */
int vkrt_debug_read_triangle_ids(vkrt_scene* scene, uint32_t* out, uint64_t bytes);
/* The references triangle pre-splitting (VKRT_OPT_SPLIT_BUDGET) makes of the scene for a budget of split_percent % (1..100) extra
 * references (synchronises the device; a test hook like the other vkrt_debug_* calls, no kernel of its own, no struct change, so
 * VKRT_ABI_VERSION stays 4): the flattening and the pre-split stage of the device builders, the very functions a PLOC or LBVH build runs,
 * on the scene's current arrays with its current VKRT_OPT_WATERTIGHT, and nothing after them.  With T = instanced triangles:
 * prio[T] (or NULL) = the split priority of every flattened triangle, scale[1] (or NULL) = D, the splits per unit of priority -- triangle g
 * is cut min((unsigned)(D * prio[g]), 255) times; both are zeros when T * split_percent / 100 is 0 or T < 2 --, *ref_count = the
 * references, ref_tri[r] = the flattened triangle of reference r and ref_box[6 r .. 6 r + 5] = its box (lo3, hi3), in emission order: the
 * pieces of a triangle are contiguous and the triangles appear in id order.  When nothing was split: the identity list with the
 * whole-triangle boxes.  Needs no tree and does not touch the installed one.  capacity (in references) < T + T * split_percent / 100, a
 * percent outside 1..100, or a NULL scene, ref_tri, ref_box or ref_count: VKRT_ERR_INVALID_ARGUMENT; without a device:
 * VKRT_ERR_NO_DEVICE. */
int vkrt_debug_split_references(vkrt_scene* scene, uint32_t split_percent /* 1..100 */,
                                float* prio /* [T] or NULL */, float* scale /* [1] = D, or NULL */,
                                uint32_t* ref_tri, float* ref_box /* 6 per reference */, uint64_t capacity,
                                uint32_t* ref_count);
/* The live attributes of vertices [first, first+count) as the kernels read them (synchronises the device; a test hook like the other
 * vkrt_debug_* calls, no kernel of its own), into host arrays laid out as at vkrt_scene_create: positions vec3 (from the position
 * array the builders and the refit read), normals vec3, tangents vec4 and texcoords0 vec2 (unpacked from the 48-B shading records).
 * A NULL array is skipped.  Needs no tree.  A NULL scene, a range outside the scene's vertices or all four arrays NULL:
 * VKRT_ERR_INVALID_ARGUMENT. */
int vkrt_debug_read_vertices(vkrt_scene* scene, uint32_t first, uint32_t count, float* positions, float* normals, float* tangents, float* texcoords0);
/* The instance records of nodes [first, first+count) exactly as the kernels read them (synchronises the device; a test hook like the
 * other vkrt_debug_* calls, no kernel of its own), 96 B per node: float o2w[12], the object->world rows, row-major 3x4; float w2o[9],
 * the row-major inverse of their 3x3; int32 primMesh; uint32 visibility word (bits 0-7 mask, bits 8-15 vkrt_instance_flags, bit 16 set
 * when the 3x3 has a negative determinant); int32 pad = 0.  Needs no tree.  A NULL scene or out, a range outside the scene's nodes or
 * bytes != 96 * count: VKRT_ERR_INVALID_ARGUMENT. */
int vkrt_debug_read_instances(vkrt_scene* scene, uint32_t first, uint32_t count, void* out, uint64_t bytes);
/* The light records [first, first+count) (32 B each, GltfLight), the material records [first, first+count) (192 B each: the 128-B record
 * of the queries and the G-buffer -- GltfPBRMaterial, pad, alpha mode, alpha cutoff, four 16-B texture references --, then the 64-B record
 * of the hit shader) and one level of one texture, exactly as the kernels read them (each synchronises the device; test hooks like the
 * other vkrt_debug_* calls, no kernel of their own).  vkrt_debug_read_texture: texels = the level's RGBA8 texels, max(1, width >> level)
 * x max(1, height >> level) of them; for level 0, when quads != NULL, also the texture's footprint records, 16 B per texel (the texels
 * (x, y) (x+1, y) (x, y+1) (x+1, y+1), wrapped): VKRT_ERR_UNSUPPORTED when the scene has no footprint pool.  None needs a tree.  A NULL
 * scene or out / texels, a range, texture or level outside the scene's, quads with a level above 0, or a byte count that is not the
 * records': VKRT_ERR_INVALID_ARGUMENT. */
int vkrt_debug_read_lights(vkrt_scene* scene, uint32_t first, uint32_t count, void* out, uint64_t bytes);
int vkrt_debug_read_materials(vkrt_scene* scene, uint32_t first, uint32_t count, void* out, uint64_t bytes);
int vkrt_debug_read_texture(vkrt_scene* scene, uint32_t texture, uint32_t level, void* texels, uint64_t texel_bytes, void* quads, uint64_t quad_bytes);
/* The work of vkrt_closest_point on n queries of a HOST array (synchronises the device; a test hook like the other vkrt_debug_* calls):
 * out[0] = nodes visited, out[1] = triangle records tested, summed over the queries, by an instrumented instantiation of the same
 * walk.  opts and the order of errors as vkrt_closest_point; a NULL out: VKRT_ERR_INVALID_ARGUMENT. */
int vkrt_debug_closest_point_work(vkrt_scene* scene, const vkrt_point_query* host_queries, uint32_t n, const vkrt_query_opts* opts,
                                  uint64_t out[2]);
/* Closest-hit query for n rays: o,d = vec3[n] host arrays; tmin/tmax scalars.
 * Writes t,u,v (float[n]) and the flattened triangle id gid (int32[n], -1 = miss). */
int vkrt_debug_trace_rays(vkrt_scene* scene, uint32_t n, const float* origins,
                          const float* directions, float tmin, float tmax, int any_hit,
                          float* t, float* u, float* v, int32_t* gid);
/* Evaluate a device math primitive elementwise (op: 0 sin, 1 cos, 2 sqrt, 3 a/b,
 * 4 pow5, 5 1/sqrt-normalise x of (a,b,0)); host arrays in/out. */
int vkrt_debug_eval_math(int device, int op, uint32_t n, const float* a, const float* b,
                         float* out);
/* Evaluate the BRDF tail of the hit shader (lobe draw, next-event estimation, cosine / GGX sample, payload outputs) on n records of
 * HOST arrays (synchronises the device; a test hook like vkrt_debug_eval_math): the device builds the shading inputs the hit shader's
 * front half hands over for an untextured material and runs the functions the frame kernels run.  Words marked (bits) are integers
 * stored in the float's bits.
 *   in : 40 floats per record:
 *     [0:3] worldPos [3:6] worldNrm [6:9] tangent [9:12] binormal [12:15] worldRayDir
 *     [15:19] baseColorFactor [19] metallic [20] roughness [21:24] emissive
 *     [24:27] light.position [27:30] light.color [30] intensity [31] light.type (bits)
 *     [32] seed (bits) [33] depth (bits) [34] isSpecular (bits) [35] lightsCount (bits) [36:40] pad
 *   out: 20 floats per record:
 *     [0:3] hitValue [3:6] rayOrigin [6:9] rayDirection [9:12] weight [12] isSpecular (0.0 or 1.0)
 *     [13] lightDist [14:17] shadowRayDir [17] seed (bits) [18:20] pad (0)
 * Every one of the record's lightsCount lights is the record's light, so the index the shader draws always finds it; lightsCount is
 * 1 to 16, any other value in any record: VKRT_ERR_INVALID_ARGUMENT.  The factors are taken as given (no range check: the clamps are
 * the shader's).  NULL in or out with n > 0: VKRT_ERR_INVALID_ARGUMENT; n == 0: VKRT_OK. */
int vkrt_debug_eval_shade(int device, uint32_t n, const float* in, float* out);

#ifdef __cplusplus
}
#endif
#endif /* VKRT_H */
