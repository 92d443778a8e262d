"""ctypes mirror of include/vkrt.h and include/vkrt_host_device.h.

Harness-side only: the product is the C-ABI library (csrc/ -> libvkrt.so); this module
declares its structs and prototypes so tests and bench.py can call it.  Layout sizes
are asserted against the reference contract (reference: shaders/host_device.h:68-137,
SURVEY.md Appendix B).
"""
import ctypes as C

c_f = C.c_float
c_i = C.c_int32
c_u = C.c_uint32
c_u64 = C.c_uint64


class Mat4(C.Structure):
    _fields_ = [("m", c_f * 16)]


class GlobalUniforms(C.Structure):
    _fields_ = [("viewProj", Mat4), ("viewInverse", Mat4), ("projInverse", Mat4)]


class PushConstantRay(C.Structure):
    _fields_ = [
        ("clearColor", c_f * 4),
        ("frame", c_i),
        ("lightsCount", c_i),
        ("samples", c_i),
        ("depth", c_i),
        ("useShadows", c_i),
        ("useAO", c_i),
        ("useGI", c_i),
    ]


class PrimMeshInfo(C.Structure):
    _fields_ = [("indexOffset", c_u), ("vertexOffset", c_u), ("materialIndex", c_i)]


class GltfPBRMaterial(C.Structure):
    _fields_ = [
        ("pbrBaseColorFactor", c_f * 4),
        ("pbrBaseColorTexture", c_i),
        ("metallicFactor", c_f),
        ("roughnessFactor", c_f),
        ("metallicRoughnessTexture", c_i),
        ("normalTexture", c_i),
        ("emissiveFactor", c_f * 3),
        ("emissiveTexture", c_i),
    ]


class GltfLight(C.Structure):
    _fields_ = [("position", c_f * 3), ("color", c_f * 3), ("intensity", c_f), ("type", c_i)]


class PrimMesh(C.Structure):
    _fields_ = [
        ("firstIndex", c_u),
        ("indexCount", c_u),
        ("vertexOffset", c_u),
        ("vertexCount", c_u),
        ("materialIndex", c_i),
    ]


class Node(C.Structure):
    _fields_ = [("worldMatrix", c_f * 16), ("primMesh", c_i)]


class Texture(C.Structure):
    _fields_ = [("width", c_u), ("height", c_u), ("rgba8", C.c_void_p), ("is_srgb", c_i)]


class SceneDesc(C.Structure):
    _fields_ = [
        ("struct_size", c_u),
        ("vertex_count", c_u),
        ("positions", C.c_void_p),
        ("normals", C.c_void_p),
        ("tangents", C.c_void_p),
        ("texcoords0", C.c_void_p),
        ("indices", C.c_void_p),
        ("index_count", c_u),
        ("prim_mesh_count", c_u),
        ("prim_meshes", C.c_void_p),
        ("materials", C.c_void_p),
        ("material_count", c_u),
        ("light_count", c_u),
        ("lights", C.c_void_p),
        ("nodes", C.c_void_p),
        ("node_count", c_u),
        ("texture_count", c_u),
        ("textures", C.c_void_p),
    ]


class Shard(C.Structure):
    _fields_ = [
        ("full_width", c_u),
        ("full_height", c_u),
        ("strip_rows", c_u),
        ("shard_count", c_u),
        ("shard_index", c_u),
    ]


class AccelCheck(C.Structure):
    _fields_ = [("nodes_reached", C.c_uint64), ("triangles_referenced", C.c_uint64), ("triangles_missing", C.c_uint64),
                ("triangles_repeated", C.c_uint64), ("box_violations", C.c_uint64), ("bad_references", C.c_uint64),
                ("max_depth", c_u), ("layout", c_u), ("triangles_uncovered", C.c_uint64), ("triangles_split", C.c_uint64)]


class TraceOpts(C.Structure):
    _fields_ = [("seed", c_u), ("flags", c_u)]


class Counters(C.Structure):
    _fields_ = [
        ("rays_closest", c_u64),
        ("rays_shadow", c_u64),
        ("hits", c_u64),
        ("diffuse_hits", c_u64),
        ("tex_taps", c_u64),
        ("pixels", c_u64),
        ("nodes_visited", c_u64),
        ("tris_tested", c_u64),
        ("wave_node_steps", c_u64),
        ("wave_tri_steps", c_u64),
        ("traversal_faults", c_u64),
        ("pair_records", c_u64),
    ]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class AccelInfo(C.Structure):
    _fields_ = [
        ("triangle_count", c_u),
        ("node_count", c_u),
        ("max_depth", c_u),
        ("build_flags", c_u),
        ("sah_cost", c_f),
        ("build_ms", c_f),
        ("node_bytes", c_u64),
        ("triangle_bytes", c_u64),
        ("reference_count", c_u),
        ("reserved", c_u),
    ]


class Gbuffer(C.Structure):
    _fields_ = [("color", C.c_void_p), ("position", C.c_void_p), ("normal", C.c_void_p), ("roughMetal", C.c_void_p)]


class NrdPlanes(C.Structure):
    _fields_ = [("normalRoughness", C.c_void_p), ("viewZ", C.c_void_p), ("diffRadianceHitDist", C.c_void_p)]


class PushConstantPost(C.Structure):
    _fields_ = [("aspectRatio", c_f), ("rtMode", c_i), ("viewAccumulated", c_i), ("useGI", c_i)]


class DenoiseSettings(C.Structure):
    _fields_ = [("struct_size", c_u), ("atrous_iterations", c_i), ("max_history", c_i)]


class TraceTiming(C.Structure):
    _fields_ = [("total_ms", c_f), ("traverse_ms", c_f), ("traverse_launches", c_u), ("mode", c_u), ("shade_ms", c_f), ("shade_launches", c_u)]


# ray queries (vkrt_intersect / vkrt_occluded): records of device arrays, 32 B each
class Ray(C.Structure):
    _fields_ = [("origin", c_f * 3), ("tmin", c_f), ("direction", c_f * 3), ("tmax", c_f)]


class Hit(C.Structure):
    _fields_ = [("t", c_f), ("u", c_f), ("v", c_f), ("instance", C.c_int32), ("primitive", C.c_int32), ("prim_mesh", C.c_int32),
                ("triangle", C.c_int32), ("material", C.c_int32)]


# shading inputs at hit records (vkrt_hit_surface): records of a device array, 128 B each = eight float4
class Surface(C.Structure):
    _fields_ = [("position", c_f * 3), ("texcoord_u", c_f), ("geometric_normal", c_f * 3), ("texcoord_v", c_f), ("normal", c_f * 3), ("alpha", c_f),
                ("shading_normal", c_f * 3), ("metallic", c_f), ("tangent", c_f * 3), ("roughness", c_f), ("binormal", c_f * 3), ("material", C.c_int32),
                ("base_color", c_f * 3), ("valid", C.c_int32), ("emission", c_f * 3), ("reserved", c_u)]


# instance visibility and query options (vkrt_scene_set_instance_visibility, vkrt_intersect_ex / vkrt_occluded_ex)
class InstanceVisibility(C.Structure):
    _fields_ = [("mask", C.c_uint8), ("flags", C.c_uint8), ("reserved", C.c_uint16)]


# alpha-tested materials (vkrt_scene_set_material_alpha)
class MaterialAlpha(C.Structure):
    _fields_ = [("mode", c_u), ("cutoff", c_f)]


class QueryOpts(C.Structure):
    _fields_ = [("struct_size", c_u), ("ray_flags", c_u), ("cull_mask", c_u), ("anyhit_seed", c_u)]


# closest-point queries (vkrt_closest_point): records of a device array, 16 B each
class PointQuery(C.Structure):
    _fields_ = [("point", c_f * 3), ("radius", c_f)]


# deforming meshes (vkrt_scene_update_vertices): the four arrays are host or device pointers, by `memory`
class VertexUpdate(C.Structure):
    _fields_ = [("struct_size", c_u), ("first", c_u), ("count", c_u), ("memory", c_u), ("positions", C.c_void_p), ("normals", C.c_void_p),
                ("tangents", C.c_void_p), ("texcoords0", C.c_void_p)]


# moving instances from host or device memory (vkrt_scene_update_node_transforms): the two arrays are host or device pointers, by `memory`
class NodeUpdate(C.Structure):
    _fields_ = [("struct_size", c_u), ("first", c_u), ("count", c_u), ("memory", c_u), ("world_matrices", C.c_void_p), ("node_indices", C.c_void_p)]


# skinned meshes (vkrt_scene_add_skin): joints (u16 x 4 per vertex) and weights (f32 x 4 per vertex) are host pointers
class SkinDesc(C.Structure):
    _fields_ = [("struct_size", c_u), ("first", c_u), ("count", c_u), ("joint_count", c_u), ("joints", C.c_void_p), ("weights", C.c_void_p)]


# morph targets (vkrt_scene_add_morph): host pointers to float32 [target_count][count][3], NULL for an attribute that is not morphed
VKRT_MORPH_TARGETS_MAX = 256


class MorphDesc(C.Structure):
    _fields_ = [("struct_size", c_u), ("first", c_u), ("count", c_u), ("target_count", c_u), ("position_deltas", C.c_void_p),
                ("normal_deltas", C.c_void_p), ("tangent_deltas", C.c_void_p)]


# editing a live scene (vkrt_scene_update_lights / vkrt_scene_update_texture): `lights` / `rgba8` are host or device pointers, by `memory`
class LightUpdate(C.Structure):
    _fields_ = [("struct_size", c_u), ("first", c_u), ("count", c_u), ("memory", c_u), ("lights", C.c_void_p)]


class TextureUpdate(C.Structure):
    _fields_ = [("struct_size", c_u), ("texture", c_u), ("width", c_u), ("height", c_u), ("memory", c_u), ("rgba8", C.c_void_p)]


assert C.sizeof(LightUpdate) == 24
assert C.sizeof(TextureUpdate) == 32
assert C.sizeof(VertexUpdate) == 48
assert C.sizeof(NodeUpdate) == 32
assert C.sizeof(SkinDesc) == 32
assert C.sizeof(MorphDesc) == 40
assert C.sizeof(Ray) == 32
assert C.sizeof(Hit) == 32
assert C.sizeof(Surface) == 128
assert C.sizeof(InstanceVisibility) == 4
assert C.sizeof(QueryOpts) == 16
assert C.sizeof(MaterialAlpha) == 8

# layout contract
assert C.sizeof(GlobalUniforms) == 192
assert C.sizeof(PushConstantRay) == 44
assert C.sizeof(PrimMeshInfo) == 12
assert C.sizeof(GltfPBRMaterial) == 52
assert C.sizeof(GltfLight) == 32
assert C.sizeof(PrimMesh) == 20
assert C.sizeof(Node) == 68

VKRT_OK, VKRT_ERR_INVALID_ARGUMENT, VKRT_ERR_NO_DEVICE, VKRT_ERR_HIP, VKRT_ERR_OUT_OF_MEMORY, VKRT_ERR_NOT_BUILT, VKRT_ERR_UNSUPPORTED = range(7)
VKRT_BUILD_LBVH_GPU = 0x1
VKRT_BUILD_SAH_HOST = 0x2
VKRT_BUILD_PLOC_GPU = 0x4
VKRT_TRACE_SEED_INDEX_ROW_MAJOR = 0x1
VKRT_TRACE_COUNT_TRAVERSAL = 0x2
VKRT_TRACE_TIME_KERNELS = 0x4
VKRT_TRACE_SAME_SEED_EVERY_FRAME = 0x8
VKRT_ABI_VERSION = 4
# vkrt_option
VKRT_OPT_MODE, VKRT_OPT_BVH_LAYOUT, VKRT_OPT_WF_SUBFRAMES, VKRT_OPT_WF_TRAV_BLOCK = 1, 2, 3, 4
VKRT_OPT_WF_SHARE, VKRT_OPT_TRI_THRESHOLD, VKRT_OPT_WF_SHARE_PERIOD, VKRT_OPT_WF_SHARE_FLAGS = 5, 6, 7, 8
VKRT_OPT_GBUFFER_MIPS = 9
VKRT_OPT_WATERTIGHT, VKRT_OPT_SKIP_DEAD_SHADOW_RAYS, VKRT_OPT_ANYHIT_DISSOLVE = 10, 11, 12
VKRT_OPT_WF_FRAMES_IN_FLIGHT, VKRT_OPT_SPLIT_BUDGET = 13, 14
VKRT_OPT_WF_SAMPLE_SYNC = 15
VKRT_OPT_WF_CAMERA_ROUNDS = 16
VKRT_OPT_WF_TRI_LEND = 17
VKRT_OPT_ALPHA_TEST = 18
VKRT_INFO_ANYHIT_ORDER = 100  # read-only: what the build resolved the any-hit child order to
VKRT_INFO_SPLIT_BUDGET = 101  # read-only: the pre-splitting budget the build used (what -1 resolved to)
# vkrt_instance_flags / vkrt_ray_flags (the gl_RayFlags*EXT values)
VKRT_INSTANCE_FACING_CULL_DISABLE, VKRT_INSTANCE_FLIP_FACING = 0x1, 0x2
VKRT_RAY_OPAQUE, VKRT_RAY_CULL_BACK_FACING, VKRT_RAY_CULL_FRONT_FACING = 0x1, 0x10, 0x20
VKRT_MEMORY_HOST, VKRT_MEMORY_DEVICE = 0, 1  # vkrt_memory
VKRT_SURFACE_GEOMETRY, VKRT_SURFACE_MATERIAL = 0x1, 0x2  # vkrt_surface_fields
VKRT_ALPHA_OPAQUE, VKRT_ALPHA_MASK = 0, 1  # vkrt_alpha_mode
VKRT_MULTIHIT_MAX = 16  # the largest max_hits of vkrt_intersect_multi

# every symbol include/vkrt.h declares (tests check the built library exports them all)
VKRT_SYMBOLS = [
    "vkrt_abi_version",
    "vkrt_last_error",
    "vkrt_device_count",
    "vkrt_scene_create",
    "vkrt_scene_destroy",
    "vkrt_scene_set_option",
    "vkrt_scene_get_option",
    "vkrt_reserve",
    "vkrt_reserve_frames",
    "vkrt_accel_build",
    "vkrt_accel_get_info",
    "vkrt_scene_update_nodes",
    "vkrt_accel_refit",
    "vkrt_scene_update_vertices",
    "vkrt_scene_update_node_transforms",
    "vkrt_scene_add_skin",
    "vkrt_scene_skin_vertices",
    "vkrt_scene_add_morph",
    "vkrt_scene_morph_vertices",
    "vkrt_intersect",
    "vkrt_occluded",
    "vkrt_scene_set_instance_visibility",
    "vkrt_scene_get_instance_visibility",
    "vkrt_intersect_ex",
    "vkrt_occluded_ex",
    "vkrt_intersect_multi",
    "vkrt_closest_point",
    "vkrt_hit_surface",
    "vkrt_scene_motion_mark",
    "vkrt_hit_motion",
    "vkrt_scene_set_material_alpha",
    "vkrt_scene_get_material_alpha",
    "vkrt_scene_update_lights",
    "vkrt_scene_update_materials",
    "vkrt_scene_update_texture",
    "vkrt_shard_rows",
    "vkrt_pathtrace",
    "vkrt_pathtrace_frames",
    "vkrt_gbuffer_raycast",
    "vkrt_hybrid_trace",
    "vkrt_gbuffer_raycast_nrd",
    "vkrt_hybrid_trace_nrd",
    "vkrt_gbuffer_raycast_hits",
    "vkrt_post",
    "vkrt_denoiser_create",
    "vkrt_denoiser_destroy",
    "vkrt_denoiser_reset",
    "vkrt_denoise_diffuse",
    "vkrt_denoise_diffuse_motion",
    "vkrt_counters_reset",
    "vkrt_counters_read",
    "vkrt_last_trace_ms",
    "vkrt_last_trace_timing",
    "vkrt_debug_check_accel",
    "vkrt_debug_read_accel",
    "vkrt_debug_read_node_masks",
    "vkrt_debug_read_triangle_ids",
    "vkrt_debug_split_references",
    "vkrt_debug_read_vertices",
    "vkrt_debug_read_instances",
    "vkrt_debug_read_lights",
    "vkrt_debug_read_materials",
    "vkrt_debug_read_texture",
    "vkrt_debug_closest_point_work",
    "vkrt_debug_trace_rays",
    "vkrt_debug_eval_math",
    "vkrt_debug_eval_shade",
]


def declare_vkrt(lib):
    """Attach argtypes/restype for the C ABI to a loaded libvkrt.so."""
    P = C.POINTER
    lib.vkrt_abi_version.restype = C.c_int
    lib.vkrt_last_error.restype = C.c_char_p
    lib.vkrt_device_count.restype = C.c_int
    lib.vkrt_scene_create.argtypes = [P(SceneDesc), C.c_int, P(C.c_void_p)]
    lib.vkrt_scene_create.restype = C.c_int
    lib.vkrt_scene_destroy.argtypes = [C.c_void_p]
    lib.vkrt_scene_destroy.restype = None
    lib.vkrt_scene_set_option.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.vkrt_scene_set_option.restype = C.c_int
    lib.vkrt_scene_get_option.argtypes = [C.c_void_p, C.c_int, P(C.c_int)]
    lib.vkrt_scene_get_option.restype = C.c_int
    lib.vkrt_reserve.argtypes = [C.c_void_p, P(Shard), C.c_void_p]
    lib.vkrt_reserve.restype = C.c_int
    lib.vkrt_reserve_frames.argtypes = [C.c_void_p, P(Shard), C.c_uint32, C.c_void_p]
    lib.vkrt_reserve_frames.restype = C.c_int
    lib.vkrt_accel_build.argtypes = [C.c_void_p, c_u, C.c_void_p]
    lib.vkrt_accel_build.restype = C.c_int
    lib.vkrt_accel_get_info.argtypes = [C.c_void_p, P(AccelInfo)]
    lib.vkrt_accel_get_info.restype = C.c_int
    lib.vkrt_scene_update_nodes.argtypes = [C.c_void_p, c_u, c_u, P(Node), C.c_void_p]
    lib.vkrt_scene_update_nodes.restype = C.c_int
    lib.vkrt_accel_refit.argtypes = [C.c_void_p, C.c_void_p]
    lib.vkrt_accel_refit.restype = C.c_int
    lib.vkrt_scene_update_vertices.argtypes = [C.c_void_p, P(VertexUpdate), C.c_void_p]
    lib.vkrt_scene_update_vertices.restype = C.c_int
    lib.vkrt_scene_update_node_transforms.argtypes = [C.c_void_p, P(NodeUpdate), C.c_void_p]
    lib.vkrt_scene_update_node_transforms.restype = C.c_int
    # (scene, first, count, out: host pointer to 96-B records, bytes)
    lib.vkrt_debug_read_instances.argtypes = [C.c_void_p, c_u, c_u, C.c_void_p, C.c_uint64]
    lib.vkrt_debug_read_instances.restype = C.c_int
    # editing a live scene: (scene, update, stream) / (scene, first, count, host materials, stream) / (scene, update, stream)
    lib.vkrt_scene_update_lights.argtypes = [C.c_void_p, P(LightUpdate), C.c_void_p]
    lib.vkrt_scene_update_lights.restype = C.c_int
    lib.vkrt_scene_update_materials.argtypes = [C.c_void_p, c_u, c_u, C.c_void_p, C.c_void_p]
    lib.vkrt_scene_update_materials.restype = C.c_int
    lib.vkrt_scene_update_texture.argtypes = [C.c_void_p, P(TextureUpdate), C.c_void_p]
    lib.vkrt_scene_update_texture.restype = C.c_int
    # (scene, first, count, out: host pointer to 32-B / 192-B records, bytes); (scene, texture, level, texels, bytes, quads or NULL, bytes)
    lib.vkrt_debug_read_lights.argtypes = [C.c_void_p, c_u, c_u, C.c_void_p, C.c_uint64]
    lib.vkrt_debug_read_lights.restype = C.c_int
    lib.vkrt_debug_read_materials.argtypes = [C.c_void_p, c_u, c_u, C.c_void_p, C.c_uint64]
    lib.vkrt_debug_read_materials.restype = C.c_int
    lib.vkrt_debug_read_texture.argtypes = [C.c_void_p, c_u, c_u, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    lib.vkrt_debug_read_texture.restype = C.c_int
    # (scene, desc, stream, out_skin) / (scene, skin, joint matrices: host or device pointer by `memory`, memory, stream)
    lib.vkrt_scene_add_skin.argtypes = [C.c_void_p, P(SkinDesc), C.c_void_p, P(c_u)]
    lib.vkrt_scene_add_skin.restype = C.c_int
    lib.vkrt_scene_skin_vertices.argtypes = [C.c_void_p, c_u, C.c_void_p, c_u, C.c_void_p]
    lib.vkrt_scene_skin_vertices.restype = C.c_int
    # (scene, desc, stream, out_morph) / (scene, morph, weights: host or device pointer by `memory`, memory, stream)
    lib.vkrt_scene_add_morph.argtypes = [C.c_void_p, P(MorphDesc), C.c_void_p, P(c_u)]
    lib.vkrt_scene_add_morph.restype = C.c_int
    lib.vkrt_scene_morph_vertices.argtypes = [C.c_void_p, c_u, C.c_void_p, c_u, C.c_void_p]
    lib.vkrt_scene_morph_vertices.restype = C.c_int
    # (scene, first, count, positions, normals, tangents, texcoords0: host pointers, any may be NULL)
    lib.vkrt_debug_read_vertices.argtypes = [C.c_void_p, c_u, c_u, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vkrt_debug_read_vertices.restype = C.c_int
    # (rays, hits, occluded: device pointers)
    lib.vkrt_intersect.argtypes = [C.c_void_p, C.c_void_p, c_u, c_u, C.c_void_p, C.c_void_p]
    lib.vkrt_intersect.restype = C.c_int
    lib.vkrt_occluded.argtypes = [C.c_void_p, C.c_void_p, c_u, c_u, C.c_void_p, C.c_void_p]
    lib.vkrt_occluded.restype = C.c_int
    lib.vkrt_scene_set_instance_visibility.argtypes = [C.c_void_p, c_u, c_u, P(InstanceVisibility), C.c_void_p]
    lib.vkrt_scene_set_instance_visibility.restype = C.c_int
    lib.vkrt_scene_get_instance_visibility.argtypes = [C.c_void_p, c_u, c_u, P(InstanceVisibility)]
    lib.vkrt_scene_get_instance_visibility.restype = C.c_int
    lib.vkrt_intersect_ex.argtypes = [C.c_void_p, C.c_void_p, c_u, P(QueryOpts), C.c_void_p, C.c_void_p]
    lib.vkrt_intersect_ex.restype = C.c_int
    lib.vkrt_occluded_ex.argtypes = [C.c_void_p, C.c_void_p, c_u, P(QueryOpts), C.c_void_p, C.c_void_p]
    lib.vkrt_occluded_ex.restype = C.c_int
    # (rays, hits, counts: device pointers; counts may be NULL)
    lib.vkrt_intersect_multi.argtypes = [C.c_void_p, C.c_void_p, c_u, P(QueryOpts), c_u, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vkrt_intersect_multi.restype = C.c_int
    # (queries, hits: device pointers; opts may be NULL)
    lib.vkrt_closest_point.argtypes = [C.c_void_p, C.c_void_p, c_u, P(QueryOpts), C.c_void_p, C.c_void_p]
    lib.vkrt_closest_point.restype = C.c_int
    # (host queries)
    lib.vkrt_debug_closest_point_work.argtypes = [C.c_void_p, C.c_void_p, c_u, P(QueryOpts), P(C.c_uint64)]
    lib.vkrt_debug_closest_point_work.restype = C.c_int
    # (hits, out: device pointers)
    lib.vkrt_hit_surface.argtypes = [C.c_void_p, C.c_void_p, c_u, c_u, C.c_void_p, C.c_void_p]
    lib.vkrt_hit_surface.restype = C.c_int
    # motion (scene, stream) / (scene, hits, n, current, previous, stream: device pointers, either output may be NULL)
    lib.vkrt_scene_motion_mark.argtypes = [C.c_void_p, C.c_void_p]
    lib.vkrt_scene_motion_mark.restype = C.c_int
    lib.vkrt_hit_motion.argtypes = [C.c_void_p, C.c_void_p, c_u, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vkrt_hit_motion.restype = C.c_int
    lib.vkrt_scene_set_material_alpha.argtypes = [C.c_void_p, c_u, c_u, P(MaterialAlpha), C.c_void_p]
    lib.vkrt_scene_set_material_alpha.restype = C.c_int
    lib.vkrt_scene_get_material_alpha.argtypes = [C.c_void_p, c_u, c_u, P(MaterialAlpha)]
    lib.vkrt_scene_get_material_alpha.restype = C.c_int
    lib.vkrt_debug_read_node_masks.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.vkrt_debug_read_node_masks.restype = C.c_int
    lib.vkrt_debug_read_triangle_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.vkrt_debug_read_triangle_ids.restype = C.c_int
    # (scene, percent, prio, scale, ref_tri, ref_box: host pointers, the first two may be NULL; capacity in references; ref_count)
    lib.vkrt_debug_split_references.argtypes = [C.c_void_p, c_u, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, P(c_u)]
    lib.vkrt_debug_split_references.restype = C.c_int
    lib.vkrt_debug_check_accel.argtypes = [C.c_void_p, P(AccelCheck)]
    lib.vkrt_debug_check_accel.restype = C.c_int
    lib.vkrt_debug_read_accel.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, P(C.c_int32)]
    lib.vkrt_debug_read_accel.restype = C.c_int
    lib.vkrt_shard_rows.argtypes = [P(Shard)]
    lib.vkrt_shard_rows.restype = c_u
    lib.vkrt_pathtrace.argtypes = [
        C.c_void_p, P(PushConstantRay), P(GlobalUniforms), P(TraceOpts), P(Shard), C.c_void_p, C.c_void_p,
    ]
    lib.vkrt_pathtrace.restype = C.c_int
    lib.vkrt_pathtrace_frames.argtypes = [
        C.c_void_p, P(PushConstantRay), P(GlobalUniforms), P(TraceOpts), P(Shard), C.c_void_p, c_u, C.c_void_p,
    ]
    lib.vkrt_pathtrace_frames.restype = C.c_int
    lib.vkrt_gbuffer_raycast.argtypes = [C.c_void_p, P(c_f * 4), C.c_int, P(GlobalUniforms), P(Shard), P(Gbuffer), C.c_void_p]
    lib.vkrt_gbuffer_raycast.restype = C.c_int
    lib.vkrt_hybrid_trace.argtypes = [C.c_void_p, P(PushConstantRay), P(GlobalUniforms), P(TraceOpts), P(Shard), P(Gbuffer), C.c_void_p, C.c_void_p]
    lib.vkrt_hybrid_trace.restype = C.c_int
    lib.vkrt_gbuffer_raycast_nrd.argtypes = [C.c_void_p, P(c_f * 4), C.c_int, P(GlobalUniforms), P(c_f * 16), P(Shard), P(Gbuffer), P(NrdPlanes), C.c_void_p]
    lib.vkrt_gbuffer_raycast_nrd.restype = C.c_int
    lib.vkrt_hybrid_trace_nrd.argtypes = [C.c_void_p, P(PushConstantRay), P(GlobalUniforms), P(TraceOpts), P(Shard), P(Gbuffer), P(NrdPlanes), C.c_void_p,
                                          C.c_void_p]
    lib.vkrt_hybrid_trace_nrd.restype = C.c_int
    # (view matrix and NRD planes: both NULL or both given; hits: device pointer)
    lib.vkrt_gbuffer_raycast_hits.argtypes = [C.c_void_p, P(c_f * 4), C.c_int, P(GlobalUniforms), P(c_f * 16), P(Shard), P(Gbuffer), P(NrdPlanes), C.c_void_p,
                                              C.c_void_p]
    lib.vkrt_gbuffer_raycast_hits.restype = C.c_int
    lib.vkrt_post.argtypes = [C.c_int, P(PushConstantPost), c_u, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vkrt_post.restype = C.c_int
    lib.vkrt_denoiser_create.argtypes = [C.c_int, c_u, c_u, P(C.c_void_p)]
    lib.vkrt_denoiser_create.restype = C.c_int
    lib.vkrt_denoiser_destroy.argtypes = [C.c_void_p]
    lib.vkrt_denoiser_destroy.restype = None
    lib.vkrt_denoiser_reset.argtypes = [C.c_void_p]
    lib.vkrt_denoiser_reset.restype = C.c_int
    lib.vkrt_denoise_diffuse.argtypes = [C.c_void_p, P(DenoiseSettings), P(GlobalUniforms), P(Gbuffer), P(NrdPlanes), C.c_void_p, C.c_void_p]
    lib.vkrt_denoise_diffuse.restype = C.c_int
    lib.vkrt_denoise_diffuse_motion.argtypes = [C.c_void_p, P(DenoiseSettings), P(GlobalUniforms), P(Gbuffer), P(NrdPlanes), C.c_void_p, C.c_void_p,
                                                C.c_void_p]
    lib.vkrt_denoise_diffuse_motion.restype = C.c_int
    lib.vkrt_counters_reset.argtypes = [C.c_void_p, C.c_void_p]
    lib.vkrt_counters_reset.restype = C.c_int
    lib.vkrt_counters_read.argtypes = [C.c_void_p, P(Counters)]
    lib.vkrt_counters_read.restype = C.c_int
    lib.vkrt_last_trace_ms.argtypes = [C.c_void_p, P(c_f)]
    lib.vkrt_last_trace_ms.restype = C.c_int
    lib.vkrt_last_trace_timing.argtypes = [C.c_void_p, P(TraceTiming)]
    lib.vkrt_last_trace_timing.restype = C.c_int
    lib.vkrt_debug_trace_rays.argtypes = [
        C.c_void_p, c_u, C.c_void_p, C.c_void_p, c_f, c_f, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
    ]
    lib.vkrt_debug_trace_rays.restype = C.c_int
    lib.vkrt_debug_eval_math.argtypes = [C.c_int, C.c_int, c_u, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vkrt_debug_eval_math.restype = C.c_int
    lib.vkrt_debug_eval_shade.argtypes = [C.c_int, c_u, C.c_void_p, C.c_void_p]
    lib.vkrt_debug_eval_shade.restype = C.c_int
    return lib
