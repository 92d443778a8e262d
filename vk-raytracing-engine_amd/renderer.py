"""Harness-side wrapper of the C ABI (include/vkrt.h): torch owns device memory and streams,
libvkrt.so does all the work.  Mirrors the call order of the reference's main():
loadGltfScene -> createBottomLevelASGltf/createTopLevelAsGltf -> per frame pathtrace
(main.cpp:226-240, 504-508)."""
import ctypes as C
import os

import numpy as np

from . import LIB_PATH, abi
from .flat_scene import LIGHT_DTYPE, MAT_DTYPE

_lib = None


def load_library():
    """Load libvkrt.so; fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        # torch bundles its own libamdhip64.so.7; it must be the first HIP runtime mapped into the
        # process (loading /opt/rocm's copy first leaves torch with "No HIP GPUs are available").
        import torch  # noqa: F401

        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: build it with __graft_entry__.build() "
                               "(there is no CPU fallback for the ray-tracing path)")
        _lib = abi.declare_vkrt(C.CDLL(LIB_PATH))
        if _lib.vkrt_abi_version() != abi.VKRT_ABI_VERSION:
            raise RuntimeError("libvkrt.so ABI version mismatch")
    return _lib


_HOST, _DEVICE = abi.VKRT_MEMORY_HOST, abi.VKRT_MEMORY_DEVICE
_torch = None  # the module, once a tensor has been vetted (imported late: load_library says why)


def _import_torch():
    global _torch
    import torch

    _torch = torch
    return torch


class _AnyLength:
    """a dimension of an expected shape that may have any length: equal to every int, written as its letter"""
    __hash__ = None

    def __init__(self, letter):
        self.letter = letter

    def __eq__(self, other):
        return True

    def __ne__(self, other):
        return False

    def __repr__(self):
        return self.letter


_N, _T = _AnyLength("n"), _AnyLength("T")
_VERTEX_ARRAYS = (("positions", (_N, 3)), ("normals", (_N, 3)), ("tangents", (_N, 4)), ("texcoords0", (_N, 2)))  # update_vertices, in vkrt_vertex_update's order
ALPHA_OPAQUE, ALPHA_MASK = abi.VKRT_ALPHA_OPAQUE, abi.VKRT_ALPHA_MASK  # vkrt_alpha_mode, for Renderer.set_material_alpha
# one 96-B instance record (Renderer.read_instances; include/vkrt.h vkrt_debug_read_instances)
INSTANCE_DTYPE = np.dtype([("o2w", "<f4", 12), ("w2o", "<f4", 9), ("primMesh", "<i4"), ("vis", "<u4"), ("pad", "<i4")])
assert INSTANCE_DTYPE.itemsize == 96
# the records of vkrt_debug_read_materials: the 128-B record of the queries and the G-buffer, then the 64-B record of the hit shader
MATERIAL_RECORD_DTYPE = np.dtype([("m", MAT_DTYPE), ("pad", "<i4"), ("alphaMode", "<u4"), ("alphaCutoff", "<f4"), ("tex", "<u4", (4, 4)),
                                  ("f", "<f4", 8), ("ref", "<u4", 8)])
assert MATERIAL_RECORD_DTYPE.itemsize == 192


class VkrtError(RuntimeError):
    pass


def _check(rc, what):
    if rc != 0:
        raise VkrtError(f"{what} failed ({rc}): {load_library().vkrt_last_error().decode()}")


def whole_image_shard(width, height):
    return abi.Shard(width, height, 0, 1, 0)


def pack_rays(origins, directions, tmin=0.001, tmax=1e4):
    """vkrt_ray records for Renderer.intersect / occluded: origins, directions [N, 3] torch tensors; tmin, tmax scalars or [N]
    tensors.  Returns a contiguous float32 [N, 8] tensor on the origins' device: (origin.xyz, tmin, direction.xyz, tmax) per row."""
    import torch

    o = torch.as_tensor(origins)
    dev = o.device
    o = o.to(torch.float32).reshape(-1, 3)
    d = torch.as_tensor(directions, device=dev).to(torch.float32).reshape(-1, 3)
    if o.shape[0] != d.shape[0]:
        raise VkrtError(f"pack_rays: {o.shape[0]} origins, {d.shape[0]} directions")
    n = o.shape[0]
    out = torch.empty((n, 8), dtype=torch.float32, device=dev)
    out[:, 0:3] = o
    out[:, 4:7] = d
    for col, b in ((3, tmin), (7, tmax)):
        b = torch.as_tensor(b, dtype=torch.float32, device=dev)
        if b.dim() > 0 and b.numel() != n:
            raise VkrtError(f"pack_rays: {b.numel()} bounds for {n} rays")
        out[:, col] = b.reshape(-1) if b.dim() > 0 else b
    return out


class RayHits:
    """Result of Renderer.intersect: views of one [N, 8] 4-byte buffer laid out like vkrt_hit.  t, u, v: float32 [N]; instance,
    primitive, prim_mesh, triangle, material: int32 [N] (-1 = miss; t = tmax, u = v = 0 there)."""

    def __init__(self, buffer):
        import torch

        self.buffer = buffer
        f, i = buffer.view(torch.float32), buffer.view(torch.int32)
        self.t, self.u, self.v = f[:, 0], f[:, 1], f[:, 2]
        self.instance, self.primitive, self.prim_mesh, self.triangle, self.material = (i[:, k] for k in range(3, 8))


class MultiHits:
    """Result of Renderer.intersect_multi: views of one [N, K, 8] 4-byte buffer of vkrt_hit records, K per ray in the order (t, triangle
    id), and count, int32 [N]: how many of a ray's records are hits.  t, u, v: float32 [N, K]; instance, primitive, prim_mesh, triangle,
    material: int32 [N, K].  Records behind a ray's count are misses (-1; t = tmax, u = v = 0)."""

    def __init__(self, buffer, count):
        import torch

        self.buffer, self.count = buffer, count
        f, i = buffer.view(torch.float32), buffer.view(torch.int32)
        self.t, self.u, self.v = f[:, :, 0], f[:, :, 1], f[:, :, 2]
        self.instance, self.primitive, self.prim_mesh, self.triangle, self.material = (i[:, :, k] for k in range(3, 8))

    def flat(self):
        """The same records as a RayHits over [N * K, 8] (a view, no copy): record i * K + j is hit j of ray i, so
        Renderer.surface(h.flat()) is the surface of every returned hit."""
        return RayHits(self.buffer.view(-1, 8))


class Surfaces:
    """Result of Renderer.surface: views of one [N, 32] 4-byte buffer laid out like vkrt_surface.  position, geometric_normal, normal,
    shading_normal, tangent, binormal, base_color, emission: float32 [N, 3]; texcoord_u, texcoord_v, alpha, metallic, roughness:
    float32 [N]; material, valid: int32 [N] (material = -1 and valid = 0 where the record was not a hit of the scene: all else 0)."""

    def __init__(self, buffer):
        import torch

        self.buffer = buffer
        f, i = buffer.view(torch.float32), buffer.view(torch.int32)
        (self.position, self.geometric_normal, self.normal, self.shading_normal, self.tangent, self.binormal, self.base_color,
         self.emission) = (f[:, 4 * k:4 * k + 3] for k in range(8))
        self.texcoord_u, self.texcoord_v, self.alpha, self.metallic, self.roughness = (f[:, 4 * k + 3] for k in range(5))
        self.material, self.valid, self.reserved = i[:, 23], i[:, 27], i[:, 31]

    @property
    def texcoord(self):
        """[N, 2] view of (texcoord_u, texcoord_v): the two scalars sit four words apart in the record"""
        return self.buffer.view(self.position.dtype)[:, 3:8:4]


class Renderer:
    def __init__(self, flat, device=0, build="ploc", options=None):
        """options: {abi.VKRT_OPT_*: value} applied before the build (per-handle execution options, include/vkrt.h)."""
        import time

        self.lib = load_library()
        self.device = device
        desc, keep = flat.to_desc()
        h = C.c_void_p()
        t0 = time.perf_counter()
        _check(self.lib.vkrt_scene_create(C.byref(desc), device, C.byref(h)), "vkrt_scene_create")
        self.upload_ms = (time.perf_counter() - t0) * 1e3  # scene upload (hello_vulkan.cpp:353-381), host wall time
        self._h = h
        del keep
        self.lights_count = int(flat.lights.shape[0])
        self._prim_mesh = np.array(flat.nodes["primMesh"], np.int32)  # update_nodes keeps every node's primMesh
        self._vertex_count = int(flat.positions.shape[0])
        self._material_count = int(flat.materials.shape[0])
        self._texture_sizes = [(int(t["rgba8"].shape[1]), int(t["rgba8"].shape[0])) for t in flat.textures]  # (width, height), fixed
        self._triangle_count = int((np.asarray(flat.prim_meshes["indexCount"], np.int64)[self._prim_mesh] // 3).sum())  # instanced
        self._skins = []  # (first, count, joint_count) of every add_skin, in the library's numbering
        self._morphs = []  # (first, count, target_count) of every add_morph, in the library's numbering
        for k, v in (options or {}).items():
            self.set_option(k, v)
        if getattr(flat, "material_alpha", None) is not None:
            self.set_material_alpha(0, flat.material_alpha["mode"], flat.material_alpha["cutoff"])
        if build:
            self.build(build)

    def set_option(self, option, value):
        _check(self.lib.vkrt_scene_set_option(self._h, int(option), int(value)), "vkrt_scene_set_option")

    def get_option(self, option):
        v = C.c_int()
        _check(self.lib.vkrt_scene_get_option(self._h, int(option), C.byref(v)), "vkrt_scene_get_option")
        return int(v.value)

    def reserve(self, shard, stream=None, frames_per_call=None):
        """Size the working set for launches of this shard geometry (no allocation / host sync inside later pathtrace calls);
        frames_per_call: the frames the caller hands to one pathtrace_frames call (None: whatever the options keep in flight)."""
        st = C.c_void_p(stream.cuda_stream) if stream is not None else None
        if frames_per_call is None:
            _check(self.lib.vkrt_reserve(self._h, C.byref(shard), st), "vkrt_reserve")
        else:
            _check(self.lib.vkrt_reserve_frames(self._h, C.byref(shard), int(frames_per_call), st), "vkrt_reserve_frames")

    def build(self, kind="ploc"):
        flags = {"sah": abi.VKRT_BUILD_SAH_HOST, "lbvh": abi.VKRT_BUILD_LBVH_GPU, "ploc": abi.VKRT_BUILD_PLOC_GPU}[kind]
        _check(self.lib.vkrt_accel_build(self._h, flags, None), "vkrt_accel_build")
        self.build_kind = kind

    def update_nodes(self, first, world_matrices, stream=None, indices=None):
        """New transforms for nodes [first, first + n), or with `indices` for the n nodes it names (then first must be 0).
        world_matrices: (n, 16) float32, column-major like vkrt_node.worldMatrix and FlatScene.nodes["worldMatrix"]; every node keeps
        its primMesh and its visibility.  Enqueued on `stream` (a torch stream; None = the default stream); the tree is stale until
        refit() or build().
        numpy arrays take the host path (vkrt_scene_update_nodes; with indices the host form of vkrt_scene_update_node_transforms):
        checked finite, copied before return, no wait.  A contiguous float32 torch tensor on the scene's device takes the device path
        (vkrt_scene_update_node_transforms with VKRT_MEMORY_DEVICE): one launch, no copy, no synchronisation, values not inspected, an
        index >= the node count skips its entry; indices is then an int32 or uint32 tensor of n entries on that device, and both
        tensors must live until `stream` has passed the call.  Refused here, before the call: a wrong dtype, shape or device, a
        non-contiguous tensor, numpy and torch mixed in one call, a range outside the scene, first != 0 with indices."""
        who = "update_nodes"
        torch = _torch or _import_torch()
        st = C.c_void_p(stream.cuda_stream) if stream is not None else None
        tensors = [isinstance(a, torch.Tensor) for a in (world_matrices, indices) if a is not None]
        if any(tensors) and not all(tensors):
            raise VkrtError(f"{who}: numpy arrays and torch tensors mixed in one call")
        count = self._prim_mesh.shape[0]
        if any(tensors) or indices is not None:
            if isinstance(first, bool) or not isinstance(first, (int, np.integer)) or first < 0 or (indices is not None and first != 0):
                raise VkrtError(f"{who}: first is {first!r}: an integer >= 0, and 0 with indices")
            if any(tensors):
                mptr, memory, have = self._float_source(who, "world_matrices", world_matrices, (_N, 16), align=16)
                n, iptr = int(have[0]), None
                if indices is not None:
                    if not indices.is_cuda or indices.device.index != self.device:
                        raise VkrtError(f"{who}: indices is on {indices.device}, the scene is on cuda:{self.device}")
                    if indices.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                        raise VkrtError(f"{who}: indices is {indices.dtype}, expected int32 or uint32")
                    if not indices.is_contiguous():
                        raise VkrtError(f"{who}: indices must be contiguous")
                    if tuple(indices.shape) != (n,):
                        raise VkrtError(f"{who}: indices has shape {tuple(indices.shape)}, expected ({n},)")
                    iptr = indices.data_ptr()
                    if iptr % 4:
                        raise VkrtError(f"{who}: indices must be 4-byte aligned")
            else:  # the sparse host form
                m = np.ascontiguousarray(world_matrices, np.float32).reshape(-1, 16)
                ix = np.asarray(indices)
                n = m.shape[0]
                if ix.dtype.kind not in "iu" or ix.shape != (n,) or np.any(ix < 0) or np.any(ix >= count):
                    raise VkrtError(f"{who}: indices must be {n} integers in [0, {count})")
                ix = np.ascontiguousarray(ix, np.uint32)
                mptr, iptr, memory = m.ctypes.data, ix.ctypes.data, _HOST
            if indices is None and int(first) + n > count:
                raise VkrtError(f"{who}: nodes [{first}, {first + n}) outside the scene's {count} nodes")
            u = abi.NodeUpdate(C.sizeof(abi.NodeUpdate), int(first), n, memory, mptr, iptr)
            _check(self.lib.vkrt_scene_update_node_transforms(self._h, C.byref(u), st), "vkrt_scene_update_node_transforms")
            return
        m = np.ascontiguousarray(world_matrices, np.float32).reshape(-1, 16)
        first, n = int(first), m.shape[0]
        if first < 0 or first + n > self._prim_mesh.shape[0]:
            raise VkrtError(f"update_nodes: nodes [{first}, {first + n}) outside the scene's {self._prim_mesh.shape[0]} nodes")
        arr = (abi.Node * max(n, 1))()
        for i in range(n):
            arr[i].worldMatrix[:] = [float(v) for v in m[i]]
            arr[i].primMesh = int(self._prim_mesh[first + i])
        st = C.c_void_p(stream.cuda_stream) if stream is not None else None
        _check(self.lib.vkrt_scene_update_nodes(self._h, first, n, arr, st), "vkrt_scene_update_nodes")

    def _float_source(self, who, name, a, shape, numpy_only=False, align=1, finite=False):
        """One float32 source of the vertex calls, vetted before the library sees it: a C-contiguous numpy array (host memory) or, unless
        numpy_only, a contiguous torch tensor on the scene's device whose address is a multiple of `align`.  shape: the one it must
        have as a tuple, _N or _T where any length will do, e.g. (_N, 3); finite: a host array holds no non-finite value.  Returns (pointer,
        memory kind, the array's shape).  The device path of update_vertices runs this per array at 8 us per call: it is written to be
        cheap (profiles/r13_experiments.md)."""
        if isinstance(a, np.ndarray):
            memory, f32, contiguous, ptr = _HOST, np.float32, a.flags.c_contiguous, a.ctypes.data
        else:
            torch = _torch or _import_torch()
            if numpy_only or not isinstance(a, torch.Tensor):
                raise VkrtError(f"{who}: {name} must be a numpy array{'' if numpy_only else ' or a torch tensor'}, got {type(a).__name__}")
            if not a.is_cuda or a.device.index != self.device:
                raise VkrtError(f"{who}: {name} is on {a.device}, the scene is on cuda:{self.device}")
            memory, f32, contiguous, ptr = _DEVICE, torch.float32, a.is_contiguous(), a.data_ptr()
        if a.dtype != f32:
            raise VkrtError(f"{who}: {name} is {a.dtype}, expected float32")
        if not contiguous:
            raise VkrtError(f"{who}: {name} must be contiguous")
        if ptr % align and memory == _DEVICE:
            raise VkrtError(f"{who}: {name} must be {align}-byte aligned")
        have = a.shape
        if have != shape:  # (one tuple comparison: an _AnyLength in `shape` equals every length)
            raise VkrtError(f"{who}: {name} has shape {tuple(have)}, expected {shape}")
        if finite and memory == _HOST and not np.all(np.isfinite(a)):
            raise VkrtError(f"{who}: {name} holds a non-finite value")
        return ptr, memory, have

    def _vertex_range(self, who, first, n, empty_ok=True):
        """`first` as an int, with vertices [first, first + n) inside the scene"""
        if isinstance(first, bool) or not isinstance(first, (int, np.integer)) or first < 0 or int(first) + n > self._vertex_count or not (n or empty_ok):
            raise VkrtError(f"{who}: first: vertices [{first}, {first} + {n}) {'' if empty_ok else 'empty or '}outside the scene's "
                            f"{self._vertex_count} vertices")
        return int(first)

    @staticmethod
    def _overlapping(ranges, first, n):
        """the number of the skin or morph in `ranges` ((first, count, ...) each) that overlaps vertices [first, first + n), or None"""
        for k, (f0, c0, _) in enumerate(ranges):
            if first < f0 + c0 and f0 < first + n:
                return k
        return None

    def update_vertices(self, first, positions=None, normals=None, tangents=None, texcoords0=None, stream=None):
        """vkrt_scene_update_vertices: new attributes for vertices [first, first + n) of the scene's shared vertex arrays (absolute
        indices, a mesh's vertexOffset included).  positions, normals: (n, 3); tangents: (n, 4); texcoords0: (n, 2); float32; None
        keeps the attribute.  numpy arrays take the host path (copied before return, the call waits for `stream`); torch tensors on
        the scene's device take the device path: no copy, no synchronisation, the tensors must live until `stream` has passed the
        call.  Enqueued on `stream` (a torch stream; None = the default stream).  With positions the tree is stale until refit() or
        build().  Refused here, before the call: a wrong dtype or shape, a non-contiguous tensor, a tensor on another device, numpy and
        torch mixed in one call, lengths that differ, a range outside the scene."""
        n, memory, ptr = None, _HOST, [None, None, None, None]
        for i, a in enumerate((positions, normals, tangents, texcoords0)):
            if a is None:
                continue
            k, shape = _VERTEX_ARRAYS[i]
            ptr[i], kind, have = self._float_source("update_vertices", k, a, shape)
            if n is not None and kind != memory:
                raise VkrtError(f"update_vertices: {k}: numpy arrays and torch tensors mixed in one call")
            if n is not None and have[0] != n:
                raise VkrtError(f"update_vertices: {k} has {have[0]} vertices, the arrays before it {n}")
            n, memory = int(have[0]), kind
        n = n or 0
        first = self._vertex_range("update_vertices", first, n)
        u = abi.VertexUpdate(C.sizeof(abi.VertexUpdate), first, n, memory, *ptr)
        st = C.c_void_p(stream.cuda_stream) if stream is not None else None
        _check(self.lib.vkrt_scene_update_vertices(self._h, C.byref(u), st), "vkrt_scene_update_vertices")

    def add_skin(self, first, joints, weights, joint_count=None, stream=None):
        """vkrt_scene_add_skin: bind four influences per vertex to vertices [first, first + n) (absolute indices) and capture their
        positions, normals and tangents, as they are at this point of `stream`, as the bind pose.  joints: integer (n, 4) numpy array
        (glTF JOINTS_0); weights: float32 (n, 4) numpy array (WEIGHTS_0, used as given); joint_count: how many joint matrices skin()
        takes (default joints.max() + 1).  Returns the skin's number.  Refused here, before the call: a wrong dtype or shape, a
        non-contiguous array, lengths that differ, an empty range or one outside the scene or overlapping an earlier skin's, a joint
        index outside [0, joint_count), a non-finite weight."""
        if not isinstance(joints, np.ndarray):
            raise VkrtError(f"add_skin: joints must be a numpy array, got {type(joints).__name__}")
        if joints.dtype.kind not in "iu":
            raise VkrtError(f"add_skin: joints is {joints.dtype}, expected an integer dtype")
        if joints.ndim != 2 or joints.shape[1] != 4:
            raise VkrtError(f"add_skin: joints has shape {tuple(joints.shape)}, expected (n, 4)")
        if not joints.flags["C_CONTIGUOUS"]:
            raise VkrtError("add_skin: joints must be contiguous")
        n = int(joints.shape[0])
        weights_ptr, _, _ = self._float_source("add_skin", "weights", weights, (_N, 4), numpy_only=True, finite=True)
        if weights.shape[0] != n:
            raise VkrtError(f"add_skin: weights has {weights.shape[0]} vertices, joints {n}")
        first = self._vertex_range("add_skin", first, n, empty_ok=False)
        k = self._overlapping(self._skins, first, n)
        if k is not None:
            raise VkrtError(f"add_skin: first: vertices [{first}, {first + n}) overlap skin {k}'s [{self._skins[k][0]}, {sum(self._skins[k][:2])})")
        k = self._overlapping(self._morphs, first, n)  # skins come first: a morph inside one captured its bind pose
        if k is not None:
            raise VkrtError(f"add_skin: first: vertices [{first}, {first + n}) overlap morph {k}'s [{self._morphs[k][0]}, {sum(self._morphs[k][:2])}): "
                            "add skins before morphs")
        if joint_count is None:
            joint_count = int(joints.max()) + 1
        if isinstance(joint_count, bool) or not isinstance(joint_count, (int, np.integer)) or not 1 <= joint_count <= 65536:
            raise VkrtError(f"add_skin: joint_count {joint_count!r} outside 1..65536")
        if int(joints.min()) < 0 or int(joints.max()) >= joint_count:
            raise VkrtError(f"add_skin: joints holds indices in [{int(joints.min())}, {int(joints.max())}], joint_count is {joint_count}")
        j16 = np.ascontiguousarray(joints, np.uint16)
        d = abi.SkinDesc(C.sizeof(abi.SkinDesc), first, n, int(joint_count), j16.ctypes.data, weights_ptr)
        out = abi.c_u()
        st = C.c_void_p(stream.cuda_stream) if stream is not None else None
        _check(self.lib.vkrt_scene_add_skin(self._h, C.byref(d), st, C.byref(out)), "vkrt_scene_add_skin")
        self._skins.append((first, n, int(joint_count)))
        return int(out.value)

    def skin(self, skin, joint_matrices, stream=None):
        """vkrt_scene_skin_vertices: pose skin `skin` from joint_matrices, (joint_count, 16) float32, column-major like
        vkrt_node.worldMatrix.  A numpy array takes the host path (checked finite, copied before return, the call waits for `stream`);
        a torch tensor on the scene's device takes the device path: no copy, no synchronisation, the tensor must live until `stream`
        has passed the call.  One kernel launch on `stream` (a torch stream; None = the default stream) writes positions, normals and
        tangents of the skin's vertices from the captured bind pose; the tree is stale until refit() or build().  Refused here, before
        the call: a skin index out of range, a wrong dtype or shape, a non-contiguous or misaligned tensor, a tensor on another
        device, a non-finite host matrix."""
        if isinstance(skin, bool) or not isinstance(skin, (int, np.integer)) or not 0 <= skin < len(self._skins):
            raise VkrtError(f"skin: skin {skin!r} outside the scene's {len(self._skins)} skins")
        ptr, memory, _ = self._float_source("skin", "joint_matrices", joint_matrices, (self._skins[int(skin)][2], 16), align=16, finite=True)
        st = C.c_void_p(stream.cuda_stream) if stream is not None else None
        _check(self.lib.vkrt_scene_skin_vertices(self._h, int(skin), ptr, memory, st), "vkrt_scene_skin_vertices")

    def add_morph(self, first, position_deltas=None, normal_deltas=None, tangent_deltas=None, stream=None):
        """vkrt_scene_add_morph: bind T morph targets to vertices [first, first + n) (absolute indices) and capture their positions,
        normals and tangents, as they are at this point of `stream`, as the base shape.  Each deltas array is a float32 (T, n, 3) numpy
        array (target-major, glTF's POSITION / NORMAL / TANGENT of primitives[].targets) or None for an attribute that is not morphed.
        A range inside a skin's range morphs that skin's bind pose (morph, then skin); add skins first.  Returns the morph's number.
        Refused here, before the call: no array at all, a wrong dtype or shape, a non-contiguous array, shapes that differ, more than
        VKRT_MORPH_TARGETS_MAX targets, an empty range or one outside the scene, overlapping an earlier morph's or straddling a skin's
        boundary, a non-finite delta."""
        given = [(k, a) for k, a in (("position_deltas", position_deltas), ("normal_deltas", normal_deltas), ("tangent_deltas", tangent_deltas))
                 if a is not None]
        if not given:
            raise VkrtError("add_morph: position_deltas, normal_deltas and tangent_deltas are all None")
        ptr = {}
        for k, a in given:
            ptr[k], _, _ = self._float_source("add_morph", k, a, (_T, _N, 3), numpy_only=True, finite=True)
            if a.shape != given[0][1].shape:
                raise VkrtError(f"add_morph: {k} has shape {tuple(a.shape)}, {given[0][0]} {tuple(given[0][1].shape)}")
        T, n = int(given[0][1].shape[0]), int(given[0][1].shape[1])
        if not 1 <= T <= abi.VKRT_MORPH_TARGETS_MAX:
            raise VkrtError(f"add_morph: {given[0][0]} has {T} targets, outside 1..{abi.VKRT_MORPH_TARGETS_MAX}")
        first = self._vertex_range("add_morph", first, n, empty_ok=False)
        k = self._overlapping(self._morphs, first, n)
        if k is not None:
            raise VkrtError(f"add_morph: first: vertices [{first}, {first + n}) overlap morph {k}'s [{self._morphs[k][0]}, {sum(self._morphs[k][:2])})")
        k = self._overlapping(self._skins, first, n)  # (the skins are disjoint: a range inside one touches no other)
        if k is not None and (first < self._skins[k][0] or first + n > sum(self._skins[k][:2])):
            raise VkrtError(f"add_morph: first: vertices [{first}, {first + n}) straddle the boundary of skin {k}'s [{self._skins[k][0]}, "
                            f"{sum(self._skins[k][:2])})")
        d = abi.MorphDesc(C.sizeof(abi.MorphDesc), first, n, T, ptr.get("position_deltas"), ptr.get("normal_deltas"), ptr.get("tangent_deltas"))
        out = abi.c_u()
        st = C.c_void_p(stream.cuda_stream) if stream is not None else None
        _check(self.lib.vkrt_scene_add_morph(self._h, C.byref(d), st, C.byref(out)), "vkrt_scene_add_morph")
        self._morphs.append((first, n, T))
        return int(out.value)

    def morph(self, morph, weights, stream=None):
        """vkrt_scene_morph_vertices: pose morph `morph` from weights, (T,) float32.  A numpy array takes the host path (checked
        finite, copied before return, the call waits for `stream`); a torch tensor on the scene's device takes the device path: no
        copy, no synchronisation, the tensor must live until `stream` has passed the call.  One kernel launch on `stream` (a torch
        stream; None = the default stream) writes base + sum(w * delta); a weight of exactly zero skips its target.  A morph outside
        every skin writes the scene's positions, normals and tangents, and the tree is stale until refit() or build(); a morph inside
        a skin writes that skin's bind pose, which the skin's next skin() carries into the scene.  Refused here, before the call: a
        morph index out of range, a wrong dtype or shape, a non-contiguous or misaligned tensor, a tensor on another device, a
        non-finite host weight."""
        if isinstance(morph, bool) or not isinstance(morph, (int, np.integer)) or not 0 <= morph < len(self._morphs):
            raise VkrtError(f"morph: morph {morph!r} outside the scene's {len(self._morphs)} morphs")
        ptr, memory, _ = self._float_source("morph", "weights", weights, (self._morphs[int(morph)][2],), align=4, finite=True)
        st = C.c_void_p(stream.cuda_stream) if stream is not None else None
        _check(self.lib.vkrt_scene_morph_vertices(self._h, int(morph), ptr, memory, st), "vkrt_scene_morph_vertices")

    def read_vertices(self, first, count):
        """The live attributes of vertices [first, first + count) (vkrt_debug_read_vertices, synchronises): a dict of float32 arrays,
        positions (count, 3), normals (count, 3), tangents (count, 4), texcoords0 (count, 2)."""
        ok = all(not isinstance(x, bool) and isinstance(x, (int, np.integer)) for x in (first, count))
        if not ok or first < 0 or count < 0 or int(first) + int(count) > self._vertex_count:
            raise VkrtError(f"read_vertices: first: vertices [{first}, {first} + {count}) outside the scene's {self._vertex_count} vertices")
        out = {k: np.zeros((int(count), w), np.float32) for k, w in (("positions", 3), ("normals", 3), ("tangents", 4), ("texcoords0", 2))}
        _check(self.lib.vkrt_debug_read_vertices(self._h, int(first), int(count), *(out[k].ctypes.data for k in ("positions", "normals", "tangents",
                                                                                                         "texcoords0"))), "vkrt_debug_read_vertices")
        return out

    def read_instances(self, first, count):
        """The instance records of nodes [first, first + count) as the kernels read them (vkrt_debug_read_instances, synchronises): a
        numpy array of INSTANCE_DTYPE, 96 B per node -- o2w (12 floats, row-major 3x4), w2o (9 floats), primMesh, vis, pad."""
        ok = all(not isinstance(x, bool) and isinstance(x, (int, np.integer)) for x in (first, count))
        nodes = self._prim_mesh.shape[0]
        if not ok or first < 0 or count < 0 or int(first) + int(count) > nodes:
            raise VkrtError(f"read_instances: nodes [{first}, {first} + {count}) outside the scene's {nodes} nodes")
        out = np.zeros(max(int(count), 1), INSTANCE_DTYPE)
        _check(self.lib.vkrt_debug_read_instances(self._h, int(first), int(count), out.ctypes.data, 96 * int(count)), "vkrt_debug_read_instances")
        return out[:int(count)]

    def set_instance_visibility(self, first, masks, flags=None, stream=None):
        """vkrt_scene_set_instance_visibility for nodes [first, first + n): masks = n ints in 1..255 (the instance masks of the
        ray-query cull mask); flags = n ints of VKRT_INSTANCE_* bits, or None to keep the nodes' current flags.  Enqueued on `stream`
        (a torch stream; None = the default stream); queries enqueued after it on that stream see the new values.  Bad values and
        ranges are refused here, before the call."""
        m = np.asarray(masks).reshape(-1)
        first, n = int(first), m.shape[0]
        nodes = self._prim_mesh.shape[0]
        if first < 0 or first + n > nodes:
            raise VkrtError(f"set_instance_visibility: nodes [{first}, {first + n}) outside the scene's {nodes} nodes")
        if m.dtype.kind not in "iu" or np.any(m < 1) or np.any(m > 255):
            raise VkrtError("set_instance_visibility: masks must be integers in 1..255 (hide an instance with a zero-scale transform)")
        if flags is None:
            f = self.instance_visibility()[1][first:first + n]
        else:
            f = np.asarray(flags).reshape(-1)
            known = abi.VKRT_INSTANCE_FACING_CULL_DISABLE | abi.VKRT_INSTANCE_FLIP_FACING
            if f.shape[0] != n or f.dtype.kind not in "iu" or np.any(f.astype(np.int64) & ~known) or np.any(f < 0):
                raise VkrtError(f"set_instance_visibility: flags must be {n} integers of VKRT_INSTANCE_* bits")
        arr = (abi.InstanceVisibility * max(n, 1))()
        for i in range(n):
            arr[i].mask, arr[i].flags, arr[i].reserved = int(m[i]), int(f[i]), 0
        st = C.c_void_p(stream.cuda_stream) if stream is not None else None
        _check(self.lib.vkrt_scene_set_instance_visibility(self._h, first, n, arr, st), "vkrt_scene_set_instance_visibility")

    def instance_visibility(self):
        """(masks, flags): uint8 [nodes] each, the host copy of every node's visibility (vkrt_scene_get_instance_visibility)."""
        n = self._prim_mesh.shape[0]
        arr = (abi.InstanceVisibility * max(n, 1))()
        _check(self.lib.vkrt_scene_get_instance_visibility(self._h, 0, n, arr), "vkrt_scene_get_instance_visibility")
        return (np.array([arr[i].mask for i in range(n)], np.uint8), np.array([arr[i].flags for i in range(n)], np.uint8))

    def set_material_alpha(self, first, modes, cutoffs=0.5, stream=None):
        """vkrt_scene_set_material_alpha for materials [first, first + n): modes = n ints, ALPHA_OPAQUE or ALPHA_MASK (glTF's alphaMode);
        cutoffs = one finite number >= 0 for all of them or n of them (glTF's alphaCutoff).  A candidate hit of intersect, occluded
        and intersect_multi on a MASK material is ignored when its alpha (Surfaces.alpha at that hit) is not >= the cutoff.  Enqueued
        on `stream` (a torch stream; None = the default stream); queries enqueued after it on that stream see the new values.  Bad
        values and ranges are refused here, before the call."""
        m = np.asarray(modes).reshape(-1)
        if isinstance(first, bool) or not isinstance(first, (int, np.integer)):
            raise VkrtError(f"set_material_alpha: first must be an integer, got {type(first).__name__}")
        first, n = int(first), m.shape[0]
        if first < 0 or first + n > self._material_count:
            raise VkrtError(f"set_material_alpha: materials [{first}, {first + n}) outside the scene's {self._material_count} materials")
        if m.dtype.kind not in "iu" or np.any((m != ALPHA_OPAQUE) & (m != ALPHA_MASK)):
            raise VkrtError("set_material_alpha: modes must be integers, ALPHA_OPAQUE (0) or ALPHA_MASK (1)")
        c = np.asarray(cutoffs)
        if c.dtype.kind not in "fiu":
            raise VkrtError(f"set_material_alpha: cutoffs must be numbers, got {c.dtype}")
        c = c.astype(np.float32).reshape(-1)
        if c.shape[0] == 1:
            c = np.repeat(c, n)
        if c.shape[0] != n or not np.all(np.isfinite(c)) or np.any(c < 0):
            raise VkrtError(f"set_material_alpha: cutoffs must be one or {n} finite numbers >= 0")
        arr = (abi.MaterialAlpha * max(n, 1))()
        for i in range(n):
            arr[i].mode, arr[i].cutoff = int(m[i]), float(c[i])
        st = C.c_void_p(stream.cuda_stream) if stream is not None else None
        _check(self.lib.vkrt_scene_set_material_alpha(self._h, first, n, arr, st), "vkrt_scene_set_material_alpha")

    def material_alpha(self):
        """(modes, cutoffs): uint32 and float32 [materials], the host copy of every material's alpha mode
        (vkrt_scene_get_material_alpha)."""
        n = self._material_count
        arr = (abi.MaterialAlpha * max(n, 1))()
        _check(self.lib.vkrt_scene_get_material_alpha(self._h, 0, n, arr), "vkrt_scene_get_material_alpha")
        return (np.array([arr[i].mode for i in range(n)], np.uint32), np.array([arr[i].cutoff for i in range(n)], np.float32))

    @staticmethod
    def _int_range(who, what, first, n, total):
        """`first` as an int, with [first, first + n) inside the scene's `total` records"""
        ok = not isinstance(first, bool) and isinstance(first, (int, np.integer)) and not isinstance(n, bool) and isinstance(n, (int, np.integer))
        if not ok or first < 0 or n < 0 or int(first) + int(n) > total:
            raise VkrtError(f"{who}: {what} [{first}, {first} + {n}) outside the scene's {total} {what}")
        return int(first)

    def _device_tensor(self, who, name, a, dtype, shape):
        """the address of a contiguous, 16-byte aligned torch tensor of `dtype` and `shape` on the scene's device"""
        if not a.is_cuda or a.device.index != self.device:
            raise VkrtError(f"{who}: {name} is on {a.device}, the scene is on cuda:{self.device}")
        if a.dtype != dtype:
            raise VkrtError(f"{who}: {name} is {a.dtype}, expected {dtype}")
        if not a.is_contiguous():
            raise VkrtError(f"{who}: {name} must be contiguous")
        if a.shape != shape:
            raise VkrtError(f"{who}: {name} has shape {tuple(a.shape)}, expected {shape}")
        if a.data_ptr() % 16:
            raise VkrtError(f"{who}: {name} must be 16-byte aligned")
        return a.data_ptr()

    def update_lights(self, first, lights, stream=None):
        """vkrt_scene_update_lights: new records for lights [first, first + n), taken as given.  lights: a numpy array of LIGHT_DTYPE
        (n,) takes the host path (copied before return, no wait); a contiguous float32 (n, 8) torch tensor on the scene's device --
        position, color, intensity, and the bits of the int32 type -- takes the device path: one stream-ordered copy, no
        synchronisation, the tensor must live until `stream` has passed the call.  Enqueued on `stream` (a torch stream; None = the
        default stream); the next frame on it sees the new lights, without a refit.  Refused here, before the call: a wrong dtype,
        shape or device, a non-contiguous or misaligned tensor, a range outside the scene's lights."""
        who = "update_lights"
        if isinstance(lights, np.ndarray):
            if lights.dtype != LIGHT_DTYPE or lights.ndim != 1:
                raise VkrtError(f"{who}: lights is {lights.dtype} of shape {lights.shape}, expected LIGHT_DTYPE (n,)")
            keep = np.ascontiguousarray(lights)
            n, ptr, memory = int(keep.shape[0]), keep.ctypes.data, _HOST
        else:
            torch = _torch or _import_torch()
            if not isinstance(lights, torch.Tensor):
                raise VkrtError(f"{who}: lights must be a numpy array or a torch tensor, got {type(lights).__name__}")
            ptr, memory = self._device_tensor(who, "lights", lights, torch.float32, (_N, 8)), _DEVICE
            n = int(lights.shape[0])
        first = self._int_range(who, "lights", first, n, self.lights_count)
        u = abi.LightUpdate(C.sizeof(abi.LightUpdate), first, n, memory, ptr)
        st = C.c_void_p(stream.cuda_stream) if stream is not None else None
        _check(self.lib.vkrt_scene_update_lights(self._h, C.byref(u), st), "vkrt_scene_update_lights")

    def update_materials(self, first, materials, stream=None):
        """vkrt_scene_update_materials: new materials [first, first + n) from a numpy array of MAT_DTYPE (n,), copied before return;
        both device records of each are re-made as at scene creation and enqueued on `stream` (a torch stream; None = the default
        stream) with no wait.  Alpha modes and cutoffs stay (set_material_alpha); texture indices may change among the scene's
        textures.  Under VKRT_OPT_ANYHIT_DISSOLVE a material that becomes non-opaque (alpha < 1) asks for build() before the next
        trace (include/vkrt.h).  Refused here, before the call: a wrong dtype or shape, a range outside the scene's materials, a
        texture index beyond the scene's textures."""
        who = "update_materials"
        if not isinstance(materials, np.ndarray) or materials.dtype != MAT_DTYPE or materials.ndim != 1:
            raise VkrtError(f"{who}: materials must be a numpy array of MAT_DTYPE (n,), got {getattr(materials, 'dtype', type(materials).__name__)}")
        keep = np.ascontiguousarray(materials)
        n = int(keep.shape[0])
        first = self._int_range(who, "materials", first, n, self._material_count)
        textures = len(self._texture_sizes)
        for k in ("pbrBaseColorTexture", "metallicRoughnessTexture", "normalTexture", "emissiveTexture"):
            if textures and n and int(keep[k].max()) >= textures:
                raise VkrtError(f"{who}: {k} {int(keep[k].max())} beyond the scene's {textures} textures")
        st = C.c_void_p(stream.cuda_stream) if stream is not None else None
        _check(self.lib.vkrt_scene_update_materials(self._h, first, n, keep.ctypes.data, st), "vkrt_scene_update_materials")

    def update_texture(self, texture, rgba8, stream=None):
        """vkrt_scene_update_texture: a new image for texture `texture`, uint8 (height, width, 4) of the texture's own size.  A numpy
        array takes the host path (staged, the call waits for `stream`); a contiguous torch tensor on the scene's device takes the
        device path: no copy, no synchronisation, the tensor must live until `stream` has passed the call.  Level 0, the footprint
        records and every mip level are rebuilt on the device, bit for bit what scene creation packs from the image.  Enqueued on
        `stream` (a torch stream; None = the default stream); no refit is needed.  Refused here, before the call: a texture index out
        of range, a wrong dtype, size or device, a non-contiguous or misaligned tensor."""
        who = "update_texture"
        if isinstance(texture, bool) or not isinstance(texture, (int, np.integer)) or not 0 <= texture < len(self._texture_sizes):
            raise VkrtError(f"{who}: texture {texture!r} outside the scene's {len(self._texture_sizes)} textures")
        w, h = self._texture_sizes[int(texture)]
        if isinstance(rgba8, np.ndarray):
            if rgba8.dtype != np.uint8 or rgba8.shape != (h, w, 4):
                raise VkrtError(f"{who}: rgba8 is {rgba8.dtype} of shape {rgba8.shape}, expected uint8 ({h}, {w}, 4)")
            keep = np.ascontiguousarray(rgba8)
            ptr, memory = keep.ctypes.data, _HOST
        else:
            torch = _torch or _import_torch()
            if not isinstance(rgba8, torch.Tensor):
                raise VkrtError(f"{who}: rgba8 must be a numpy array or a torch tensor, got {type(rgba8).__name__}")
            ptr, memory = self._device_tensor(who, "rgba8", rgba8, torch.uint8, (h, w, 4)), _DEVICE
        u = abi.TextureUpdate(C.sizeof(abi.TextureUpdate), int(texture), w, h, memory, ptr)
        st = C.c_void_p(stream.cuda_stream) if stream is not None else None
        _check(self.lib.vkrt_scene_update_texture(self._h, C.byref(u), st), "vkrt_scene_update_texture")

    def read_lights(self, first, count):
        """The light records [first, first + count) as the kernels read them (vkrt_debug_read_lights, synchronises): LIGHT_DTYPE."""
        first = self._int_range("read_lights", "lights", first, count, self.lights_count)
        out = np.zeros(max(int(count), 1), LIGHT_DTYPE)
        _check(self.lib.vkrt_debug_read_lights(self._h, first, int(count), out.ctypes.data, 32 * int(count)), "vkrt_debug_read_lights")
        return out[:int(count)]

    def read_materials(self, first, count):
        """Both device records of materials [first, first + count) (vkrt_debug_read_materials, synchronises): MATERIAL_RECORD_DTYPE,
        192 B per material."""
        first = self._int_range("read_materials", "materials", first, count, self._material_count)
        out = np.zeros(max(int(count), 1), MATERIAL_RECORD_DTYPE)
        _check(self.lib.vkrt_debug_read_materials(self._h, first, int(count), out.ctypes.data, 192 * int(count)), "vkrt_debug_read_materials")
        return out[:int(count)]

    def read_texture(self, texture, level=0, quads=False):
        """One level of one texture as the kernels read it (vkrt_debug_read_texture, synchronises): uint8 (h, w, 4) of the level's
        size; with quads (level 0 only) a pair of it and the texture's footprint records, uint32 (h, w, 4).  A scene without a
        footprint pool refuses quads with VKRT_ERR_UNSUPPORTED."""
        who = "read_texture"
        if isinstance(texture, bool) or not isinstance(texture, (int, np.integer)) or not 0 <= texture < len(self._texture_sizes):
            raise VkrtError(f"{who}: texture {texture!r} outside the scene's {len(self._texture_sizes)} textures")
        w, h = self._texture_sizes[int(texture)]
        levels = int(np.floor(np.log2(max(w, h)))) + 1
        if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 0 <= level < min(levels, 16) or (quads and level != 0):
            raise VkrtError(f"{who}: level {level!r} outside texture {texture}'s {min(levels, 16)} levels (quads: level 0 only)")
        lw, lh = max(1, w >> int(level)), max(1, h >> int(level))
        texels = np.zeros((lh, lw, 4), np.uint8)
        q = np.zeros((lh, lw, 4), np.uint32) if quads else None
        _check(self.lib.vkrt_debug_read_texture(self._h, int(texture), int(level), texels.ctypes.data, texels.nbytes, q.ctypes.data if quads else None,
                                                q.nbytes if quads else 0), "vkrt_debug_read_texture")
        return (texels, q) if quads else texels

    def read_node_masks(self):
        """The wide8 tree's node-mask table (vkrt_debug_read_node_masks): uint8 [nodes, 8], byte s = the OR of the instance masks
        under child slot s."""
        nb = int(self.accel_info()["node_bytes"]) // 80 * 8
        out = np.zeros(max(nb, 8), np.uint8)
        _check(self.lib.vkrt_debug_read_node_masks(self._h, out.ctypes.data, nb), "vkrt_debug_read_node_masks")
        return out[:nb].reshape(-1, 8)

    def read_triangle_ids(self):
        """The flattened triangle id of every slot of the installed tree (vkrt_debug_read_triangle_ids): uint32 [slots], in the
        order of read_accel()["tris"]."""
        nb = int(self.accel_info()["triangle_bytes"]) // 48 * 4
        out = np.zeros(max(nb, 4) // 4, np.uint32)
        _check(self.lib.vkrt_debug_read_triangle_ids(self._h, out.ctypes.data, nb), "vkrt_debug_read_triangle_ids")
        return out[: nb // 4]

    def split_references(self, percent):
        """What triangle pre-splitting makes of the scene for a budget of `percent` % (vkrt_debug_split_references, synchronises; needs no
        tree): a dict of numpy arrays -- "prio" float32 [T], "scale" float32 (D), "ref_tri" uint32 [R] and "ref_box" float32 [R, 6] (lo3,
        hi3) in emission order, and "ref_count" = R."""
        T = self._triangle_count
        cap = T + T * int(percent) // 100
        prio = np.zeros(max(T, 1), np.float32)
        scale = np.zeros(1, np.float32)
        tri = np.zeros(max(cap, 1), np.uint32)
        box = np.zeros((max(cap, 1), 6), np.float32)
        n = C.c_uint32(0)
        _check(self.lib.vkrt_debug_split_references(self._h, int(percent), prio.ctypes.data, scale.ctypes.data, tri.ctypes.data, box.ctypes.data, cap,
                                                    C.byref(n)), "vkrt_debug_split_references")
        R = int(n.value)
        return {"prio": prio[:T], "scale": scale[0], "ref_tri": tri[:R].copy(), "ref_box": box[:R].copy(), "ref_count": R}

    def refit(self, stream=None):
        """vkrt_accel_refit: the built tree follows the current node transforms and vertices (same topology, new boxes), enqueued on
        `stream`."""
        st = C.c_void_p(stream.cuda_stream) if stream is not None else None
        _check(self.lib.vkrt_accel_refit(self._h, st), "vkrt_accel_refit")

    def close(self):
        if getattr(self, "_h", None):
            self.lib.vkrt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def accel_info(self):
        info = abi.AccelInfo()
        _check(self.lib.vkrt_accel_get_info(self._h, C.byref(info)), "vkrt_accel_get_info")
        return {n: getattr(info, n) for n, _ in info._fields_}

    def check_accel(self):
        """Structural check of the built tree (vkrt_debug_check_accel): dict of counts; a sound tree has every triangle once and
        no violations."""
        c = abi.AccelCheck()
        _check(self.lib.vkrt_debug_check_accel(self._h, C.byref(c)), "vkrt_debug_check_accel")
        return {n: getattr(c, n) for n, _ in c._fields_}

    def read_accel(self):
        """The installed tree as the kernels read it (vkrt_debug_read_accel): {"layout": 1 wide8 / 0 BVH2, "root_ref": int,
        "nodes": uint32 [N, 20] (wide8) or float32 [N, 16] (BVH2), "tris": float32 [T, 12] records in slot order}."""
        info = self.accel_info()
        nb, tb = int(info["node_bytes"]), int(info["triangle_bytes"])
        nodes = np.zeros(max(nb, 4) // 4, np.uint32)
        tris = np.zeros(max(tb, 4) // 4, np.float32)
        root = C.c_int32()
        _check(self.lib.vkrt_debug_read_accel(self._h, nodes.ctypes.data, nb, tris.ctypes.data, tb, C.byref(root)), "vkrt_debug_read_accel")
        layout = int(self.check_accel()["layout"])
        nodes, tris = nodes[: nb // 4], tris[: tb // 4]
        nodes = nodes.reshape(-1, 20) if layout == 1 else nodes.view(np.float32).reshape(-1, 16)
        return {"layout": layout, "root_ref": int(root.value), "nodes": nodes, "tris": tris.reshape(-1, 12)}

    def shard_rows(self, shard):
        return int(self.lib.vkrt_shard_rows(C.byref(shard)))

    def pathtrace(self, pc, cam, width, height, seed=0, flags=0, shard=None, image=None, stream=None):
        """One launch (one frame).  image: torch float32 CUDA tensor [rows, width, 4] (in/out when pc.frame > 0)."""
        import torch

        shard = shard or whole_image_shard(width, height)
        rows = self.shard_rows(shard)
        if image is None:
            image = torch.zeros((rows, width, 4), dtype=torch.float32, device=f"cuda:{self.device}")
        assert image.is_cuda and image.dtype == torch.float32 and image.is_contiguous() and tuple(image.shape) == (rows, width, 4)
        if stream is None:
            stream = torch.cuda.current_stream(image.device)
        opts = abi.TraceOpts(seed & 0xFFFFFFFF, flags)
        _check(self.lib.vkrt_pathtrace(self._h, C.byref(pc), C.byref(cam), C.byref(opts), C.byref(shard),
                                       C.c_void_p(image.data_ptr()), C.c_void_p(stream.cuda_stream)), "vkrt_pathtrace")
        return image

    def pathtrace_frames(self, pc, cam, width, height, n_frames, seed=0, flags=0, shard=None, image=None, stream=None):
        """n_frames progressive frames in one call (vkrt_pathtrace_frames): frame i uses pc.frame + i and seed + i."""
        import torch

        shard = shard or whole_image_shard(width, height)
        rows = self.shard_rows(shard)
        if image is None:
            image = torch.zeros((rows, width, 4), dtype=torch.float32, device=f"cuda:{self.device}")
        assert image.is_cuda and image.dtype == torch.float32 and image.is_contiguous() and tuple(image.shape) == (rows, width, 4)
        if stream is None:
            stream = torch.cuda.current_stream(image.device)
        opts = abi.TraceOpts(seed & 0xFFFFFFFF, flags)
        _check(self.lib.vkrt_pathtrace_frames(self._h, C.byref(pc), C.byref(cam), C.byref(opts), C.byref(shard),
                                              C.c_void_p(image.data_ptr()), int(n_frames), C.c_void_p(stream.cuda_stream)), "vkrt_pathtrace_frames")
        return image

    # ---- hybrid mode (reference rtMode == 0) ---------------------------------------------------------
    def gbuffer_raycast(self, cam, width, height, lights_count=None, clear_color=(1.0, 1.0, 1.0, 1.0), shard=None, stream=None, view_matrix=None,
                        hits=False, motion=False):
        """Stand-in for rasterizeGltf: returns dict of torch CUDA planes color/position/normal [rows,W,4], roughMetal [rows,W,2].
        view_matrix (16 floats, column-major pcRaster.viewMatrix): also the NRD front-end planes nrdNormalRoughness [rows,W,4],
        nrdViewZ [rows,W], nrdRadianceHitDist [rows,W,4] (vkrt_gbuffer_raycast_nrd).
        hits=True: also "hits" [rows,W,8], one vkrt_hit per pixel (vkrt_gbuffer_raycast_hits; RayHits(g["hits"].view(-1, 8)) names its
        fields).  motion=True: hits, and "prevPosition" [rows,W,4], where each pixel's surface point was at the last motion_mark()
        (hit_motion on the same stream): Denoiser.denoise then follows moving and deforming geometry."""
        import torch

        shard = shard or whole_image_shard(width, height)
        rows = self.shard_rows(shard)
        dev = f"cuda:{self.device}"
        g = {"color": torch.zeros((rows, width, 4), dtype=torch.float32, device=dev), "position": torch.zeros((rows, width, 4), dtype=torch.float32, device=dev),
             "normal": torch.zeros((rows, width, 4), dtype=torch.float32, device=dev), "roughMetal": torch.zeros((rows, width, 2), dtype=torch.float32, device=dev)}
        stream = stream or torch.cuda.current_stream(g["color"].device)
        gb = abi.Gbuffer(*(g[k].data_ptr() for k in ("color", "position", "normal", "roughMetal")))
        cc = (C.c_float * 4)(*clear_color)
        n = self.lights_count if lights_count is None else lights_count
        nrd = vm = None
        if view_matrix is not None:
            g["nrdNormalRoughness"] = torch.zeros((rows, width, 4), dtype=torch.float32, device=dev)
            g["nrdViewZ"] = torch.zeros((rows, width), dtype=torch.float32, device=dev)
            g["nrdRadianceHitDist"] = torch.zeros((rows, width, 4), dtype=torch.float32, device=dev)
            nrd = abi.NrdPlanes(g["nrdNormalRoughness"].data_ptr(), g["nrdViewZ"].data_ptr(), g["nrdRadianceHitDist"].data_ptr())
            vm = (C.c_float * 16)(*[float(v) for v in view_matrix])
        if hits or motion:
            g["hits"] = torch.zeros((rows, width, 8), dtype=torch.float32, device=dev)
            _check(self.lib.vkrt_gbuffer_raycast_hits(self._h, C.byref(cc), n, C.byref(cam), None if vm is None else C.byref(vm), C.byref(shard), C.byref(gb),
                                                      None if nrd is None else C.byref(nrd), C.c_void_p(g["hits"].data_ptr()),
                                                      C.c_void_p(stream.cuda_stream)), "vkrt_gbuffer_raycast_hits")
            if motion:
                g["prevPosition"] = self.hit_motion(g["hits"].view(-1, 8), current=False, previous=True, stream=stream)[1].view(rows, width, 4)
            return g
        if view_matrix is not None:
            _check(self.lib.vkrt_gbuffer_raycast_nrd(self._h, C.byref(cc), n, C.byref(cam), C.byref(vm), C.byref(shard), C.byref(gb), C.byref(nrd),
                                                     C.c_void_p(stream.cuda_stream)), "vkrt_gbuffer_raycast_nrd")
            return g
        _check(self.lib.vkrt_gbuffer_raycast(self._h, C.byref(cc), n, C.byref(cam), C.byref(shard), C.byref(gb), C.c_void_p(stream.cuda_stream)),
               "vkrt_gbuffer_raycast")
        return g

    def hybrid_trace(self, pc, cam, width, height, gbuffer, seed=0, flags=0, shard=None, accum=None, stream=None):
        """raytraceHybrid.rgen: accum [rows,W,4] (in/out when pc.frame > 0)."""
        import torch

        shard = shard or whole_image_shard(width, height)
        rows = self.shard_rows(shard)
        if accum is None:
            accum = torch.zeros((rows, width, 4), dtype=torch.float32, device=f"cuda:{self.device}")
        stream = stream or torch.cuda.current_stream(accum.device)
        gb = abi.Gbuffer(*(gbuffer[k].data_ptr() for k in ("color", "position", "normal", "roughMetal")))
        opts = abi.TraceOpts(seed & 0xFFFFFFFF, flags)
        if "nrdViewZ" in gbuffer:  # planes from gbuffer_raycast(view_matrix=...): also pack the REBLUR input (rgen:273-281)
            nrd = abi.NrdPlanes(gbuffer["nrdNormalRoughness"].data_ptr(), gbuffer["nrdViewZ"].data_ptr(), gbuffer["nrdRadianceHitDist"].data_ptr())
            _check(self.lib.vkrt_hybrid_trace_nrd(self._h, C.byref(pc), C.byref(cam), C.byref(opts), C.byref(shard), C.byref(gb), C.byref(nrd),
                                                  C.c_void_p(accum.data_ptr()), C.c_void_p(stream.cuda_stream)), "vkrt_hybrid_trace_nrd")
            return accum
        _check(self.lib.vkrt_hybrid_trace(self._h, C.byref(pc), C.byref(cam), C.byref(opts), C.byref(shard), C.byref(gb),
                                          C.c_void_p(accum.data_ptr()), C.c_void_p(stream.cuda_stream)), "vkrt_hybrid_trace")
        return accum

    def post(self, main_img, rt_img=None, rt_mode=0, view_accumulated=0, use_gi=0, stream=None):
        """post.frag composite + gamma; returns a new [.,.,4] tensor."""
        import torch

        out = torch.empty_like(main_img)
        stream = stream or torch.cuda.current_stream(main_img.device)
        pcp = abi.PushConstantPost(1.0, rt_mode, view_accumulated, use_gi)
        _check(self.lib.vkrt_post(self.device, C.byref(pcp), main_img.numel() // 4, C.c_void_p(main_img.data_ptr()),
                                  C.c_void_p(rt_img.data_ptr()) if rt_img is not None else None, C.c_void_p(out.data_ptr()),
                                  C.c_void_p(stream.cuda_stream)), "vkrt_post")
        return out

    def reset_counters(self, stream=None):
        _check(self.lib.vkrt_counters_reset(self._h, C.c_void_p(stream.cuda_stream) if stream is not None else None),
               "vkrt_counters_reset")

    def counters(self):
        c = abi.Counters()
        _check(self.lib.vkrt_counters_read(self._h, C.byref(c)), "vkrt_counters_read")
        return c.as_dict()

    def last_trace_ms(self):
        ms = C.c_float()
        _check(self.lib.vkrt_last_trace_ms(self._h, C.byref(ms)), "vkrt_last_trace_ms")
        return float(ms.value)

    def last_trace_timing(self):
        t = abi.TraceTiming()
        _check(self.lib.vkrt_last_trace_timing(self._h, C.byref(t)), "vkrt_last_trace_timing")
        return {"total_ms": float(t.total_ms), "traverse_ms": float(t.traverse_ms), "traverse_launches": int(t.traverse_launches),
                "mode": "wavefront" if t.mode == 1 else "megakernel", "shade_ms": float(t.shade_ms), "shade_launches": int(t.shade_launches)}

    # ---- ray queries (vkrt_intersect / vkrt_occluded) --------------------------------------------------------------------------
    def _query_args(self, rays, what):
        """Refuse what the C ABI cannot take, before the call: rays must be a contiguous, 16-byte aligned float32 [N, 8] tensor on
        this renderer's device."""
        import torch

        if not isinstance(rays, torch.Tensor):
            raise VkrtError(f"{what}: rays must be a torch tensor (pack_rays), got {type(rays).__name__}")
        if not rays.is_cuda:
            raise VkrtError(f"{what}: rays are on {rays.device}, the scene is on cuda:{self.device}")
        if rays.device.index != self.device:
            raise VkrtError(f"{what}: rays are on {rays.device}, the scene is on cuda:{self.device}")
        if rays.dtype != torch.float32:
            raise VkrtError(f"{what}: rays are {rays.dtype}, expected torch.float32")
        if rays.dim() != 2 or rays.shape[1] != 8:
            raise VkrtError(f"{what}: rays have shape {tuple(rays.shape)}, expected [N, 8]")
        if not rays.is_contiguous() or rays.data_ptr() % 16 != 0:
            raise VkrtError(f"{what}: rays must be contiguous and 16-byte aligned")
        if rays.shape[0] >= 1 << 32:
            raise VkrtError(f"{what}: {rays.shape[0]} rays, at most 2^32 - 1 per call")
        return int(rays.shape[0])

    def _query_out(self, out, shape, what, align):
        import torch

        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.device.index != self.device:
            raise VkrtError(f"{what}: out must be a tensor on cuda:{self.device}")
        if out.dtype not in (torch.float32, torch.int32) or tuple(out.shape) != shape:
            raise VkrtError(f"{what}: out is {out.dtype} {tuple(out.shape)}, expected a 4-byte dtype of shape {shape}")
        if not out.is_contiguous() or out.data_ptr() % align != 0:
            raise VkrtError(f"{what}: out must be contiguous and {align}-byte aligned")
        return out

    @staticmethod
    def _query_opts(cull_mask, ray_flags, seed, what):
        """None for the defaults (the call of vkrt_intersect / vkrt_occluded), else the vkrt_query_opts of the _ex call; refuses what
        the library would refuse."""
        if isinstance(cull_mask, bool) or not isinstance(cull_mask, (int, np.integer)) or not 0 <= int(cull_mask) <= 0xFF:
            raise VkrtError(f"{what}: cull_mask must be an integer in 0..255, got {cull_mask!r}")
        known = abi.VKRT_RAY_OPAQUE | abi.VKRT_RAY_CULL_BACK_FACING | abi.VKRT_RAY_CULL_FRONT_FACING
        if isinstance(ray_flags, bool) or not isinstance(ray_flags, (int, np.integer)) or int(ray_flags) < 0 or int(ray_flags) & ~known:
            raise VkrtError(f"{what}: ray_flags must combine VKRT_RAY_OPAQUE / CULL_BACK_FACING / CULL_FRONT_FACING, got {ray_flags!r}")
        both = abi.VKRT_RAY_CULL_BACK_FACING | abi.VKRT_RAY_CULL_FRONT_FACING
        if int(ray_flags) & both == both:
            raise VkrtError(f"{what}: ray_flags: CULL_BACK_FACING and CULL_FRONT_FACING together")
        if int(cull_mask) == 0xFF and int(ray_flags) == 0:
            return None
        return abi.QueryOpts(C.sizeof(abi.QueryOpts), int(ray_flags), int(cull_mask), int(seed) & 0xFFFFFFFF)

    def intersect(self, rays, seed=0, out=None, stream=None, cull_mask=0xFF, ray_flags=0):
        """Closest hit of every ray (vkrt_intersect), enqueued on `stream` (default: the current stream of the scene's device).
        rays: float32 [N, 8] from pack_rays; seed: the any-hit stage's payload seed (VKRT_OPT_ANYHIT_DISSOLVE); out: an optional
        float32 / int32 [N, 8] buffer to write into.  cull_mask (0..255) / ray_flags (VKRT_RAY_*): the options of vkrt_intersect_ex,
        against the masks and flags of set_instance_visibility.  Returns a RayHits of views of that buffer."""
        import torch

        n = self._query_args(rays, "intersect")
        opts = self._query_opts(cull_mask, ray_flags, seed, "intersect")
        if stream is None:
            stream = torch.cuda.current_stream(rays.device)
        if out is None:
            with torch.cuda.stream(stream):  # (allocated on the stream that writes it)
                out = torch.empty((n, 8), dtype=torch.float32, device=rays.device)
        self._query_out(out, (n, 8), "intersect", 16)
        if opts is None:
            _check(self.lib.vkrt_intersect(self._h, C.c_void_p(rays.data_ptr()), n, int(seed) & 0xFFFFFFFF, C.c_void_p(out.data_ptr()),
                                           C.c_void_p(stream.cuda_stream)), "vkrt_intersect")
        else:
            _check(self.lib.vkrt_intersect_ex(self._h, C.c_void_p(rays.data_ptr()), n, C.byref(opts), C.c_void_p(out.data_ptr()),
                                              C.c_void_p(stream.cuda_stream)), "vkrt_intersect_ex")
        return RayHits(out)

    def intersect_multi(self, rays, max_hits, seed=0, out=None, counts=None, stream=None, cull_mask=0xFF, ray_flags=0):
        """The first max_hits (1..VKRT_MULTIHIT_MAX) hits along every ray in the order (t, triangle id) (vkrt_intersect_multi), enqueued
        like intersect() and with its seed / cull_mask / ray_flags.  out: an optional float32 / int32 [N, max_hits, 8] buffer, counts: an
        optional int32 [N] buffer to write into.  Returns a MultiHits of views of the two."""
        import torch

        n = self._query_args(rays, "intersect_multi")
        if isinstance(max_hits, bool) or not isinstance(max_hits, (int, np.integer)) or not 1 <= int(max_hits) <= abi.VKRT_MULTIHIT_MAX:
            raise VkrtError(f"intersect_multi: max_hits must be an integer in 1..{abi.VKRT_MULTIHIT_MAX}, got {max_hits!r}")
        k = int(max_hits)
        opts = self._query_opts(cull_mask, ray_flags, seed, "intersect_multi")
        if opts is None:
            opts = abi.QueryOpts(C.sizeof(abi.QueryOpts), 0, 0xFF, int(seed) & 0xFFFFFFFF)
        if stream is None:
            stream = torch.cuda.current_stream(rays.device)
        with torch.cuda.stream(stream):  # (allocated on the stream that writes them)
            if out is None:
                out = torch.empty((n, k, 8), dtype=torch.float32, device=rays.device)
            if counts is None:
                counts = torch.empty((n,), dtype=torch.int32, device=rays.device)
        self._query_out(out, (n, k, 8), "intersect_multi", 16)
        if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32:
            raise VkrtError("intersect_multi: counts must be an int32 tensor")
        self._query_out(counts, (n,), "intersect_multi", 4)
        _check(self.lib.vkrt_intersect_multi(self._h, C.c_void_p(rays.data_ptr()), n, C.byref(opts), k, C.c_void_p(out.data_ptr()),
                                             C.c_void_p(counts.data_ptr()), C.c_void_p(stream.cuda_stream)), "vkrt_intersect_multi")
        return MultiHits(out, counts)

    def occluded(self, rays, seed=0, out=None, stream=None, cull_mask=0xFF, ray_flags=0):
        """1 where some hit lies in (tmin, tmax), else 0 (vkrt_occluded): int32 [N] (or `out`), enqueued like intersect(), with the
        same cull_mask / ray_flags options."""
        import torch

        n = self._query_args(rays, "occluded")
        opts = self._query_opts(cull_mask, ray_flags, seed, "occluded")
        if stream is None:
            stream = torch.cuda.current_stream(rays.device)
        if out is None:
            with torch.cuda.stream(stream):
                out = torch.empty((n,), dtype=torch.int32, device=rays.device)
        self._query_out(out, (n,), "occluded", 4)
        if opts is None:
            _check(self.lib.vkrt_occluded(self._h, C.c_void_p(rays.data_ptr()), n, int(seed) & 0xFFFFFFFF, C.c_void_p(out.data_ptr()),
                                          C.c_void_p(stream.cuda_stream)), "vkrt_occluded")
        else:
            _check(self.lib.vkrt_occluded_ex(self._h, C.c_void_p(rays.data_ptr()), n, C.byref(opts), C.c_void_p(out.data_ptr()),
                                             C.c_void_p(stream.cuda_stream)), "vkrt_occluded_ex")
        return out.view(torch.int32)

    # ---- closest-point queries (vkrt_closest_point) -------------------------------------------------------------------------------
    def _point_args(self, points, radius, what):
        """The float32 [N, 4] query tensor (point.xyz, radius) of a call: `points` itself when it is [N, 4], else [N, 3] points packed
        with `radius` (a scalar or [N] values).  Refuses what intersect() refuses of its rays."""
        import torch

        if not isinstance(points, torch.Tensor):
            raise VkrtError(f"{what}: points must be a torch tensor, got {type(points).__name__}")
        if not points.is_cuda or points.device.index != self.device:
            raise VkrtError(f"{what}: points are on {points.device}, the scene is on cuda:{self.device}")
        if points.dtype != torch.float32:
            raise VkrtError(f"{what}: points are {points.dtype}, expected torch.float32")
        if points.dim() != 2 or points.shape[1] not in (3, 4):
            raise VkrtError(f"{what}: points have shape {tuple(points.shape)}, expected [N, 4] or [N, 3]")
        if points.shape[0] >= 1 << 32:
            raise VkrtError(f"{what}: {points.shape[0]} points, at most 2^32 - 1 per call")
        if points.shape[1] == 3:
            n = int(points.shape[0])
            r = torch.as_tensor(radius, dtype=torch.float32, device=points.device)
            if r.dim() > 0 and r.numel() != n:
                raise VkrtError(f"{what}: {r.numel()} radii for {n} points")
            q = torch.empty((n, 4), dtype=torch.float32, device=points.device)
            q[:, 0:3] = points
            q[:, 3] = r.reshape(-1) if r.dim() > 0 else r
            points = q
        if not points.is_contiguous() or points.data_ptr() % 16 != 0:
            raise VkrtError(f"{what}: points must be contiguous and 16-byte aligned")
        return points

    @staticmethod
    def _point_opts(cull_mask, what):
        if isinstance(cull_mask, bool) or not isinstance(cull_mask, (int, np.integer)) or not 0 <= int(cull_mask) <= 0xFF:
            raise VkrtError(f"{what}: cull_mask must be an integer in 0..255, got {cull_mask!r}")
        return None if int(cull_mask) == 0xFF else abi.QueryOpts(C.sizeof(abi.QueryOpts), 0, int(cull_mask), 0)

    def closest_point(self, points, radius=float("inf"), out=None, stream=None, cull_mask=0xFF):
        """The nearest point of the scene's surface to every query point, within its radius (vkrt_closest_point), enqueued like
        intersect().  points: float32 [N, 4] (point.xyz, radius) on the scene's device, or [N, 3] with `radius` a scalar or [N] values;
        cull_mask (0..255): against the masks of set_instance_visibility.  Returns a RayHits: t = the distance, (instance, primitive, u,
        v) = the surface point -- what surface() takes -- and -1 / t = radius where nothing lies within the radius."""
        import torch

        q = self._point_args(points, radius, "closest_point")
        n = int(q.shape[0])
        opts = self._point_opts(cull_mask, "closest_point")
        if stream is None:
            stream = torch.cuda.current_stream(q.device)
        if out is None:
            with torch.cuda.stream(stream):  # (allocated on the stream that writes it)
                out = torch.empty((n, 8), dtype=torch.float32, device=q.device)
        self._query_out(out, (n, 8), "closest_point", 16)
        _check(self.lib.vkrt_closest_point(self._h, C.c_void_p(q.data_ptr()), n, None if opts is None else C.byref(opts),
                                           C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream)), "vkrt_closest_point")
        return RayHits(out)

    def closest_point_work(self, points, radius=float("inf"), cull_mask=0xFF):
        """Test hook (vkrt_debug_closest_point_work): the work of closest_point() on these queries -- host arrays, float32 [N, 4] or
        [N, 3] with `radius` -- as (nodes visited, triangle records tested) in total.  Synchronises."""
        p = np.asarray(points, np.float32)
        if p.ndim != 2 or p.shape[1] not in (3, 4):
            raise VkrtError(f"closest_point_work: points have shape {p.shape}, expected [N, 4] or [N, 3]")
        if p.shape[1] == 3:
            q = np.empty((p.shape[0], 4), np.float32)
            q[:, 0:3] = p
            q[:, 3] = np.asarray(radius, np.float32)
            p = q
        p = np.ascontiguousarray(p)
        opts = self._point_opts(cull_mask, "closest_point_work")
        work = (C.c_uint64 * 2)()
        _check(self.lib.vkrt_debug_closest_point_work(self._h, p.ctypes.data, int(p.shape[0]), None if opts is None else C.byref(opts), work),
               "vkrt_debug_closest_point_work")
        return int(work[0]), int(work[1])

    def _hits_arg(self, hits, what):
        """(buffer, n) of a RayHits or a float32 / int32 [N, 8] tensor of vkrt_hit records; refuses what the C ABI cannot take"""
        import torch

        buf = hits.buffer if isinstance(hits, RayHits) else hits
        if not isinstance(buf, torch.Tensor):
            raise VkrtError(f"{what}: hits must be a RayHits or a torch tensor, got {type(hits).__name__}")
        if not buf.is_cuda or buf.device.index != self.device:
            raise VkrtError(f"{what}: hits are on {buf.device}, the scene is on cuda:{self.device}")
        if buf.dtype not in (torch.float32, torch.int32):
            raise VkrtError(f"{what}: hits are {buf.dtype}, expected torch.float32 or torch.int32")
        if buf.dim() != 2 or buf.shape[1] != 8:
            raise VkrtError(f"{what}: hits have shape {tuple(buf.shape)}, expected [N, 8]")
        if not buf.is_contiguous() or buf.data_ptr() % 16 != 0:
            raise VkrtError(f"{what}: hits must be contiguous and 16-byte aligned")
        if buf.shape[0] >= 1 << 32:
            raise VkrtError(f"{what}: {buf.shape[0]} records, at most 2^32 - 1 per call")
        return buf, int(buf.shape[0])

    def surface(self, hits, material=True, out=None, stream=None):
        """Shading inputs at hit records (vkrt_hit_surface), enqueued on `stream` like intersect(): hits = a RayHits or a float32 /
        int32 [N, 8] tensor of vkrt_hit records on the scene's device; material=False: the geometry alone (no texel is read, the
        material fields are 0); out: an optional float32 / int32 [N, 32] buffer to write into.  Needs no tree: it works before
        build() and between update_nodes / update_vertices and refit().  Returns a Surfaces of views of that buffer."""
        import torch

        buf, n = self._hits_arg(hits, "surface")
        fields = abi.VKRT_SURFACE_GEOMETRY | (abi.VKRT_SURFACE_MATERIAL if material else 0)
        if stream is None:
            stream = torch.cuda.current_stream(buf.device)
        if out is None:
            with torch.cuda.stream(stream):
                out = torch.empty((n, 32), dtype=torch.float32, device=buf.device)
        self._query_out(out, (n, 32), "surface", 16)
        _check(self.lib.vkrt_hit_surface(self._h, C.c_void_p(buf.data_ptr()), n, fields, C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream)),
               "vkrt_hit_surface")
        return Surfaces(out)

    # ---- motion (vkrt_scene_motion_mark / vkrt_hit_motion) -----------------------------------------------------------------------
    def motion_mark(self, stream=None):
        """vkrt_scene_motion_mark: the node transforms and vertex positions as they are at this point of `stream` (a torch stream;
        None = the current one) become the scene's previous state -- call it before the frame's update_nodes / update_vertices.  The
        first call allocates the snapshot; before any call the previous state is the current one."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(torch.device("cuda", self.device))
        _check(self.lib.vkrt_scene_motion_mark(self._h, C.c_void_p(stream.cuda_stream)), "vkrt_scene_motion_mark")

    def hit_motion(self, hits, current=True, previous=True, stream=None):
        """The surface point of hit records now and at the last motion_mark() (vkrt_hit_motion), enqueued on `stream` like
        intersect(): hits = a RayHits or a float32 / int32 [N, 8] tensor of vkrt_hit records (g["hits"].view(-1, 8) of
        gbuffer_raycast(hits=True), or a caller's intersect()).  Returns (current, previous): float32 [N, 4] tensors (x, y, z, 1),
        all zero where the record is not a hit of the scene; None for the one not asked for.  Needs no tree, like surface()."""
        import torch

        buf, n = self._hits_arg(hits, "hit_motion")
        if not current and not previous:
            raise VkrtError("hit_motion: neither current nor previous asked for")
        if stream is None:
            stream = torch.cuda.current_stream(buf.device)
        with torch.cuda.stream(stream):  # (allocated on the stream that writes them)
            cur = torch.empty((n, 4), dtype=torch.float32, device=buf.device) if current else None
            prev = torch.empty((n, 4), dtype=torch.float32, device=buf.device) if previous else None
        _check(self.lib.vkrt_hit_motion(self._h, C.c_void_p(buf.data_ptr()), n, None if cur is None else C.c_void_p(cur.data_ptr()),
                                        None if prev is None else C.c_void_p(prev.data_ptr()), C.c_void_p(stream.cuda_stream)), "vkrt_hit_motion")
        return cur, prev

    def trace_rays(self, origins, directions, tmin=0.001, tmax=10000.0, any_hit=False):
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        n = o.shape[0]
        t, u, v = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        gid = np.zeros(n, np.int32)
        _check(self.lib.vkrt_debug_trace_rays(self._h, n, o.ctypes.data, d.ctypes.data, tmin, tmax, 1 if any_hit else 0,
                                              t.ctypes.data, u.ctypes.data, v.ctypes.data, gid.ctypes.data), "vkrt_debug_trace_rays")
        return t, u, v, gid


class Denoiser:
    """vkrt_denoise_diffuse: SVGF of the hybrid GI term (include/vkrt.h).  One handle per device and width x height; it keeps the
    history between calls, so hand it consecutive frames of one camera path (reset() at a cut)."""

    def __init__(self, device, width, height):
        self.lib = load_library()
        self.device, self.width, self.height = int(device), int(width), int(height)
        h = C.c_void_p()
        _check(self.lib.vkrt_denoiser_create(self.device, self.width, self.height, C.byref(h)), "vkrt_denoiser_create")
        self._h = h

    def denoise(self, cam, gbuffer, out=None, iterations=5, max_history=32, stream=None):
        """gbuffer: the dict Renderer.gbuffer_raycast(view_matrix=...) returns, after hybrid_trace filled its radiance plane; with a
        "prevPosition" plane in it (gbuffer_raycast(motion=True)) the call is vkrt_denoise_diffuse_motion.
        out: torch float32 [H, W, 4] on this device (.xyz written where there is geometry, the rest untouched); a zeroed one
        when None.  Returns out."""
        import torch

        W, H = self.width, self.height
        for k, ch in (("color", 4), ("position", 4), ("normal", 4), ("roughMetal", 2), ("nrdRadianceHitDist", 4)):
            t = gbuffer[k]
            if tuple(t.shape) != (H, W, ch) or t.dtype != torch.float32 or not t.is_contiguous():
                raise VkrtError(f"denoise: plane {k} is {tuple(t.shape)}, the denoiser was made for {(H, W, ch)}")
        if tuple(gbuffer["nrdViewZ"].shape) != (H, W):
            raise VkrtError(f"denoise: plane nrdViewZ is {tuple(gbuffer['nrdViewZ'].shape)}, the denoiser was made for {(H, W)}")
        if out is None:
            out = torch.zeros((H, W, 4), dtype=torch.float32, device=f"cuda:{self.device}")
        if tuple(out.shape) != (H, W, 4) or out.dtype != torch.float32 or not out.is_contiguous():
            raise VkrtError(f"denoise: out is {tuple(out.shape)}, the denoiser was made for {(H, W, 4)}")
        stream = stream or torch.cuda.current_stream(out.device)
        gb = abi.Gbuffer(*(gbuffer[k].data_ptr() for k in ("color", "position", "normal", "roughMetal")))
        nrd = abi.NrdPlanes(gbuffer["nrdNormalRoughness"].data_ptr() if "nrdNormalRoughness" in gbuffer else None,
                            gbuffer["nrdViewZ"].data_ptr(), gbuffer["nrdRadianceHitDist"].data_ptr())
        st = abi.DenoiseSettings(C.sizeof(abi.DenoiseSettings), int(iterations), int(max_history))
        if "prevPosition" in gbuffer:  # planes from gbuffer_raycast(motion=True): the history follows moving and deforming geometry
            t = gbuffer["prevPosition"]
            if tuple(t.shape) != (H, W, 4) or t.dtype != torch.float32 or not t.is_contiguous():
                raise VkrtError(f"denoise: plane prevPosition is {tuple(t.shape)}, the denoiser was made for {(H, W, 4)}")
            _check(self.lib.vkrt_denoise_diffuse_motion(self._h, C.byref(st), C.byref(cam), C.byref(gb), C.byref(nrd), C.c_void_p(t.data_ptr()),
                                                        C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream)), "vkrt_denoise_diffuse_motion")
            return out
        _check(self.lib.vkrt_denoise_diffuse(self._h, C.byref(st), C.byref(cam), C.byref(gb), C.byref(nrd), C.c_void_p(out.data_ptr()),
                                             C.c_void_p(stream.cuda_stream)), "vkrt_denoise_diffuse")
        return out

    def reset(self):
        _check(self.lib.vkrt_denoiser_reset(self._h), "vkrt_denoiser_reset")

    def close(self):
        if getattr(self, "_h", None):
            self.lib.vkrt_denoiser_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def eval_math(op, a, b=None, device=0):
    lib = load_library()
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(a if b is None else b, np.float32)
    out = np.zeros_like(a)
    _check(lib.vkrt_debug_eval_math(device, op, a.size, a.ctypes.data, b.ctypes.data, out.ctypes.data), "vkrt_debug_eval_math")
    return out


def eval_shade(records, device=0):
    """The hit shader's BRDF tail on [n, 40] float32 records -> [n, 20] (layout: include/vkrt.h vkrt_debug_eval_shade)."""
    lib = load_library()
    records = np.ascontiguousarray(records, np.float32).reshape(-1, 40)
    out = np.zeros((records.shape[0], 20), np.float32)
    _check(lib.vkrt_debug_eval_shade(device, records.shape[0], records.ctypes.data, out.ctypes.data), "vkrt_debug_eval_shade")
    return out
