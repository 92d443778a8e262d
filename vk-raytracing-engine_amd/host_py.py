"""ctypes access to the C++ host layer (libvkrt_host.so) for the test harness."""
import ctypes as C
import os

import numpy as np

from . import HOST_LIB_PATH, abi
from .flat_scene import ALPHA_DTYPE, FlatScene, LIGHT_DTYPE, MAT_DTYPE, NODE_DTYPE, PRIM_DTYPE

_lib = None


def lib():
    global _lib
    if _lib is None:
        import torch  # noqa: F401  (same HIP-runtime load-order rule as renderer.load_library)

        if not os.path.exists(HOST_LIB_PATH):
            raise RuntimeError(f"{HOST_LIB_PATH} missing: run __graft_entry__.build()")
        L = C.CDLL(HOST_LIB_PATH)
        L.vkrt_host_last_error.restype = C.c_char_p
        L.vkrt_host_load_gltf.argtypes = [C.c_char_p]
        L.vkrt_host_load_gltf.restype = C.c_void_p
        L.vkrt_host_free_scene.argtypes = [C.c_void_p]
        L.vkrt_host_scene_counts.argtypes = [C.c_void_p, C.c_void_p]
        L.vkrt_host_scene_copy.argtypes = [C.c_void_p] + [C.c_void_p] * 9
        L.vkrt_host_scene_material_alpha.argtypes = [C.c_void_p, C.c_void_p]
        L.vkrt_host_scene_warnings.argtypes = [C.c_void_p]
        L.vkrt_host_scene_warnings.restype = C.c_char_p
        L.vkrt_host_scene_skin_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.vkrt_host_scene_skin_counts.restype = C.c_uint32
        L.vkrt_host_scene_skin_copy.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
        L.vkrt_host_scene_morph_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.vkrt_host_scene_morph_counts.restype = C.c_uint32
        L.vkrt_host_scene_morph_copy.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 4
        L.vkrt_host_texture_info.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.vkrt_host_texture_copy.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.vkrt_host_global_uniforms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.POINTER(abi.GlobalUniforms)]
        L.vkrt_host_parse_config.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_int]
        L.vkrt_host_parse_config.restype = C.c_int
        L.vkrt_host_config_alpha_test.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
        L.vkrt_host_config_alpha_test.restype = C.c_int
        L.vkrt_host_render_gltf.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_void_p]
        L.vkrt_host_render_gltf.restype = C.c_int
        L.vkrt_host_render_gltf_moved.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  C.c_void_p, C.c_void_p]
        L.vkrt_host_render_gltf_moved.restype = C.c_int
        L.vkrt_host_render_gltf_deformed.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vkrt_host_render_gltf_deformed.restype = C.c_int
        L.vkrt_host_render_gltf_skinned.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                    C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]
        L.vkrt_host_render_gltf_skinned.restype = C.c_int
        L.vkrt_host_render_gltf_morphed.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                    C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]
        L.vkrt_host_render_gltf_morphed.restype = C.c_int
        L.vkrt_host_render_gltf_hybrid.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_float, C.c_uint32, C.c_uint32, C.c_void_p]
        L.vkrt_host_render_gltf_hybrid.restype = C.c_int
        L.vkrt_host_decode_png.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
        L.vkrt_host_decode_png.restype = C.c_int
        L.vkrt_host_decode_image.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
        L.vkrt_host_decode_image.restype = C.c_int
        L.vkrt_host_write_png.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
        L.vkrt_host_write_png.restype = C.c_int
        L.vkrt_host_strip_rows.argtypes = [C.c_uint32] * 4
        L.vkrt_host_strip_rows.restype = C.c_uint32
        L.vkrt_host_strip_source.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint32)] * 2
        L.vkrt_host_unpack_strips.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.vkrt_host_unpack_strips.restype = C.c_int
        _lib = L
    return _lib


def strip_rows(height, world, rank, strip_rows_=16):
    """rows of `rank`'s strip buffer in the C++ host's multi-GPU layout (host/strip_gather.h)"""
    return int(lib().vkrt_host_strip_rows(height, strip_rows_, world, rank))


def strip_source(height, world, y, strip_rows_=16):
    """(rank, local row) that holds global row y"""
    r, l = C.c_uint32(), C.c_uint32()
    lib().vkrt_host_strip_source(height, strip_rows_, world, y, C.byref(r), C.byref(l))
    return int(r.value), int(l.value)


def unpack_strips(gathered, full, world, strip_rows_=16, stream=None):
    """HIP un-interleave kernel of the C++ host: gathered [world, cap, W, 4] -> full [H, W, 4] (torch CUDA tensors)."""
    H, W = int(full.shape[0]), int(full.shape[1])
    rc = lib().vkrt_host_unpack_strips(C.c_void_p(gathered.data_ptr()), C.c_void_p(full.data_ptr()), W, H, strip_rows_, world,
                                       C.c_void_p(stream.cuda_stream) if stream is not None else None)
    if rc != 0:
        raise RuntimeError(lib().vkrt_host_last_error().decode())
    return full


def load_gltf(path):
    """C++ loader -> FlatScene."""
    L = lib()
    h = L.vkrt_host_load_gltf(os.fsencode(path))
    if not h:
        raise RuntimeError("vkrt_host_load_gltf: " + L.vkrt_host_last_error().decode())
    try:
        cnt = np.zeros(7, np.uint32)
        L.vkrt_host_scene_counts(h, cnt.ctypes.data)
        V, I, P, N, M, Lc, T = (int(x) for x in cnt)
        pos, nrm = np.zeros((V, 3), np.float32), np.zeros((V, 3), np.float32)
        tan, uv = np.zeros((V, 4), np.float32), np.zeros((V, 2), np.float32)
        idx = np.zeros(I, np.uint32)
        pm, nd = np.zeros(P, PRIM_DTYPE), np.zeros(N, NODE_DTYPE)
        mats, lights = np.zeros(M, MAT_DTYPE), np.zeros(Lc, LIGHT_DTYPE)
        L.vkrt_host_scene_copy(h, *(a.ctypes.data for a in (pos, nrm, tan, uv, idx, pm, nd, mats, lights)))
        tex = []
        for i in range(T):
            whs = np.zeros(3, np.uint32)
            L.vkrt_host_texture_info(h, i, whs.ctypes.data)
            px = np.zeros((int(whs[1]), int(whs[0]), 4), np.uint8)
            L.vkrt_host_texture_copy(h, i, px.ctypes.data)
            tex.append({"rgba8": px, "is_srgb": bool(whs[2])})
        # glTF's alphaMode / alphaCutoff per material; carried only when the file has a MASK material (else every material is opaque)
        alpha = np.zeros(M, ALPHA_DTYPE)
        L.vkrt_host_scene_material_alpha(h, alpha.ctypes.data)
        return FlatScene(pos, nrm, tan, uv, idx, pm, mats, lights, nd, tex, alpha if np.any(alpha["mode"] != 0) else None)
    finally:
        L.vkrt_host_free_scene(h)


def load_gltf_skins(path):
    """C++ loader -> the skinning data of a glTF file: dict(joints0 uint16 (V, 4), weights0 float32 (V, 4) -- both (0, 4) when the file
    has no skin --, skins = [dict(joint_nodes int32 (J,), inverse_bind (J, 16), rest_joint_matrices (J, 16) float32
    column-major, vertex_ranges uint32 (R, 2) of (first, count))], warnings = the loader's GltfScene::warnings)."""
    L = lib()
    h = L.vkrt_host_load_gltf(os.fsencode(path))
    if not h:
        raise RuntimeError("vkrt_host_load_gltf: " + L.vkrt_host_last_error().decode())
    try:
        need = int(L.vkrt_host_scene_skin_counts(h, None, 0))
        cnt = np.zeros(need, np.uint32)
        L.vkrt_host_scene_skin_counts(h, cnt.ctypes.data, need)
        S, V = int(cnt[0]), int(cnt[1])
        joints0, weights0 = np.zeros((V, 4), np.uint16), np.zeros((V, 4), np.float32)
        L.vkrt_host_scene_skin_copy(h, 0xFFFFFFFF, joints0.ctypes.data, weights0.ctypes.data, None, None, None, None)
        skins = []
        for k in range(S):
            J, R = int(cnt[2 + 2 * k]), int(cnt[3 + 2 * k])
            nodes, ranges = np.zeros(J, np.int32), np.zeros((R, 2), np.uint32)
            ib, rest = np.zeros((J, 16), np.float32), np.zeros((J, 16), np.float32)
            L.vkrt_host_scene_skin_copy(h, k, None, None, nodes.ctypes.data, ib.ctypes.data, rest.ctypes.data, ranges.ctypes.data)
            skins.append({"joint_nodes": nodes, "inverse_bind": ib, "rest_joint_matrices": rest, "vertex_ranges": ranges})
        return {"joints0": joints0, "weights0": weights0, "skins": skins, "warnings": L.vkrt_host_scene_warnings(h).decode()}
    finally:
        L.vkrt_host_free_scene(h)


def load_gltf_morphs(path):
    """C++ loader -> the morph targets of a glTF file: a list, in vertex order, of dict(first, count, target_count, position_deltas,
    normal_deltas, tangent_deltas float32 (T, count, 3) or None, weights float32 (T,): mesh.weights, overridden by the weights of the
    first node that instances the mesh)."""
    L = lib()
    h = L.vkrt_host_load_gltf(os.fsencode(path))
    if not h:
        raise RuntimeError("vkrt_host_load_gltf: " + L.vkrt_host_last_error().decode())
    try:
        need = int(L.vkrt_host_scene_morph_counts(h, None, 0))
        cnt = np.zeros(need, np.uint32)
        L.vkrt_host_scene_morph_counts(h, cnt.ctypes.data, need)
        out = []
        for m in range(int(cnt[0])):
            first, count, T, hp, hn, ht = (int(x) for x in cnt[1 + 6 * m:7 + 6 * m])
            d = [np.zeros((T, count, 3), np.float32) if has else None for has in (hp, hn, ht)]
            w = np.zeros(T, np.float32)
            L.vkrt_host_scene_morph_copy(h, m, *(None if a is None else a.ctypes.data for a in d), w.ctypes.data)
            out.append({"first": first, "count": count, "target_count": T, "position_deltas": d[0], "normal_deltas": d[1], "tangent_deltas": d[2],
                        "weights": w})
        return out
    finally:
        L.vkrt_host_free_scene(h)


def global_uniforms(eye=(0, 0, 15), center=(0, 0, 0), up=(0, 1, 0), fov=60.0, width=1280, height=720):
    u = abi.GlobalUniforms()
    e, c, p = (np.asarray(v, np.float32) for v in (eye, center, up))
    lib().vkrt_host_global_uniforms(e.ctypes.data, c.ctypes.data, p.ctypes.data, fov, width, height, C.byref(u))
    return u


def parse_config(text):
    out = np.zeros(13, np.int32)
    path = C.create_string_buffer(1024)
    rc = lib().vkrt_host_parse_config(text.encode(), out.ctypes.data, path, 1024)
    if rc != 0:
        raise ValueError(lib().vkrt_host_last_error().decode())
    keys = ["scene", "vsync", "width", "height", "samples", "depth", "frames", "seed", "nscenes", "framesPerCall", "watertight", "anyHitDissolve",
            "skipDeadShadowRays"]
    d = dict(zip(keys, (int(x) for x in out)))
    d["scene_path"] = path.value.decode()
    alpha = C.c_int(0)
    if lib().vkrt_host_config_alpha_test(text.encode(), C.byref(alpha)) != 0:
        raise ValueError(lib().vkrt_host_last_error().decode())
    d["alphaTest"] = int(alpha.value)
    return d


def render_gltf(path, width, height, samples=1, depth=3, frames=1, seed0=0, eye=(0, 0, 15), center=(0, 0, 0), up=(0, 1, 0), fov=60.0,
                build=abi.VKRT_BUILD_PLOC_GPU, device=0):
    img = np.zeros((height, width, 4), np.float32)
    e, c, p = (np.asarray(v, np.float32) for v in (eye, center, up))
    rc = lib().vkrt_host_render_gltf(os.fsencode(path), device, width, height, samples, depth, frames, seed0, e.ctypes.data,
                                     c.ctypes.data, p.ctypes.data, fov, build, img.ctypes.data)
    if rc != 0:
        raise RuntimeError("vkrt_host_render_gltf: " + lib().vkrt_host_last_error().decode())
    return img


def render_gltf_moved(path, width, height, first, matrices, samples=1, depth=3, frames=1, seed0=0, eye=(0, 0, 15), center=(0, 0, 0), up=(0, 1, 0),
                      fov=60.0, build=abi.VKRT_BUILD_PLOC_GPU, device=0):
    """render_gltf after moving nodes through the C++ HelloVkrt: matrices (steps, count, 16) column-major; each step is
    updateNodeTransforms(first, matrices[step]) + refitAccel()."""
    m = np.ascontiguousarray(matrices, np.float32)
    if m.ndim == 2:
        m = m[None]
    img = np.zeros((height, width, 4), np.float32)
    e, c, p = (np.asarray(v, np.float32) for v in (eye, center, up))
    rc = lib().vkrt_host_render_gltf_moved(os.fsencode(path), device, width, height, samples, depth, frames, seed0, e.ctypes.data, c.ctypes.data,
                                           p.ctypes.data, fov, build, first, m.shape[1], m.shape[0], m.ctypes.data, img.ctypes.data)
    if rc != 0:
        raise RuntimeError("vkrt_host_render_gltf_moved: " + lib().vkrt_host_last_error().decode())
    return img


def render_gltf_deformed(path, width, height, first, positions, normals=None, tangents=None, texcoords0=None, samples=1, depth=3, frames=1, seed0=0,
                         eye=(0, 0, 15), center=(0, 0, 0), up=(0, 1, 0), fov=60.0, build=abi.VKRT_BUILD_PLOC_GPU, device=0):
    """render_gltf after deforming vertices [first, first + count) through the C++ HelloVkrt: positions (steps, count, 3) -- normals
    (steps, count, 3), tangents (steps, count, 4), texcoords0 (steps, count, 2) or None = kept; each step is
    updateVertices(first, ...) + refitAccel()."""
    arrays = []
    shape = None
    for a, w in ((positions, 3), (normals, 3), (tangents, 4), (texcoords0, 2)):
        if a is None:
            arrays.append(None)
            continue
        a = np.ascontiguousarray(a, np.float32)
        a = a[None] if a.ndim == 2 else a
        if a.ndim != 3 or a.shape[2] != w or (shape is not None and a.shape[:2] != shape):
            raise ValueError(f"render_gltf_deformed: an array of shape {a.shape}, expected (steps, count, {w}) with one steps x count")
        shape = a.shape[:2]
        arrays.append(a)
    if shape is None:
        raise ValueError("render_gltf_deformed: no array given")
    img = np.zeros((height, width, 4), np.float32)
    e, c, p = (np.asarray(v, np.float32) for v in (eye, center, up))
    ptrs = [C.c_void_p(a.ctypes.data) if a is not None else None for a in arrays]
    rc = lib().vkrt_host_render_gltf_deformed(os.fsencode(path), device, width, height, samples, depth, frames, seed0, e.ctypes.data, c.ctypes.data, p.ctypes.data, fov, build,
                                              int(first), shape[1], shape[0], *ptrs, img.ctypes.data)
    if rc != 0:
        raise RuntimeError("vkrt_host_render_gltf_deformed: " + lib().vkrt_host_last_error().decode())
    return img


def render_gltf_skinned(path, width, height, skin, joint_matrices, samples=1, depth=3, frames=1, seed0=0, eye=(0, 0, 15), center=(0, 0, 0),
                        up=(0, 1, 0), fov=60.0, build=abi.VKRT_BUILD_PLOC_GPU, device=0):
    """render_gltf after posing skin `skin` of the file through the C++ HelloVkrt: joint_matrices (steps, joints, 16) column-major; each
    step is skinVertices(skin, joint_matrices[step]) + refitAccel().  Returns (image, HelloVkrt::skinCount())."""
    m = np.ascontiguousarray(joint_matrices, np.float32)
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3 or m.shape[2] != 16:
        raise ValueError(f"render_gltf_skinned: joint_matrices of shape {m.shape}, expected (steps, joints, 16)")
    img = np.zeros((height, width, 4), np.float32)
    e, c, p = (np.asarray(v, np.float32) for v in (eye, center, up))
    count = C.c_uint32(0)
    rc = lib().vkrt_host_render_gltf_skinned(os.fsencode(path), device, width, height, samples, depth, frames, seed0, e.ctypes.data, c.ctypes.data,
                                             p.ctypes.data, fov, build, int(skin), m.shape[1], m.shape[0], m.ctypes.data, C.byref(count), img.ctypes.data)
    if rc != 0:
        raise RuntimeError("vkrt_host_render_gltf_skinned: " + lib().vkrt_host_last_error().decode())
    return img, int(count.value)


def render_gltf_morphed(path, width, height, morph=0, weights=None, samples=1, depth=3, frames=1, seed0=0, eye=(0, 0, 15), center=(0, 0, 0),
                        up=(0, 1, 0), fov=60.0, build=abi.VKRT_BUILD_PLOC_GPU, device=0):
    """render_gltf of a file with morph targets through the C++ HelloVkrt: the file's default weights are applied at load; weights
    (steps, targets), if given, are then posed one after the other on morph `morph`, each step morphVertices(morph, weights[step]) +
    refitAccel().  Returns (image, HelloVkrt::morphCount())."""
    w = np.zeros((0, 1), np.float32) if weights is None else np.ascontiguousarray(weights, np.float32)
    if w.ndim == 1:
        w = w[None]
    if w.ndim != 2:
        raise ValueError(f"render_gltf_morphed: weights of shape {w.shape}, expected (steps, targets)")
    img = np.zeros((height, width, 4), np.float32)
    e, c, p = (np.asarray(v, np.float32) for v in (eye, center, up))
    count = C.c_uint32(0)
    rc = lib().vkrt_host_render_gltf_morphed(os.fsencode(path), device, width, height, samples, depth, frames, seed0, e.ctypes.data, c.ctypes.data,
                                             p.ctypes.data, fov, build, int(morph), w.shape[1], w.shape[0], w.ctypes.data, C.byref(count), img.ctypes.data)
    if rc != 0:
        raise RuntimeError("vkrt_host_render_gltf_morphed: " + lib().vkrt_host_last_error().decode())
    return img, int(count.value)


def render_gltf_hybrid(path, width, height, depth=3, frames=1, seed0=0, eye=(0, 0, 15), center=(0, 0, 0), up=(0, 1, 0), fov=60.0, rank=0, world=1, device=0):
    """The reference's hybrid frame sequence through the C++ HelloVkrt for one rank of `world`: that rank's display strips [rows, W, 4]."""
    rows = strip_rows(height, world, rank) if world > 1 else height
    img = np.zeros((rows, width, 4), np.float32)
    e, c, p = (np.asarray(v, np.float32) for v in (eye, center, up))
    rc = lib().vkrt_host_render_gltf_hybrid(os.fsencode(path), device, width, height, depth, frames, seed0, e.ctypes.data, c.ctypes.data, p.ctypes.data, fov,
                                            rank, world, img.ctypes.data)
    if rc != 0:
        raise RuntimeError("vkrt_host_render_gltf_hybrid: " + lib().vkrt_host_last_error().decode())
    return img


def decode_png(data):
    wh = np.zeros(2, np.uint32)
    buf = np.frombuffer(data, np.uint8)
    if lib().vkrt_host_decode_png(buf.ctypes.data, buf.size, wh.ctypes.data, None, 0) != 0:
        raise ValueError(lib().vkrt_host_last_error().decode())
    out = np.zeros((int(wh[1]), int(wh[0]), 4), np.uint8)
    lib().vkrt_host_decode_png(buf.ctypes.data, buf.size, wh.ctypes.data, out.ctypes.data, out.size)
    return out


def decode_image(data):
    """PNG or JPEG bytes -> (H, W, 4) uint8 through the C++ host's decoders (the texels the loader hands to the library)."""
    wh = np.zeros(2, np.uint32)
    buf = np.frombuffer(data, np.uint8)
    if lib().vkrt_host_decode_image(buf.ctypes.data, buf.size, wh.ctypes.data, None, 0) != 0:
        raise ValueError(lib().vkrt_host_last_error().decode())
    out = np.zeros((int(wh[1]), int(wh[0]), 4), np.uint8)
    lib().vkrt_host_decode_image(buf.ctypes.data, buf.size, wh.ctypes.data, out.ctypes.data, out.size)
    return out


def write_png(path, display_rgba):
    """8-bit RGBA PNG of a display image (float32 [H,W,4] in [0,1], i.e. after post.frag's gamma)."""
    a = np.ascontiguousarray(display_rgba, np.float32)
    if lib().vkrt_host_write_png(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0]) != 0:
        raise RuntimeError(lib().vkrt_host_last_error().decode())
