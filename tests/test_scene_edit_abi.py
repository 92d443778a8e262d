"""CPU-side checks of vkrt_scene_update_lights, vkrt_scene_update_materials, vkrt_scene_update_texture and the three readers: declared,
exported, laid out like the ctypes records, refused without a scene in the order the header states (each message naming its argument),
the Python layer's refusals before the call, what the header owes its reader, and the kernels' resource report."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import vkrt_amd
from vkrt_amd import abi
from vkrt_amd.flat_scene import LIGHT_DTYPE, MAT_DTYPE

ROOT = vkrt_amd.REPO_ROOT
NEW = ("vkrt_scene_update_lights", "vkrt_scene_update_materials", "vkrt_scene_update_texture", "vkrt_debug_read_lights", "vkrt_debug_read_materials",
       "vkrt_debug_read_texture")
KERNELS = ("k_se_lights", "k_se_materials", "k_se_level0", "k_se_mip", "k_se_mip_tail")
BAD = abi.VKRT_ERR_INVALID_ARGUMENT
HOST, DEVICE = abi.VKRT_MEMORY_HOST, abi.VKRT_MEMORY_DEVICE


def _lib():
    assert os.path.exists(vkrt_amd.LIB_PATH), "run __graft_entry__.build() first"
    return abi.declare_vkrt(C.CDLL(vkrt_amd.LIB_PATH))


def _header():
    return open(os.path.join(ROOT, "include", "vkrt.h")).read()


def test_scene_edit_symbols_are_declared_and_exported():
    header = _header()
    declared = set(re.findall(r"\b(vkrt_[a-z_]+)\s*\(", header))
    lib = C.CDLL(vkrt_amd.LIB_PATH)
    for name in NEW:
        assert name in declared and name in abi.VKRT_SYMBOLS and hasattr(lib, name), name
    assert _lib().vkrt_abi_version() == 4 == abi.VKRT_ABI_VERSION  # added without a version change: detect by symbol
    for name in abi.VKRT_SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    assert C.sizeof(abi.GltfLight) == 32 and C.sizeof(abi.GltfPBRMaterial) == 52 and C.sizeof(abi.Texture) == 24  # no existing struct changed
    csrc = os.path.join(ROOT, "vk-raytracing-engine_amd", "csrc")
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    for unit in ("scene_edit.hip", "api_edit.cpp"):
        assert unit in srcs and os.path.exists(os.path.join(csrc, unit))
    assert os.path.exists(os.path.join(csrc, "scene_edit.h")) and os.path.exists(os.path.join(csrc, "texture_pack.h"))


def test_the_header_states_ordering_staleness_dissolve_and_exactness():
    header = _header()
    sec = header[header.index("editing a live scene's lights, materials and textures"):header.index("/* ---- path trace")]
    for phrase in ("Ordering: each of the three calls is enqueued on hip_stream", "ordered after what was enqueued there before",
                   "Not stale: none of them makes the tree stale", "work on a stale tree and before vkrt_accel_build", "without a refit",
                   "A refused call changes nothing; the first failing check of a call's list wins",
                   "Dissolve:", "ran with VKRT_OPT_ANYHIT_DISSOLVE = 1", "did not have alpha < 1 at\n * that build", "the tree needs a rebuild, not only a refit",
                   "return VKRT_ERR_NOT_BUILT with a message naming vkrt_scene_update_materials", "The opposite direction",
                   "bit for bit what vkrt_scene_create packs", "The alpha mode and cutoff of a material are kept", "192 B per material",
                   "at most 1 + VKRT_MAX_MIPS (16) kernel launches", "a table of thresholds the host derived from its own encode function",
                   "the call waits for the\n *                       stream before it returns", "with no allocation and no host synchronisation"):
        assert phrase in sec, phrase
    tail = header[header.index("int vkrt_debug_read_instances"):]
    for phrase in ("32 B each", "192 B each", "VKRT_ERR_UNSUPPORTED when the scene has no footprint pool", "no kernel of their own"):
        assert phrase in tail, phrase


def test_the_header_lists_the_refusals_in_the_order_the_library_applies():
    header = _header()
    sec = header[header.index("editing a live scene's lights, materials and textures"):header.index("/* ---- path trace")]
    lights = sec[sec.index("vkrt_scene_update_lights: new records"):sec.index("typedef struct vkrt_light_update")]
    materials = sec[sec.index("vkrt_scene_update_materials: new materials"):sec.index("int vkrt_scene_update_materials")]
    texture = sec[sec.index("vkrt_scene_update_texture: replaces"):sec.index("typedef struct vkrt_texture_update")]
    for text, seq in ((lights, ["a NULL update", "struct_size < sizeof(vkrt_light_update)", "a memory value", "a NULL scene", "a range outside the scene's lights",
                                "NULL lights", "not 16-byte aligned", "count == 0: VKRT_OK", "VKRT_ERR_NO_DEVICE"]),
                      (materials, ["a NULL array with count > 0", "a texture index >= texture_count", "a NULL scene", "a range outside the scene's materials",
                                   "VKRT_ERR_UNSUPPORTED", "count == 0: VKRT_OK", "VKRT_ERR_NO_DEVICE"]),
                      (texture, ["a NULL update", "struct_size < sizeof(vkrt_texture_update)", "a memory value", "a NULL scene", "a texture index out of range",
                                 "a width or height", "NULL rgba8", "not 16-byte aligned", "VKRT_ERR_NO_DEVICE"])):
        text = text[text.index("Refused"):]
        at = [text.index(p) for p in seq]
        assert at == sorted(at), seq


def test_scene_edit_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of the two update structs, compiled as C and as C++ under -Wall -Werror, equal the ctypes records."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vkrt.h"', "int main(void){"]
    expect = []
    for cname, rec in (("vkrt_light_update", abi.LightUpdate), ("vkrt_texture_update", abi.TextureUpdate)):
        lines.append(f'  printf("%zu\\n", sizeof({cname}));')
        expect.append(C.sizeof(rec))
        for fname, _ in rec._fields_:
            lines.append(f'  printf("%zu\\n", offsetof({cname}, {fname}));')
            expect.append(getattr(rec, fname).offset)
    lines += ['  printf("%zu %zu %d\\n", sizeof(GltfLight), sizeof(GltfPBRMaterial), VKRT_ABI_VERSION);', "  return 0; }"]
    expect += [32, 52, 4]
    for ext, cc in (("c", "gcc"), ("cpp", "g++")):
        src = tmp_path / f"layout.{ext}"
        src.write_text("\n".join(lines) + "\n")
        exe = tmp_path / f"layout_{cc}"
        subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
        assert [int(x) for x in out] == expect
    assert (C.sizeof(abi.LightUpdate), C.sizeof(abi.TextureUpdate)) == (24, 32)
    assert [f for f, _ in abi.LightUpdate._fields_] == ["struct_size", "first", "count", "memory", "lights"]
    assert [f for f, _ in abi.TextureUpdate._fields_] == ["struct_size", "texture", "width", "height", "memory", "rgba8"]


# ---- refusals without a scene, and without a device --------------------------------------------------------------------------------------
def _light_update(first=0, count=2, memory=HOST, size=None, lights=None):
    ptr = lights if lights is None or isinstance(lights, int) else lights.ctypes.data
    return abi.LightUpdate(C.sizeof(abi.LightUpdate) if size is None else size, first, count, memory, ptr)


def _texture_update(texture=0, width=4, height=4, memory=HOST, size=None, rgba8=None):
    ptr = rgba8 if rgba8 is None or isinstance(rgba8, int) else rgba8.ctypes.data
    return abi.TextureUpdate(C.sizeof(abi.TextureUpdate) if size is None else size, texture, width, height, memory, ptr)


def test_light_update_refusals_without_a_scene_come_in_the_headers_order():
    lib = _lib()
    who = b"vkrt_scene_update_lights: "
    lights = np.zeros(2, LIGHT_DTYPE)

    def refused(u, text, absent=()):
        assert lib.vkrt_scene_update_lights(None, None if u is None else C.byref(u), None) == BAD
        msg = lib.vkrt_last_error()
        assert msg.startswith(who) and text in msg and not any(a in msg for a in absent), msg

    refused(None, b"update is NULL")
    for size in (0, 16, C.sizeof(abi.LightUpdate) - 1):  # everything behind struct_size is wrong as well
        refused(_light_update(size=size, first=9, memory=7), b"vkrt_light_update.struct_size %d < 24 (ABI mismatch)" % size)
    for memory in (2, 7, 0xFFFFFFFF):
        refused(_light_update(first=9, memory=memory), b"memory %d is neither VKRT_MEMORY_HOST nor VKRT_MEMORY_DEVICE" % memory, absent=(b"struct_size",))
    # a good head reaches the scene check, whatever the range and the array are; a larger struct_size (a later, longer struct) is accepted
    for u in (_light_update(), _light_update(memory=DEVICE), _light_update(lights=lights), _light_update(count=0), _light_update(size=64, first=9),
              _light_update(memory=DEVICE, lights=0x1004), _light_update(first=0xFFFFFFFF, count=0xFFFFFFFF)):
        refused(u, b"scene is NULL", absent=(b"memory", b"lights ["))


def test_texture_update_refusals_without_a_scene_come_in_the_headers_order():
    lib = _lib()
    who = b"vkrt_scene_update_texture: "
    img = np.zeros((4, 4, 4), np.uint8)

    def refused(u, text, absent=()):
        assert lib.vkrt_scene_update_texture(None, None if u is None else C.byref(u), None) == BAD
        msg = lib.vkrt_last_error()
        assert msg.startswith(who) and text in msg and not any(a in msg for a in absent), msg

    refused(None, b"update is NULL")
    for size in (0, 24, C.sizeof(abi.TextureUpdate) - 1):
        refused(_texture_update(size=size, memory=7), b"vkrt_texture_update.struct_size %d < 32 (ABI mismatch)" % size)
    for memory in (2, 0xFFFFFFFF):
        refused(_texture_update(memory=memory), b"memory %d is neither VKRT_MEMORY_HOST nor VKRT_MEMORY_DEVICE" % memory, absent=(b"struct_size",))
    for u in (_texture_update(), _texture_update(rgba8=img), _texture_update(memory=DEVICE, rgba8=0x1004), _texture_update(texture=0xFFFFFFFF, width=0, height=0),
              _texture_update(size=64)):
        refused(u, b"scene is NULL", absent=(b"memory", b"rgba8", b"texture 0"))


def test_material_update_refusals_without_a_scene():
    """a NULL array with count > 0 wins over the NULL scene; a texture index can be judged against a scene only, so every array reaches
    the scene check"""
    lib = _lib()
    fn = lib.vkrt_scene_update_materials
    mats = np.zeros(2, MAT_DTYPE)
    mats["pbrBaseColorTexture"] = 10 ** 6
    assert fn(None, 0, 2, None, None) == BAD
    assert lib.vkrt_last_error() == b"vkrt_scene_update_materials: materials is NULL"
    for first, count, ptr in ((0, 2, mats.ctypes.data), (0, 0, None), (0xFFFFFFFF, 0xFFFFFFFF, mats.ctypes.data), (5, 0, mats.ctypes.data)):
        assert fn(None, first, count, ptr, None) == BAD
        assert lib.vkrt_last_error() == b"vkrt_scene_update_materials: scene is NULL"


def test_readers_refuse_null_arguments():
    lib = _lib()
    out = np.zeros(64, np.uint32)
    for name, call in (("vkrt_debug_read_lights", lambda: lib.vkrt_debug_read_lights(None, 0, 1, out.ctypes.data, 32)),
                       ("vkrt_debug_read_materials", lambda: lib.vkrt_debug_read_materials(None, 0, 1, out.ctypes.data, 192)),
                       ("vkrt_debug_read_texture", lambda: lib.vkrt_debug_read_texture(None, 0, 0, out.ctypes.data, 4, None, 0))):
        assert call() == BAD
        assert name.encode() in lib.vkrt_last_error() and b"NULL" in lib.vkrt_last_error()


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def _renderer():
    from renderer_stand_ins import renderer_without_scene

    r = renderer_without_scene(10)
    r.lights_count, r._material_count, r._texture_sizes = 2, 4, [(37, 21), (1, 1), (8, 2)]
    return r


def test_python_refuses_bad_edits_before_the_call():
    import torch
    from vkrt_amd.renderer import VkrtError

    r = _renderer()
    L = lambda n: np.zeros(n, LIGHT_DTYPE)  # noqa: E731
    M = lambda n: np.zeros(n, MAT_DTYPE)  # noqa: E731
    img = np.zeros((21, 37, 4), np.uint8)
    bad = [
        (r.update_lights, (1, L(2)), "outside"), (r.update_lights, (-1, L(1)), "outside"), (r.update_lights, (0, L(3)), "outside"),
        (r.update_lights, (1.5, L(1)), "outside"), (r.update_lights, (0, np.zeros((2, 8), np.float32)), "LIGHT_DTYPE"),
        (r.update_lights, (0, [1, 2]), "numpy array or a torch tensor"), (r.update_lights, (0, torch.zeros(2, 8)), "lights is on cpu"),
        (r.update_materials, (3, M(2)), "outside"), (r.update_materials, (-1, M(1)), "outside"), (r.update_materials, (0, np.zeros((2, 13), np.float32)), "MAT_DTYPE"),
        (r.update_materials, (0, torch.zeros(2, 13)), "MAT_DTYPE"),
        (r.update_texture, (3, img), "outside"), (r.update_texture, (-1, img), "outside"), (r.update_texture, (True, img), "outside"),
        (r.update_texture, (0, np.zeros((37, 21, 4), np.uint8)), "expected uint8 \\(21, 37, 4\\)"), (r.update_texture, (0, img.astype(np.float32)), "float32"),
        (r.update_texture, (0, img[..., :3]), "expected uint8"), (r.update_texture, (0, torch.zeros(21, 37, 4, dtype=torch.uint8)), "rgba8 is on cpu"),
        (r.read_lights, (1, 2), "outside"), (r.read_lights, (0, -1), "outside"), (r.read_materials, (0, 5), "outside"), (r.read_materials, (4, 1), "outside"),
        (r.read_texture, (3,), "outside"), (r.read_texture, (0, 6), "level"), (r.read_texture, (1, 1), "level"), (r.read_texture, (0, 1, True), "level 0 only"),
    ]
    for fn, args, word in bad:
        with pytest.raises(VkrtError, match=word):
            fn(*args)
    m = M(2)
    m["normalTexture"][1] = 3
    with pytest.raises(VkrtError, match="normalTexture 3 beyond the scene's 3 textures"):
        r.update_materials(0, m)
    # good calls reach the library (here: the stand-in that refuses to be reached)
    m["normalTexture"][1] = 2
    m["emissiveTexture"] = -1
    for fn, args, name in ((r.update_lights, (0, L(2)), "vkrt_scene_update_lights"), (r.update_lights, (2, L(0)), "vkrt_scene_update_lights"),
                           (r.update_materials, (2, m), "vkrt_scene_update_materials"), (r.update_texture, (0, img), "vkrt_scene_update_texture"),
                           (r.update_texture, (1, np.zeros((1, 1, 4), np.uint8)), "vkrt_scene_update_texture"), (r.read_lights, (0, 2), "vkrt_debug_read_lights"),
                           (r.read_materials, (1, 3), "vkrt_debug_read_materials"), (r.read_texture, (0, 5), "vkrt_debug_read_texture"),
                           (r.read_texture, (2, 0, True), "vkrt_debug_read_texture")):
        with pytest.raises(AssertionError, match=name):
            fn(*args)


def test_python_refuses_tensor_faults_through_a_stand_in():
    import torch
    from renderer_stand_ins import Fake
    from vkrt_amd.renderer import VkrtError

    r = _renderer()
    u8 = torch.uint8
    bad = [
        (r.update_lights, (0, Fake((2, 8), index=1)), "cuda:1"), (r.update_lights, (0, Fake((2, 8), dtype=torch.float64)), "float64"),
        (r.update_lights, (0, Fake((2, 8), contiguous=False)), "contiguous"), (r.update_lights, (0, Fake((2, 8), ptr=0x1008)), "16-byte aligned"),
        (r.update_lights, (0, Fake((16,))), "shape"), (r.update_lights, (0, Fake((3, 8))), "outside"), (r.update_lights, (1, Fake((2, 8))), "outside"),
        (r.update_texture, (0, Fake((21, 37, 4), dtype=u8, index=1)), "cuda:1"), (r.update_texture, (0, Fake((21, 37, 4))), "float32"),
        (r.update_texture, (0, Fake((21, 37, 4), dtype=u8, contiguous=False)), "contiguous"), (r.update_texture, (0, Fake((21, 37, 4), dtype=u8, ptr=0x1004)), "16-byte"),
        (r.update_texture, (0, Fake((37, 21, 4), dtype=u8)), "shape"), (r.update_texture, (2, Fake((21, 37, 4), dtype=u8)), "shape"),
    ]
    for fn, args, word in bad:
        with pytest.raises(VkrtError, match=word):
            fn(*args)
    for fn, args, name in ((r.update_lights, (0, Fake((2, 8))), "vkrt_scene_update_lights"), (r.update_lights, (1, Fake((1, 8))), "vkrt_scene_update_lights"),
                           (r.update_texture, (0, Fake((21, 37, 4), dtype=u8)), "vkrt_scene_update_texture"),
                           (r.update_texture, (2, Fake((2, 8, 4), dtype=u8)), "vkrt_scene_update_texture")):
        with pytest.raises(AssertionError, match=name):
            fn(*args)


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------
def test_scene_edit_kernels_have_no_private_segment():
    """the compiler's resource report (tools/kernel_resources.py) for gfx950 equals the committed copy of it: no scratch, no spills"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    kernels, problems = kernel_resources.measure("scene_edit.hip", KERNELS)
    assert not problems, problems
    assert set(kernels) == set(KERNELS)
    for k, v in kernels.items():
        assert v["scratch_bytes"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (k, v)
        assert v["static_lds_bytes"] == (3072 if k.startswith("k_se_mip") else 0), (k, v)  # the decode table and the thresholds
    doc = json.load(open(os.path.join(ROOT, "profiles", "scene_edit_kernel_resources.json")))
    assert doc["conditions_met"] and not doc["problems"]
    assert doc["kernels"] == kernels  # the committed report is the one of this tree
