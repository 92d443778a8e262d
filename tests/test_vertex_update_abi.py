"""CPU-side checks of vkrt_scene_update_vertices: declared, exported, laid out like the ctypes record, refused without a device in the
order the header states (each message naming the argument), and the Python layer's refusals before the call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import vkrt_amd
from vkrt_amd import abi

ROOT = vkrt_amd.REPO_ROOT
NEW = "vkrt_scene_update_vertices"


def _lib():
    assert os.path.exists(vkrt_amd.LIB_PATH), "run __graft_entry__.build() first"
    return abi.declare_vkrt(C.CDLL(vkrt_amd.LIB_PATH))


def test_vertex_update_symbol_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    declared = set(re.findall(r"\b(vkrt_[a-z_]+)\s*\(", header))
    assert NEW in declared and NEW in abi.VKRT_SYMBOLS
    assert hasattr(C.CDLL(vkrt_amd.LIB_PATH), NEW)
    assert _lib().vkrt_abi_version() == 4 == abi.VKRT_ABI_VERSION  # added without a version change: detect by symbol
    assert (abi.VKRT_MEMORY_HOST, abi.VKRT_MEMORY_DEVICE) == (0, 1)
    assert "no vertex deformation" not in header
    # every symbol the header declares is still in abi.VKRT_SYMBOLS and exported
    lib = C.CDLL(vkrt_amd.LIB_PATH)
    for name in abi.VKRT_SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    # the new translation unit is part of the library's build
    mk = open(os.path.join(ROOT, "vk-raytracing-engine_amd", "csrc", "Makefile")).read()
    assert "vertex_update.hip" in mk and os.path.exists(os.path.join(ROOT, "vk-raytracing-engine_amd", "csrc", "vertex_update.hip"))


def test_vertex_update_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of vkrt_vertex_update, compiled as C and as C++, equal the ctypes record; the enum values equal abi.py's."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vkrt.h"', "int main(void){", '  printf("%zu\\n", sizeof(vkrt_vertex_update));']
    expect = [C.sizeof(abi.VertexUpdate)]
    for fname, _ in abi.VertexUpdate._fields_:
        lines.append(f'  printf("%zu\\n", offsetof(vkrt_vertex_update, {fname}));')
        expect.append(getattr(abi.VertexUpdate, fname).offset)
    for name in ("VKRT_MEMORY_HOST", "VKRT_MEMORY_DEVICE"):
        lines.append(f'  printf("%d\\n", (int){name});')
        expect.append(getattr(abi, name))
    lines.append("  return 0; }")
    for ext, cc in (("c", "gcc"), ("cpp", "g++")):
        src = tmp_path / f"layout.{ext}"
        src.write_text("\n".join(lines) + "\n")
        exe = tmp_path / f"layout_{cc}"
        subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
        assert [int(x) for x in out] == expect
    assert C.sizeof(abi.VertexUpdate) == 48


def _update(first=0, count=2, memory=abi.VKRT_MEMORY_HOST, size=None, positions=None):
    return abi.VertexUpdate(C.sizeof(abi.VertexUpdate) if size is None else size, first, count, memory,
                            positions.ctypes.data if positions is not None else None, None, None, None)


def test_refusals_that_need_no_device_come_in_the_headers_order():
    """NULL update, then struct_size, then memory, then the NULL scene: each refusal wins over every later one, and names its argument."""
    lib = _lib()
    nan = np.full((2, 3), np.nan, np.float32)
    fn = lib.vkrt_scene_update_vertices
    assert fn(None, None, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"update is NULL" in lib.vkrt_last_error()
    # a struct that is too small, with a bad memory value, a NULL scene and NaN positions behind it
    for size in (0, 16, C.sizeof(abi.VertexUpdate) - 1):
        assert fn(None, C.byref(_update(size=size, memory=7, positions=nan)), None) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert b"struct_size" in lib.vkrt_last_error(), lib.vkrt_last_error()
    for memory in (2, 7, 0xFFFFFFFF):
        assert fn(None, C.byref(_update(memory=memory, positions=nan)), None) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert b"memory" in lib.vkrt_last_error() and b"struct_size" not in lib.vkrt_last_error(), lib.vkrt_last_error()
    # good struct and memory reach the scene check, whatever the arrays hold; a larger struct_size (a later, longer struct) is accepted
    for u in (_update(), _update(memory=abi.VKRT_MEMORY_DEVICE), _update(positions=nan), _update(count=0), _update(size=64)):
        assert fn(None, C.byref(u), None) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert b"scene is NULL" in lib.vkrt_last_error(), lib.vkrt_last_error()


def test_python_refuses_bad_arrays_and_ranges_before_the_call():
    import torch
    from renderer_stand_ins import renderer_without_scene
    from vkrt_amd.renderer import VkrtError

    r = renderer_without_scene(10)
    f32 = lambda n, w: np.zeros((n, w), np.float32)  # noqa: E731
    bad = [
        (dict(first=0, positions=np.zeros((2, 3), np.float64)), "positions"),          # dtype
        (dict(first=0, normals=np.zeros((2, 3), np.int32)), "normals"),
        (dict(first=0, positions=f32(2, 4)), "positions"),                             # shape
        (dict(first=0, tangents=f32(2, 3)), "tangents"),
        (dict(first=0, texcoords0=f32(2, 3)), "texcoords0"),
        (dict(first=0, positions=np.zeros(6, np.float32)), "positions"),
        (dict(first=0, positions=np.zeros((4, 3), np.float32)[::2]), "positions"),     # not contiguous
        (dict(first=0, positions=[[0.0, 0.0, 0.0]]), "positions"),                     # neither numpy nor torch
        (dict(first=0, positions=f32(2, 3), normals=f32(3, 3)), "normals"),            # lengths differ
        (dict(first=0, positions=f32(2, 3), texcoords0=f32(1, 2)), "texcoords0"),
        (dict(first=9, positions=f32(2, 3)), "first"),                                 # range outside the scene
        (dict(first=-1, positions=f32(2, 3)), "first"),
        (dict(first=11), "first"),
        (dict(first=0, positions=f32(11, 3)), "first"),
        (dict(first=1.5, positions=f32(2, 3)), "first"),
        (dict(first=0, positions=torch.zeros(2, 3)), "positions"),                     # a tensor that is not on the scene's device
        (dict(first=0, positions=f32(2, 3), normals=torch.zeros(2, 3)), "normals"),    # (refused as a CPU tensor before the mix is seen)
    ]
    for kw, word in bad:
        with pytest.raises(VkrtError, match=word):
            r.update_vertices(**kw)


def test_python_refuses_tensor_faults_through_a_stand_in():
    """Device tensors without a device: a stand-in that answers like a tensor on cuda:0 reaches the dtype, contiguity, device and
    numpy / torch mix checks."""
    import torch
    from renderer_stand_ins import Fake, renderer_without_scene
    from vkrt_amd.renderer import VkrtError

    r = renderer_without_scene(10)
    bad = [
        (dict(first=0, positions=Fake((2, 3), index=1)), "positions"),                          # another device
        (dict(first=0, positions=Fake((2, 3), dtype=torch.float64)), "positions"),              # dtype
        (dict(first=0, tangents=Fake((2, 4), contiguous=False)), "tangents"),                   # not contiguous
        (dict(first=0, positions=Fake((2, 3)), normals=np.zeros((2, 3), np.float32)), "mixed"),  # numpy and torch in one call
        (dict(first=0, positions=np.zeros((2, 3), np.float32), normals=Fake((2, 3))), "mixed"),
        (dict(first=0, positions=Fake((2, 3)), normals=Fake((3, 3))), "normals"),               # lengths differ
        (dict(first=9, positions=Fake((2, 3))), "first"),                                       # range
    ]
    for kw, word in bad:
        with pytest.raises(VkrtError, match=word):
            r.update_vertices(**kw)
    # and a good call reaches the library (here: the stand-in that refuses to be reached)
    with pytest.raises(AssertionError, match="vkrt_scene_update_vertices"):
        r.update_vertices(0, positions=Fake((2, 3)), texcoords0=Fake((2, 2)))
    with pytest.raises(AssertionError, match="vkrt_scene_update_vertices"):
        r.update_vertices(8, positions=np.zeros((2, 3), np.float32))
