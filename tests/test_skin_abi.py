"""CPU-side checks of vkrt_scene_add_skin / vkrt_scene_skin_vertices / vkrt_debug_read_vertices: declared, exported, laid out like the
ctypes record, refused without a device in the order the header states (each message naming its argument), the Python layer's refusals
before the call, and the kernels' register report."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import vkrt_amd
from vkrt_amd import abi

ROOT = vkrt_amd.REPO_ROOT
NEW = ("vkrt_scene_add_skin", "vkrt_scene_skin_vertices", "vkrt_debug_read_vertices")


def _lib():
    assert os.path.exists(vkrt_amd.LIB_PATH), "run __graft_entry__.build() first"
    return abi.declare_vkrt(C.CDLL(vkrt_amd.LIB_PATH))


def test_skin_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    declared = set(re.findall(r"\b(vkrt_[a-z_]+)\s*\(", header))
    lib = C.CDLL(vkrt_amd.LIB_PATH)
    for name in NEW:
        assert name in declared and name in abi.VKRT_SYMBOLS and hasattr(lib, name), name
    assert _lib().vkrt_abi_version() == 4 == abi.VKRT_ABI_VERSION  # added without a version change: detect by symbol
    for name in abi.VKRT_SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    mk = open(os.path.join(ROOT, "vk-raytracing-engine_amd", "csrc", "Makefile")).read()
    assert "skin.hip" in mk and os.path.exists(os.path.join(ROOT, "vk-raytracing-engine_amd", "csrc", "skin.hip"))
    # what the header owes its reader: the arithmetic, the untouched texture coordinates, the limit of the normal transform
    for phrase in ("M[r][c] = ((w0*J[j0][r][c] + w1*J[j1][r][c]) + w2*J[j2][r][c]) + w3*J[j3][r][c]", "Texture coordinates are never touched",
                   "non-uniform scale", "not renormalised"):
        assert phrase in header, phrase


def test_skin_desc_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of vkrt_skin_desc, compiled as C and as C++, equal the ctypes record."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vkrt.h"', "int main(void){", '  printf("%zu\\n", sizeof(vkrt_skin_desc));']
    expect = [C.sizeof(abi.SkinDesc)]
    for fname, _ in abi.SkinDesc._fields_:
        lines.append(f'  printf("%zu\\n", offsetof(vkrt_skin_desc, {fname}));')
        expect.append(getattr(abi.SkinDesc, fname).offset)
    lines.append("  return 0; }")
    for ext, cc in (("c", "gcc"), ("cpp", "g++")):
        src = tmp_path / f"layout.{ext}"
        src.write_text("\n".join(lines) + "\n")
        exe = tmp_path / f"layout_{cc}"
        subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
        assert [int(x) for x in out] == expect
    assert C.sizeof(abi.SkinDesc) == 32 and [f for f, _ in abi.SkinDesc._fields_] == ["struct_size", "first", "count", "joint_count", "joints", "weights"]


def test_add_skin_refusals_that_need_no_device_come_in_the_headers_order():
    """NULL desc, struct_size, joint_count, NULL arrays, a joint index, a weight, NULL out_skin, NULL scene: each refusal wins over every
    later one and names its argument."""
    lib = _lib()
    fn = lib.vkrt_scene_add_skin
    out = abi.c_u(99)
    good_j, good_w = np.zeros((3, 4), np.uint16), np.full((3, 4), 0.25, np.float32)
    bad_j, bad_w = good_j.copy(), good_w.copy()
    bad_j[2, 1] = 5
    bad_w[1, 3] = np.inf

    def desc(size=None, count=3, joint_count=5, joints=good_j, weights=good_w):
        return abi.SkinDesc(C.sizeof(abi.SkinDesc) if size is None else size, 0, count, joint_count, None if joints is None else joints.ctypes.data,
                            None if weights is None else weights.ctypes.data)

    def refused(d, word, no_out=False, absent=()):
        assert fn(None, None if d is None else C.byref(d), None, None if no_out else C.byref(out)) == abi.VKRT_ERR_INVALID_ARGUMENT
        msg = lib.vkrt_last_error()
        assert word in msg and b"vkrt_scene_add_skin" in msg and not any(a in msg for a in absent), msg

    refused(None, b"desc is NULL", no_out=True)
    # everything behind struct_size is wrong as well
    for size in (0, 16, C.sizeof(abi.SkinDesc) - 1):
        refused(desc(size=size, joint_count=0, joints=None, weights=None), b"struct_size", no_out=True)
    for jc in (0, 65537, 0xFFFFFFFF):
        refused(desc(joint_count=jc, joints=None, weights=None), b"joint_count", no_out=True, absent=(b"struct_size",))
    refused(desc(joints=None, weights=None), b"joints is NULL", no_out=True)
    refused(desc(weights=None, joints=bad_j), b"weights is NULL", no_out=True)
    refused(desc(joints=bad_j, weights=bad_w), b"joints[9]", no_out=True)
    refused(desc(joints=bad_j, joint_count=5, weights=bad_w), b"joint_count is 5", no_out=True)
    refused(desc(weights=bad_w), b"weights[7]", no_out=True)
    refused(desc(), b"out_skin is NULL", no_out=True)
    # a good desc reaches the scene check (joint_count 65536 and index 5 of 6 are in range; a longer struct is accepted; count 0 comes later)
    bad_j6 = desc(joints=bad_j, joint_count=6)
    for d in (desc(), desc(joint_count=65536), bad_j6, desc(size=64), desc(count=0), desc(count=0, joints=None, weights=None)):
        refused(d, b"scene is NULL")
    assert out.value == 99


def test_skin_vertices_and_read_vertices_refusals_without_a_device():
    lib = _lib()
    fn = lib.vkrt_scene_skin_vertices
    m = np.zeros((1, 16), np.float32)
    for memory in (2, 7, 0xFFFFFFFF):
        assert fn(None, 0, None, memory, None) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert b"memory" in lib.vkrt_last_error() and b"scene is NULL" not in lib.vkrt_last_error()
    for memory, ptr in ((abi.VKRT_MEMORY_HOST, m.ctypes.data), (abi.VKRT_MEMORY_DEVICE, None), (abi.VKRT_MEMORY_DEVICE, 4)):
        assert fn(None, 3, ptr, memory, None) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert b"vkrt_scene_skin_vertices: scene is NULL" in lib.vkrt_last_error()
    assert lib.vkrt_debug_read_vertices(None, 0, 1, m.ctypes.data, None, None, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"vkrt_debug_read_vertices: scene is NULL" in lib.vkrt_last_error()


def test_python_refuses_bad_skins_before_the_call():
    from renderer_stand_ins import renderer_without_scene
    from vkrt_amd.renderer import VkrtError

    r = renderer_without_scene(10, skins=[(6, 2, 3)])
    j, w = (lambda n: np.zeros((n, 4), np.uint16)), (lambda n: np.full((n, 4), 0.25, np.float32))
    nan = w(2)
    nan[1, 2] = np.nan
    bad = [
        (dict(first=0, joints=np.zeros((2, 4), np.float32), weights=w(2)), "joints"),           # dtype
        (dict(first=0, joints=j(2), weights=np.zeros((2, 4), np.float64)), "weights"),
        (dict(first=0, joints=j(2), weights=np.zeros((2, 4), np.int32)), "weights"),
        (dict(first=0, joints=np.zeros((2, 3), np.uint16), weights=w(2)), "joints"),            # shape
        (dict(first=0, joints=j(2), weights=np.zeros(8, np.float32)), "weights"),
        (dict(first=0, joints=np.zeros((4, 4), np.uint16)[::2], weights=w(2)), "joints"),       # not contiguous
        (dict(first=0, joints=[[0, 0, 0, 0]], weights=w(1)), "joints"),                         # not numpy
        (dict(first=0, joints=j(2), weights=w(3)), "weights"),                                  # lengths differ
        (dict(first=9, joints=j(2), weights=w(2)), "first"),                                    # range
        (dict(first=-1, joints=j(2), weights=w(2)), "first"),
        (dict(first=1.5, joints=j(2), weights=w(2)), "first"),
        (dict(first=0, joints=j(0), weights=w(0)), "first"),                                    # empty
        (dict(first=5, joints=j(2), weights=w(2)), "overlap"),                                  # an existing skin's range
        (dict(first=7, joints=j(1), weights=w(1)), "overlap"),
        (dict(first=0, joints=j(2) + 3, weights=w(2), joint_count=3), "joints"),                # index outside joint_count
        (dict(first=0, joints=np.full((2, 4), -1, np.int32), weights=w(2), joint_count=3), "joints"),
        (dict(first=0, joints=j(2), weights=w(2), joint_count=0), "joint_count"),
        (dict(first=0, joints=j(2), weights=w(2), joint_count=65537), "joint_count"),
        (dict(first=0, joints=j(2), weights=nan), "weights"),                                   # non-finite
    ]
    for kw, word in bad:
        with pytest.raises(VkrtError, match=word):
            r.add_skin(**kw)
    assert r._skins == [(6, 2, 3)]
    # good calls reach the library (here: the stand-in that refuses to be reached): any integer dtype, ranges touching the skin's
    for kw in (dict(first=4, joints=j(2), weights=w(2)), dict(first=8, joints=np.ones((2, 4), np.int64), weights=w(2), joint_count=65536)):
        with pytest.raises(AssertionError, match="vkrt_scene_add_skin"):
            r.add_skin(**kw)
    m = np.zeros((3, 16), np.float32)
    inf = m.copy()
    inf[2, 15] = np.inf
    bad = [
        (dict(skin=1, joint_matrices=m), "skin 1"),                                             # skin index
        (dict(skin=-1, joint_matrices=m), "skin -1"),
        (dict(skin=0.0, joint_matrices=m), "skin 0.0"),
        (dict(skin=0, joint_matrices=m.astype(np.float64)), "joint_matrices"),                  # dtype
        (dict(skin=0, joint_matrices=np.zeros((2, 16), np.float32)), "joint_matrices"),         # shape: the skin's joint_count
        (dict(skin=0, joint_matrices=np.zeros((3, 4, 4), np.float32)), "joint_matrices"),
        (dict(skin=0, joint_matrices=np.zeros((6, 16), np.float32)[::2]), "joint_matrices"),    # not contiguous
        (dict(skin=0, joint_matrices=m.tolist()), "joint_matrices"),                            # neither numpy nor torch
        (dict(skin=0, joint_matrices=inf), "non-finite"),
    ]
    import torch

    bad.append((dict(skin=0, joint_matrices=torch.zeros(3, 16)), "joint_matrices"))             # a tensor that is not on the scene's device
    for kw, word in bad:
        with pytest.raises(VkrtError, match=word):
            r.skin(**kw)
    with pytest.raises(AssertionError, match="vkrt_scene_skin_vertices"):
        r.skin(0, m)
    for first, count in ((9, 2), (-1, 1), (0, 11), (0.5, 1), (0, -1)):
        with pytest.raises(VkrtError, match="first"):
            r.read_vertices(first, count)
    with pytest.raises(AssertionError, match="vkrt_debug_read_vertices"):
        r.read_vertices(8, 2)


def test_python_refuses_tensor_faults_through_a_stand_in():
    """Device matrices without a device: a stand-in that answers like a tensor on cuda:0 reaches the dtype, contiguity, alignment, device
    and shape checks."""
    import torch
    from renderer_stand_ins import Fake, renderer_without_scene
    from vkrt_amd.renderer import VkrtError

    r = renderer_without_scene(10, skins=[(0, 4, 3)])
    bad = [
        (Fake((3, 16), index=1), "cuda:1"),
        (Fake((3, 16), dtype=torch.float64), "float64"),
        (Fake((3, 16), contiguous=False), "contiguous"),
        (Fake((3, 16), ptr=0x1004), "16-byte aligned"),
        (Fake((4, 16)), "shape"),
        (Fake((48,)), "shape"),
    ]
    for m, word in bad:
        with pytest.raises(VkrtError, match=word):
            r.skin(0, m)
    with pytest.raises(AssertionError, match="vkrt_scene_skin_vertices"):
        r.skin(0, Fake((3, 16)))


def test_skin_kernels_use_no_scratch_and_spill_nothing():
    """the compiler's resource report (tools/kernel_resources.py) for gfx950, and the committed copy of it"""
    import json

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    kernels, problems = kernel_resources.measure("skin.hip", ("k_skin", "k_skin_capture"))
    assert not problems, problems
    assert set(kernels) == {"k_skin", "k_skin_capture"}
    for k, v in kernels.items():
        assert v["scratch_bytes"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (k, v)
    doc = json.load(open(os.path.join(ROOT, "profiles", "skin_kernel_resources.json")))
    assert doc["conditions_met"] and set(doc["kernels"]) == set(kernels)
