"""CPU-side checks of vkrt_scene_add_morph / vkrt_scene_morph_vertices: declared, exported, laid out like the ctypes record, refused
without a device in the order the header states (each message naming its argument), the Python layer's refusals before the call, and
the kernels' register report."""
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

ROOT = vkrt_amd.REPO_ROOT
NEW = ("vkrt_scene_add_morph", "vkrt_scene_morph_vertices")
F = np.float32


def _lib():
    assert os.path.exists(vkrt_amd.LIB_PATH), "run __graft_entry__.build() first"
    return abi.declare_vkrt(C.CDLL(vkrt_amd.LIB_PATH))


def test_morph_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    declared = set(re.findall(r"\b(vkrt_[a-z_]+)\s*\(", header))
    lib = C.CDLL(vkrt_amd.LIB_PATH)
    for name in NEW:
        assert name in declared and name in abi.VKRT_SYMBOLS and hasattr(lib, name), name
    assert _lib().vkrt_abi_version() == 4 == abi.VKRT_ABI_VERSION  # added without a version change: detect by symbol
    for name in abi.VKRT_SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    assert re.search(r"#define\s+VKRT_MORPH_TARGETS_MAX\s+256\b", header) and abi.VKRT_MORPH_TARGETS_MAX == 256
    mk = open(os.path.join(ROOT, "vk-raytracing-engine_amd", "csrc", "Makefile")).read()
    assert "morph.hip" in mk and os.path.exists(os.path.join(ROOT, "vk-raytracing-engine_amd", "csrc", "morph.hip"))
    # what the header owes its reader: the arithmetic, the skipped zero weight, the two destinations, the order of skins and morphs
    for phrase in ("P = p;  for k = 0..T-1 in index order:  if (w[k] != 0)  P = P + w[k] * dP[k]",
                   "n'      = (the morph has normal deltas and some w[k] != 0) ? normalizeGuarded(N) : n",
                   "(d > 0 && d < inf) ? a * (1.0f / sqrtf(d)) : a", "binary32, in source order, no contraction",
                   "A weight of exactly zero, of either sign, skips its target", "texture coordinates are never", "morph, then skin",
                   "writes that bind pose and nothing else", "a range that\n * overlaps an existing morph's"):
        assert phrase in header, phrase


def test_morph_desc_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of vkrt_morph_desc, compiled as C and as C++, equal the ctypes record."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vkrt.h"', "int main(void){", '  printf("%zu\\n", sizeof(vkrt_morph_desc));']
    expect = [C.sizeof(abi.MorphDesc)]
    for fname, _ in abi.MorphDesc._fields_:
        lines.append(f'  printf("%zu\\n", offsetof(vkrt_morph_desc, {fname}));')
        expect.append(getattr(abi.MorphDesc, fname).offset)
    lines.append("  return 0; }")
    for ext, cc in (("c", "gcc"), ("cpp", "g++")):
        src = tmp_path / f"layout.{ext}"
        src.write_text("\n".join(lines) + "\n")
        exe = tmp_path / f"layout_{cc}"
        subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
        assert [int(x) for x in out] == expect
    assert C.sizeof(abi.MorphDesc) == 40
    assert [f for f, _ in abi.MorphDesc._fields_] == ["struct_size", "first", "count", "target_count", "position_deltas", "normal_deltas", "tangent_deltas"]


def test_add_morph_refusals_that_need_no_device_come_in_the_headers_order():
    """NULL desc, struct_size, target_count, no delta array, a non-finite delta (positions, then normals, then tangents), NULL
    out_morph, NULL scene: each refusal wins over every later one and names its argument."""
    lib = _lib()
    fn = lib.vkrt_scene_add_morph
    out = abi.c_u(99)
    good = np.zeros((2, 3, 3), F)
    bad_p, bad_n, bad_t = good.copy(), good.copy(), good.copy()
    bad_p[1, 2, 0] = np.nan   # element 15: target 1, vertex 2 (+ first)
    bad_n[0, 1, 1] = np.inf   # element 4
    bad_t[1, 0, 2] = -np.inf  # element 11

    def desc(size=None, first=0, count=3, targets=2, p=good, n=None, t=None):
        ptr = [None if a is None else a.ctypes.data for a in (p, n, t)]
        return abi.MorphDesc(C.sizeof(abi.MorphDesc) if size is None else size, first, count, targets, *ptr)

    def refused(d, word, no_out=False, absent=()):
        assert fn(None, None if d is None else C.byref(d), None, None if no_out else C.byref(out)) == abi.VKRT_ERR_INVALID_ARGUMENT
        msg = lib.vkrt_last_error()
        assert word in msg and b"vkrt_scene_add_morph" in msg and not any(a in msg for a in absent), msg

    refused(None, b"desc is NULL", no_out=True)
    # everything behind struct_size is wrong as well
    for size in (0, 16, C.sizeof(abi.MorphDesc) - 1):
        refused(desc(size=size, targets=0, p=None), b"struct_size", no_out=True)
    for T in (0, 257, 0xFFFFFFFF):
        refused(desc(targets=T, p=None), b"target_count", no_out=True, absent=(b"struct_size",))
    refused(desc(p=None), b"all NULL", no_out=True, absent=(b"target_count",))
    refused(desc(p=bad_p, n=bad_n, t=bad_t), b"position_deltas[15] (target 1, vertex 2)", no_out=True)
    refused(desc(first=7, p=bad_p), b"position_deltas[15] (target 1, vertex 9)", no_out=True)
    refused(desc(p=good, n=bad_n, t=bad_t), b"normal_deltas[4] (target 0, vertex 1)", no_out=True)
    refused(desc(p=None, n=good, t=bad_t), b"tangent_deltas[11] (target 1, vertex 0)", no_out=True)
    refused(desc(), b"out_morph is NULL", no_out=True)
    # a good desc reaches the scene check (256 targets are in range; a longer struct is accepted; count 0 comes later, and has no deltas
    # to inspect; any one array is enough)
    many = np.zeros((256, 1, 3), F)
    for d in (desc(), desc(p=None, n=good), desc(p=None, t=good), desc(p=good, n=good, t=good), desc(count=1, targets=256, p=many), desc(size=64),
              desc(count=0, p=bad_p)):
        refused(d, b"scene is NULL")
    assert out.value == 99


def test_morph_vertices_refusals_without_a_device():
    lib = _lib()
    fn = lib.vkrt_scene_morph_vertices
    w = np.zeros(4, F)
    for memory in (2, 7, 0xFFFFFFFF):
        assert fn(None, 0, None, memory, None) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert b"memory" in lib.vkrt_last_error() and b"scene is NULL" not in lib.vkrt_last_error()
    for memory, ptr in ((abi.VKRT_MEMORY_HOST, w.ctypes.data), (abi.VKRT_MEMORY_DEVICE, None), (abi.VKRT_MEMORY_DEVICE, 2)):
        assert fn(None, 3, ptr, memory, None) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert b"vkrt_scene_morph_vertices: scene is NULL" in lib.vkrt_last_error()


def test_the_header_lists_the_refusals_in_the_order_the_library_applies():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    sec = header[header.index("vkrt_scene_add_morph binds"):header.index("#define VKRT_MORPH_TARGETS_MAX")]
    add = ["a NULL desc", "struct_size < sizeof(vkrt_morph_desc)", "target_count 0 or above", "all three delta arrays NULL", "a non-finite delta",
           "a NULL out_morph", "a NULL scene", "a range outside the scene's vertices", "count == 0", "overlaps an existing", "straddles a skin's boundary",
           "VKRT_ERR_NO_DEVICE", "VKRT_ERR_OUT_OF_MEMORY"]
    at = [sec.index(p) for p in add]
    assert at == sorted(at), add
    pose = sec[sec.index("vkrt_scene_morph_vertices poses"):]
    seq = ["a memory value that is neither", "a NULL scene", "morph index out of range", "misaligned weights", "a non-finite weight", "VKRT_ERR_NO_DEVICE"]
    at = [pose.index(p) for p in seq]
    assert at == sorted(at), seq


def test_python_refuses_bad_morphs_before_the_call():
    from renderer_stand_ins import renderer_without_scene
    from vkrt_amd.renderer import VkrtError

    r = renderer_without_scene(20, skins=[(10, 6, 3)], morphs=[(4, 2, 3)])
    d = lambda n, T=2: np.zeros((T, n, 3), F)  # noqa: E731
    nan = d(2)
    nan[1, 0, 2] = np.nan
    bad = [
        (dict(first=0), "all None"),
        (dict(first=0, position_deltas=np.zeros((2, 2, 3), np.float64)), "position_deltas"),        # dtype
        (dict(first=0, normal_deltas=np.zeros((2, 2, 3), np.int32)), "normal_deltas"),
        (dict(first=0, tangent_deltas=np.zeros((2, 2, 4), F)), "tangent_deltas"),                   # shape: xyz only
        (dict(first=0, position_deltas=np.zeros((2, 3), F)), "position_deltas"),
        (dict(first=0, position_deltas=np.zeros((2, 4, 3), F)[:, ::2]), "position_deltas"),         # not contiguous
        (dict(first=0, position_deltas=[[[0.0, 0.0, 0.0]]]), "position_deltas"),                    # not numpy
        (dict(first=0, position_deltas=d(2), normal_deltas=d(3)), "normal_deltas"),                 # shapes differ
        (dict(first=0, position_deltas=d(2), tangent_deltas=d(2, 3)), "tangent_deltas"),
        (dict(first=0, position_deltas=d(1, 257)), "targets"),                                      # target count
        (dict(first=0, position_deltas=d(2, 0)), "targets"),
        (dict(first=19, position_deltas=d(2)), "first"),                                            # range
        (dict(first=-1, position_deltas=d(2)), "first"),
        (dict(first=1.5, position_deltas=d(2)), "first"),
        (dict(first=0, position_deltas=d(0)), "first"),                                             # empty
        (dict(first=3, position_deltas=d(2)), "overlap"),                                           # an existing morph's range
        (dict(first=5, position_deltas=d(1)), "overlap"),
        (dict(first=9, position_deltas=d(2)), "straddle"),                                          # across a skin's boundary
        (dict(first=15, position_deltas=d(2)), "straddle"),
        (dict(first=8, position_deltas=d(10)), "straddle"),
        (dict(first=0, position_deltas=nan), "position_deltas"),                                    # non-finite
        (dict(first=0, position_deltas=d(2), normal_deltas=nan), "normal_deltas"),
    ]
    for kw, word in bad:
        with pytest.raises(VkrtError, match=word):
            r.add_morph(**kw)
    assert r._morphs == [(4, 2, 3)]
    # good calls reach the library (here: the stand-in that refuses to be reached): ranges touching the morph's, inside the skin's, at
    # the skin's edges, the skin's whole range, the scene's last vertex
    for kw in (dict(first=2, position_deltas=d(2)), dict(first=6, normal_deltas=d(4)), dict(first=11, tangent_deltas=d(3)),
               dict(first=10, position_deltas=d(6)), dict(first=16, position_deltas=d(4, 256))):
        with pytest.raises(AssertionError, match="vkrt_scene_add_morph"):
            r.add_morph(**kw)
    # a skin over a morph: skins come first
    with pytest.raises(VkrtError, match="overlap morph 0"):
        r.add_skin(3, np.zeros((2, 4), np.uint16), np.full((2, 4), 0.25, F))
    with pytest.raises(AssertionError, match="vkrt_scene_add_skin"):
        r.add_skin(6, np.zeros((2, 4), np.uint16), np.full((2, 4), 0.25, F))
    w = np.zeros(3, F)
    inf = w.copy()
    inf[2] = np.inf
    bad = [
        (dict(morph=1, weights=w), "morph 1"),                                                      # morph index
        (dict(morph=-1, weights=w), "morph -1"),
        (dict(morph=0.0, weights=w), "morph 0.0"),
        (dict(morph=0, weights=w.astype(np.float64)), "weights"),                                   # dtype
        (dict(morph=0, weights=np.zeros(2, F)), "weights"),                                         # shape: the morph's target count
        (dict(morph=0, weights=np.zeros((3, 1), F)), "weights"),
        (dict(morph=0, weights=np.zeros(6, F)[::2]), "weights"),                                    # not contiguous
        (dict(morph=0, weights=w.tolist()), "weights"),                                             # neither numpy nor torch
        (dict(morph=0, weights=inf), "non-finite"),
    ]
    import torch

    bad.append((dict(morph=0, weights=torch.zeros(3)), "weights"))                                  # a tensor that is not on the scene's device
    for kw, word in bad:
        with pytest.raises(VkrtError, match=word):
            r.morph(**kw)
    with pytest.raises(AssertionError, match="vkrt_scene_morph_vertices"):
        r.morph(0, w)


def test_python_refuses_tensor_faults_through_a_stand_in():
    """Device weights without a device: a stand-in that answers like a tensor on cuda:0 reaches the dtype, contiguity, alignment, device
    and shape checks."""
    import torch
    from renderer_stand_ins import Fake, renderer_without_scene
    from vkrt_amd.renderer import VkrtError

    r = renderer_without_scene(10, morphs=[(0, 4, 3)])
    bad = [
        (Fake((3,), index=1), "cuda:1"),
        (Fake((3,), dtype=torch.float64), "float64"),
        (Fake((3,), contiguous=False), "contiguous"),
        (Fake((3,), ptr=0x1002), "4-byte aligned"),
        (Fake((4,)), "shape"),
        (Fake((3, 1)), "shape"),
    ]
    for w, word in bad:
        with pytest.raises(VkrtError, match=word):
            r.morph(0, w)
    with pytest.raises(AssertionError, match="vkrt_scene_morph_vertices"):
        r.morph(0, Fake((3,), ptr=0x1004))  # (4-byte alignment is enough)


def test_morph_kernels_use_no_scratch_and_spill_nothing():
    """the compiler's resource report (tools/kernel_resources.py) for gfx950 equals the committed copy of it"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    kernels, problems = kernel_resources.measure("morph.hip", ("k_morph_live", "k_morph_bind"))
    assert not problems, problems
    assert set(kernels) == {"k_morph_live", "k_morph_bind"}
    for k, v in kernels.items():
        assert v["scratch_bytes"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (k, v)
    doc = json.load(open(os.path.join(ROOT, "profiles", "morph_kernel_resources.json")))
    assert doc["conditions_met"] and not doc["problems"]
    assert doc["kernels"] == kernels  # the committed report is the one of this tree
