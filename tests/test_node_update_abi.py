"""CPU-side checks of vkrt_scene_update_node_transforms and vkrt_debug_read_instances: declared, exported, laid out like the ctypes
record, refused without a scene in the order the header states (each message naming its argument), the Python layer's refusals before the
call, and the kernels' register report."""
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
NEW = ("vkrt_scene_update_node_transforms", "vkrt_debug_read_instances")
F = np.float32
BAD = abi.VKRT_ERR_INVALID_ARGUMENT


def _lib():
    assert os.path.exists(vkrt_amd.LIB_PATH), "run __graft_entry__.build() first"
    return abi.declare_vkrt(C.CDLL(vkrt_amd.LIB_PATH))


def test_node_update_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    declared = set(re.findall(r"\b(vkrt_[a-z_]+)\s*\(", header))
    lib = C.CDLL(vkrt_amd.LIB_PATH)
    for name in NEW:
        assert name in declared and name in abi.VKRT_SYMBOLS and hasattr(lib, name), name
    assert _lib().vkrt_abi_version() == 4 == abi.VKRT_ABI_VERSION  # added without a version change: detect by symbol
    for name in abi.VKRT_SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    assert C.sizeof(abi.Node) == 68  # no existing struct changed
    mk = open(os.path.join(ROOT, "vk-raytracing-engine_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert "node_update.hip" in srcs and os.path.exists(os.path.join(ROOT, "vk-raytracing-engine_amd", "csrc", "node_update.hip"))
    # what the header owes its reader: the record's formulas and layout, the scope of an update, the two memory kinds
    for phrase in ("o2w[4 r + c] = M[4 c + r]", "inv = 1.0 / det", "may differ between the two",
                   "the call changes transforms only", "the motion snapshot (vkrt_scene_motion_mark) is untouched",
                   "world_matrices 16-byte and node_indices 4-byte aligned", "The call is one kernel launch on hip_stream",
                   "An index >= node_count skips its entry", "which\n *   entry wins is unspecified", "the last entry wins",
                   "float o2w[12]", "float w2o[9]", "bytes != 96 * count"):
        assert phrase in header, phrase


def test_node_update_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of vkrt_node_update, compiled as C and as C++ under -Wall -Werror, equal the ctypes record."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vkrt.h"', "int main(void){", '  printf("%zu\\n", sizeof(vkrt_node_update));']
    expect = [C.sizeof(abi.NodeUpdate)]
    for fname, _ in abi.NodeUpdate._fields_:
        lines.append(f'  printf("%zu\\n", offsetof(vkrt_node_update, {fname}));')
        expect.append(getattr(abi.NodeUpdate, fname).offset)
    lines.append('  printf("%zu\\n", sizeof(vkrt_node));')
    expect.append(68)
    lines.append("  return 0; }")
    for ext, cc in (("c", "gcc"), ("cpp", "g++")):
        src = tmp_path / f"layout.{ext}"
        src.write_text("\n".join(lines) + "\n")
        exe = tmp_path / f"layout_{cc}"
        subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
        assert [int(x) for x in out] == expect
    assert C.sizeof(abi.NodeUpdate) == 32
    assert [f for f, _ in abi.NodeUpdate._fields_] == ["struct_size", "first", "count", "memory", "world_matrices", "node_indices"]


def _update(first=0, count=2, memory=abi.VKRT_MEMORY_HOST, size=None, matrices=None, indices=None):
    ptr = [a if a is None or isinstance(a, int) else a.ctypes.data for a in (matrices, indices)]
    return abi.NodeUpdate(C.sizeof(abi.NodeUpdate) if size is None else size, first, count, memory, *ptr)


def test_refusals_without_a_scene_come_in_the_headers_order():
    """NULL update, struct_size, memory, first != 0 with indices, NULL scene: each refusal wins over every later one and names its
    argument; what needs the scene (ranges, NULL or misaligned arrays, values) comes behind the NULL scene."""
    lib = _lib()
    fn = lib.vkrt_scene_update_node_transforms
    who = b"vkrt_scene_update_node_transforms: "
    nan = np.full((2, 16), np.nan, F)
    idx = np.array([0xFFFFFFFF, 7], np.uint32)

    def refused(u, text, absent=()):
        assert fn(None, None if u is None else C.byref(u), None) == BAD
        msg = lib.vkrt_last_error()
        assert msg.startswith(who) and text in msg and not any(a in msg for a in absent), msg

    refused(None, b"update is NULL")
    # everything behind struct_size is wrong as well
    for size in (0, 16, C.sizeof(abi.NodeUpdate) - 1):
        refused(_update(size=size, first=3, memory=7, matrices=nan, indices=idx), b"vkrt_node_update.struct_size %d < 32 (ABI mismatch)" % size)
    for memory in (2, 7, 0xFFFFFFFF):
        refused(_update(first=3, memory=memory, matrices=nan, indices=idx), b"memory %d is neither VKRT_MEMORY_HOST nor VKRT_MEMORY_DEVICE" % memory,
                absent=(b"struct_size",))
    for memory in (abi.VKRT_MEMORY_HOST, abi.VKRT_MEMORY_DEVICE):
        refused(_update(first=3, memory=memory, matrices=nan, indices=idx), b"first is 3 with node_indices given", absent=(b"memory",))
        refused(_update(first=1, count=0, memory=memory, indices=idx), b"first is 1 with node_indices given")
    # a good head reaches the scene check, whatever the arrays are: NULL, misaligned, non-finite, indices out of range, count 0; a larger
    # struct_size (a later, longer struct) is accepted
    for u in (_update(), _update(memory=abi.VKRT_MEMORY_DEVICE), _update(matrices=nan), _update(matrices=nan, indices=idx), _update(count=0),
              _update(size=64, first=9), _update(memory=abi.VKRT_MEMORY_DEVICE, matrices=0x1004, indices=0x1002), _update(first=0xFFFFFFFF, count=0xFFFFFFFF)):
        refused(u, b"scene is NULL", absent=(b"first is",))


def test_read_instances_refuses_null_arguments():
    lib = _lib()
    out = np.zeros(24, np.uint32)
    assert lib.vkrt_debug_read_instances(None, 0, 1, out.ctypes.data, 96) == BAD
    assert b"vkrt_debug_read_instances" in lib.vkrt_last_error()


def test_the_header_lists_the_refusals_in_the_order_the_library_applies():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    sec = header[header.index("moving instances from device memory"):header.index("typedef struct vkrt_node_update")]
    sec = sec[sec.index("Refused with VKRT_ERR_INVALID_ARGUMENT"):]
    seq = ["a NULL update", "struct_size < sizeof(vkrt_node_update)", "a\n * memory value that is neither", "first != 0 together with node_indices",
           "a NULL scene", "a dense range outside", "NULL world_matrices", "a misaligned array", "an index out of range", "a\n * non-finite element",
           "count == 0: VKRT_OK", "VKRT_ERR_NO_DEVICE"]
    at = [sec.index(p) for p in seq]
    assert at == sorted(at), seq


def _renderer(nodes=10):
    from renderer_stand_ins import renderer_without_scene

    r = renderer_without_scene(10)
    r._prim_mesh = np.zeros(nodes, np.int32)
    return r


def test_python_refuses_bad_updates_before_the_call():
    import torch
    from vkrt_amd.renderer import VkrtError

    r = _renderer(10)
    m = lambda n: np.zeros((n, 16), F)  # noqa: E731
    bad = [
        (dict(first=9, world_matrices=m(2)), "outside"),                                            # dense range (the host path as before)
        (dict(first=-1, world_matrices=m(2)), "outside"),
        (dict(first=1, world_matrices=m(2), indices=np.array([1, 2])), "first"),                    # first != 0 with indices
        (dict(first=0, world_matrices=m(2), indices=np.array([1, 10])), "indices"),                 # index out of range
        (dict(first=0, world_matrices=m(2), indices=np.array([-1, 2])), "indices"),
        (dict(first=0, world_matrices=m(2), indices=np.array([1, 2, 3])), "indices"),               # lengths differ
        (dict(first=0, world_matrices=m(2), indices=np.array([1.0, 2.0])), "indices"),              # dtype
        (dict(first=0, world_matrices=m(2), indices=torch.zeros(2, dtype=torch.int32)), "mixed"),   # numpy and torch
        (dict(first=0, world_matrices=torch.zeros(2, 16), indices=np.array([1, 2])), "mixed"),
        (dict(first=0, world_matrices=torch.zeros(2, 16)), "world_matrices"),                       # a tensor that is not on the scene's device
    ]
    for kw, word in bad:
        with pytest.raises(VkrtError, match=word):
            r.update_nodes(**kw)
    # good calls reach the library (here: the stand-in that refuses to be reached)
    with pytest.raises(AssertionError, match="vkrt_scene_update_nodes"):
        r.update_nodes(8, m(2))
    with pytest.raises(AssertionError, match="vkrt_scene_update_node_transforms"):
        r.update_nodes(0, m(3), indices=np.array([9, 0, 9]))
    for first, count in ((0, 11), (-1, 1), (10, 1), (0, -1), (1.5, 1)):
        with pytest.raises(VkrtError, match="read_instances"):
            r.read_instances(first, count)
    with pytest.raises(AssertionError, match="vkrt_debug_read_instances"):
        r.read_instances(0, 10)


def test_python_refuses_tensor_faults_through_a_stand_in():
    """Device tensors without a device: a stand-in that answers like a tensor on cuda:0 reaches the dtype, shape, contiguity, alignment
    and device checks of both tensors."""
    import torch
    from renderer_stand_ins import Fake
    from vkrt_amd.renderer import VkrtError

    r = _renderer(10)
    good, gi = Fake((3, 16)), Fake((3,), dtype=torch.int32)
    bad = [
        (dict(world_matrices=Fake((3, 16), index=1)), "cuda:1"),
        (dict(world_matrices=Fake((3, 16), dtype=torch.float64)), "float64"),
        (dict(world_matrices=Fake((3, 16), contiguous=False)), "contiguous"),
        (dict(world_matrices=Fake((3, 16), ptr=0x1008)), "16-byte aligned"),
        (dict(world_matrices=Fake((3, 4, 4))), "shape"),
        (dict(world_matrices=Fake((48,))), "shape"),
        (dict(world_matrices=Fake((11, 16))), "outside"),                                            # dense range
        (dict(world_matrices=good, first=8), "outside"),
        (dict(world_matrices=good, first=1, indices=gi), "first"),
        (dict(world_matrices=good, indices=Fake((3,), dtype=torch.int32, index=1)), "cuda:1"),
        (dict(world_matrices=good, indices=Fake((3,), dtype=torch.int64)), "int64"),
        (dict(world_matrices=good, indices=Fake((3,))), "float32"),
        (dict(world_matrices=good, indices=Fake((3,), dtype=torch.int32, contiguous=False)), "contiguous"),
        (dict(world_matrices=good, indices=Fake((4,), dtype=torch.int32)), "shape"),
        (dict(world_matrices=good, indices=Fake((3, 1), dtype=torch.int32)), "shape"),
        (dict(world_matrices=good, indices=Fake((3,), dtype=torch.int32, ptr=0x1002)), "4-byte aligned"),
    ]
    for kw, word in bad:
        with pytest.raises(VkrtError, match=word):
            r.update_nodes(**{"first": 0, **kw})
    for kw in (dict(first=7, world_matrices=good), dict(first=0, world_matrices=good, indices=gi),
               dict(first=0, world_matrices=Fake((30, 16)), indices=Fake((30,), dtype=torch.int32, ptr=0x1004))):  # (a sparse update may be longer than the scene)
        with pytest.raises(AssertionError, match="vkrt_scene_update_node_transforms"):
            r.update_nodes(**kw)


def test_node_update_kernels_use_no_scratch_and_spill_nothing():
    """the compiler's resource report (tools/kernel_resources.py) for gfx950 equals the committed copy of it"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    names = ("k_nu_transforms", "k_nu_visibility")
    kernels, problems = kernel_resources.measure("node_update.hip", names)
    assert not problems, problems
    assert set(kernels) == set(names)
    for k, v in kernels.items():
        assert v["scratch_bytes"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["static_lds_bytes"] == 0, (k, v)
    doc = json.load(open(os.path.join(ROOT, "profiles", "node_update_kernel_resources.json")))
    assert doc["conditions_met"] and not doc["problems"]
    assert doc["kernels"] == kernels  # the committed report is the one of this tree
