"""CPU-side checks of vkrt_debug_split_references: declared, exported, its ctypes declaration, and its refusals before any device is
looked for.  (What it shows of a scene, capacities against a live scene and the installed tree left alone: tests/test_gpu_split_refs.py.)"""
import ctypes as C
import os
import re

import vkrt_amd
from vkrt_amd import abi

ROOT = vkrt_amd.REPO_ROOT
NEW = ("vkrt_debug_split_references",)


def _lib():
    assert os.path.exists(vkrt_amd.LIB_PATH), "run __graft_entry__.build() first"
    return abi.declare_vkrt(C.CDLL(vkrt_amd.LIB_PATH))


def test_split_references_symbol_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    declared = set(re.findall(r"\b(vkrt_[a-z_]+)\s*\(", header))
    lib = _lib()
    for name in NEW:
        assert name in declared and name in abi.VKRT_SYMBOLS, name
        assert hasattr(lib, name), name
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"int vkrt_debug_split_references\(vkrt_scene\* scene, uint32_t split_percent\s*,\s*float\* prio\s*, float\* scale\s*,\s*"
                     r"uint32_t\* ref_tri, float\* ref_box\s*, uint64_t capacity,\s*uint32_t\* ref_count\);", flat)
    fn = lib.vkrt_debug_split_references
    p = C.sizeof(C.c_void_p)
    assert fn.restype is C.c_int and [C.sizeof(t) for t in fn.argtypes] == [p, 4, p, p, p, p, 8, p]
    assert lib.vkrt_abi_version() == 4 == abi.VKRT_ABI_VERSION  # a test hook: no struct changed


def test_split_references_refuses_bad_arguments_before_any_device_check():
    lib = _lib()
    tri = (C.c_uint32 * 4)(7, 7, 7, 7)
    box = (C.c_float * 24)(*([7.0] * 24))
    n = C.c_uint32(7)
    scene = C.create_string_buffer(4096)  # stands for a scene: a percent outside 1..100 is refused before the scene is looked at
    fn = lib.vkrt_debug_split_references
    for args in ((None, 30, None, None, tri, box, 4, C.byref(n)), (scene, 30, None, None, None, box, 4, C.byref(n)),
                 (scene, 30, None, None, tri, None, 4, C.byref(n)), (scene, 30, None, None, tri, box, 4, None)):
        assert fn(*args) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert b"NULL" in lib.vkrt_last_error()
    for percent in (0, 101, 0xFFFFFFFF):
        assert fn(scene, percent, None, None, tri, box, 4, C.byref(n)) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert b"vkrt_debug_split_references" in lib.vkrt_last_error() and b"1..100" in lib.vkrt_last_error()
    assert list(tri) == [7, 7, 7, 7] and list(box) == [7.0] * 24 and n.value == 7


def test_renderer_sizes_its_buffers_from_the_budget():
    """Renderer.split_references: room for T + T * percent / 100 references, arrays cut to the count that came back, the status passed
    on."""
    import numpy as np
    import pytest
    from vkrt_amd.renderer import Renderer, VkrtError

    class Lib:
        def vkrt_debug_split_references(self, h, percent, prio, scale, tri, box, capacity, count):
            self.seen = (h, percent, capacity)
            R = 12
            (C.c_float * 10).from_address(prio)[:] = [0.5] * 10
            (C.c_float * 1).from_address(scale)[0] = 3.0
            (C.c_uint32 * R).from_address(tri)[:] = range(R)
            (C.c_float * (6 * R)).from_address(box)[:] = [float(k) for k in range(6 * R)]
            count._obj.value = R
            return self.status

    r = Renderer.__new__(Renderer)
    r._h, r.lib, r._triangle_count = None, Lib(), 10
    r.lib.status = 0
    out = r.split_references(30)
    assert r.lib.seen == (None, 30, 13) and out["ref_count"] == 12
    assert out["prio"].dtype == np.float32 and out["prio"].tolist() == [0.5] * 10 and out["scale"] == np.float32(3.0)
    assert out["ref_tri"].dtype == np.uint32 and out["ref_tri"].tolist() == list(range(12))
    assert out["ref_box"].shape == (12, 6) and out["ref_box"][11].tolist() == [66.0, 67.0, 68.0, 69.0, 70.0, 71.0]
    r.lib.status = abi.VKRT_ERR_INVALID_ARGUMENT
    with pytest.raises(VkrtError):
        r.split_references(30)
