"""CPU-side checks of vkrt_debug_read_triangle_ids: declared, exported, its ctypes declaration, and its refusals before any device is
looked for.  (Byte counts against a built tree, the stale tree and both layouts: tests/test_gpu_bvh_topology.py.)"""
import ctypes as C
import os
import re

import vkrt_amd
from vkrt_amd import abi

ROOT = vkrt_amd.REPO_ROOT
NEW = ("vkrt_debug_read_triangle_ids",)


def _lib():
    assert os.path.exists(vkrt_amd.LIB_PATH), "run __graft_entry__.build() first"
    return abi.declare_vkrt(C.CDLL(vkrt_amd.LIB_PATH))


def test_triangle_ids_symbol_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    declared = set(re.findall(r"\b(vkrt_[a-z_]+)\s*\(", header))
    lib = _lib()
    for name in NEW:
        assert name in declared and name in abi.VKRT_SYMBOLS, name
        assert hasattr(lib, name), name
    assert re.search(r"int vkrt_debug_read_triangle_ids\(vkrt_scene\* scene, uint32_t\* out, uint64_t bytes\);", header)
    fn = lib.vkrt_debug_read_triangle_ids
    assert fn.restype is C.c_int and [C.sizeof(t) for t in fn.argtypes] == [C.sizeof(C.c_void_p), C.sizeof(C.c_void_p), 8]
    assert lib.vkrt_abi_version() == 4 == abi.VKRT_ABI_VERSION  # a test hook: no struct changed


def test_triangle_ids_refuses_null_arguments_before_any_device_check():
    lib = _lib()
    buf = (C.c_uint32 * 4)(7, 7, 7, 7)
    for scene, out, n in ((None, buf, 16), (None, None, 0), (None, buf, 0)):
        assert lib.vkrt_debug_read_triangle_ids(scene, out, n) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert b"NULL" in lib.vkrt_last_error()
    assert list(buf) == [7, 7, 7, 7]


def test_renderer_reads_one_id_per_slot():
    """Renderer.read_triangle_ids sizes its buffer from triangle_bytes (48 B per slot) and passes the status on."""
    import numpy as np
    import pytest
    from vkrt_amd.renderer import Renderer, VkrtError

    class Lib:
        def vkrt_debug_read_triangle_ids(self, h, out, nbytes):
            self.seen = (h, nbytes)
            (C.c_uint32 * (nbytes // 4)).from_address(out)[:] = range(nbytes // 4)
            return self.status

    r = Renderer.__new__(Renderer)
    r._h, r.lib = None, Lib()
    r.accel_info = lambda: {"triangle_bytes": 5 * 48}
    r.lib.status = 0
    assert np.array_equal(r.read_triangle_ids(), np.arange(5, dtype=np.uint32)) and r.lib.seen == (None, 20)
    r.accel_info = lambda: {"triangle_bytes": 0}
    assert r.read_triangle_ids().size == 0 and r.lib.seen == (None, 0)
    r.lib.status = abi.VKRT_ERR_NOT_BUILT
    with pytest.raises(VkrtError):
        r.read_triangle_ids()
