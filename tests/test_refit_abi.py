"""CPU-side checks of the instance-update / refit entry points (vkrt_scene_update_nodes, vkrt_accel_refit): declared, exported,
argument-checked, and without a device nothing computes."""
import ctypes as C
import os
import re
import subprocess

import vkrt_amd
from vkrt_amd import abi

ROOT = vkrt_amd.REPO_ROOT
NEW = ("vkrt_scene_update_nodes", "vkrt_accel_refit")


def _lib():
    assert os.path.exists(vkrt_amd.LIB_PATH), "run __graft_entry__.build() first"
    return abi.declare_vkrt(C.CDLL(vkrt_amd.LIB_PATH))


def test_refit_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    declared = set(re.findall(r"\b(vkrt_[a-z_]+)\s*\(", header))
    lib = C.CDLL(vkrt_amd.LIB_PATH)
    for name in NEW:
        assert name in declared and name in abi.VKRT_SYMBOLS
        assert hasattr(lib, name), name
    # additive: the ABI version stays 4 and no struct grew
    assert _lib().vkrt_abi_version() == 4 == abi.VKRT_ABI_VERSION
    assert C.sizeof(abi.Node) == 68 and C.sizeof(abi.AccelInfo) == 48


def test_refit_null_arguments_are_refused():
    lib = _lib()
    node = abi.Node()
    assert lib.vkrt_scene_update_nodes(None, 0, 1, C.byref(node), None) == 1  # VKRT_ERR_INVALID_ARGUMENT
    assert b"NULL" in lib.vkrt_last_error()
    assert lib.vkrt_scene_update_nodes(None, 0, 0, None, None) == 1
    assert lib.vkrt_accel_refit(None, None) == 1
    assert b"NULL" in lib.vkrt_last_error()


def test_without_a_device_no_scene_exists_to_refit():
    """Without a HIP device vkrt_scene_create refuses (no CPU path), so there is nothing an update or a refit could compute on."""
    lib = _lib()
    if lib.vkrt_device_count() > 0:
        return  # (a GPU machine: the GPU suite covers the computing side)
    d = abi.SceneDesc()
    d.struct_size = C.sizeof(abi.SceneDesc)
    h = C.c_void_p()
    assert lib.vkrt_scene_create(C.byref(d), 0, C.byref(h)) != 0 and not h.value


def test_header_with_refit_compiles_as_c_and_cxx(tmp_path):
    body = ("#include \"vkrt.h\"\n"
            "int main(void){ int (*u)(vkrt_scene*, uint32_t, uint32_t, const vkrt_node*, void*) = vkrt_scene_update_nodes;\n"
            " int (*r)(vkrt_scene*, void*) = vkrt_accel_refit; return (u != 0 && r != 0) ? 0 : 1; }\n")
    for ext, cc in (("c", "gcc"), ("cpp", "g++")):
        src = tmp_path / f"t.{ext}"
        src.write_text(body)
        obj = tmp_path / f"t_{cc}.o"
        subprocess.run([cc, "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(obj)], check=True)
