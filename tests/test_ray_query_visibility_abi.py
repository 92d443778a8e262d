"""CPU-side checks of instance visibility and query options (vkrt_scene_set/get_instance_visibility, vkrt_intersect_ex,
vkrt_occluded_ex, vkrt_debug_read_node_masks): declared, exported, laid out like the ctypes records, refused without a device in the
order the header states, and the Python layer's refusals before the call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import vkrt_amd
from vkrt_amd import abi

ROOT = vkrt_amd.REPO_ROOT
NEW = ("vkrt_scene_set_instance_visibility", "vkrt_scene_get_instance_visibility", "vkrt_intersect_ex", "vkrt_occluded_ex",
       "vkrt_debug_read_node_masks")


def _lib():
    assert os.path.exists(vkrt_amd.LIB_PATH), "run __graft_entry__.build() first"
    return abi.declare_vkrt(C.CDLL(vkrt_amd.LIB_PATH))


def test_visibility_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    declared = set(re.findall(r"\b(vkrt_[a-z_]+)\s*\(", header))
    lib = C.CDLL(vkrt_amd.LIB_PATH)
    for name in NEW:
        assert name in declared and name in abi.VKRT_SYMBOLS, name
        assert hasattr(lib, name), name
    assert _lib().vkrt_abi_version() == 4 == abi.VKRT_ABI_VERSION
    # the flag values are traceRayEXT's (gl_RayFlagsOpaqueEXT, gl_RayFlagsCullBackFacingTrianglesEXT, ...FrontFacing...)
    assert (abi.VKRT_RAY_OPAQUE, abi.VKRT_RAY_CULL_BACK_FACING, abi.VKRT_RAY_CULL_FRONT_FACING) == (0x1, 0x10, 0x20)
    assert (abi.VKRT_INSTANCE_FACING_CULL_DISABLE, abi.VKRT_INSTANCE_FLIP_FACING) == (0x1, 0x2)


def test_visibility_and_opts_layout_match_the_header(tmp_path):
    """sizeof / offsetof of vkrt_instance_visibility and vkrt_query_opts, compiled as C and as C++, equal the ctypes records; the
    enum values equal abi.py's."""
    fields = {"vkrt_instance_visibility": abi.InstanceVisibility, "vkrt_query_opts": abi.QueryOpts}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vkrt.h"', "int main(void){"]
    expect = []
    for cname, py in fields.items():
        lines.append(f'  printf("%zu\\n", sizeof({cname}));')
        expect.append(C.sizeof(py))
        for fname, _ in py._fields_:
            lines.append(f'  printf("%zu\\n", offsetof({cname}, {fname}));')
            expect.append(getattr(py, fname).offset)
    for name in ("VKRT_INSTANCE_FACING_CULL_DISABLE", "VKRT_INSTANCE_FLIP_FACING", "VKRT_RAY_OPAQUE", "VKRT_RAY_CULL_BACK_FACING",
                 "VKRT_RAY_CULL_FRONT_FACING"):
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
    assert C.sizeof(abi.InstanceVisibility) == 4 and C.sizeof(abi.QueryOpts) == 16


def _opts(flags=0, cull=0xFF, size=None):
    return abi.QueryOpts(C.sizeof(abi.QueryOpts) if size is None else size, flags, cull, 0)


def test_query_opts_are_refused_before_any_device_check():
    """Bad options are refused first (the message names them), whatever the scene and arrays: no device needed to see it."""
    lib = _lib()
    rays = (abi.Ray * 2)()
    hits = (abi.Hit * 2)()
    occ = (C.c_int32 * 2)()
    bad = [(_opts(size=12), b"struct_size"), (_opts(flags=0x2), b"ray_flags"), (_opts(flags=0x4), b"ray_flags"),
           (_opts(flags=0x40), b"ray_flags"), (_opts(flags=0x80000000), b"ray_flags"), (_opts(flags=0x30), b"together"),
           (_opts(cull=0x100), b"cull_mask"), (_opts(cull=0xFFFFFFFF), b"cull_mask")]
    for fn, out in ((lib.vkrt_intersect_ex, C.addressof(hits)), (lib.vkrt_occluded_ex, C.addressof(occ))):
        assert fn(None, C.addressof(rays), 2, None, out, None) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert b"opts is NULL" in lib.vkrt_last_error()
        for o, word in bad:
            for n in (0, 2):
                assert fn(None, C.addressof(rays), n, C.byref(o), out, None) == abi.VKRT_ERR_INVALID_ARGUMENT
                assert word in lib.vkrt_last_error(), (o.ray_flags, o.cull_mask, lib.vkrt_last_error())
        # good options reach the checks of vkrt_intersect: the NULL scene
        for good in (_opts(), _opts(flags=0x31 & ~0x20), _opts(flags=0x21), _opts(cull=0), _opts(size=64)):
            assert fn(None, C.addressof(rays), 2, C.byref(good), out, None) == abi.VKRT_ERR_INVALID_ARGUMENT
            assert b"scene is NULL" in lib.vkrt_last_error()


def test_visibility_values_are_refused_before_any_device_check():
    lib = _lib()
    V = abi.InstanceVisibility
    assert lib.vkrt_scene_set_instance_visibility(None, 0, 1, None, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"vis is NULL" in lib.vkrt_last_error()
    for entry, word in ((V(0, 1, 0), b"mask 0"), (V(1, 4, 0), b"flag"), (V(1, 0x80, 0), b"flag"), (V(7, 0, 1), b"reserved")):
        arr = (V * 3)(V(0xFF, 1, 0), entry, V(1, 3, 0))
        assert lib.vkrt_scene_set_instance_visibility(None, 0, 3, arr, None) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert word in lib.vkrt_last_error(), lib.vkrt_last_error()
    good = (V * 2)(V(1, 0, 0), V(0xFF, 3, 0))
    assert lib.vkrt_scene_set_instance_visibility(None, 0, 2, good, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"scene is NULL" in lib.vkrt_last_error()
    out = (V * 2)()
    assert lib.vkrt_scene_get_instance_visibility(None, 0, 2, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"out is NULL" in lib.vkrt_last_error()
    assert lib.vkrt_scene_get_instance_visibility(None, 0, 2, out) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"scene is NULL" in lib.vkrt_last_error()
    buf = (C.c_uint8 * 16)()
    assert lib.vkrt_debug_read_node_masks(None, buf, 16) == abi.VKRT_ERR_INVALID_ARGUMENT


def _renderer_without_scene(nodes=5):
    from vkrt_amd.renderer import Renderer

    r = Renderer.__new__(Renderer)  # no scene: the checks run before any use of the handle
    r.device = 0
    r._prim_mesh = np.zeros(nodes, np.int32)
    return r


def test_python_refuses_bad_masks_flags_and_ranges_before_the_call():
    from vkrt_amd.renderer import VkrtError

    r = _renderer_without_scene(5)
    bad = [dict(first=0, masks=[0]), dict(first=0, masks=[256]), dict(first=0, masks=[-1]), dict(first=0, masks=[1.5]),
           dict(first=4, masks=[1, 2]), dict(first=-1, masks=[1]), dict(first=0, masks=[1, 2], flags=[1]),
           dict(first=0, masks=[1], flags=[4]), dict(first=0, masks=[1], flags=[-1]), dict(first=0, masks=[1], flags=[0.5])]
    for kw in bad:
        with pytest.raises(VkrtError):
            r.set_instance_visibility(**kw)


def test_python_refuses_bad_query_options_before_the_call():
    import torch
    from vkrt_amd.renderer import Renderer, VkrtError

    for cull, flags in ((256, 0), (-1, 0), (1.0, 0), (True, 0), (0xFF, 0x30), (0xFF, 0x2), (0xFF, 0x100), (0xFF, -1), (0xFF, None)):
        with pytest.raises(VkrtError):
            Renderer._query_opts(cull, flags, 0, "intersect")
    assert Renderer._query_opts(0xFF, 0, 5, "intersect") is None  # the defaults are the call of vkrt_intersect itself
    o = Renderer._query_opts(3, abi.VKRT_RAY_OPAQUE | abi.VKRT_RAY_CULL_FRONT_FACING, -1, "occluded")
    assert (o.struct_size, o.ray_flags, o.cull_mask, o.anyhit_seed) == (16, 0x21, 3, 0xFFFFFFFF)
    assert Renderer._query_opts(0, 0, 0, "intersect").cull_mask == 0
    # a CPU tensor is still refused first, and bad options before the library is reached
    from vkrt_amd.renderer import pack_rays

    r = _renderer_without_scene()
    rays = pack_rays(torch.zeros(4, 3), torch.ones(4, 3))
    for fn in (r.intersect, r.occluded):
        with pytest.raises(VkrtError):
            fn(rays, cull_mask=3)
