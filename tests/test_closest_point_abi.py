"""CPU-side checks of vkrt_closest_point: declared, exported, listed, ABI still 4; vkrt_point_query is 16 bytes on both sides; refused
without a device in the order the header states (options -- a ray flag among them -- then the checks of vkrt_intersect); the Python
layer's refusals before the call; the kernels of csrc/closest.hip use no scratch memory."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import vkrt_amd
from vkrt_amd import abi

ROOT = vkrt_amd.REPO_ROOT
CSRC = os.path.join(vkrt_amd.PKG_DIR, "csrc")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


def _lib():
    assert os.path.exists(vkrt_amd.LIB_PATH), "run __graft_entry__.build() first"
    return abi.declare_vkrt(C.CDLL(vkrt_amd.LIB_PATH))


def test_closest_point_symbols_are_declared_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    declared = set(re.findall(r"\b(vkrt_[a-z_]+)\s*\(", header))
    for sym in ("vkrt_closest_point", "vkrt_debug_closest_point_work"):
        assert sym in declared
        assert sym in abi.VKRT_SYMBOLS
        assert hasattr(C.CDLL(vkrt_amd.LIB_PATH), sym)
    assert _lib().vkrt_abi_version() == 4 == abi.VKRT_ABI_VERSION
    assert re.search(r"#define\s+VKRT_ABI_VERSION\s+4\b", header)


def test_point_query_is_16_bytes_on_both_sides(tmp_path):
    assert C.sizeof(abi.PointQuery) == 16
    assert abi.PointQuery.radius.offset == 12
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vkrt.h"\n'
                   'int main(void){ printf("%d %d\\n", (int)sizeof(vkrt_point_query), (int)offsetof(vkrt_point_query, radius)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["16", "12"]


def _opts(flags=0, cull=0xFF, size=None):
    return abi.QueryOpts(C.sizeof(abi.QueryOpts) if size is None else size, flags, cull, 0)


def test_refusal_order_without_a_device():
    """bad options first (n = 0 and n = 2, whatever the scene), then the NULL scene -- before n == 0 --, and with a scene the arrays"""
    lib = _lib()
    fn = lib.vkrt_closest_point
    E = abi.VKRT_ERR_INVALID_ARGUMENT
    store = (C.c_char * 256)()
    base = (C.addressof(store) + 15) & ~15  # a 16-byte aligned host address (never read: every call below is refused)
    q, h = base, base + 64
    bad = [(_opts(size=12), b"struct_size"), (_opts(flags=0x2), b"ray_flags"), (_opts(flags=0x40), b"ray_flags"), (_opts(flags=0x30), b"together"),
           (_opts(cull=0x100), b"cull_mask"), (_opts(cull=0xFFFFFFFF), b"cull_mask"),
           (_opts(flags=0x1), b"ray flag"), (_opts(flags=0x10), b"ray flag"), (_opts(flags=0x20), b"ray flag"), (_opts(flags=0x11), b"ray flag")]
    for o, word in bad:
        for n in (0, 2):
            for qq, hh in ((q, h), (None, None), (q + 4, h)):  # (bad arrays do not come first)
                assert fn(None, qq, n, C.byref(o), hh, None) == E
                assert word in lib.vkrt_last_error(), (o.ray_flags, o.cull_mask, n, lib.vkrt_last_error())
    good = (None, _opts(), _opts(cull=0), _opts(cull=0x5), _opts(size=64))
    for o in good:
        ref = None if o is None else C.byref(o)
        for n in (2, 0):  # (the NULL scene comes before n == 0, and before the arrays)
            for qq, hh in ((q, h), (None, None), (q + 4, h + 8)):
                assert fn(None, qq, n, ref, hh, None) == E
                assert b"scene is NULL" in lib.vkrt_last_error(), lib.vkrt_last_error()
    # the work hook refuses the same options first
    out = (C.c_uint64 * 2)()
    for o, word in bad:
        assert lib.vkrt_debug_closest_point_work(None, q, 2, C.byref(o), out) == E
        assert word in lib.vkrt_last_error()
    assert lib.vkrt_debug_closest_point_work(None, q, 2, None, out) == E


def _renderer_without_scene():
    from vkrt_amd.renderer import Renderer

    r = Renderer.__new__(Renderer)  # no scene: the checks run before any use of the handle
    r.device = 0
    r._prim_mesh = np.zeros(5, np.int32)
    return r


def test_python_refuses_bad_arguments_before_the_call():
    import torch
    from vkrt_amd.renderer import VkrtError

    r = _renderer_without_scene()
    with pytest.raises(VkrtError, match="scene is on"):
        r.closest_point(torch.zeros(4, 4))  # a CPU tensor
    with pytest.raises(VkrtError, match="scene is on"):
        r.closest_point(torch.zeros(4, 3), radius=1.0)
    with pytest.raises(VkrtError, match="torch tensor"):
        r.closest_point(np.zeros((4, 4), np.float32))
    with pytest.raises(VkrtError, match="torch tensor"):
        r.closest_point(None)
    for what in (np.zeros((4, 5), np.float32), np.zeros(4, np.float32), np.zeros((2, 2, 4), np.float32)):
        with pytest.raises(VkrtError, match="shape"):
            r.closest_point_work(what)


@pytest.mark.parametrize("cull", [256, -1, 1.0, True, None, "1"])
def test_python_refuses_bad_cull_masks(cull):
    from vkrt_amd.renderer import Renderer, VkrtError

    with pytest.raises(VkrtError, match="cull_mask"):
        Renderer._point_opts(cull, "closest_point")
    assert Renderer._point_opts(0xFF, "closest_point") is None  # (the NULL opts of the C call)
    o = Renderer._point_opts(0x5, "closest_point")
    assert (o.struct_size, o.ray_flags, o.cull_mask) == (16, 0, 5)


# ---- the kernels use no scratch memory: one field of the kernel descriptors' metadata -------------------------------------------
def _makefile_var(name):
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(rf"^{name}\s*[:?]?=\s*(.*)$", line)
        if m:
            return m.group(1).strip()
    raise KeyError(name)


def _hipcc_version():
    out = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout
    m = re.search(r"HIP version:\s*(\S+)", out)
    return m.group(1) if m else "unknown"


def test_makefile_builds_the_unit_with_flags_of_its_own():
    assert "closest.hip" in _makefile_var("SRCS").split()
    assert _makefile_var("FLAGS_closest")
    assert "-ffp-contract=off" in _makefile_var("FLAGS").split()  # the binary64 point/triangle function must not be contracted


def test_closest_point_kernels_use_no_scratch(tmp_path):
    if not HIPCC:
        pytest.skip("hipcc not found")
    want = json.load(open(os.path.join(ROOT, "profiles", "isa_mix.json"))).get("hipcc")
    if want and want != _hipcc_version():
        pytest.skip(f"hipcc {_hipcc_version()} is not the compiler of profiles/isa_mix.json ({want})")
    flags = _makefile_var("FLAGS").replace("$(ARCH)", _makefile_var("ARCH")).replace("-fPIC", "").split()
    flags += _makefile_var("FLAGS_closest").split()
    out = tmp_path / "closest.s"
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", "-o", str(out), "closest.hip"], cwd=CSRC, check=True, stderr=subprocess.DEVNULL)
    text = open(out).read()
    kernels = re.findall(r"\.amdhsa_kernel (\S*k_closest_point\S*)(.*?)\.end_amdhsa_kernel", text, flags=re.S)
    assert len(kernels) == 6, [k for k, _ in kernels]  # wide8 / BVH2 x unfiltered / filtered, and one instrumented per layout
    for name, meta in kernels:
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1))
        assert scratch == 0, (name, scratch)
