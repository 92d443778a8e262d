"""CPU-side checks of vkrt_intersect_multi: declared, exported, listed; VKRT_MULTIHIT_MAX on both sides; refused without a device in
the order the header states (options, then max_hits, then the checks of vkrt_intersect); the Python layer's refusals before the call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import vkrt_amd
from vkrt_amd import abi

ROOT = vkrt_amd.REPO_ROOT


def _lib():
    assert os.path.exists(vkrt_amd.LIB_PATH), "run __graft_entry__.build() first"
    return abi.declare_vkrt(C.CDLL(vkrt_amd.LIB_PATH))


def test_multihit_symbol_is_declared_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    declared = set(re.findall(r"\b(vkrt_[a-z_]+)\s*\(", header))
    assert "vkrt_intersect_multi" in declared
    assert "vkrt_intersect_multi" in abi.VKRT_SYMBOLS
    assert hasattr(C.CDLL(vkrt_amd.LIB_PATH), "vkrt_intersect_multi")
    assert _lib().vkrt_abi_version() == 4 == abi.VKRT_ABI_VERSION
    assert re.search(r"#define\s+VKRT_ABI_VERSION\s+4\b", header)


def test_multihit_max_is_16_on_both_sides(tmp_path):
    assert abi.VKRT_MULTIHIT_MAX == 16
    src = tmp_path / "max.c"
    src.write_text('#include <stdio.h>\n#include "vkrt.h"\nint main(void){ printf("%d\\n", (int)VKRT_MULTIHIT_MAX); return 0; }\n')
    exe = tmp_path / "max"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert int(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout) == 16


def _opts(flags=0, cull=0xFF, size=None):
    return abi.QueryOpts(C.sizeof(abi.QueryOpts) if size is None else size, flags, cull, 0)


def test_refusal_order_without_a_device():
    """bad options first (n = 0 and n = 2), then max_hits, then the NULL scene -- whatever the other arguments are"""
    lib = _lib()
    rays = (abi.Ray * 2)()
    hits = (abi.Hit * 32)()
    counts = (C.c_int32 * 2)()
    fn = lib.vkrt_intersect_multi
    E = abi.VKRT_ERR_INVALID_ARGUMENT
    assert fn(None, C.addressof(rays), 2, None, 4, C.addressof(hits), C.addressof(counts), None) == E
    assert b"opts is NULL" in lib.vkrt_last_error()
    bad = [(_opts(size=12), b"struct_size"), (_opts(flags=0x2), b"ray_flags"), (_opts(flags=0x40), b"ray_flags"), (_opts(flags=0x30), b"together"),
           (_opts(cull=0x100), b"cull_mask"), (_opts(cull=0xFFFFFFFF), b"cull_mask")]
    for o, word in bad:
        for n in (0, 2):
            for k in (4, 0, 17):  # (a bad max_hits does not come first)
                assert fn(None, C.addressof(rays), n, C.byref(o), k, C.addressof(hits), C.addressof(counts), None) == E
                assert word in lib.vkrt_last_error(), (o.ray_flags, o.cull_mask, n, k, lib.vkrt_last_error())
    good = (_opts(), _opts(flags=0x11), _opts(flags=0x21), _opts(cull=0), _opts(size=64))
    for o in good:
        for k in (0, 17, 2 ** 32 - 1):
            for n in (0, 2):
                assert fn(None, C.addressof(rays), n, C.byref(o), k, C.addressof(hits), C.addressof(counts), None) == E
                assert b"max_hits" in lib.vkrt_last_error(), lib.vkrt_last_error()
        for k in (1, 4, 16):
            for cnt in (C.addressof(counts), None):
                assert fn(None, C.addressof(rays), 2, C.byref(o), k, C.addressof(hits), cnt, None) == E
                assert b"scene is NULL" in lib.vkrt_last_error(), lib.vkrt_last_error()
            assert fn(None, None, 0, C.byref(o), k, None, None, None) == E  # (the NULL scene comes before n == 0)
            assert b"scene is NULL" in lib.vkrt_last_error()


def _renderer_without_scene():
    from vkrt_amd.renderer import Renderer

    r = Renderer.__new__(Renderer)  # no scene: the checks run before any use of the handle
    r.device = 0
    r._prim_mesh = np.zeros(5, np.int32)
    return r


def test_python_refuses_bad_arguments_before_the_call():
    import torch
    from vkrt_amd.renderer import MultiHits, RayHits, VkrtError, pack_rays

    r = _renderer_without_scene()
    rays = pack_rays(torch.zeros(4, 3), torch.ones(4, 3))
    with pytest.raises(VkrtError):
        r.intersect_multi(rays, 4)  # a CPU tensor
    with pytest.raises(VkrtError):
        r.intersect_multi(np.zeros((4, 8), np.float32), 4)
    # the views of a result, on the CPU: shapes, aliasing, flat()
    buf = torch.arange(3 * 5 * 8, dtype=torch.int32).view(3, 5, 8)
    h = MultiHits(buf.view(torch.float32), torch.zeros(3, dtype=torch.int32))
    for name in ("t", "u", "v", "instance", "primitive", "prim_mesh", "triangle", "material"):
        assert tuple(getattr(h, name).shape) == (3, 5), name
    assert h.t.dtype == torch.float32 and h.triangle.dtype == torch.int32 and h.count.dtype == torch.int32
    assert h.triangle[2, 3].item() == (2 * 5 + 3) * 8 + 6 and h.instance[1, 0].item() == 5 * 8 + 3
    f = h.flat()
    assert isinstance(f, RayHits) and tuple(f.buffer.shape) == (15, 8) and f.buffer.data_ptr() == buf.data_ptr()
    assert f.triangle[2 * 5 + 3].item() == h.triangle[2, 3].item()


@pytest.mark.parametrize("k", [0, 17, -1, 1.0, True, None, "4", 2 ** 32])
def test_python_refuses_bad_max_hits(k, monkeypatch):
    from vkrt_amd.renderer import VkrtError

    r = _renderer_without_scene()
    monkeypatch.setattr(r, "_query_args", lambda rays, what: 4, raising=False)  # (rays accepted: max_hits is what is judged)
    with pytest.raises(VkrtError, match="max_hits"):
        r.intersect_multi(None, k)
    for cull, flags in ((256, 0), (0xFF, 0x30), (0xFF, 0x2)):
        with pytest.raises(VkrtError):
            r.intersect_multi(None, 4, cull_mask=cull, ray_flags=flags)
