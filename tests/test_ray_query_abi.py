"""CPU-side checks of the ray-query entry points (vkrt_intersect, vkrt_occluded): declared, exported, laid out like the ctypes
records, argument-checked without a device, and the Python layer's packing and refusals."""
import ctypes as C
import os
import re
import subprocess

import pytest

import vkrt_amd
from vkrt_amd import abi

ROOT = vkrt_amd.REPO_ROOT
NEW = ("vkrt_intersect", "vkrt_occluded")


def _lib():
    assert os.path.exists(vkrt_amd.LIB_PATH), "run __graft_entry__.build() first"
    return abi.declare_vkrt(C.CDLL(vkrt_amd.LIB_PATH))


def test_query_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    declared = set(re.findall(r"\b(vkrt_[a-z_]+)\s*\(", header))
    lib = C.CDLL(vkrt_amd.LIB_PATH)
    for name in NEW:
        assert name in declared and name in abi.VKRT_SYMBOLS
        assert hasattr(lib, name), name
    # additive: the ABI version stays 4 and no existing struct changed
    assert _lib().vkrt_abi_version() == 4 == abi.VKRT_ABI_VERSION
    assert C.sizeof(abi.Node) == 68 and C.sizeof(abi.AccelInfo) == 48


def test_ray_and_hit_layout_match_the_header(tmp_path):
    """sizeof / offsetof of vkrt_ray and vkrt_hit, compiled as C and as C++, equal the ctypes records."""
    fields = {"vkrt_ray": abi.Ray, "vkrt_hit": abi.Hit}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vkrt.h"', "int main(void){"]
    expect = []
    for cname, py in fields.items():
        lines.append(f'  printf("%zu\\n", sizeof({cname}));')
        expect.append(C.sizeof(py))
        for fname, _ in py._fields_:
            lines.append(f'  printf("%zu\\n", offsetof({cname}, {fname}));')
            expect.append(getattr(py, fname).offset)
    lines.append("  return 0; }")
    for ext, cc in (("c", "gcc"), ("cpp", "g++")):
        src = tmp_path / f"layout.{ext}"
        src.write_text("\n".join(lines) + "\n")
        exe = tmp_path / f"layout_{cc}"
        subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
        assert [int(x) for x in out] == expect
    assert C.sizeof(abi.Ray) == 32 and C.sizeof(abi.Hit) == 32


def test_header_with_queries_compiles_as_c_and_cxx(tmp_path):
    body = ("#include \"vkrt.h\"\n"
            "int main(void){ int (*i)(vkrt_scene*, const vkrt_ray*, uint32_t, uint32_t, vkrt_hit*, void*) = vkrt_intersect;\n"
            " int (*o)(vkrt_scene*, const vkrt_ray*, uint32_t, uint32_t, int32_t*, void*) = vkrt_occluded; return (i != 0 && o != 0) ? 0 : 1; }\n")
    for ext, cc in (("c", "gcc"), ("cpp", "g++")):
        src = tmp_path / f"t.{ext}"
        src.write_text(body)
        subprocess.run([cc, "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / f"t_{cc}.o")], check=True)


def test_null_arguments_are_refused_before_any_device_check():
    lib = _lib()
    rays = (abi.Ray * 2)()
    hits = (abi.Hit * 2)()
    occ = (C.c_int32 * 2)()
    for fn, out in ((lib.vkrt_intersect, C.addressof(hits)), (lib.vkrt_occluded, C.addressof(occ))):
        assert fn(None, C.addressof(rays), 2, 0, out, None) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert b"NULL" in lib.vkrt_last_error()
        assert fn(None, None, 0, 0, None, None) == abi.VKRT_ERR_INVALID_ARGUMENT  # a NULL scene even with n == 0
        assert fn(None, None, 2, 0, None, None) == abi.VKRT_ERR_INVALID_ARGUMENT


def test_pack_rays_layout_on_cpu_tensors():
    import torch
    from vkrt_amd.renderer import pack_rays

    o = torch.arange(15, dtype=torch.float64).reshape(5, 3)
    d = -torch.arange(15, dtype=torch.float32).reshape(5, 3) - 1
    r = pack_rays(o, d)
    assert r.dtype == torch.float32 and r.is_contiguous() and tuple(r.shape) == (5, 8) and r.device == o.device
    assert torch.equal(r[:, 0:3], o.float()) and torch.equal(r[:, 4:7], d)
    assert torch.all(r[:, 3] == torch.tensor(0.001, dtype=torch.float32)) and torch.all(r[:, 7] == 1e4)
    tmin = torch.linspace(0, 1, 5)
    tmax = torch.tensor([1.0, 2.0, float("inf"), 4.0, 5.0])
    r = pack_rays(o, d, tmin=tmin, tmax=tmax)
    assert torch.equal(r[:, 3], tmin) and torch.equal(r[:, 7], tmax)
    # the packed rows are vkrt_ray records
    rec = abi.Ray.from_buffer_copy(r[2].numpy().tobytes())
    assert list(rec.origin) == [6.0, 7.0, 8.0] and rec.tmin == pytest.approx(0.5) and list(rec.direction) == [-7.0, -8.0, -9.0]
    assert rec.tmax == float("inf")
    with pytest.raises(Exception):
        pack_rays(o, d[:4])
    with pytest.raises(Exception):
        pack_rays(o, d, tmin=torch.zeros(3))


def test_python_refuses_bad_ray_tensors_before_the_call():
    """intersect / occluded check the tensor before anything reaches the library (no scene handle is needed to refuse)."""
    import torch
    from vkrt_amd.renderer import Renderer, VkrtError, pack_rays

    r = Renderer.__new__(Renderer)  # no scene: the checks run before any use of the handle
    r.device = 0
    good = pack_rays(torch.zeros(4, 3), torch.ones(4, 3))
    bad = [good,                                     # a CPU tensor
           good.double(),                            # wrong dtype
           good[:, :7],                              # wrong shape
           good.reshape(-1),
           good.t(),                                 # not contiguous
           good.numpy()]                             # not a tensor
    for rays in bad:
        for fn in (r.intersect, r.occluded):
            with pytest.raises(VkrtError):
                fn(rays)
