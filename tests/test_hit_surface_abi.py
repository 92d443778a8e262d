"""CPU-side checks of vkrt_hit_surface: declared, exported, laid out like the ctypes record, argument-checked in the documented order
without a device, and the Python layer's refusals."""
import ctypes as C
import os
import re
import subprocess

import pytest

import vkrt_amd
from vkrt_amd import abi

ROOT = vkrt_amd.REPO_ROOT
BOTH = abi.VKRT_SURFACE_GEOMETRY | abi.VKRT_SURFACE_MATERIAL


def _lib():
    assert os.path.exists(vkrt_amd.LIB_PATH), "run __graft_entry__.build() first"
    return abi.declare_vkrt(C.CDLL(vkrt_amd.LIB_PATH))


def test_surface_symbol_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    declared = set(re.findall(r"\b(vkrt_[a-z_]+)\s*\(", header))
    assert "vkrt_hit_surface" in declared and "vkrt_hit_surface" in abi.VKRT_SYMBOLS
    assert hasattr(C.CDLL(vkrt_amd.LIB_PATH), "vkrt_hit_surface")
    assert re.search(r"VKRT_SURFACE_GEOMETRY\s*=\s*0x1\b", header) and re.search(r"VKRT_SURFACE_MATERIAL\s*=\s*0x2\b", header)
    assert (abi.VKRT_SURFACE_GEOMETRY, abi.VKRT_SURFACE_MATERIAL) == (1, 2)
    # additive: the ABI version stays 4 and no existing struct changed
    assert _lib().vkrt_abi_version() == 4 == abi.VKRT_ABI_VERSION
    assert C.sizeof(abi.Node) == 68 and C.sizeof(abi.AccelInfo) == 48 and C.sizeof(abi.Ray) == 32 and C.sizeof(abi.Hit) == 32


def test_surface_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of vkrt_surface (and of the records beside it), compiled as C and as C++, equal the ctypes records."""
    fields = {"vkrt_surface": abi.Surface, "vkrt_hit": abi.Hit, "vkrt_ray": abi.Ray}
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
    assert C.sizeof(abi.Surface) == 128
    # eight float4: every vec3 starts a quad, its fourth word is the scalar the header puts there
    quads = ["position", "geometric_normal", "normal", "shading_normal", "tangent", "binormal", "base_color", "emission"]
    scalars = ["texcoord_u", "texcoord_v", "alpha", "metallic", "roughness", "material", "valid", "reserved"]
    for k, (q, s) in enumerate(zip(quads, scalars)):
        assert getattr(abi.Surface, q).offset == 16 * k and getattr(abi.Surface, s).offset == 16 * k + 12


def test_header_with_surface_compiles_as_c_and_cxx(tmp_path):
    body = ("#include \"vkrt.h\"\n"
            "int main(void){ int (*f)(vkrt_scene*, const vkrt_hit*, uint32_t, uint32_t, vkrt_surface*, void*) = vkrt_hit_surface;\n"
            " vkrt_surface s; s.reserved = 0u; s.valid = 0; s.material = -1; s.position[2] = 0.0f;\n"
            " return (f != 0 && (VKRT_SURFACE_GEOMETRY | VKRT_SURFACE_MATERIAL) == 3 && s.reserved == 0u && s.valid == 0 && s.material < 0"
            " && s.position[2] == 0.0f) ? 0 : 1; }\n")
    for ext, cc in (("c", "gcc"), ("cpp", "g++")):
        src = tmp_path / f"t.{ext}"
        src.write_text(body)
        subprocess.run([cc, "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / f"t_{cc}.o")], check=True)


def test_refusals_in_the_documented_order_without_a_device():
    """A NULL scene first; then, for n > 0, NULL and misaligned pointers; then `fields`; then n == 0 is VKRT_OK.  The header promises
    that all of these come before anything of the scene is read, so a handle that is only a non-NULL address is enough to see the
    order (nothing here reaches a device)."""
    lib = _lib()
    hits = (abi.Hit * 4)()
    out = (abi.Surface * 4)()
    ph, po = C.addressof(hits), C.addressof(out)
    assert ph % 16 == 0 or (ph + 8) % 16 == 0  # ctypes arrays are at least 8-byte aligned
    ph += ph % 16
    po += po % 16
    assert ph % 16 == 0 and po % 16 == 0
    bad = abi.VKRT_ERR_INVALID_ARGUMENT
    f = lib.vkrt_hit_surface
    # 1. a NULL scene, whatever else is wrong or right, n == 0 included
    for args in ((ph, 2, BOTH, po), (None, 0, BOTH, None), (None, 2, 0, None), (ph + 4, 2, 7, po + 4)):
        assert f(None, args[0], args[1], args[2], args[3], None) == bad
        assert b"scene is NULL" in lib.vkrt_last_error()
    handle = C.addressof(C.create_string_buffer(64))  # never dereferenced by the checks below
    # 2. n > 0: NULL pointers, before alignment and before fields
    for h, o in ((None, po), (ph, None), (None, None)):
        assert f(handle, h, 2, 99, o, None) == bad
        assert b"NULL array" in lib.vkrt_last_error()
    # 3. n > 0: misaligned pointers, before fields
    for h, o in ((ph + 4, po), (ph, po + 8), (ph + 8, po + 4)):
        assert f(handle, h, 2, 99, o, None) == bad
        assert b"misaligned" in lib.vkrt_last_error()
    # 4. fields: only GEOMETRY and GEOMETRY | MATERIAL, for n > 0 and for n == 0
    for fields in (0, abi.VKRT_SURFACE_MATERIAL, 4, 5, 7, 0x80000001, 0xFFFFFFFF):
        assert f(handle, ph, 2, fields, po, None) == bad
        assert b"fields" in lib.vkrt_last_error()
        assert f(handle, None, 0, fields, None, None) == bad
    # 5. n == 0 with good fields: VKRT_OK, nothing enqueued, pointers not looked at
    for fields in (abi.VKRT_SURFACE_GEOMETRY, BOTH):
        assert f(handle, None, 0, fields, None, None) == abi.VKRT_OK
        assert f(handle, ph + 4, 0, fields, po + 4, None) == abi.VKRT_OK


def test_surfaces_views_on_a_cpu_buffer():
    """Surfaces is a set of views of one [N, 32] buffer laid out like vkrt_surface."""
    import numpy as np
    import torch
    from vkrt_amd.renderer import Surfaces

    n = 5
    rec = (abi.Surface * n)()
    for k in range(n):
        r = rec[k]
        for j, name in enumerate(("position", "geometric_normal", "normal", "shading_normal", "tangent", "binormal", "base_color", "emission")):
            getattr(r, name)[:] = [100 * k + 10 * j + c for c in range(3)]
        r.texcoord_u, r.texcoord_v, r.alpha, r.metallic, r.roughness = 0.5 + k, 0.25 + k, 0.125 + k, 0.75 + k, 0.375 + k
        r.material, r.valid, r.reserved = k - 1, k & 1, 0
    buf = torch.from_numpy(np.frombuffer(bytes(rec), np.float32).reshape(n, 32).copy())
    s = Surfaces(buf)
    for j, name in enumerate(("position", "geometric_normal", "normal", "shading_normal", "tangent", "binormal", "base_color", "emission")):
        v = getattr(s, name)
        assert tuple(v.shape) == (n, 3)
        assert v.tolist() == [[100.0 * k + 10 * j + c for c in range(3)] for k in range(n)]
    assert s.texcoord.tolist() == [[0.5 + k, 0.25 + k] for k in range(n)] and tuple(s.texcoord.shape) == (n, 2)
    assert s.texcoord_u.tolist() == [0.5 + k for k in range(n)] and s.texcoord_v.tolist() == [0.25 + k for k in range(n)]
    assert s.alpha.tolist() == [0.125 + k for k in range(n)] and s.metallic.tolist() == [0.75 + k for k in range(n)]
    assert s.roughness.tolist() == [0.375 + k for k in range(n)]
    assert s.material.dtype == torch.int32 and s.material.tolist() == [k - 1 for k in range(n)]
    assert s.valid.tolist() == [k & 1 for k in range(n)] and s.reserved.tolist() == [0] * n
    s.position[2, 1] = -7.0  # views, not copies
    assert buf[2, 1] == -7.0


def test_python_refuses_bad_hit_tensors_before_the_call():
    """Renderer.surface checks the tensor before anything reaches the library (no scene handle is needed to refuse)."""
    import torch
    from vkrt_amd.renderer import Renderer, VkrtError

    r = Renderer.__new__(Renderer)  # no scene: the checks run before any use of the handle
    r.device = 0
    good = torch.zeros(4, 8)
    bad = [good,                       # a CPU tensor
           good.to(torch.int32),       # a CPU tensor of the other accepted dtype
           good.double(),              # wrong dtype
           good[:, :7],                # wrong shape
           good.reshape(-1),
           good.t(),                   # not contiguous
           good.numpy(),               # not a tensor
           None]
    for hits in bad:
        for material in (True, False):
            with pytest.raises(VkrtError):
                r.surface(hits, material=material)
