"""CPU-side checks of alpha-tested materials (vkrt_scene_set/get_material_alpha): declared, exported, laid out like the ctypes record,
refused without a device in the order the header states, the Python layer's refusals before the call, and the way the modes travel:
glTF alphaMode / alphaCutoff through the exporter and the C++ loader, and FlatScene.material_alpha through the npz."""
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
from vkrt_amd.flat_scene import ALPHA_DTYPE, FlatScene, LIGHT_DTYPE, MAT_DTYPE, NODE_DTYPE, PRIM_DTYPE

ROOT = vkrt_amd.REPO_ROOT
NEW = ("vkrt_scene_set_material_alpha", "vkrt_scene_get_material_alpha")


def _lib():
    assert os.path.exists(vkrt_amd.LIB_PATH), "run __graft_entry__.build() first"
    return abi.declare_vkrt(C.CDLL(vkrt_amd.LIB_PATH))


def test_material_alpha_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    declared = set(re.findall(r"\b(vkrt_[a-z_]+)\s*\(", header))
    lib = C.CDLL(vkrt_amd.LIB_PATH)
    for name in NEW:
        assert name in declared and name in abi.VKRT_SYMBOLS, name
        assert hasattr(lib, name), name
    assert _lib().vkrt_abi_version() == 4 == abi.VKRT_ABI_VERSION  # the entry points came after ABI 4 without changing it
    from vkrt_amd import renderer

    assert (renderer.ALPHA_OPAQUE, renderer.ALPHA_MASK) == (abi.VKRT_ALPHA_OPAQUE, abi.VKRT_ALPHA_MASK) == (0, 1)


def test_material_alpha_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of vkrt_material_alpha, compiled as C and as C++, equal the ctypes record and the numpy dtype; the enum values
    equal abi.py's."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vkrt.h"', "int main(void){",
             '  printf("%zu\\n", sizeof(vkrt_material_alpha));']
    expect = [C.sizeof(abi.MaterialAlpha)]
    for fname, _ in abi.MaterialAlpha._fields_:
        lines.append(f'  printf("%zu\\n", offsetof(vkrt_material_alpha, {fname}));')
        expect.append(getattr(abi.MaterialAlpha, fname).offset)
        assert ALPHA_DTYPE.fields[fname][1] == getattr(abi.MaterialAlpha, fname).offset
    for name in ("VKRT_ALPHA_OPAQUE", "VKRT_ALPHA_MASK"):
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
    assert C.sizeof(abi.MaterialAlpha) == 8 == ALPHA_DTYPE.itemsize


def test_material_alpha_values_are_refused_before_any_device_check():
    """The order of the header: a NULL array, then a bad entry (whatever the scene), then the NULL scene."""
    lib = _lib()
    A = abi.MaterialAlpha
    assert lib.vkrt_scene_set_material_alpha(None, 0, 1, None, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"alpha is NULL" in lib.vkrt_last_error()
    for entry, word in ((A(2, 0.5), b"mode"), (A(0xFFFFFFFF, 0.5), b"mode"), (A(1, float("nan")), b"cutoff"), (A(1, float("inf")), b"cutoff"),
                        (A(0, -0.25), b"cutoff"), (A(1, -float("inf")), b"cutoff")):
        arr = (A * 3)(A(1, 0.5), entry, A(0, 0.0))
        assert lib.vkrt_scene_set_material_alpha(None, 0, 3, arr, None) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert word in lib.vkrt_last_error() and b"entry 1" in lib.vkrt_last_error(), lib.vkrt_last_error()
    good = (A * 3)(A(1, 0.0), A(0, 0.5), A(1, 1.0e30))
    assert lib.vkrt_scene_set_material_alpha(None, 0, 3, good, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"scene is NULL" in lib.vkrt_last_error()
    assert lib.vkrt_scene_set_material_alpha(None, 0, 0, None, None) == abi.VKRT_ERR_INVALID_ARGUMENT  # count 0: the scene is still checked
    assert b"scene is NULL" in lib.vkrt_last_error()
    out = (A * 2)()
    assert lib.vkrt_scene_get_material_alpha(None, 0, 2, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"out is NULL" in lib.vkrt_last_error()
    assert lib.vkrt_scene_get_material_alpha(None, 0, 2, out) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"scene is NULL" in lib.vkrt_last_error()


def test_python_refuses_bad_modes_cutoffs_and_ranges_before_the_call():
    from vkrt_amd.renderer import Renderer, VkrtError

    r = Renderer.__new__(Renderer)  # no scene: the checks run before any use of the handle
    r.device = 0
    r._material_count = 4
    bad = [dict(first=0, modes=[2]), dict(first=0, modes=[-1]), dict(first=0, modes=[1.0]), dict(first=0, modes=[True]),
           dict(first=3, modes=[1, 1]), dict(first=-1, modes=[1]), dict(first=1.0, modes=[1]), dict(first=0, modes=[1, 0], cutoffs=[0.5, 0.5, 0.5]),
           dict(first=0, modes=[1], cutoffs=-0.1), dict(first=0, modes=[1], cutoffs=float("nan")), dict(first=0, modes=[1], cutoffs=float("inf")),
           dict(first=0, modes=[1], cutoffs="0.5"), dict(first=0, modes=[1, 1], cutoffs=[0.5, -1.0])]
    for kw in bad:
        with pytest.raises(VkrtError):
            r.set_material_alpha(**kw)


def _three_material_scene():
    """One quad per material: material 0 MASK with cutoff 0.3 over a texture, 1 and 2 plain."""
    quad = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    pos = np.concatenate([quad + np.float32([0, 0, k]) for k in range(3)])
    nrm = np.tile(np.float32([0, 0, 1]), (12, 1))
    tan = np.tile(np.float32([1, 0, 0, 1]), (12, 1))
    uv = np.tile(quad[:, :2], (3, 1))
    idx = np.tile(np.uint32([0, 1, 2, 0, 2, 3]), 3)
    pm = np.zeros(3, PRIM_DTYPE)
    nodes = np.zeros(3, NODE_DTYPE)
    mats = np.zeros(3, MAT_DTYPE)
    for k in range(3):
        pm[k] = (6 * k, 6, 4 * k, 4, k)
        nodes[k] = (np.eye(4, dtype=np.float32).reshape(-1), k)
        mats[k]["pbrBaseColorFactor"] = (1, 1, 1, 0.75)
        mats[k]["metallicFactor"] = mats[k]["roughnessFactor"] = 1
        for t in ("pbrBaseColorTexture", "metallicRoughnessTexture", "normalTexture", "emissiveTexture"):
            mats[k][t] = -1
    mats[0]["pbrBaseColorTexture"] = 0
    lights = np.zeros(1, LIGHT_DTYPE)
    lights["intensity"] = 1
    tex = [{"rgba8": np.random.default_rng(5).integers(0, 256, (3, 5, 4), dtype=np.uint8), "is_srgb": True}]
    alpha = np.array([(1, 0.3), (0, 0.5), (0, 0.5)], ALPHA_DTYPE)
    return FlatScene(pos, nrm, tan, uv, idx, pm, mats, lights, nodes, tex, alpha)


def test_gltf_round_trip_keeps_mask_and_cutoff_and_reads_blend_as_opaque(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gltf_export
    from vkrt_amd import host_py

    flat = _three_material_scene()
    path = str(tmp_path / "alpha.gltf")
    gltf_export.export_gltf(flat, path)
    g = json.load(open(path))
    assert g["materials"][0]["alphaMode"] == "MASK" and abs(g["materials"][0]["alphaCutoff"] - 0.3) < 1e-6
    assert all("alphaMode" not in m and "alphaCutoff" not in m for m in g["materials"][1:])  # glTF's defaults are not written
    g["materials"][1]["alphaMode"] = "BLEND"  # no counterpart in the ray queries: arrives as OPAQUE
    json.dump(g, open(path, "w"))
    back = host_py.load_gltf(path)
    assert back.material_alpha is not None and back.material_alpha.dtype == ALPHA_DTYPE
    assert back.material_alpha["mode"].tolist() == [abi.VKRT_ALPHA_MASK, abi.VKRT_ALPHA_OPAQUE, abi.VKRT_ALPHA_OPAQUE]
    assert back.material_alpha["cutoff"].tolist() == [np.float32(0.3), 0.5, 0.5]
    assert np.array_equal(back.materials, flat.materials)
    # MASK without a cutoff: glTF's default 0.5; a scene without any MASK material carries no array, as before
    del g["materials"][0]["alphaCutoff"]
    json.dump(g, open(path, "w"))
    assert host_py.load_gltf(path).material_alpha["cutoff"].tolist() == [0.5, 0.5, 0.5]
    del g["materials"][0]["alphaMode"]
    json.dump(g, open(path, "w"))
    assert host_py.load_gltf(path).material_alpha is None
    # and the exporter writes nothing for a scene without the array
    flat.material_alpha = None
    gltf_export.export_gltf(flat, path)
    assert all("alphaMode" not in m for m in json.load(open(path))["materials"])


def test_flat_scene_npz_round_trip_with_and_without_material_alpha(tmp_path):
    flat = _three_material_scene()
    flat.save_npz(str(tmp_path / "with.npz"))
    back = FlatScene.load_npz(str(tmp_path / "with.npz"))
    assert back.material_alpha.dtype == ALPHA_DTYPE and np.array_equal(back.material_alpha, flat.material_alpha)
    flat.material_alpha = None
    flat.save_npz(str(tmp_path / "without.npz"))
    assert "material_alpha" not in np.load(str(tmp_path / "without.npz")).files
    assert FlatScene.load_npz(str(tmp_path / "without.npz")).material_alpha is None
    # a stored scene from before the field loads as it did
    assert FlatScene.load_npz(os.path.join(ROOT, "tests", "golden", "cornell_flat.npz")).material_alpha is None
    with pytest.raises(ValueError):
        FlatScene(flat.positions, flat.normals, flat.tangents, flat.texcoords0, flat.indices, flat.prim_meshes, flat.materials, flat.lights,
                  flat.nodes, flat.textures, np.zeros(2, ALPHA_DTYPE))
