"""The host side of the scene-edit entry points on the CPU, bit for bit: make_material (what vkrt_scene_update_materials re-makes a record
with) against pack_scene's material tables; the per-texel functions of texture_pack.h -- exactly what the kernels of scene_edit.hip run --
against pack_scene's texel pool, level by level, and its footprint pool; the thresholds of the sRGB encode against the host's own powf
quantisation, exhaustively over [0, 1]; and the new checks and pack functions on degenerate inputs under the address and
undefined-behaviour sanitizers, as a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from vkrt_amd import abi
from vkrt_amd.flat_scene import MAT_DTYPE

import test_scene_pack as SP
from scene_edit_scenes import SLOTS, base_scene, target_scene

CSRC = SP.CSRC
SOURCES = SP.SOURCES + [os.path.join(CSRC, "entry_checks.cpp")]
MAX_MIPS = SP.MAX_MIPS

SHIM = SP.SHIM + r"""
#include <thread>
#include <vector>
#include "texture_pack.h"
extern "C" {
const uint32_t* shim_quad_first(const PackedScene* p) { return p->texQuadFirst.data(); }
const float* shim_packed_thresholds(const PackedScene* p) { return p->srgbEncode; }
int shim_make_material(const GltfPBRMaterial* m, const DevTexture* table, uint32_t textures, const uint32_t* quadFirst, int wantQuads, void* out192, char* msg,
                       int cap)
{
  std::string err;
  DevMaterial mat;
  DevShadeMaterial sm;
  const int rc = make_material(*m, table, textures, quadFirst, wantQuads != 0, mat, sm, err);
  memcpy(out192, &mat, sizeof mat);
  memcpy((char*)out192 + sizeof mat, &sm, sizeof sm);
  return message(rc, err, msg, cap);
}
void shim_thresholds(float* T) { make_srgb_encode_table(T); }
void shim_mip_level(const uint32_t* src, uint32_t sw, uint32_t sh, uint32_t* dst, uint32_t dw, uint32_t dh, int srgb, const float* lut, const float* T)
{
  for(uint32_t y = 0; y < dh; y++)
    for(uint32_t x = 0; x < dw; x++) dst[(size_t)y * dw + x] = vkrt_mip_texel(src, sw, sh, dw, dh, x, y, srgb != 0, lut, T);
}
void shim_footprints(const uint32_t* src, uint32_t w, uint32_t h, uint32_t* out)
{
  for(uint32_t y = 0; y < h; y++)
    for(uint32_t x = 0; x < w; x++) vkrt_footprint(src, w, h, x, y, out + ((size_t)y * w + x) * 4);
}
// how many of n values the table gives another code than the host's own encode
uint64_t shim_table_mismatches(const float* T, const float* v, uint64_t n)
{
  uint64_t bad = 0;
  for(uint64_t i = 0; i < n; i++) bad += vkrt_srgb_quantise(T, v[i]) != srgb_encode_code(v[i]) ? 1 : 0;
  return bad;
}
// every binary32 value of [0, 1]: out[0] = values whose table code differs, out[1] = places where the host's code decreases
void shim_sweep_unit_interval(const float* T, uint64_t out[2])
{
  const uint32_t last = 0x3f800000u, threads = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
  std::vector<uint64_t> bad(threads, 0), down(threads, 0);
  std::vector<std::thread> pool;
  for(uint32_t t = 0; t < threads; t++)
    pool.emplace_back([&, t] {
      uint64_t nbad = 0, ndown = 0;  // (thread-local: the shared vectors are written once)
      const uint64_t chunk = 1ull << 20;  // dealt round-robin: the powf part of the interval is its upper fourteenth
      for(uint64_t lo = chunk * t; lo <= last; lo += chunk * threads)
      {
        const uint64_t hi = std::min<uint64_t>(lo + chunk, last + 1ull);
        uint32_t prev = 0;
        for(uint64_t b = lo ? lo - 1 : 0; b < hi; b++)
        {
          const uint32_t bits = (uint32_t)b;
          float v;
          memcpy(&v, &bits, 4);
          const uint32_t code = srgb_encode_code(v);
          if(b >= lo)
          {
            nbad += vkrt_srgb_quantise(T, v) != code ? 1 : 0;
            ndown += code < prev ? 1 : 0;
          }
          prev = code;
        }
      }
      bad[t] = nbad; down[t] = ndown;
    });
  for(std::thread& th : pool) th.join();
  out[0] = out[1] = 0;
  for(uint32_t t = 0; t < threads; t++) { out[0] += bad[t]; out[1] += down[t]; }
}
}
"""

RECORD_DTYPE = np.dtype([("material", SP.MATERIAL_DTYPE), ("shade", SP.SHADE_DTYPE)])
assert RECORD_DTYPE.itemsize == 192


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_edit_shim")
    src, so = d / "shim.cpp", d / "libshim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC, str(src), *SP.SOURCES, "-o",
                    str(so)], check=True)
    lib = C.CDLL(str(so))
    P = C.c_void_p
    lib.shim_validate.argtypes = [C.POINTER(abi.SceneDesc), C.c_char_p, C.c_int]
    lib.shim_pack.argtypes, lib.shim_pack.restype = [C.POINTER(abi.SceneDesc), C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_int], P
    lib.shim_table.argtypes, lib.shim_table.restype = [P, C.c_int, C.POINTER(C.c_uint64)], P
    lib.shim_free.argtypes = [P]
    lib.shim_quad_first.argtypes, lib.shim_quad_first.restype = [P], P
    lib.shim_packed_thresholds.argtypes, lib.shim_packed_thresholds.restype = [P], P
    lib.shim_make_material.argtypes = [P, P, C.c_uint32, P, C.c_int, P, C.c_char_p, C.c_int]
    lib.shim_thresholds.argtypes = [P]
    lib.shim_mip_level.argtypes = [P, C.c_uint32, C.c_uint32, P, C.c_uint32, C.c_uint32, C.c_int, P, P]
    lib.shim_footprints.argtypes = [P, C.c_uint32, C.c_uint32, P]
    lib.shim_table_mismatches.argtypes, lib.shim_table_mismatches.restype = [P, P, C.c_uint64], C.c_uint64
    lib.shim_sweep_unit_interval.argtypes = [P, P]
    return lib


def _pack(lib, flat, quads=True):
    """SP.pack, and what the scene keeps for its edits: each texture's first footprint record and the thresholds"""
    desc, keep = flat.to_desc()
    msg, rc = C.create_string_buffer(600), C.c_int(-1)
    h = lib.shim_pack(C.byref(desc), int(quads), C.byref(rc), msg, 600)
    assert (rc.value, msg.value) == (abi.VKRT_OK, b"")
    out = {}
    for name, (which, dtype) in SP.TABLES.items():
        n = C.c_uint64()
        p = lib.shim_table(h, which, C.byref(n))
        out[name] = np.frombuffer(C.string_at(p, n.value), dtype).copy() if n.value else np.zeros(0, dtype)
    out["quadFirst"] = np.frombuffer(C.string_at(lib.shim_quad_first(h), 4 * len(flat.textures)), np.uint32).copy()
    out["thresholds"] = np.frombuffer(C.string_at(lib.shim_packed_thresholds(h), 4 * 256), np.float32).copy()
    lib.shim_free(h)
    return out


@pytest.fixture(scope="module")
def scenes(shim):
    a, b = base_scene(), target_scene()
    return {"A": (a, _pack(shim, a, True), _pack(shim, a, False)), "B": (b, _pack(shim, b, True), _pack(shim, b, False))}


@pytest.fixture(scope="module")
def thresholds(shim):
    T = np.zeros(256, np.float32)
    shim.shim_thresholds(T.ctypes.data)
    return T


def _make(lib, material, tables, quads):
    out = np.zeros(1, RECORD_DTYPE)
    m = np.ascontiguousarray(material, MAT_DTYPE).reshape(1)
    msg = C.create_string_buffer(600)
    rc = lib.shim_make_material(m.ctypes.data, tables["textures"].ctypes.data, tables["textures"].size, tables["quadFirst"].ctypes.data, int(quads),
                                out.ctypes.data, msg, 600)
    return rc, msg.value.decode(), out[0]


# ---- 2. host pack ------------------------------------------------------------------------------------------------------------------------
def test_make_material_gives_the_bytes_pack_scene_gives(shim, scenes):
    """every material of the fixture and of B, with and without a footprint pool -- and B's materials made against A's texture tables
    (what vkrt_scene_update_materials does: the tables of a scene do not depend on its texels or materials)"""
    made = 0
    for name, (flat, with_quads, without) in scenes.items():
        for tables, quads in ((with_quads, True), (without, False)):
            for against in (tables, scenes["A"][1 if quads else 2]):
                for mi, m in enumerate(flat.materials):
                    rc, msg, rec = _make(shim, m, against, quads)
                    assert (rc, msg) == (abi.VKRT_OK, "")
                    assert rec["material"].tobytes() == tables["materials"][mi].tobytes(), (name, quads, mi)
                    assert rec["shade"].tobytes() == tables["shadeMaterials"][mi].tobytes(), (name, quads, mi)
                    made += 1
    assert made == 2 * 2 * 2 * 4
    assert np.array_equal(scenes["A"][1]["textures"].view(np.uint8), scenes["B"][1]["textures"].view(np.uint8))
    assert np.array_equal(scenes["A"][1]["quadFirst"], scenes["B"][1]["quadFirst"]) and np.array_equal(scenes["A"][1]["texMips"], scenes["B"][1]["texMips"])
    assert scenes["A"][1]["materials"].tobytes() != scenes["B"][1]["materials"].tobytes()  # the target does differ


def test_without_a_footprint_pool_the_references_fall_back_to_texel_offsets(shim, scenes):
    flat, with_quads, without = scenes["B"]
    first, _ = SP._quad_first(flat)
    offsets, _ = SP._texel_offsets(flat)
    assert list(with_quads["quadFirst"]) == first and list(without["quadFirst"]) == first and without["texQuads"].size == 0
    seen = set()
    for mi, m in enumerate(flat.materials):
        _, _, rec = _make(shim, m, without, False)
        _, _, recq = _make(shim, m, with_quads, True)
        for k, slot in enumerate(SLOTS):
            ti = int(m[slot])
            seen.add(ti)
            srgb = int(ti >= 0 and flat.textures[ti]["is_srgb"])
            assert rec["shade"]["ref"][2 * k + 1] == (offsets[ti][0] if ti >= 0 else 0) | (srgb << 31) and rec["material"]["tex"][k][3] == 0
            assert recq["shade"]["ref"][2 * k + 1] == (first[ti] if ti >= 0 else 0) | (srgb << 31)
            assert recq["material"]["tex"][k][3] == (first[ti] if ti >= 0 else 0)
    assert seen == {-1, 0, 1, 2, 3, 4, 5, 6}


def test_make_material_refuses_a_side_above_32768(shim, scenes):
    tables = {k: v.copy() for k, v in scenes["A"][1].items()}
    tables["textures"][2]["width"] = 32769
    m = scenes["A"][0].materials[0].copy()
    m["normalTexture"] = 2
    rc, msg, _ = _make(shim, m, tables, True)
    assert rc == abi.VKRT_ERR_UNSUPPORTED and msg == "texture 2 is 32769x2 (supported: 1..32768 per side)"
    m["normalTexture"] = -1
    m["pbrBaseColorTexture"] = m["metallicRoughnessTexture"] = m["emissiveTexture"] = 3  # the oversized one is not referenced
    assert _make(shim, m, tables, True)[:2] == (abi.VKRT_OK, "")


def test_the_per_texel_functions_reproduce_every_level_and_the_footprint_pool(shim, scenes, thresholds):
    """vkrt_mip_texel with the threshold table, level L from level L - 1 of pack_scene's pool, and vkrt_footprint from level 0: the
    functions the kernels run, on the host"""
    levels_seen = 0
    for name, (flat, tables, _) in scenes.items():
        assert np.array_equal(tables["thresholds"].view(np.uint32), thresholds.view(np.uint32))
        pool, lut = tables["texels"], tables["srgbLut"]
        quads = tables["texQuads"].reshape(-1, 4)
        for ti, (w, h) in enumerate(SP._sizes(flat)):
            row = tables["texMips"][ti * MAX_MIPS:(ti + 1) * MAX_MIPS]
            levels = int(tables["textures"][ti]["srgb"]) >> 8
            srgb = int(tables["textures"][ti]["srgb"]) & 1
            assert srgb == int(flat.textures[ti]["is_srgb"])
            src = np.ascontiguousarray(pool[row[0]:row[0] + w * h])
            assert np.array_equal(src.view(np.uint8).reshape(h, w, 4), flat.textures[ti]["rgba8"])
            got = np.zeros((w * h, 4), np.uint32)
            shim.shim_footprints(src.ctypes.data, w, h, got.ctypes.data)
            first = int(tables["quadFirst"][ti])
            assert np.array_equal(got, quads[first:first + w * h]), (name, ti)
            sw, sh = w, h
            for L in range(1, levels):
                dw, dh = max(1, sw // 2), max(1, sh // 2)
                dst = np.zeros(dw * dh, np.uint32)
                shim.shim_mip_level(src.ctypes.data, sw, sh, dst.ctypes.data, dw, dh, srgb, lut.ctypes.data, thresholds.ctypes.data)
                want = pool[row[L]:row[L] + dw * dh]
                assert np.array_equal(dst, want), (name, ti, L, int((dst != want).sum()))
                src, sw, sh = np.ascontiguousarray(want), dw, dh
                levels_seen += 1
            assert (sw, sh) == (1, 1)
    assert levels_seen == 2 * (5 + 6 + 3 + 2 + 0 + 7 + 8)  # 37x21, 64x64, 8x2, 5x3, 1x1, 128x32, 256x256


# ---- 3. the encode table ------------------------------------------------------------------------------------------------------------------
def test_thresholds_are_sorted_and_tight(shim, thresholds):
    T = thresholds
    assert T[0] == 0.0 and (np.diff(T) >= 0).all() and (np.diff(T[1:]) > 0).all() and T[1] > 0 and T[255] <= 1.0
    # each is the first value of its code: the value one ulp below has a smaller code
    below = (T[1:].view(np.uint32) - 1).view(np.float32)
    at = np.ascontiguousarray(T[1:])
    assert shim.shim_table_mismatches(T.ctypes.data, at.ctypes.data, 255) == 0 and shim.shim_table_mismatches(T.ctypes.data, below.ctypes.data, 255) == 0
    curve = np.where(T <= 0.0031308, 12.92 * T.astype(np.float64), 1.055 * T.astype(np.float64) ** (1 / 2.4) - 0.055) * 255.0
    assert np.abs(curve[1:] - (np.arange(1, 256) - 0.5)).max() < 1e-3  # the thresholds sit where the curve crosses q - 1/2


def test_table_lookup_equals_the_hosts_quantisation(shim, scenes, thresholds):
    """the windows of +-4096 ulps around every threshold, all 256 decode values, 2^24 random binary32 values of [0, 1.0001], and values
    beyond: one mismatch anywhere would flip a texel"""
    T = thresholds
    bits = (T[1:].view(np.uint32).astype(np.int64)[:, None] + np.arange(-4096, 4097)[None, :]).ravel()
    window = np.ascontiguousarray(bits[bits >= 0].astype(np.uint32).view(np.float32))
    lut = np.ascontiguousarray(scenes["A"][1]["srgbLut"][:256])
    rng = np.random.default_rng(5)
    rnd = np.concatenate([rng.uniform(0.0, 1.0001, 1 << 23).astype(np.float32),
                          np.exp2(rng.uniform(-40.0, 0.0002, 1 << 23)).astype(np.float32)])  # half of them spread over the exponents
    assert rnd.size == 1 << 24 and rnd.min() >= 0 and rnd.max() <= np.float32(1.0002)
    edge = np.array([0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)), 1.5, 1e30, np.inf, 1e-45, 0.0031308, np.nextafter(np.float32(0.0031308), np.float32(1))],
                    np.float32)
    for name, v in (("window", window), ("lut", lut), ("random", rnd), ("edge", edge)):
        assert shim.shim_table_mismatches(T.ctypes.data, v.ctypes.data, v.size) == 0, name


def test_table_lookup_is_exact_on_every_float_of_the_unit_interval(shim, thresholds):
    """all 1 065 353 217 binary32 values of [0, 1]: the table's code is the host's, and the host's code never decreases (which is what makes
    a table of thresholds a complete description of it)"""
    out = (C.c_uint64 * 2)()
    shim.shim_sweep_unit_interval(thresholds.ctypes.data, out)
    assert (out[0], out[1]) == (0, 0)


# ---- 4. under the sanitizers ---------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "entry_checks.h"
#include "scene_pack.h"
#include "texture_pack.h"
using namespace vkrt;

static int failures = 0;
#define CHECK(cond) do { if(!(cond)) { printf("FAILED %s (line %d)\n", #cond, __LINE__); failures++; } } while(0)

static GltfPBRMaterial material(int base, int mr, int normal, int emissive)
{
  GltfPBRMaterial m;
  memset(&m, 0, sizeof m);
  for(int k = 0; k < 4; k++) m.pbrBaseColorFactor[k] = 1.0f;
  m.pbrBaseColorTexture = base; m.metallicRoughnessTexture = mr; m.normalTexture = normal; m.emissiveTexture = emissive;
  return m;
}

// every level and the footprints of one w x h texture through the per-texel functions, against pack_scene's pools
static void chain(uint32_t w, uint32_t h, bool srgb)
{
  std::vector<uint8_t> texels((size_t)w * h * 4);
  for(size_t k = 0; k < texels.size(); k++) texels[k] = (uint8_t)(29 * k + 7 * w + h);
  const vkrt_texture tex = {w, h, texels.data(), srgb ? 1 : 0};
  const GltfPBRMaterial m = material(0, -1, 0, -1);
  GltfLight light;
  memset(&light, 0, sizeof light);
  vkrt_scene_desc d;
  memset(&d, 0, sizeof d);
  d.struct_size = sizeof d;
  d.materials = &m; d.material_count = 1; d.lights = &light; d.light_count = 1; d.textures = &tex; d.texture_count = 1;
  PackedScene p;
  std::string err;
  CHECK(validate_scene(&d, err) == VKRT_OK && pack_scene(&d, true, p, err) == VKRT_OK);
  CHECK(p.texQuadFirst.size() == 1 && p.texQuadFirst[0] == 1u && p.texQuads.size() == 4 * (1 + (size_t)w * h));
  for(uint32_t y = 0; y < h; y++)
    for(uint32_t x = 0; x < w; x++)
    {
      uint32_t q[4];
      vkrt_footprint(p.texels.data(), w, h, x, y, q);
      CHECK(memcmp(q, &p.texQuads[4 * (1 + (size_t)y * w + x)], 16) == 0);
    }
  const uint32_t levels = p.textures[0].srgb >> 8;
  uint32_t sw = w, sh = h;
  for(uint32_t L = 1; L < levels; L++)
  {
    const uint32_t dw = sw / 2 ? sw / 2 : 1, dh = sh / 2 ? sh / 2 : 1;
    for(uint32_t y = 0; y < dh; y++)
      for(uint32_t x = 0; x < dw; x++)
        CHECK(vkrt_mip_texel(&p.texels[p.texMips[L - 1]], sw, sh, dw, dh, x, y, srgb, p.srgbLut, p.srgbEncode) == p.texels[p.texMips[L] + (size_t)y * dw + x]);
    sw = dw; sh = dh;
  }
  CHECK(sw == 1 && sh == 1);
}

int main()
{
  std::string err;
  const uint32_t sizes[][2] = {{1, 1}, {1, 9}, {9, 1}, {2, 1}, {1, 2}, {3, 5}, {16, 16}};
  for(const auto& s : sizes)
    for(int srgb = 0; srgb < 2; srgb++) chain(s[0], s[1], srgb != 0);
  {  // make_material: index -1 and index texture_count - 1 in every slot, a table that ends with the referenced texture
    const DevTexture table[3] = {{0u, 1u, 1u, 1u | (1u << 8)}, {1u, 1u, 9u, 4u << 8}, {14u, 9u, 1u, 1u | (4u << 8)}};
    const uint32_t quadFirst[3] = {1u, 2u, 11u};
    for(int slot = 0; slot < 4; slot++)
      for(int quads = 0; quads < 2; quads++)
      {
        int idx[4] = {-1, -1, -1, -1};
        idx[slot] = 2;
        DevMaterial mat;
        DevShadeMaterial sm;
        CHECK(make_material(material(idx[0], idx[1], idx[2], idx[3]), table, 3, quadFirst, quads != 0, mat, sm, err) == VKRT_OK);
        for(int k = 0; k < 4; k++)
        {
          CHECK(mat.tex[k].flags == (k == slot ? 3u : 0u) && mat.tex[k].quads == (k == slot && quads ? 11u : 0u));
          CHECK(sm.ref[2 * k + 1] == (k == slot ? ((quads ? 11u : 14u) | (1u << 31)) : 0u));
        }
        CHECK(make_material(material(idx[0], idx[1], idx[2], idx[3]), nullptr, 0, nullptr, quads != 0, mat, sm, err) == VKRT_OK);  // a scene without textures
        CHECK(mat.tex[slot].flags == 0u);
      }
  }
  {  // the checks: count 0, ranges that end at the table's end, one beyond, NULL and misaligned arrays
    GltfLight lights[2];
    memset(lights, 0, sizeof lights);
    vkrt_light_update u = {sizeof(vkrt_light_update), 2, 0, VKRT_MEMORY_HOST, nullptr};
    CHECK(check_light_update_desc(nullptr, err) == VKRT_ERR_INVALID_ARGUMENT && check_light_update_desc(&u, err) == VKRT_OK);
    CHECK(check_light_update_range(u, 2, err) == VKRT_OK);  // empty, at the end, no array
    u.first = 0; u.count = 2; u.lights = lights;
    CHECK(check_light_update_range(u, 2, err) == VKRT_OK);
    u.first = 1;
    CHECK(check_light_update_range(u, 2, err) == VKRT_ERR_INVALID_ARGUMENT);
    u.first = 0xffffffffu; u.count = 0xffffffffu;
    CHECK(check_light_update_range(u, 2, err) == VKRT_ERR_INVALID_ARGUMENT);
    u.first = 0; u.count = 1; u.memory = VKRT_MEMORY_DEVICE; u.lights = (const GltfLight*)((const char*)lights + 4);
    CHECK(check_light_update_range(u, 2, err) == VKRT_ERR_INVALID_ARGUMENT && err.find("16-byte") != std::string::npos);
    u.struct_size = 8;
    CHECK(check_light_update_desc(&u, err) == VKRT_ERR_INVALID_ARGUMENT);
    const GltfPBRMaterial m[2] = {material(-1, 2, -1, 2), material(3, -1, -1, -1)};
    CHECK(check_material_update_values("t", 0, nullptr, 3, err) == VKRT_OK && check_material_update_values("t", 1, nullptr, 3, err) == VKRT_ERR_INVALID_ARGUMENT);
    CHECK(check_material_update_values("t", 1, m, 3, err) == VKRT_OK && check_material_update_values("t", 2, m, 3, err) == VKRT_ERR_INVALID_ARGUMENT);
    CHECK(check_material_update_values("t", 2, m, 0, err) == VKRT_OK);  // a scene without textures: every index is the invalid reference
    CHECK(check_material_range("t", 2, 0, 2, err) == VKRT_OK && check_material_range("t", 1, 2, 2, err) == VKRT_ERR_INVALID_ARGUMENT);
    uint8_t texel[4] = {1, 2, 3, 4};
    vkrt_texture_update t = {sizeof(vkrt_texture_update), 2, 1, 1, VKRT_MEMORY_HOST, texel};
    CHECK(check_texture_update_desc(&t, err) == VKRT_OK && check_texture_index("t", 2, 3, err) == VKRT_OK);
    CHECK(check_texture_index("t", 3, 3, err) == VKRT_ERR_INVALID_ARGUMENT && check_texture_index("t", 0, 0, err) == VKRT_ERR_INVALID_ARGUMENT);
    CHECK(check_texture_update_image(t, 1, 1, err) == VKRT_OK && check_texture_update_image(t, 1, 2, err) == VKRT_ERR_INVALID_ARGUMENT);
    t.rgba8 = nullptr;
    CHECK(check_texture_update_image(t, 1, 1, err) == VKRT_ERR_INVALID_ARGUMENT);
    t.memory = 9;
    CHECK(check_texture_update_desc(&t, err) == VKRT_ERR_INVALID_ARGUMENT);
  }
  float T[VKRT_SRGB_THRESHOLDS];
  make_srgb_encode_table(T);
  CHECK(vkrt_srgb_quantise(T, 0.0f) == 0u && vkrt_srgb_quantise(T, 1.0f) == 255u && vkrt_srgb_quantise(T, 2.0f) == 255u && vkrt_srgb_quantise(T, -1.0f) == 0u);
  printf("failures %d\n", failures);
  return failures ? 1 : 0;
}
"""


def test_checks_and_pack_functions_run_cleanly_under_the_sanitizers(tmp_path):
    src, exe = tmp_path / "edit.cpp", tmp_path / "edit"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(src), *SOURCES, "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("failures 0"), (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
