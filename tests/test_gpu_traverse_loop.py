"""The sharing traversal loop (csrc/traverse_share.h) after its bookkeeping was trimmed (profiles/r11_experiments.md): stack cursors
as LDS addresses, one step bound for the wave, one vote for the triangle step and the lending, the ray's result address kept beside
its home lane, the octant word shuffled with an adopted ray.  None of that may move a bit: images of 100 x 70 pixels (no multiple of
the 8 x 8 tile; 7000 camera rays, so the last wave of every stream is partial and its tail lanes help from the first step), 2 spp,
depth 4, two progressive frames in one vkrt_pathtrace_frames call, on the Cornell box and on the 20 k-triangle atrium in its uniform
and its artist-like tessellation (strips that give one node test up to 24 triangles: parked groups, the flush path, triangle gifts,
lending), each under the defaults, without sharing, without lending, on the BVH2 layout, and with the watertight test and the dissolve
stage (each of those two with and without sharing).

Checks: the Cornell images equal the oracle's bit for bit (the oracle with the same test / stage); on the atrium scenes the variants
of one arithmetic give ONE image hash and the same ray, pair-record, hit and pixel counters (profiles/r01_experiments.md #42); the
default variant stands to the oracle as tests/test_gpu_parity.py demands of textured atrium frames; traversal_faults is 0 everywhere.
The watertight test and the dissolve stage are arithmetics of their own, each with its own oracle (tests/test_gpu_parity.py), so
their variants are compared among themselves.  Every variant runs a plain launch (the product kernels) and an instrumented one
(their counting twins: `hits` is only tallied there), and the two must agree as well.

The library has no way to force stackCap below what a tree needs (it is derived from the tree's depth, csrc/api_accel.cpp), so the
case "parked groups tested out for lack of room" is not forced here; the strips of the artist-like atrium reach the flush path
through VKRT_W8_MAX_POSTPONED instead.

Ray queries run the same walk: 5000 rays on the atrium with two tmin values inside every wave (the query kernel then walks lane by
lane), closest hits and occlusion bit for bit between the wide layout and BVH2."""
import hashlib
import inspect
import os
import re
import sys

import numpy as np
import pytest

import test_gpu_parity as P
import test_gpu_ray_query as Q
from conftest import default_camera

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
THREADS = min(16, os.cpu_count() or 1)
W, H = 100, 70
SPP, DEPTH, FRAMES, SEED = 2, 4, 2, 33
COUNTED = ("rays_closest", "rays_shadow", "pair_records", "pixels")


def _variants():
    from vkrt_amd import abi

    return {"defaults": {}, "share_off": {abi.VKRT_OPT_WF_SHARE: 0}, "lend_off": {abi.VKRT_OPT_WF_TRI_LEND: 0}, "bvh2": {abi.VKRT_OPT_BVH_LAYOUT: 0},
            "dissolve": {abi.VKRT_OPT_ANYHIT_DISSOLVE: 1}, "dissolve_share_off": {abi.VKRT_OPT_ANYHIT_DISSOLVE: 1, abi.VKRT_OPT_WF_SHARE: 0},
            "watertight": {abi.VKRT_OPT_WATERTIGHT: 1}, "watertight_share_off": {abi.VKRT_OPT_WATERTIGHT: 1, abi.VKRT_OPT_WF_SHARE: 0}}


NAMES = ("defaults", "share_off", "lend_off", "bvh2", "dissolve", "dissolve_share_off", "watertight", "watertight_share_off")


def _atrium_rule():
    """(rmse bound, mismatch bound) tests/test_gpu_parity.py sets for textured atrium frames, read from that test"""
    src = inspect.getsource(P.test_atrium_small_textured_full_image)
    return P.RMSE_TOL, float(re.search(r"mismatch_fraction\(img, ref\) < ([0-9.e-]+)", src).group(1))


@pytest.fixture(scope="module")
def scenes(cornell_flat):
    import atrium

    return {"cornell": (cornell_flat, {}), "default": (atrium.build_atrium(20000, seed=4, with_textures=True)[0], atrium.DEFAULT_CAMERA),
            "nonuniform": (atrium.build_atrium(20000, seed=4, with_textures=True, variant="nonuniform")[0], atrium.DEFAULT_CAMERA)}


_ORACLE = {}


def _oracle_frames(scenes, scene, watertight=False, dissolve=False):
    """the oracle's image after the two frames, rendered once per (scene, arithmetic)"""
    import oracle_py
    from vkrt_amd.flat_scene import make_push_constants

    key = (scene, watertight, dissolve)
    if key not in _ORACLE:
        flat, camkw = scenes[scene]
        orc = oracle_py.OracleScene(flat)
        orc.set_watertight(watertight)
        orc.set_dissolve(dissolve)
        img = None
        for f in range(FRAMES):
            pc = make_push_constants(samples=SPP, depth=DEPTH, frame=f, lights_count=len(flat.lights))
            img, _ = orc.render(pc, default_camera(W, H, **camkw), W, H, seed=SEED + f, image=img, threads=THREADS)
        _ORACLE[key] = img
    return _ORACLE[key]


_GOT = {}


def _render(scenes, scene, name):
    """image hash, image and counters of the plain and of the instrumented call of one variant; rendered once"""
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Renderer

    if (scene, name) not in _GOT:
        flat, camkw = scenes[scene]
        r = Renderer(flat, device=0, build="ploc", options=_variants()[name])
        pc = make_push_constants(samples=SPP, depth=DEPTH, frame=0, lights_count=len(flat.lights))
        out = []
        for flags in (0, abi.VKRT_TRACE_COUNT_TRAVERSAL):
            r.reset_counters()
            img = r.pathtrace_frames(pc, default_camera(W, H, **camkw), W, H, FRAMES, seed=SEED, flags=flags).cpu().numpy()
            out.append((hashlib.sha256(img.tobytes()).hexdigest(), img, r.counters()))
        r.close()
        _GOT[(scene, name)] = out
    return _GOT[(scene, name)]


@pytest.mark.parametrize("name", NAMES)
def test_cornell_equals_the_oracle_bit_for_bit(scenes, name):
    ref = _oracle_frames(scenes, "cornell", watertight=name.startswith("watertight"), dissolve=name.startswith("dissolve"))
    for what, (_, img, c) in zip(("plain", "instrumented"), _render(scenes, "cornell", name)):
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (name, what, P.mismatch_fraction(img, ref))
        assert c["traversal_faults"] == 0, (name, what)


@pytest.mark.parametrize("name", NAMES[1:])
@pytest.mark.parametrize("scene", ["default", "nonuniform"])
def test_atrium_variants_give_one_image_and_the_same_counters(scenes, scene, name):
    base = name.split("_")[0] if name.startswith(("watertight", "dissolve")) else "defaults"
    want, got = _render(scenes, scene, base), _render(scenes, scene, name)
    print(scene, name, got[0][0][:16], got[1][0][:16], "against", base, want[0][0][:16], {k: got[0][2][k] for k in COUNTED}, "hits", got[1][2]["hits"])
    for k in (0, 1):
        assert got[k][2]["traversal_faults"] == 0 and want[k][2]["traversal_faults"] == 0
        assert got[k][0] == want[0][0], (scene, name, k, P.mismatch_fraction(got[k][1], want[0][1]))
        for key in COUNTED:
            assert got[k][2][key] == want[0][2][key], (scene, name, k, key)
    assert got[1][2]["hits"] == want[1][2]["hits"] > 0


@pytest.mark.parametrize("scene", ["default", "nonuniform"])
def test_atrium_default_variant_agrees_with_the_oracle(scenes, scene):
    ref = _oracle_frames(scenes, scene)
    rmse_tol, mismatch_tol = _atrium_rule()
    for _, img, c in _render(scenes, scene, "defaults"):
        print(scene, "rmse", P.rmse(img, ref), "pixels that differ", P.mismatch_fraction(img, ref))
        assert P.rmse(img, ref) < rmse_tol
        assert P.mismatch_fraction(img, ref) < mismatch_tol
        assert c["traversal_faults"] == 0


def test_ray_queries_with_two_tmin_values_in_a_wave(scenes):
    """closest hits and occlusion of 5000 rays whose tmin alternates inside every wave: the wide layout against BVH2, bit for bit"""
    flat, _ = scenes["default"]
    o, d = Q._hostile_rays(flat, 5000, seed=91)
    tmin = np.where(np.arange(5000) % 3 == 1, 0.75, 0.001).astype(np.float32)
    rays = Q._pack(o, d, tmin, 10000.0)
    got = []
    for layout in (1, 0):
        r = Q._renderer(flat, "ploc", layout=layout)
        got.append((Q._intersect(r, rays), Q._occluded(r, rays)))
        assert r.counters()["traversal_faults"] == 0
        r.close()
    assert np.array_equal(got[0][0]["raw"], got[1][0]["raw"])
    assert np.array_equal(got[0][1], got[1][1])
    hit = got[0][0]["ints"][:, 3] >= 0
    assert 100 < hit.sum() < 5000 and got[0][1].sum() == hit.sum()
    assert np.all(got[0][0]["t"][hit] > tmin[hit])  # the larger tmin cut hits away: rays that start on a triangle see past it
