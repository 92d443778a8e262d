"""Six traversal waves per SIMD (profiles/r12_experiments.md) on the device: the product traversal kernels with 80 registers, the
320-word result block and the match of a sharing / lending step made in registers (csrc/traverse_share.h, DONOR_LDS = false) must not
move a bit, on either side of the depth at which a tree's waves stop fitting six to a SIMD.

Shallow trees (wide depth <= 9: five LDS granules per wave, six waves): the Cornell box (depth 8), the smallest atrium of the GPU tests
(2000 triangles, textured; depth 7) and the `far` scene of tests/split_scenes.py seen from three units away (depth 9, exactly the
boundary; no scene of tests/test_gpu_bvh_topology.py or tests/split_scenes.py is deeper under any builder).  Deep trees (a sixth granule,
five waves; the same kernels with a larger stack): a graded strip made for the purpose -- 200 triangles along x, each 1.1 times the
size of the one before, seen from inside at a small field of view so that a quarter of the camera rays hit -- whose wide tree is 13
levels deep under `lbvh` and 12 under `sah`.  The depth is read through vkrt_accel_get_info and asserted on its side of the boundary;
what csrc/trav_lds.h makes of it is restated in tests/test_six_waves_isa.py (lds_plan, checked against the header on the CPU).

64 x 48 pixels, 2 spp, depth 3: frame 0, frame 1 on top of it, and one call of three frames; each as a plain launch (the product
kernels) and as an instrumented one (their counting twins).  Images equal the oracle's bit for bit, rays_closest / rays_shadow / pixels
are the oracle's, traversal_faults is 0, the instrumented launch has the plain one's pair_records and its own `hits`.  One batch of 4096
ray queries (closest hit and occlusion) on the atrium is bit-equal between the wide layout and the BVH2 lane walk."""
import os
import sys

import numpy as np
import pytest

import test_gpu_ray_query as Q
from conftest import default_camera
from test_six_waves_isa import lds_plan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
W, H, SPP, DEPTH, SEED = 64, 48, 2, 3, 12
SHALLOW = ("cornell", "atrium", "far")
DEEP = ("strip_lbvh", "strip_sah")
SCENE_NAMES = SHALLOW + DEEP
BUILD = {"strip_lbvh": "lbvh", "strip_sah": "sah"}  # (the others: ploc)
BOUNDARY = 9  # deepest wide8 tree whose waves are charged five LDS granules (csrc/trav_lds.h)
GRANULE = 1280  # profiles/r12_six_waves.json lds_granule_bytes (tests/test_six_waves_isa.py holds the header to it)
ORACLE_COUNTED = ("rays_closest", "rays_shadow", "pixels")


def _graded_strip(n=200, ratio=1.1):
    """n triangles along x, each `ratio` times the size of the one before and 1.5 sizes further on: every builder nests them deep"""
    s = ratio ** np.arange(n)
    x = np.cumsum(s) * 1.5
    c = np.stack([x, np.zeros(n), np.zeros(n)], 1)
    tri = np.stack([c, c + s[:, None] * np.array([1, 0, 0.2]), c + s[:, None] * np.array([0, 1, 0.3])], 1)
    return tri.reshape(-1, 3).astype(np.float32)


@pytest.fixture(scope="module")
def scenes(cornell_flat):
    import atrium
    from test_gpu_bvh_bounds import _triangle_scene
    from test_gpu_split_refs import flat_scene

    strip = (_triangle_scene(_graded_strip()), dict(eye=(10, 0.5, 1), center=(30, 0.75, 0), up=(0, 0, 1), fov=12.0))
    return {"strip_lbvh": strip, "strip_sah": strip,
            "cornell": (cornell_flat, {}), "atrium": (atrium.build_atrium(2000, seed=5, with_textures=True)[0], atrium.DEFAULT_CAMERA),
            "far": (flat_scene("far"), dict(eye=(1e5, 1e5, 1e5 + 3.0), center=(1e5, 1e5, 1e5), up=(0, 1, 0), fov=60.0))}


_ORACLE = {}


def _oracle(scenes, scene):
    """{"f0", "f1", "call3": (image, summed counters)} of the oracle, rendered once per scene"""
    import oracle_py
    from vkrt_amd.flat_scene import make_push_constants

    scene = "strip" if scene in DEEP else scene  # (one oracle for both builds of the strip)
    if scene not in _ORACLE:
        flat, camkw = scenes["strip_lbvh" if scene == "strip" else scene]
        orc = oracle_py.OracleScene(flat)
        cam = default_camera(W, H, **camkw)
        img, out, total = None, {}, {k: 0 for k in ORACLE_COUNTED}
        for f in range(3):
            pc = make_push_constants(samples=SPP, depth=DEPTH, frame=f, lights_count=len(flat.lights))
            img, c = orc.render(pc, cam, W, H, seed=SEED + f, image=img, threads=min(16, os.cpu_count() or 1))
            total = {k: total[k] + c[k] for k in ORACLE_COUNTED}
            out[("f0", "f1", "call3")[f]] = (img.copy(), {k: c[k] for k in ORACLE_COUNTED} if f < 2 else dict(total))
        _ORACLE[scene] = out
    return _ORACLE[scene]


_GOT = {}


def _device(scenes, scene):
    """flags -> {"f0", "f1", "call3": (image, counters)}, and the tree's info; rendered once per scene"""
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Renderer

    if scene not in _GOT:
        flat, camkw = scenes[scene]
        r = Renderer(flat, device=0, build=BUILD.get(scene, "ploc"))
        cam = default_camera(W, H, **camkw)
        pc = lambda f: make_push_constants(samples=SPP, depth=DEPTH, frame=f, lights_count=len(flat.lights))  # noqa: E731
        got = {"info": r.accel_info()}
        for flags in (0, abi.VKRT_TRACE_COUNT_TRAVERSAL):
            out = {}
            r.reset_counters()
            img = r.pathtrace(pc(0), cam, W, H, seed=SEED, flags=flags)
            out["f0"] = (img.cpu().numpy(), r.counters())
            r.reset_counters()
            img = r.pathtrace(pc(1), cam, W, H, seed=SEED + 1, flags=flags, image=img)
            out["f1"] = (img.cpu().numpy(), r.counters())
            r.reset_counters()
            out["call3"] = (r.pathtrace_frames(pc(0), cam, W, H, 3, seed=SEED, flags=flags).cpu().numpy(), r.counters())
            got[flags] = out
        r.close()
        _GOT[scene] = got
    return _GOT[scene]


@pytest.mark.parametrize("what", ["f0", "f1", "call3"])
@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_frames_equal_the_oracle_bit_for_bit(scenes, scene, what):
    from vkrt_amd import abi

    ref, want = _oracle(scenes, scene)[what]
    got = _device(scenes, scene)
    plain, counted = got[0][what], got[abi.VKRT_TRACE_COUNT_TRAVERSAL][what]
    for name, (img, c) in (("plain", plain), ("instrumented", counted)):
        differ = float(np.mean(np.any(img.view(np.uint32) != ref.view(np.uint32), axis=-1)))
        print(scene, what, name, "pixels that differ", differ, {k: (c[k], want[k]) for k in ORACLE_COUNTED}, "faults", c["traversal_faults"])
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (scene, what, name, differ)
        for k in ORACLE_COUNTED:
            assert c[k] == want[k], (scene, what, name, k)
        assert c["traversal_faults"] == 0
    assert counted[1]["pair_records"] == plain[1]["pair_records"]
    assert counted[1]["hits"] > 0


@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_tree_depth_is_on_its_side_of_the_boundary(scenes, scene):
    depth = int(_device(scenes, scene)["info"]["max_depth"])
    cap, charged, per_cu, per_simd = lds_plan(depth, GRANULE)
    print(scene, "wide depth", depth, "stackCap", cap, "charged", charged, "waves per CU", per_cu, "per SIMD", per_simd)
    if scene in SHALLOW:
        assert depth <= BOUNDARY and per_simd == 6 and per_cu >= 24
        if scene == "far":
            assert depth == BOUNDARY  # (what makes it the boundary case; a builder that changes this gets to pick again)
    else:
        assert depth > BOUNDARY and per_simd <= 5 and per_cu < 24


def test_ray_queries_equal_the_bvh2_lane_walk(scenes):
    flat, _ = scenes["atrium"]
    o, d = Q._hostile_rays(flat, 4096, seed=17)
    rays = Q._pack(o, d, 0.001, 10000.0)
    got = []
    for layout in (1, 0):
        r = Q._renderer(flat, "ploc", layout=layout)
        got.append((Q._intersect(r, rays), Q._occluded(r, rays)))
        assert r.counters()["traversal_faults"] == 0
        r.close()
    assert np.array_equal(got[0][0]["raw"], got[1][0]["raw"])
    assert np.array_equal(got[0][1], got[1][1])
    hit = got[0][0]["ints"][:, 3] >= 0
    assert 100 < hit.sum() < 4096 and got[0][1].sum() == hit.sum()
