"""VKRT_OPT_WF_TRI_LEND: in a triangle step of the sharing traversal wave (csrc/traverse_share.h) a lane with two or more pending
triangles lends its last one to a lane that holds none, which tests it in the same step with the lender's ray.  Closest hit is the
minimum over (t bits, triangle id) and any-hit is "exists", whoever runs a test, so every case runs with the option at 0 and at 1
and both must leave the bits of the oracle: t, u, v and ids of ray queries, images and ray counters of frames.  Only tris_tested
and the wave-step counters may move, and the last test demands that they do."""
import copy
import os
import sys

import numpy as np
import pytest

import test_gpu_ray_query as Q
from conftest import default_camera

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
THREADS = min(16, os.cpu_count() or 1)
KINDS = ("ploc", "lbvh", "sah")
RAYS = ("rays_closest", "rays_shadow", "pixels")
STRIPS = 48
TMAX = 100.0
# nodes of the strip fan, in this order: flattened triangle ids are [0, 96) [96, 98) [98, 194) [194, 196)
FAN_A, BACKDROP, FAN_B, OCCLUDER = 0, 1, 2, 3


def _quad(x0, x1, y, z0, z1):
    """two triangles, counter-clockwise seen from +y"""
    return [[x0, y, z0], [x0, y, z1], [x1, y, z0], [x1, y, z0], [x0, y, z1], [x1, y, z1]]


def _strip_fan(strip_alpha=1.0):
    """48 strips of 16 x 1/3 units in the plane y = 0 (one wide node's leaves hold many of them for a ray that grazes the plane),
    instanced twice with identical vertices (FAN_A, FAN_B: equal t in every pair, the tie goes to FAN_A's smaller id; FAN_B has a
    prim mesh and a material of its own over the same indices), a backdrop at y = -2 and an occluder at y = 0.1 over a part of it."""
    from vkrt_amd.flat_scene import LIGHT_DTYPE, MAT_DTYPE, NODE_DTYPE, PRIM_DTYPE, FlatScene

    z = np.linspace(-8.0, 8.0, STRIPS + 1)
    fan = [v for k in range(STRIPS) for v in _quad(-8.0, 8.0, 0.0, z[k], z[k + 1])]
    pos = np.array(fan + _quad(-12.0, 12.0, -2.0, -12.0, 12.0) + _quad(-3.0, 5.0, 0.1, -2.0, 6.0), np.float32)
    V, F = len(pos), len(fan)
    pm = np.zeros(4, PRIM_DTYPE)
    pm[0] = (0, F, 0, V, 0)       # the fan
    pm[1] = (F, 6, 0, V, 1)       # backdrop
    pm[2] = (0, F, 0, V, 2)       # the fan again, material 2
    pm[3] = (F + 6, 6, 0, V, 3)   # occluder
    mats = np.zeros(4, MAT_DTYPE)
    mats["pbrBaseColorFactor"] = [0.8, 0.8, 0.8, 1.0]
    mats["pbrBaseColorFactor"][[0, 2], 3] = strip_alpha
    for k in ("pbrBaseColorTexture", "metallicRoughnessTexture", "normalTexture", "emissiveTexture"):
        mats[k] = -1
    mats["roughnessFactor"] = 0.5
    nodes = np.zeros(4, NODE_DTYPE)
    nodes["worldMatrix"] = np.eye(4, dtype=np.float32).ravel()
    nodes["primMesh"] = [0, 1, 2, 3]
    lights = np.zeros(1, LIGHT_DTYPE)
    lights[0] = ((0, 12, 0), (1, 1, 1), 100.0, 0)
    return FlatScene(pos, np.tile(np.array([0, 1, 0], np.float32), (V, 1)), np.tile(np.array([1, 0, 0, 1], np.float32), (V, 1)),
                     np.zeros((V, 2), np.float32), np.arange(V, dtype=np.uint32), pm, mats, lights, nodes, [])


def _subset(flat, keep):
    out = copy.copy(flat)
    out.nodes = flat.nodes[list(keep)].copy()
    return out


def _fan_rays(n, seed):
    """Every ray sees whatever it can hit from above (+y).  In each run of 64: eight graze the strip plane from just above it, under
    0.5 to 6 degrees, so they run along the strips over many leaves; the rest point up (miss everything) or start under the strips and
    point down (the backdrop at once)."""
    rng = np.random.default_rng(seed)
    o = np.zeros((n, 3), np.float32)
    d = np.zeros((n, 3), np.float32)
    for i in range(n):
        k = i % 64
        if k % 8 == 3:
            ang = rng.uniform(0, 2 * np.pi)
            run, y0 = rng.uniform(3, 6), rng.uniform(0.05, 0.3)  # reaches the plane after `run` units, inside the fan
            dip = np.arcsin(y0 / run)
            d[i] = (np.cos(ang) * np.cos(dip), -np.sin(dip), np.sin(ang) * np.cos(dip))
            o[i] = np.array([rng.uniform(-6, 6), 0.0, rng.uniform(-6, 6)]) - run * d[i].astype(np.float64)
        elif k % 2:
            o[i] = (rng.uniform(-7, 7), rng.uniform(1, 3), rng.uniform(-7, 7))
            d[i] = (rng.uniform(-0.3, 0.3), 1.0, rng.uniform(-0.3, 0.3))
        else:
            o[i] = (rng.uniform(-7, 7), -0.5, rng.uniform(-7, 7))
            d[i] = (rng.uniform(-0.2, 0.2), -1.0, rng.uniform(-0.2, 0.2))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


def _both(r, call):
    """call() with the option at 0 and at 1 -> the two results, in that order"""
    from vkrt_amd import abi

    got = []
    for lend in (0, 1):
        r.set_option(abi.VKRT_OPT_WF_TRI_LEND, lend)
        got.append(call())
    return got


def _intersect(r, rays, **kw):
    import torch

    h = r.intersect(rays, **kw)
    torch.cuda.current_stream().synchronize()
    b = h.buffer.cpu().numpy()
    return {"t": b[:, 0].copy(), "u": b[:, 1].copy(), "v": b[:, 2].copy(), "ints": b[:, 3:].view(np.int32).copy(), "raw": b.view(np.uint32).copy()}


def _occluded(r, rays, **kw):
    import torch

    occ = r.occluded(rays, **kw)
    torch.cuda.current_stream().synchronize()
    return occ.cpu().numpy()


def _check_queries(r, orc, o, d, what, gid_map=None, **kw):
    """intersect and occluded of the rays, option 0 and 1, against the oracle's brute force (gid_map: oracle id -> library id)"""
    rays = Q._pack(o, d, 0.001, TMAX)
    t, u, v, gid, _ = orc.trace_rays(o, d, 0.001, TMAX, use_bvh=False)
    _, _, _, any_gid, _ = orc.trace_rays(o, d, 0.001, TMAX, any_hit=True, use_bvh=False)
    if gid_map is not None:
        gid = np.where(gid >= 0, gid_map[np.maximum(gid, 0)], -1).astype(np.int32)
    hits = _both(r, lambda: _intersect(r, rays, **kw))
    occs = _both(r, lambda: _occluded(r, rays, **kw))
    for lend in (0, 1):
        Q._assert_matches(hits[lend], t, u, v, gid, TMAX)
        assert np.array_equal(occs[lend], (any_gid >= 0).astype(np.int32)), (what, lend)
    assert np.array_equal(hits[0]["raw"], hits[1]["raw"]), what
    return gid


# ---- 1. the strip fan ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fan():
    import oracle_py

    flat = _strip_fan()
    return flat, oracle_py.OracleScene(flat)


@pytest.mark.parametrize("kind", KINDS)
def test_strip_fan_matches_the_oracle(fan, kind):
    """1, 7, 64 and 65 rays: lanes without a ray, and a second wave with one valid lane"""
    flat, orc = fan
    r = Q._renderer(flat, kind)
    o, d = _fan_rays(65, seed=3)
    seen = []
    for n in (1, 7, 64, 65):
        seen.append(_check_queries(r, orc, o[65 - n:], d[65 - n:], (kind, n)))
    gid = seen[-1]
    assert ((gid >= 0) & (gid < 96)).sum() >= 4 and (gid == -1).sum() >= 20 and ((gid == 96) | (gid == 97)).sum() >= 20  # grazing, up, down
    assert not np.any((gid >= 98) & (gid < 194))  # the tie of every pair goes to FAN_A
    r.close()


def test_strip_fan_many_waves(fan):
    """4099 rays: whole waves of the mix, every grazing ray with an occluder query that ends at some strip"""
    flat, orc = fan
    r = Q._renderer(flat, "ploc")
    o, d = _fan_rays(4099, seed=5)
    gid = _check_queries(r, orc, o, d, "many")
    assert ((gid >= 0) & (gid < 96)).sum() > 300 and ((gid == 194) | (gid == 195)).sum() > 30
    r.close()


# ---- 2. hostile rays ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nonuniform():
    import atrium
    import oracle_py

    flat, _ = atrium.build_atrium(20000, seed=4, variant="nonuniform")
    return flat, oracle_py.OracleScene(flat)


@pytest.mark.parametrize("name", ["soup", "nonuniform"])
def test_hostile_rays(nonuniform, name):
    import oracle_py
    from vkrt_amd import abi

    if name == "soup":
        flat = Q._triangle_soup()
        orc = oracle_py.OracleScene(flat)
    else:
        flat, orc = nonuniform
    r = Q._renderer(flat, "ploc")
    o, d = Q._hostile_rays(flat, 4096, seed=77)
    rays = Q._pack(o, d, 0.001, 10000.0)
    t, u, v, gid, _ = orc.trace_rays(o, d, 0.001, 10000.0, use_bvh=False)
    _, _, _, any_gid, _ = orc.trace_rays(o, d, 0.001, 10000.0, any_hit=True, use_bvh=False)
    assert (gid >= 0).mean() > 0.15
    for lend in (0, 1):
        r.set_option(abi.VKRT_OPT_WF_TRI_LEND, lend)
        Q._assert_matches(Q._intersect(r, rays), t, u, v, gid, 10000.0)
        assert np.array_equal(Q._occluded(r, rays), (any_gid >= 0).astype(np.int32))
    r.close()


# ---- 3. what travels with a loan ---------------------------------------------------------------------------------------------------
def test_dissolve_seed_follows_the_triangle():
    import oracle_py
    from vkrt_amd import abi

    flat = _strip_fan(strip_alpha=0.5)
    orc = oracle_py.OracleScene(flat)
    orc.set_dissolve(True)
    r = Q._renderer(flat, "ploc", options={abi.VKRT_OPT_ANYHIT_DISSOLVE: 1})
    o, d = _fan_rays(4099, seed=7)
    gid = _check_queries(r, orc, o, d, "dissolve", seed=0)
    assert ((gid >= 98) & (gid < 194)).sum() > 20  # FAN_B wins where the stage ignored FAN_A's twin: the decisions are per triangle
    r.close()


def test_watertight_constants_follow_the_ray(fan):
    import oracle_py
    from vkrt_amd import abi

    flat, _ = fan
    orc = oracle_py.OracleScene(flat)
    orc.set_watertight(True)
    r = Q._renderer(flat, "ploc", options={abi.VKRT_OPT_WATERTIGHT: 1})
    o, d = _fan_rays(4099, seed=9)
    _check_queries(r, orc, o, d, "watertight")
    r.close()


def test_cull_mask_and_facing_flag_follow_the_ray(fan):
    """FAN_B flipped (back-facing from above) and the occluder under mask bit 2: a query with cull mask 1 that culls back faces sees
    FAN_A and the backdrop, whose ids are the first 98 -- the oracle on those two nodes."""
    import oracle_py
    from vkrt_amd import abi

    flat, _ = fan
    orc = oracle_py.OracleScene(_subset(flat, [FAN_A, BACKDROP]))
    r = Q._renderer(flat, "ploc")
    r.set_instance_visibility(0, [1, 1, 1, 2], [0, 0, abi.VKRT_INSTANCE_FLIP_FACING, 0])
    o, d = _fan_rays(4099, seed=11)
    gid = _check_queries(r, orc, o, d, "filter", cull_mask=1, ray_flags=abi.VKRT_RAY_CULL_BACK_FACING)
    assert ((gid >= 0) & (gid < 96)).sum() > 300
    r.close()


def test_alpha_mask_follows_the_triangle():
    """FAN_A's material is MASK with a cutoff above its alpha: every candidate on it is ignored, FAN_B's twin is the hit -- the oracle
    on the other three nodes, whose ids lie 96 higher in the whole scene."""
    import oracle_py
    from vkrt_amd import abi

    flat = _strip_fan()
    flat.materials["pbrBaseColorFactor"][0, 3] = 0.25
    orc = oracle_py.OracleScene(_subset(flat, [BACKDROP, FAN_B, OCCLUDER]))
    r = Q._renderer(flat, "ploc")
    r.set_material_alpha(0, [abi.VKRT_ALPHA_MASK], 0.5)
    o, d = _fan_rays(4099, seed=13)
    gid = _check_queries(r, orc, o, d, "alpha", gid_map=np.arange(100) + 96)
    assert ((gid >= 98) & (gid < 194)).sum() > 300
    r.close()


# ---- 4. frames of the path tracer ---------------------------------------------------------------------------------------------------
W, H = 64, 48


@pytest.fixture(scope="module")
def frame(nonuniform):
    """the small non-uniform atrium, its renderer and the oracle's two frames of 2 spp, depth 3"""
    import atrium
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Renderer

    flat, orc = nonuniform
    cam = default_camera(W, H, **atrium.DEFAULT_CAMERA)
    refs = []
    img = None
    for f in range(2):
        pc = make_push_constants(samples=2, depth=3, frame=f, lights_count=len(flat.lights))
        img, c = orc.render(pc, cam, W, H, seed=21 + f, image=img.copy() if f else None, threads=THREADS)
        refs.append((img, c))
    r = Renderer(flat, device=0, build="ploc")
    yield flat, orc, cam, refs, r
    r.close()


def _frame_call(r, call):
    def run():
        r.reset_counters()
        img = call().cpu().numpy()
        return img, r.counters()

    return _both(r, run)


def test_frame_image_and_ray_counters(frame):
    from vkrt_amd.flat_scene import make_push_constants

    flat, orc, cam, refs, r = frame
    pc = make_push_constants(samples=2, depth=3, frame=0, lights_count=len(flat.lights))
    for lend, (img, c) in enumerate(_frame_call(r, lambda: r.pathtrace(pc, cam, W, H, seed=21))):
        assert np.array_equal(img.view(np.uint32), refs[0][0].view(np.uint32)), lend
        assert c["traversal_faults"] == 0
        for k in RAYS:
            assert c[k] == refs[0][1][k], (lend, k)
    got = _frame_call(r, lambda: r.pathtrace_frames(pc, cam, W, H, 2, seed=21))
    for lend, (img, c) in enumerate(got):
        assert np.array_equal(img.view(np.uint32), refs[1][0].view(np.uint32)), lend
        assert c["traversal_faults"] == 0
        for k in RAYS[:2]:
            assert c[k] == refs[0][1][k] + refs[1][1][k], (lend, k)
    assert got[0][1]["pair_records"] == got[1][1]["pair_records"]


def test_hybrid_frame(frame):
    """the hybrid pass on the library's own G-buffer: the two options leave the same bits and the same ray counts, and both stand to
    the oracle as the hybrid pass does everywhere (tests/test_hybrid.py: its shading differs from the oracle's in the last bits of a
    few pixels whatever the option)"""
    from vkrt_amd.flat_scene import make_push_constants

    flat, orc, cam, refs, r = frame
    g = r.gbuffer_raycast(cam, W, H)
    gnp = {k: v.cpu().numpy() for k, v in g.items()}
    pc = make_push_constants(samples=1, depth=3, frame=0, lights_count=len(flat.lights))
    pc.useShadows, pc.useAO, pc.useGI = 1, 1, 1
    ref, cref = orc.hybrid(pc, cam, W, H, gnp, seed=5, threads=THREADS)
    got = _frame_call(r, lambda: r.hybrid_trace(pc, cam, W, H, g, seed=5))
    assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32))
    for k in RAYS[:2] + ("traversal_faults",):
        assert got[0][1][k] == got[1][1][k], k
    differs = float(np.mean(np.any(got[1][0].view(np.uint32) != ref.view(np.uint32), axis=-1)))
    print(f"hybrid pixels that differ from the oracle in some bit: {differs:.4f}; rays {got[1][1]['rays_closest']} / {cref['rays_closest']}")
    assert np.array_equal(got[1][0].view(np.uint32), ref.view(np.uint32))


def test_lending_engages(frame):
    """fewer triangle wave-steps, each with more lanes testing: a switch that did nothing could not pass.  (This frame, option 0 -> 1:
    4231 -> 3237 triangle wave-steps, 0.526 -> 0.677 of the lanes testing: the room is there without the option.)"""
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants

    flat, orc, cam, refs, r = frame
    pc = make_push_constants(samples=2, depth=3, frame=0, lights_count=len(flat.lights))
    got = _frame_call(r, lambda: r.pathtrace(pc, cam, W, H, seed=21, flags=abi.VKRT_TRACE_COUNT_TRAVERSAL))
    eff = []
    for img, c in got:
        assert c["traversal_faults"] == 0 and c["wave_tri_steps"] > 0
        assert np.array_equal(img.view(np.uint32), refs[0][0].view(np.uint32))
        eff.append(c["tris_tested"] / (64.0 * c["wave_tri_steps"]))
    print(f"wave_tri_steps {got[0][1]['wave_tri_steps']} -> {got[1][1]['wave_tri_steps']}, lane efficiency {eff[0]:.3f} -> {eff[1]:.3f}")
    assert got[1][1]["wave_tri_steps"] < got[0][1]["wave_tri_steps"]
    assert eff[1] > eff[0]
