"""Batched ray queries on caller rays (vkrt_intersect / vkrt_occluded, Renderer.intersect / occluded) against the oracle.

The result of a query is the result the library's walks compute everywhere else (closest t in (tmin, tmax), ties to the smallest
flattened triangle id), so the checks demand bit-identical t, u, v and triangle ids: against the oracle's brute
force and tree walk and against the existing test hook vkrt_debug_trace_rays (Renderer.trace_rays)."""
import copy
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import default_camera
from scene_motion import _row_major, apply, moved

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KINDS = ("ploc", "lbvh", "sah")


def _triangle_soup(n=6000, seed=21):
    """Random triangles over five orders of magnitude in size, some needle-shaped, some degenerate (zero area), some exactly
    axis-aligned (zero-thickness boxes), in a 20-unit cube."""
    from vkrt_amd.flat_scene import LIGHT_DTYPE, MAT_DTYPE, NODE_DTYPE, PRIM_DTYPE, FlatScene

    rng = np.random.default_rng(seed)
    c = rng.uniform(-10, 10, (n, 3))
    size = 10.0 ** rng.uniform(-4, 1, (n, 1))
    a = c + rng.normal(size=(n, 3)) * size
    b = c + rng.normal(size=(n, 3)) * size
    d = c + rng.normal(size=(n, 3)) * size
    needle = rng.random(n) < 0.15
    d[needle] = a[needle] + (b[needle] - a[needle]) * 0.5 + rng.normal(size=(needle.sum(), 3)) * size[needle] * 1e-4
    flat_axis = rng.random(n) < 0.2
    ax = rng.integers(0, 3, n)
    for k in range(3):
        m = flat_axis & (ax == k)
        b[m, k] = a[m, k]
        d[m, k] = a[m, k]
    degen = rng.random(n) < 0.02
    d[degen] = b[degen]
    pos = np.stack([a, b, d], 1).reshape(-1, 3).astype(np.float32)
    V = pos.shape[0]
    pm = np.zeros(1, PRIM_DTYPE)
    pm[0] = (0, V, 0, V, 0)
    mats = np.zeros(1, MAT_DTYPE)
    mats[0]["pbrBaseColorFactor"] = [0.8, 0.8, 0.8, 1]
    mats[0]["pbrBaseColorTexture"] = mats[0]["metallicRoughnessTexture"] = mats[0]["normalTexture"] = mats[0]["emissiveTexture"] = -1
    mats[0]["roughnessFactor"] = 0.5
    nodes = np.zeros(1, NODE_DTYPE)
    nodes[0]["worldMatrix"] = np.eye(4, dtype=np.float32).ravel()
    lights = np.zeros(1, LIGHT_DTYPE)
    lights[0] = ((0, 12, 0), (1, 1, 1), 100.0, 0)
    return FlatScene(pos, np.tile(np.array([0, 1, 0], np.float32), (V, 1)), np.tile(np.array([1, 0, 0, 1], np.float32), (V, 1)),
                     np.zeros((V, 2), np.float32), np.arange(V, dtype=np.uint32), pm, mats, lights, nodes, [])


@pytest.fixture(scope="module")
def scenes():
    import atrium
    import oracle_py
    from vkrt_amd.flat_scene import FlatScene

    cornell = FlatScene.load_npz(os.path.join(ROOT, "tests", "golden", "cornell_flat.npz"))
    small, _ = atrium.build_atrium(20000, seed=4, with_textures=False)
    soup = _triangle_soup()
    return {name: (flat, oracle_py.OracleScene(flat)) for name, flat in (("cornell", cornell), ("atrium_small", small), ("soup", soup))}


def _world_bounds(flat):
    v = np.concatenate([(np.c_[flat.positions, np.ones(len(flat.positions))] @ _row_major(n["worldMatrix"]).T)[:, :3] for n in flat.nodes])
    return v.min(0), v.max(0)


def _hostile_rays(flat, n, seed):
    """Rays from around the scene: 10 % exactly axis-parallel, 10 % with one component ~1e-7, 20 % starting on a triangle."""
    rng = np.random.default_rng(seed)
    lo, hi = _world_bounds(flat)
    pad = 0.1 * (hi - lo) + 0.1
    o = rng.uniform(lo - pad, hi + pad, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32)
    axis = rng.integers(0, 3, n)
    par = rng.random(n) < 0.1
    d[par] = 0
    d[par, axis[par]] = np.where(rng.random(par.sum()) < 0.5, 1.0, -1.0)
    tiny = rng.random(n) < 0.1
    d[tiny, axis[tiny]] = (rng.uniform(-1, 1, tiny.sum()) * 1e-7).astype(np.float32)
    on = rng.random(n) < 0.2
    tri = _world_triangles(flat)
    k = rng.integers(0, len(tri), n)
    w = rng.dirichlet((1, 1, 1), n)
    o[on] = (tri[k[on]] * w[on][:, :, None]).sum(1).astype(np.float32)
    return o, d


def _flattened(flat):
    """Per flattened triangle id: (instance, primitive, prim_mesh, material) -- nodes in order, each node's primMesh triangles in order."""
    rows = []
    for i, node in enumerate(flat.nodes):
        pm = flat.prim_meshes[node["primMesh"]]
        cnt = int(pm["indexCount"]) // 3
        rows.append(np.stack([np.full(cnt, i), np.arange(cnt), np.full(cnt, node["primMesh"]), np.full(cnt, max(0, int(pm["materialIndex"])))], 1))
    return np.concatenate(rows).astype(np.int32)


def _world_triangles(flat):
    """float64 [T, 3, 3]: every flattened triangle's vertices, transformed by its node's matrix."""
    out = []
    for node in flat.nodes:
        pm = flat.prim_meshes[node["primMesh"]]
        idx = flat.indices[int(pm["firstIndex"]): int(pm["firstIndex"]) + int(pm["indexCount"])].astype(np.int64) + int(pm["vertexOffset"])
        p = np.c_[flat.positions[idx].astype(np.float64), np.ones(len(idx))] @ _row_major(node["worldMatrix"]).T
        out.append(p[:, :3].reshape(-1, 3, 3))
    return np.concatenate(out)


def _pack(o, d, tmin, tmax):
    import torch
    from vkrt_amd.renderer import pack_rays

    dev = "cuda:0"
    to = lambda x: torch.as_tensor(np.asarray(x, np.float32), device=dev) if np.ndim(x) else float(x)  # noqa: E731
    return pack_rays(torch.as_tensor(o, device=dev), torch.as_tensor(d, device=dev), tmin=to(tmin), tmax=to(tmax))


def _intersect(r, rays, seed=0):
    import torch

    h = r.intersect(rays, seed=seed)
    torch.cuda.current_stream().synchronize()
    b = h.buffer.cpu().numpy()
    return {"t": b[:, 0].copy(), "u": b[:, 1].copy(), "v": b[:, 2].copy(), "ints": b[:, 3:].view(np.int32).copy(), "raw": b.view(np.uint32).copy()}


def _occluded(r, rays, seed=0):
    import torch

    occ = r.occluded(rays, seed=seed)
    torch.cuda.current_stream().synchronize()
    return occ.cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _assert_matches(h, t, u, v, gid, tmax):
    """h (an intersect result) against a (t, u, v, gid) reference: ids everywhere, t/u/v bit for bit on hits, the contract on misses."""
    tri = h["ints"][:, 3]
    assert np.array_equal(tri, gid), np.nonzero(tri != gid)[0][:10]
    hit = gid >= 0
    for a, b in ((h["t"], t), (h["u"], u), (h["v"], v)):
        assert np.array_equal(_bits(a[hit]), _bits(b[hit]))
    miss = ~hit
    assert np.array_equal(_bits(h["t"][miss]), _bits(np.broadcast_to(np.float32(tmax), gid.shape)[miss]))
    assert np.all(h["u"][miss] == 0) and np.all(h["v"][miss] == 0)
    assert np.all(h["ints"][miss] == -1)


def _renderer(flat, kind, layout=1, options=None):
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer

    opts = {abi.VKRT_OPT_BVH_LAYOUT: layout}
    opts.update(options or {})
    return Renderer(flat, device=0, build=kind, options=opts)


# ---- 1. closest hits: oracle brute force, oracle tree walk, vkrt_debug_trace_rays ----------------------------------------------
@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["cornell", "soup"])
def test_closest_hit_equals_oracle_and_trace_rays(scenes, name, kind, layout):
    flat, orc = scenes[name]
    r = _renderer(flat, kind, layout)
    o, d = _hostile_rays(flat, 60001, seed=5)  # (not a multiple of 64)
    h = _intersect(r, _pack(o, d, 0.001, 10000.0))
    bt, bu, bv, bg, _ = orc.trace_rays(o, d, 0.001, 10000.0, use_bvh=False)
    assert (bg >= 0).mean() > 0.2
    _assert_matches(h, bt, bu, bv, bg, 10000.0)
    vt, vu, vv, vg, _ = orc.trace_rays(o, d, 0.001, 10000.0, use_bvh=True)
    _assert_matches(h, vt, vu, vv, vg, 10000.0)
    gt, gu, gv, gg = r.trace_rays(o, d, 0.001, 10000.0)
    _assert_matches(h, gt, gu, gv, gg, 10000.0)
    r.close()


@pytest.mark.parametrize("kind,layout", [("ploc", 1), ("lbvh", 0), ("sah", 1)])
def test_million_rays_on_the_atrium(scenes, kind, layout):
    """1,000,003 rays (not a multiple of 64) on the small atrium: the oracle's tree walk, the test hook, and brute force on a slice."""
    flat, orc = scenes["atrium_small"]
    r = _renderer(flat, kind, layout)
    n = 1_000_003
    o, d = _hostile_rays(flat, n, seed=9)
    h = _intersect(r, _pack(o, d, 0.001, 10000.0))
    vt, vu, vv, vg, _ = orc.trace_rays(o, d, 0.001, 10000.0, use_bvh=True)
    assert (vg >= 0).mean() > 0.15
    _assert_matches(h, vt, vu, vv, vg, 10000.0)
    gt, gu, gv, gg = r.trace_rays(o, d, 0.001, 10000.0)
    _assert_matches(h, gt, gu, gv, gg, 10000.0)
    sl = slice(n - 3001, n)  # the tail, past the last whole wave
    bt, bu, bv, bg, _ = orc.trace_rays(o[sl], d[sl], 0.001, 10000.0, use_bvh=False)
    _assert_matches({k: x[sl] for k, x in h.items()}, bt, bu, bv, bg, 10000.0)
    r.close()


# ---- 2. per-ray bounds -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("name", ["cornell", "atrium_small", "soup"])
def test_per_ray_bounds(scenes, name, layout):
    """Four (tmin, tmax) pairs in one call, one with tmax = +inf: each group equals the oracle called with its pair.  Groups dealt at
    random (every wave mixes bounds) and in runs (most waves share one tmin)."""
    flat, orc = scenes[name]
    r = _renderer(flat, "ploc", layout)
    pairs = [(0.001, 10000.0), (0.0, 2.5), (0.5, float("inf")), (1.0, 3.0)]
    n = 40000
    o, d = _hostile_rays(flat, n, seed=13)
    rng = np.random.default_rng(14)
    for g in (rng.integers(0, 4, n), np.repeat(np.arange(4), n // 4)):
        tmin = np.array([pairs[k][0] for k in g], np.float32)
        tmax = np.array([pairs[k][1] for k in g], np.float32)
        rays = _pack(o, d, tmin, tmax)
        h = _intersect(r, rays)
        occ = _occluded(r, rays)
        for k, (lo, hi) in enumerate(pairs):
            m = g == k
            t, u, v, gid, _ = orc.trace_rays(o[m], d[m], lo, hi, use_bvh=True)
            _assert_matches({key: x[m] for key, x in h.items()}, t, u, v, gid, hi)
            _, _, _, any_gid, _ = orc.trace_rays(o[m], d[m], lo, hi, any_hit=True, use_bvh=True)
            assert np.array_equal(occ[m], (any_gid >= 0).astype(np.int32))
    r.close()


# ---- 3. instance, primitive, prim_mesh, material and the hit point ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "atrium_small"])
def test_hit_attributes_and_hit_point(scenes, name):
    flat, orc = scenes[name]
    r = _renderer(flat, "ploc")
    o, d = _hostile_rays(flat, 50000, seed=17)
    h = _intersect(r, _pack(o, d, 0.001, 10000.0))
    table = _flattened(flat)
    _, ids = orc.triangles()
    assert np.array_equal(ids[:, 1], table[:, 0]) and np.array_equal(ids[:, 2], table[:, 1])  # the oracle's (inst, prim) per gid
    ints = h["ints"]
    tri = ints[:, 3]
    hit = tri >= 0
    assert hit.mean() > 0.15
    assert np.array_equal(ints[hit][:, [0, 1, 2, 4]], table[tri[hit]])
    assert np.all(ints[~hit] == -1) and np.all(h["t"][~hit] == np.float32(10000.0))
    W = _world_triangles(flat)[tri[hit]]
    u, v, t = h["u"][hit].astype(np.float64), h["v"][hit].astype(np.float64), h["t"][hit].astype(np.float64)
    p_tri = W[:, 0] * (1 - u - v)[:, None] + W[:, 1] * u[:, None] + W[:, 2] * v[:, None]
    p_ray = o[hit].astype(np.float64) + t[:, None] * d[hit].astype(np.float64)
    # (grazing hits excluded: there t carries the rounding of the edge vectors divided by the cosine of incidence)
    nrm = np.cross(W[:, 1] - W[:, 0], W[:, 2] - W[:, 0])
    dn = d[hit].astype(np.float64)
    cos = np.abs((nrm * dn).sum(1)) / (np.linalg.norm(nrm, axis=1) * np.linalg.norm(dn, axis=1) + 1e-300)
    ok = cos > 0.05
    assert ok.mean() > 0.5
    scale = 1.0 + np.abs(o[hit]).max(1) + t
    assert np.all((np.abs(p_tri - p_ray).max(1) <= 1e-4 * scale)[ok])
    r.close()


# ---- 4. occlusion --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("kind", KINDS)
def test_occluded_equals_oracle_any_hit(scenes, kind, layout):
    flat, orc = scenes["soup"]
    r = _renderer(flat, kind, layout)
    o, d = _hostile_rays(flat, 30001, seed=19)
    rays = _pack(o, d, 0.001, 7.5)
    occ = _occluded(r, rays)
    _, _, _, ba, _ = orc.trace_rays(o, d, 0.001, 7.5, any_hit=True, use_bvh=False)
    assert 0.05 < (ba >= 0).mean() < 0.95
    assert np.array_equal(occ, (ba >= 0).astype(np.int32))
    h = _intersect(r, rays)
    assert np.array_equal(occ, (h["ints"][:, 3] >= 0).astype(np.int32))
    r.close()


# ---- 5. rays that miss without a walk --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 0])
def test_degenerate_rays_are_misses_without_faults(scenes, layout):
    flat, orc = scenes["cornell"]
    r = _renderer(flat, "ploc", layout)
    n = 4096
    o, d = _hostile_rays(flat, n, seed=23)
    tmin = np.full(n, 0.001, np.float32)
    tmax = np.full(n, 10000.0, np.float32)
    kind = np.arange(n) % 8  # 0 and 1 stay valid, the rest are rejected; every wave mixes them
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    tmin[kind == 2] = -0.5
    tmin[kind == 3] = tmax[kind == 3] = 5.0
    d[kind == 4] = 0.0
    o[kind == 5, 1] = nan
    d[kind == 6, 2] = inf
    o[kind == 7, 0] = -inf
    tmax[(kind == 3) & (np.arange(n) % 16 == 11)] = nan
    r.reset_counters()
    rays = _pack(o, d, tmin, tmax)
    h = _intersect(r, rays)
    occ = _occluded(r, rays)
    bad = kind >= 2
    assert np.all(h["ints"][bad] == -1) and np.all(h["u"][bad] == 0) and np.all(h["v"][bad] == 0)
    assert np.array_equal(_bits(h["t"][bad]), _bits(tmax[bad]))
    assert np.all(occ[bad] == 0)
    good = ~bad
    t, u, v, gid, _ = orc.trace_rays(o[good], d[good], 0.001, 10000.0, use_bvh=False)
    _assert_matches({k: x[good] for k, x in h.items()}, t, u, v, gid, 10000.0)
    c = r.counters()
    assert c["traversal_faults"] == 0
    assert all(c[k] == 0 for k in ("rays_closest", "rays_shadow", "hits", "pixels", "nodes_visited", "tris_tested")), c
    r.close()


# ---- 6. triangle modes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 0])
def test_watertight_mode_matches_oracle(scenes, layout):
    import oracle_py
    from vkrt_amd import abi

    flat, _ = scenes["soup"]
    orc = oracle_py.OracleScene(flat)
    orc.set_watertight(True)
    r = _renderer(flat, "ploc", layout, {abi.VKRT_OPT_WATERTIGHT: 1})
    o, d = _hostile_rays(flat, 30001, seed=29)
    rays = _pack(o, d, 0.001, 10000.0)
    h = _intersect(r, rays)
    t, u, v, gid, _ = orc.trace_rays(o, d, 0.001, 10000.0, use_bvh=False)
    _assert_matches(h, t, u, v, gid, 10000.0)
    _, _, _, ag, _ = orc.trace_rays(o, d, 0.001, 7.5, any_hit=True, use_bvh=False)
    assert np.array_equal(_occluded(r, _pack(o, d, 0.001, 7.5)), (ag >= 0).astype(np.int32))
    r.close()


def _dissolving(flat):
    """The scene with its materials half transparent: alpha 0.5, one of them 0 (always ignored) and one opaque."""
    out = copy.copy(flat)
    out.materials = flat.materials.copy()
    a = np.full(len(out.materials), 0.5, np.float32)
    a[0] = 1.0
    if len(a) > 2:
        a[2] = 0.0
    out.materials["pbrBaseColorFactor"][:, 3] = a
    return out


@pytest.mark.parametrize("layout", [1, 0])
def test_dissolve_mode_matches_oracle_and_seeds_are_deterministic(scenes, layout):
    import oracle_py
    from vkrt_amd import abi

    flat = _dissolving(scenes["cornell"][0])
    orc = oracle_py.OracleScene(flat)
    orc.set_dissolve(True)
    r = _renderer(flat, "ploc", layout, {abi.VKRT_OPT_ANYHIT_DISSOLVE: 1})
    o, d = _hostile_rays(flat, 30001, seed=31)
    rays = _pack(o, d, 0.001, 10000.0)
    h = _intersect(r, rays, seed=0)
    t, u, v, gid, _ = orc.trace_rays(o, d, 0.001, 10000.0, use_bvh=False)
    _assert_matches(h, t, u, v, gid, 10000.0)
    _, _, _, ag, _ = orc.trace_rays(o, d, 0.001, 10000.0, any_hit=True, use_bvh=False)
    assert np.array_equal(_occluded(r, rays, seed=0), (ag >= 0).astype(np.int32))
    h1, h2 = _intersect(r, rays, seed=12345), _intersect(r, rays, seed=12345)
    assert np.array_equal(h1["raw"], h2["raw"])
    assert not np.array_equal(h1["raw"], h["raw"])  # the seed reaches the any-hit stage
    o1, o2 = _occluded(r, rays, seed=777), _occluded(r, rays, seed=777)
    assert np.array_equal(o1, o2)
    assert np.array_equal(o1, (_intersect(r, rays, seed=777)["ints"][:, 3] >= 0).astype(np.int32))
    r.close()


# ---- 7. stream order -----------------------------------------------------------------------------------------------------------
def test_queries_are_ordered_on_the_callers_stream(scenes):
    import torch
    from vkrt_amd.renderer import pack_rays

    flat, orc = scenes["atrium_small"]
    r = _renderer(flat, "ploc")
    n = 200003
    side = torch.cuda.Stream(device=0)
    hits_buf = torch.empty((n, 8), dtype=torch.float32, device="cuda:0")
    occ_buf = torch.empty((n,), dtype=torch.int32, device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    for rep in range(3):
        o, d = _hostile_rays(flat, n, seed=40 + rep)
        o_h, d_h = torch.from_numpy(o).pin_memory(), torch.from_numpy(d).pin_memory()
        with torch.cuda.stream(side):
            busy = torch.randn(2048, 2048, device="cuda:0")
            for _ in range(4):
                busy = busy @ busy * 1e-3  # work in front of the ray writes on the same stream
            rays = pack_rays(o_h.to("cuda:0", non_blocking=True) + busy[0, 0] * 0, d_h.to("cuda:0", non_blocking=True), tmin=0.001, tmax=10000.0)
            h = r.intersect(rays, out=hits_buf, stream=side)
            occ = r.occluded(rays, out=occ_buf, stream=side)
        assert h.buffer.data_ptr() == hits_buf.data_ptr() and occ.data_ptr() == occ_buf.data_ptr()
        side.synchronize()
        b = hits_buf.cpu().numpy()
        res = {"t": b[:, 0], "u": b[:, 1], "v": b[:, 2], "ints": b[:, 3:].view(np.int32)}
        t, u, v, gid, _ = orc.trace_rays(o, d, 0.001, 10000.0, use_bvh=True)
        _assert_matches(res, t, u, v, gid, 10000.0)
        assert np.array_equal(occ_buf.cpu().numpy(), (gid >= 0).astype(np.int32))
        assert np.array_equal(h.triangle.cpu().numpy(), gid)
    r.close()


# ---- 8. moved instances ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "atrium_small"])
def test_refit_scene_answers_like_a_fresh_build(scenes, name):
    flat, _ = scenes[name]
    if name == "cornell":
        mv, mats = moved(flat, [len(flat.nodes) - 2, len(flat.nodes) - 1], 11, mirror_first=False, scale=False)
    else:
        idx = np.sort(np.random.default_rng(23).choice(len(flat.nodes), len(flat.nodes) // 3, replace=False))
        mv, mats = moved(flat, idx, 23)
    r = _renderer(flat, "ploc")
    apply(r, mats)
    r.refit()
    fresh = _renderer(mv, "ploc")
    o, d = _hostile_rays(mv, 60001, seed=47)
    rays = _pack(o, d, 0.001, 10000.0)
    a, b = _intersect(r, rays), _intersect(fresh, rays)
    assert np.array_equal(a["raw"], b["raw"])
    assert np.array_equal(_occluded(r, rays), _occluded(fresh, rays))
    assert (a["ints"][:, 3] >= 0).mean() > 0.15
    r.close()
    fresh.close()


# ---- 9. error paths --------------------------------------------------------------------------------------------------------------
def test_error_paths(scenes):
    import torch
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer, VkrtError

    flat, _ = scenes["cornell"]
    o, d = _hostile_rays(flat, 256, seed=53)
    rays = _pack(o, d, 0.001, 10000.0)
    hits = torch.empty((256, 8), dtype=torch.float32, device="cuda:0")
    occ = torch.empty((256,), dtype=torch.int32, device="cuda:0")
    unbuilt = Renderer(flat, device=0, build=None)
    lib = unbuilt.lib
    for fn, out in ((lib.vkrt_intersect, hits), (lib.vkrt_occluded, occ)):
        assert fn(unbuilt._h, rays.data_ptr(), 256, 0, out.data_ptr(), None) == abi.VKRT_ERR_NOT_BUILT
        assert fn(unbuilt._h, rays.data_ptr(), 0, 0, out.data_ptr(), None) == abi.VKRT_OK  # n == 0: nothing is enqueued
    with pytest.raises(VkrtError):
        unbuilt.intersect(rays)
    unbuilt.close()
    r = _renderer(flat, "ploc")
    h = r._h
    assert lib.vkrt_intersect(h, rays.data_ptr(), 0, 0, None, None) == abi.VKRT_OK
    assert lib.vkrt_occluded(h, None, 0, 0, None, None) == abi.VKRT_OK
    empty = r.intersect(torch.empty((0, 8), dtype=torch.float32, device="cuda:0"))
    assert empty.t.numel() == 0
    # misaligned: rays and hits need 16 bytes, occluded flags 4
    assert lib.vkrt_intersect(h, rays.data_ptr() + 4, 255, 0, hits.data_ptr(), None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert lib.vkrt_intersect(h, rays.data_ptr(), 255, 0, hits.data_ptr() + 8, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert lib.vkrt_occluded(h, rays.data_ptr() + 8, 255, 0, occ.data_ptr(), None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert lib.vkrt_occluded(h, rays.data_ptr(), 255, 0, occ.data_ptr() + 2, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert lib.vkrt_intersect(h, None, 256, 0, hits.data_ptr(), None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert lib.vkrt_occluded(h, rays.data_ptr(), 256, 0, None, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    with pytest.raises(VkrtError):
        r.intersect(rays.cpu())
    with pytest.raises(VkrtError):
        r.intersect(rays, out=torch.empty((255, 8), dtype=torch.float32, device="cuda:0"))
    if torch.cuda.device_count() > 1:
        with pytest.raises(VkrtError):
            r.occluded(rays.to("cuda:1"))
    # stale after update_nodes, traceable again after the refit
    r.update_nodes(len(flat.nodes) - 1, flat.nodes["worldMatrix"][-1:])
    assert lib.vkrt_intersect(h, rays.data_ptr(), 256, 0, hits.data_ptr(), None) == abi.VKRT_ERR_NOT_BUILT
    assert b"vkrt_scene_update_nodes" in lib.vkrt_last_error()
    assert lib.vkrt_occluded(h, rays.data_ptr(), 256, 0, occ.data_ptr(), None) == abi.VKRT_ERR_NOT_BUILT
    r.refit()
    assert lib.vkrt_intersect(h, rays.data_ptr(), 256, 0, hits.data_ptr(), None) == abi.VKRT_OK
    torch.cuda.synchronize()
    r.close()


# ---- 10. the existing pipelines are untouched ------------------------------------------------------------------------------------
def test_config1_image_unchanged_by_queries(scenes):
    from vkrt_amd.flat_scene import make_push_constants

    flat, _ = scenes["cornell"]
    W = H = 256
    cam = default_camera(W, H)
    pc = make_push_constants(samples=1, depth=1, frame=0, lights_count=len(flat.lights))

    def digest(r):
        return hashlib.sha256(r.pathtrace(pc, cam, W, H, seed=0).cpu().numpy().tobytes()).hexdigest()

    r = _renderer(flat, "ploc")
    before = digest(r)
    o, d = _hostile_rays(flat, 100000, seed=59)
    rays = _pack(o, d, 0.001, 10000.0)
    _intersect(r, rays)
    _occluded(r, rays)
    assert digest(r) == before
    other = _renderer(flat, "ploc")
    assert digest(other) == before
    r.close()
    other.close()
