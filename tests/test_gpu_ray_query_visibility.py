"""Instance visibility and ray flags of the ray queries (vkrt_scene_set_instance_visibility, vkrt_intersect_ex / vkrt_occluded_ex).

The filter is a pure function of (ray, triangle), so a filtered query must equal, bit for bit, an unfiltered query on a scene that holds
exactly the admitted triangles: the instances whose mask meets the cull mask, or per instance the triangles whose facing (object space,
decided here in float64) the ray flags keep.  Flattened ids are node-major, so the sub-scene's ids map back in order."""
import copy
import os

import numpy as np
import pytest

from scene_motion import _row_major, apply, moved

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("ploc", "lbvh", "sah")
CONFIGS = [(k, lay, wt, sp) for k in KINDS for lay in (1, 0) for wt in (0, 1) for sp in (0, -1)]
BACK, FRONT, OPAQUE = 0x10, 0x20, 0x1


def _instanced_scene(seed=3, meshes=6, tris=250, nodes=22, alpha=None):
    """Well-shaped triangles (no slivers: facing is well defined) in `meshes` primitive-meshes, instanced by `nodes` nodes with random
    rotations, non-uniform scales and translations; every third node mirrors."""
    from vkrt_amd.flat_scene import LIGHT_DTYPE, MAT_DTYPE, NODE_DTYPE, PRIM_DTYPE, FlatScene

    rng = np.random.default_rng(seed)
    pos, pms = [], np.zeros(meshes, PRIM_DTYPE)
    eq = np.array([[1, 0, 0], [-0.5, 0.866, 0], [-0.5, -0.866, 0]])
    for m in range(meshes):
        c = rng.uniform(-1, 1, (tris, 1, 3))
        q, _ = np.linalg.qr(rng.normal(size=(tris, 3, 3)))
        p = c + rng.uniform(0.05, 0.3, (tris, 1, 1)) * np.einsum("kj,tij->tki", eq, q)
        base = sum(len(x) for x in pos)
        pos.append(p.reshape(-1, 3))
        pms[m] = (base, 3 * tris, 0, base + 3 * tris, m % 4)
    pos = np.concatenate(pos).astype(np.float32)
    # (vertexOffset 0 with firstIndex = the mesh's first vertex: indices are absolute)
    V = len(pos)
    mats = np.zeros(4, MAT_DTYPE)
    for k in range(4):
        mats[k]["pbrBaseColorFactor"] = [0.8, 0.6, 0.4, 1.0 if alpha is None else alpha[k]]
        mats[k]["pbrBaseColorTexture"] = mats[k]["metallicRoughnessTexture"] = mats[k]["normalTexture"] = mats[k]["emissiveTexture"] = -1
        mats[k]["roughnessFactor"] = 0.5
    nd = np.zeros(nodes, NODE_DTYPE)
    for i in range(nodes):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        S = np.diag(rng.uniform(0.7, 1.3, 3) * (np.array([-1, 1, 1]) if i % 3 == 0 else 1))
        M = np.eye(4)
        M[:3, :3] = q @ S
        M[:3, 3] = [rng.uniform(-6, 6), rng.uniform(-2, 2), rng.uniform(-6, 6)]
        nd[i]["worldMatrix"] = np.ascontiguousarray(M.T.reshape(16), np.float32)
        nd[i]["primMesh"] = i % meshes
    lights = np.zeros(1, LIGHT_DTYPE)
    lights[0] = ((0, 12, 0), (1, 1, 1), 100.0, 0)
    return FlatScene(pos, np.tile(np.array([0, 1, 0], np.float32), (V, 1)), np.tile(np.array([1, 0, 0, 1], np.float32), (V, 1)),
                     np.zeros((V, 2), np.float32), np.arange(V, dtype=np.uint32), pms, mats, lights, nd, [])


@pytest.fixture(scope="module")
def scene():
    return _instanced_scene()


def _renderer(flat, kind="ploc", layout=1, wt=0, split=-1, dissolve=0, extra=None):
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer

    return Renderer(flat, device=0, build=kind, options={abi.VKRT_OPT_BVH_LAYOUT: layout, abi.VKRT_OPT_WATERTIGHT: wt,
                                                         abi.VKRT_OPT_SPLIT_BUDGET: split, abi.VKRT_OPT_ANYHIT_DISSOLVE: dissolve, **(extra or {})})


def _node_tris(flat, i):
    """object-space float64 [n, 3, 3] of node i's triangles"""
    pm = flat.prim_meshes[flat.nodes[i]["primMesh"]]
    idx = flat.indices[int(pm["firstIndex"]): int(pm["firstIndex"]) + int(pm["indexCount"])].astype(np.int64) + int(pm["vertexOffset"])
    return flat.positions[idx].astype(np.float64).reshape(-1, 3, 3)


def _world(flat):
    out = []
    for i, node in enumerate(flat.nodes):
        p = _node_tris(flat, i).reshape(-1, 3)
        out.append((np.c_[p, np.ones(len(p))] @ _row_major(node["worldMatrix"]).T)[:, :3].reshape(-1, 3, 3))
    return np.concatenate(out)


def _offsets(flat):
    cnt = [int(flat.prim_meshes[n["primMesh"]]["indexCount"]) // 3 for n in flat.nodes]
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)


def _query(r, rays, **kw):
    import torch

    h = r.intersect(rays, **kw)
    occ = r.occluded(rays, **kw)
    torch.cuda.current_stream().synchronize()
    b = h.buffer.cpu().numpy()
    return b[:, :3].view(np.uint32).copy(), b[:, 3:].view(np.int32).copy(), occ.cpu().numpy().copy()


def _pack(o, d, tmin, tmax):
    import torch
    from vkrt_amd.renderer import pack_rays

    to = lambda x: torch.as_tensor(np.asarray(x, np.float32), device="cuda:0") if np.ndim(x) else float(x)  # noqa: E731
    return pack_rays(torch.as_tensor(np.asarray(o, np.float32), device="cuda:0"), torch.as_tensor(np.asarray(d, np.float32), device="cuda:0"),
                     tmin=to(tmin), tmax=to(tmax))


def _ray_sets(flat, seed):
    """{name: packed rays}: camera rays, cosine-diffuse rays from their hits, shadow segments from those hits to a point light; each
    with one shared tmin and with per-ray tmin."""
    import torch

    rng = np.random.default_rng(seed)
    n = 6000
    eye = np.array([0.0, 9.0, 16.0])
    target = rng.uniform([-6, -2, -6], [6, 2, 6], (n, 3))
    d = target - eye
    cam = _pack(np.broadcast_to(eye, (n, 3)), d / np.linalg.norm(d, axis=1, keepdims=True), 0.001, 1e4)
    r = _renderer(flat)
    h = r.intersect(cam)
    torch.cuda.current_stream().synchronize()
    b = h.buffer.cpu().numpy()
    tri = b[:, 3:].view(np.int32)[:, 3]
    hit = tri >= 0
    r.close()
    W = _world(flat)[tri[hit]]
    p = eye + b[hit, 0:1].astype(np.float64) * (cam.cpu().numpy()[hit, 4:7])
    nrm = np.cross(W[:, 1] - W[:, 0], W[:, 2] - W[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    dd = cam.cpu().numpy()[hit, 4:7]
    nrm[(nrm * dd).sum(1) > 0] *= -1
    a = rng.normal(size=nrm.shape)
    t1 = np.cross(nrm, a)
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(nrm, t1)
    u1, u2 = rng.random(len(nrm)), rng.random(len(nrm))
    rr, ph = np.sqrt(u1), 2 * np.pi * u2
    diff = t1 * (rr * np.cos(ph))[:, None] + t2 * (rr * np.sin(ph))[:, None] + nrm * np.sqrt(1 - u1)[:, None]
    light = rng.uniform([-8, 4, -8], [8, 10, 8], (len(p), 3))
    m = len(p)
    tmin_r = rng.uniform(0.0, 2.0, n).astype(np.float32)
    return {"camera": cam, "camera_tmin": _pack(np.broadcast_to(eye, (n, 3)), cam.cpu().numpy()[:, 4:7], tmin_r, 1e4),
            "diffuse": _pack(p, diff, 0.001, 1e4), "diffuse_tmin": _pack(p, diff, rng.uniform(0, 0.5, m), 1e4),
            "shadow": _pack(p, light - p, 0.001, 0.999), "shadow_tmin": _pack(p, light - p, rng.uniform(0, 0.3, m), 0.999)}


def _subset(flat, keep):
    """the scene with nodes `keep` only (in order) and the map sub-gid -> full gid"""
    sub = copy.copy(flat)
    sub.nodes = flat.nodes[np.asarray(keep, np.int64)].copy()
    off = _offsets(flat)
    gmap = np.concatenate([np.arange(off[i], off[i + 1]) for i in keep] + [np.zeros(0, np.int64)])
    return sub, np.asarray(keep, np.int64), gmap


def _assert_same(full, ref, nodemap, gmap, prim_of=None):
    """full = _query of the filtered call, ref = _query of the sub-scene; ids of ref mapped back to the full scene"""
    (fb, fi, fo), (rb, ri, ro) = full, ref
    assert np.array_equal(fb, rb), np.nonzero((fb != rb).any(1))[0][:10]
    hit = ri[:, 3] >= 0
    assert np.array_equal(fi[:, 3] >= 0, hit)
    assert np.all(fi[~hit] == -1)
    assert np.array_equal(fi[hit, 0], nodemap[ri[hit, 0]])
    assert np.array_equal(fi[hit, 3], gmap[ri[hit, 3]])
    if prim_of is None:
        assert np.array_equal(fi[hit][:, [1, 2, 4]], ri[hit][:, [1, 2, 4]])
    else:
        assert np.array_equal(fi[hit, 1], prim_of[ri[hit, 3]])
        assert np.array_equal(fi[hit, 4], ri[hit, 4])
    assert np.array_equal(fo, ro)


_REF = {}


def _reference(flat, key, keep, rays, wt):
    """unfiltered results of the sub-scene (ploc, wide8, the same triangle test), cached per (key, wt, ray set)"""
    k = (key, wt)
    if k not in _REF:
        sub, nodemap, gmap = _subset(flat, keep)
        r = _renderer(sub, wt=wt)
        _REF[k] = ({name: _query(r, ry) for name, ry in rays.items()}, nodemap, gmap)
        r.close()
    return _REF[k]


def _masks(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 256, n).astype(np.uint8), rng.integers(0, 4, n).astype(np.uint8)


CULLS = (0x01, 0x12, 0x80, 0xA5, 0xFF)


# ---- 1. the defaults are today's calls ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,layout,wt,split", CONFIGS)
def test_defaults_and_any_visibility_leave_the_existing_calls_alone(scene, kind, layout, wt, split):
    rays = _ray_sets(scene, 1)
    r = _renderer(scene, kind, layout, wt, split)
    base = {k: _query(r, v) for k, v in rays.items()}
    masks, flags = _masks(len(scene.nodes), 2)
    r.set_instance_visibility(0, masks, flags)
    for k, v in rays.items():
        # the existing pair, under any visibility
        for a, b in zip(_query(r, v), base[k]):
            assert np.array_equal(a, b)
        # _ex with {0, 0xFF} through the library (the Python defaults call vkrt_intersect itself)
        import ctypes as C
        import torch
        from vkrt_amd import abi

        hits = torch.empty((v.shape[0], 8), dtype=torch.float32, device="cuda:0")
        occ = torch.empty((v.shape[0],), dtype=torch.int32, device="cuda:0")
        o = abi.QueryOpts(16, 0, 0xFF, 0)
        assert r.lib.vkrt_intersect_ex(r._h, C.c_void_p(v.data_ptr()), v.shape[0], C.byref(o), C.c_void_p(hits.data_ptr()), None) == 0
        assert r.lib.vkrt_occluded_ex(r._h, C.c_void_p(v.data_ptr()), v.shape[0], C.byref(o), C.c_void_p(occ.data_ptr()), None) == 0
        torch.cuda.synchronize()
        hb = hits.cpu().numpy()
        assert np.array_equal(hb[:, :3].view(np.uint32), base[k][0]) and np.array_equal(hb[:, 3:].view(np.int32), base[k][1])
        assert np.array_equal(occ.cpu().numpy(), base[k][2])
    r.close()


def test_visibility_leaves_pathtrace_and_hybrid_pixels_and_counters_alone():
    import torch

    from conftest import default_camera
    from vkrt_amd.flat_scene import FlatScene, make_push_constants

    flat = FlatScene.load_npz(os.path.join(ROOT, "tests", "golden", "cornell_flat.npz"))
    W = H = 48
    cam = default_camera(W, H)

    def frame(r):
        pc = make_push_constants(samples=2, depth=3, frame=0, lights_count=len(flat.lights))
        r.reset_counters()
        img = r.pathtrace(pc, cam, W, H, seed=7, flags=2).cpu().numpy().copy()
        # (wave_node_steps / wave_tri_steps count steps per wave: they follow the order of the compacted streams, not the rays alone)
        cnt = {k: v for k, v in r.counters().items() if not k.startswith("wave_")}
        gb = r.gbuffer_raycast(cam, W, H)
        pch = make_push_constants(samples=1, depth=2, frame=0, lights_count=len(flat.lights))
        pch.useShadows, pch.useAO, pch.useGI = 1, 1, 1
        acc = r.hybrid_trace(pch, cam, W, H, gb, seed=3).cpu().numpy().copy()
        torch.cuda.synchronize()
        return img.view(np.uint32), cnt, acc.view(np.uint32)

    from vkrt_amd import abi

    # (work sharing and triangle parking make a ray's node count depend on the other rays of its wave: off, so that every counter is a
    # function of the tree and the rays alone, as in test_gpu_refit.py)
    for layout in (1, 0):
        r = _renderer(flat, "ploc", layout, extra={abi.VKRT_OPT_WF_SHARE: 0, abi.VKRT_OPT_TRI_THRESHOLD: 0})
        a = frame(r)
        assert a[1] == frame(r)[1]  # (repeatable without any change)
        masks, flags = _masks(len(flat.nodes), 5)
        r.set_instance_visibility(0, masks, flags)
        b = frame(r)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
        r.close()


# ---- 2. masks equal a sub-scene; 3. after motion ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,layout,wt,split", CONFIGS)
def test_masks_equal_a_sub_scene(scene, kind, layout, wt, split):
    rays = _ray_sets(scene, 1)
    r = _renderer(scene, kind, layout, wt, split)
    masks, flags = _masks(len(scene.nodes), 11)
    r.set_instance_visibility(0, masks, flags)
    assert np.array_equal(r.instance_visibility()[0], masks) and np.array_equal(r.instance_visibility()[1], flags)
    for cull in CULLS:
        keep = [i for i in range(len(scene.nodes)) if masks[i] & cull]
        ref, nodemap, gmap = _reference(scene, ("mask", 11, cull), keep, rays, wt)
        for name, ry in rays.items():
            _assert_same(_query(r, ry, cull_mask=cull), ref[name], nodemap, gmap)
    # cull mask 0: every ray misses, results written
    for name, ry in rays.items():
        b, ints, occ = _query(r, ry, cull_mask=0)
        assert np.all(ints == -1) and np.all(occ == 0)
        assert np.array_equal(b[:, 0], ry.cpu().numpy()[:, 7].view(np.uint32)) and np.all(b[:, 1:] == 0)
    r.close()


@pytest.mark.parametrize("kind,layout", [(k, lay) for k in KINDS for lay in (1, 0)])
def test_masks_after_update_and_refit(scene, kind, layout):
    r = _renderer(scene, kind, layout)
    masks, flags = _masks(len(scene.nodes), 12)
    r.set_instance_visibility(0, masks, flags)
    mv, mats = moved(scene, [0, 3, 7, 8, 15], seed=4)
    apply(r, mats)
    r.refit()
    got = r.instance_visibility()
    assert np.array_equal(got[0], masks) and np.array_equal(got[1], flags)
    rays = _ray_sets(mv, 2)
    for cull in (0x12, 0xA5):
        keep = [i for i in range(len(mv.nodes)) if masks[i] & cull]
        ref, nodemap, gmap = _reference(mv, ("moved", 12, cull), keep, rays, 0)
        for name, ry in rays.items():
            _assert_same(_query(r, ry, cull_mask=cull), ref[name], nodemap, gmap)
    r.close()


# ---- 4. facing equals a sub-scene ------------------------------------------------------------------------------------------------
def _front(flat, i, d):
    """float64 front-facing rule of node i's triangles for world direction d (object space, before FLIP_FACING)"""
    T = _node_tris(flat, i)
    N = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    M = _row_major(flat.nodes[i]["worldMatrix"])[:3, :3]
    dob = np.linalg.solve(M, d)
    c = N @ dob / (np.linalg.norm(N, axis=1) * np.linalg.norm(dob))
    return c < 0, np.abs(c)


def _directions(flat, count, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        if min(_front(flat, i, d)[1].min() for i in range(len(flat.nodes))) > 1e-3:  # no triangle within 1e-3 of edge-on
            out.append(d)
    return out


def _parallel_rays(d, seed, n=8000):
    rng = np.random.default_rng(seed)
    a = np.cross(d, [0.3, 1.0, 0.2])
    a /= np.linalg.norm(a)
    b = np.cross(d, a)
    o = -d * 14 + a * rng.uniform(-9, 9, (n, 1)) + b * rng.uniform(-9, 9, (n, 1))
    return {"parallel": _pack(o, np.broadcast_to(d, (n, 3)), 0.001, 1e4), "parallel_tmin": _pack(o, np.broadcast_to(d, (n, 3)), rng.uniform(0, 18, n), 1e4)}


def _facing_subscene(flat, d, flags, cull):
    """per node the triangles a call with ray flag `cull` keeps for direction d, in order, under each node's own transform"""
    from vkrt_amd.flat_scene import PRIM_DTYPE

    sub = copy.copy(flat)
    pms, idx, gmap, prim_of, first = [], [], [], [], 0
    off = _offsets(flat)
    for i, node in enumerate(flat.nodes):
        pm = flat.prim_meshes[node["primMesh"]]
        front, _ = _front(flat, i, d)
        if flags[i] & 2:
            front = ~front
        keepm = np.ones(len(front), bool) if flags[i] & 1 else (front if cull == BACK else ~front)
        k = np.nonzero(keepm)[0]
        tri_idx = flat.indices[int(pm["firstIndex"]): int(pm["firstIndex"]) + int(pm["indexCount"])].reshape(-1, 3)[k]
        idx.append(tri_idx.reshape(-1))
        pms.append((first, 3 * len(k), int(pm["vertexOffset"]), int(pm["vertexCount"]), int(pm["materialIndex"])))
        first += 3 * len(k)
        gmap.append(off[i] + k)
        prim_of.append(k)
    sub.indices = np.concatenate(idx).astype(np.uint32)
    sub.prim_meshes = np.array(pms, PRIM_DTYPE)
    sub.nodes = flat.nodes.copy()
    sub.nodes["primMesh"] = np.arange(len(flat.nodes))
    return sub, np.arange(len(flat.nodes)), np.concatenate(gmap), np.concatenate(prim_of)


@pytest.mark.parametrize("kind,layout,wt,split", CONFIGS)
def test_facing_equals_a_sub_scene(scene, kind, layout, wt, split):
    r = _renderer(scene, kind, layout, wt, split)
    rng = np.random.default_rng(21)
    flags = rng.integers(0, 4, len(scene.nodes)).astype(np.uint8)  # CULL_DISABLE, FLIP_FACING, both, neither
    r.set_instance_visibility(0, np.full(len(scene.nodes), 0xFF, np.uint8), flags)
    for j, d in enumerate(_directions(scene, 2, 22)):
        rays = _parallel_rays(d, 23 + j)
        for cull in (BACK, FRONT):
            k = ("facing", j, cull)
            if (k, wt) not in _REF:
                sub, nodemap, gmap, prim_of = _facing_subscene(scene, d, flags, cull)
                rs = _renderer(sub, wt=wt)
                _REF[(k, wt)] = ({n: _query(rs, ry) for n, ry in rays.items()}, nodemap, gmap, prim_of)
                rs.close()
            ref, nodemap, gmap, prim_of = _REF[(k, wt)]
            for name, ry in rays.items():
                got = _query(r, ry, ray_flags=cull)
                assert (got[1][:, 3] >= 0).mean() > 0.01
                _assert_same(got, ref[name], nodemap, gmap, prim_of)
    r.close()


def test_one_triangle_pins_the_winding_rule():
    """p0 = (0,0,0), p1 = (1,0,0), p2 = (0,1,0): counter-clockwise seen from +z, so a ray coming down from +z sees its front face.
    Every axis and both signs (the watertight test's sign depends on the dominant axis), a mirroring node and FLIP_FACING."""
    from vkrt_amd.flat_scene import LIGHT_DTYPE, MAT_DTYPE, NODE_DTYPE, PRIM_DTYPE, FlatScene

    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    pm = np.zeros(1, PRIM_DTYPE)
    pm[0] = (0, 3, 0, 3, 0)
    mats = np.zeros(1, MAT_DTYPE)
    mats[0]["pbrBaseColorFactor"] = [1, 1, 1, 1]
    mats[0]["pbrBaseColorTexture"] = mats[0]["metallicRoughnessTexture"] = mats[0]["normalTexture"] = mats[0]["emissiveTexture"] = -1
    lights = np.zeros(1, LIGHT_DTYPE)
    # the triangle in the xy, yz and zx planes (rotations keep the winding), and mirrored in x
    rots = [np.eye(3), np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]]), np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]])]
    for R in rots:
        for mirror in (False, True):
            M = np.eye(4)
            M[:3, :3] = R @ np.diag([-1.0 if mirror else 1.0, 1, 1])
            nodes = np.zeros(1, NODE_DTYPE)
            nodes[0]["worldMatrix"] = np.ascontiguousarray(M.T.reshape(16), np.float32)
            flat = FlatScene(pos, np.zeros((3, 3), np.float32), np.zeros((3, 4), np.float32), np.zeros((3, 2), np.float32),
                             np.arange(3, dtype=np.uint32), pm, mats, lights, nodes, [])
            inside = M[:3, :3] @ np.array([0.25, 0.25, 0.0])
            nrm = R @ np.array([0.0, 0, 1])  # the object-space normal's direction, turned with the triangle
            for wt in (0, 1):
                r = _renderer(flat, "sah", 1, wt)
                for side in (1.0, -1.0):
                    o = inside + side * 2 * nrm
                    ray = _pack(o[None], (-side * nrm)[None], 0.001, 10.0)
                    front = side > 0  # coming from +normal (object +z): counter-clockwise, front
                    for flip in (0, 2):
                        r.set_instance_visibility(0, [0xFF], [flip])
                        f = front != bool(flip)
                        assert _query(r, ray)[1][0, 3] == 0
                        assert (_query(r, ray, ray_flags=BACK)[1][0, 3] == 0) == f, (R, mirror, wt, side, flip)
                        assert (_query(r, ray, ray_flags=FRONT)[1][0, 3] == 0) == (not f), (R, mirror, wt, side, flip)
                        r.set_instance_visibility(0, [0xFF], [flip | 1])  # CULL_DISABLE: both flags see it
                        assert _query(r, ray, ray_flags=BACK)[1][0, 3] == 0 and _query(r, ray, ray_flags=FRONT)[1][0, 3] == 0
                r.close()


# ---- 5. VKRT_RAY_OPAQUE ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,layout,wt", [(k, lay, wt) for k in KINDS for lay in (1, 0) for wt in (0, 1)])
def test_opaque_flag_equals_a_scene_built_without_dissolve(kind, layout, wt):
    flat = _instanced_scene(seed=5, alpha=[1.0, 0.0, 0.5, 0.8])
    rays = _ray_sets(flat, 3)
    rd = _renderer(flat, kind, layout, wt, dissolve=1)
    ro = _renderer(flat, kind, layout, wt, dissolve=0)
    differs = False
    for name, ry in rays.items():
        ref = _query(ro, ry, seed=9)
        got = _query(rd, ry, seed=9, ray_flags=OPAQUE)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b), name
        differs = differs or not np.array_equal(_query(rd, ry, seed=9)[1], ref[1])
        # with a mask as well (the filtering walk with the stage masked)
        rd.set_instance_visibility(0, np.arange(len(flat.nodes)) % 2 + 1, None)
        got = _query(rd, ry, seed=9, ray_flags=OPAQUE, cull_mask=1)
        ref1 = _query(ro, ry, seed=9)
        keep = np.arange(len(flat.nodes)) % 2 == 0
        hit = got[1][:, 3] >= 0
        assert np.all(keep[got[1][hit, 0]])
        rd.set_instance_visibility(0, np.full(len(flat.nodes), 0xFF), None)
        assert hit.sum() <= (ref1[1][:, 3] >= 0).sum()
    assert differs  # the stage did ignore hits without the flag
    rd.close()
    ro.close()


# ---- 6. the node-mask table -----------------------------------------------------------------------------------------------------
def _table(acc, vis):
    """host restatement: byte s of node k = OR of the masks under slot s (reached nodes only; others -1)"""
    nodes, tris = acc["nodes"], acc["tris"]
    inst = tris[:, 10].view(np.int32)
    out = np.full((len(nodes), 8), -1, np.int64)

    def visit(k):
        w = nodes[k]
        imask, cb, tb = int(w[3]) >> 24, int(w[4]), int(w[5])
        meta = int(w[6]) | (int(w[7]) << 32)
        row = []
        for s in range(8):
            m = (meta >> (8 * s)) & 0xFF
            if (imask >> s) & 1:
                c = cb + bin(imask & ((1 << s) - 1)).count("1")
                row.append(int(np.bitwise_or.reduce(visit(c))))
            elif m:
                first, cnt = tb + (m & 31), bin(m >> 5).count("1")
                row.append(int(np.bitwise_or.reduce(vis[inst[first:first + cnt]])))
            else:
                row.append(0)
        out[k] = row
        return np.array(row, np.int64)

    if len(nodes) and acc["root_ref"] == 0:
        visit(0)
    return out


@pytest.mark.parametrize("kind,wt,split", [(k, wt, sp) for k in KINDS for wt in (0, 1) for sp in (0, -1)])
def test_node_mask_table_is_exact(scene, kind, wt, split):
    from vkrt_amd.renderer import VkrtError

    r = _renderer(scene, kind, 1, wt, split)

    def check(masks):
        acc = r.read_accel()
        want = _table(acc, masks.astype(np.int64))
        got = r.read_node_masks().astype(np.int64)
        reached = want[:, 0] >= 0
        assert reached.sum() > 1
        assert np.array_equal(got[reached], want[reached])

    check(np.full(len(scene.nodes), 0xFF))
    masks, flags = _masks(len(scene.nodes), 31)
    r.set_instance_visibility(0, masks, flags)
    check(masks)
    mv, mats = moved(scene, [1, 2, 9], seed=6)
    apply(r, mats)
    r.refit()
    check(masks)
    r.set_instance_visibility(2, masks[2:6][::-1].copy(), None)
    masks[2:6] = masks[2:6][::-1].copy()
    check(masks)
    r.build(kind)  # a rebuild keeps the visibility and makes its table from it
    check(masks)
    r.close()
    r2 = _renderer(scene, kind, 0, wt, split)
    with pytest.raises(VkrtError):
        r2.read_node_masks()
    r2.close()


# ---- 7. stream order ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 0])
def test_set_visibility_then_query_on_one_stream(scene, layout):
    import torch

    rays = _ray_sets(scene, 1)
    ry = rays["diffuse"]
    r = _renderer(scene, "ploc", layout)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    ma, _ = _masks(len(scene.nodes), 41)
    mb, _ = _masks(len(scene.nodes), 42)
    outs = []
    with torch.cuda.stream(s):
        for m in (ma, mb, ma):
            r.set_instance_visibility(0, m, np.zeros(len(m), np.uint8), stream=s)
            h = r.intersect(ry, stream=s, cull_mask=0x33)
            outs.append((h.buffer, r.occluded(ry, stream=s, cull_mask=0x33)))
    s.synchronize()
    for m, key, (hb, occ) in zip((ma, mb, ma), (41, 42, 41), outs):
        keep = [i for i in range(len(scene.nodes)) if m[i] & 0x33]
        ref, nodemap, gmap = _reference(scene, ("mask", key, 0x33), keep, {"diffuse": ry}, 0)
        b = hb.cpu().numpy()
        got = (b[:, :3].view(np.uint32).copy(), b[:, 3:].view(np.int32).copy(), occ.cpu().numpy().copy())
        _assert_same(got, ref["diffuse"], nodemap, gmap)
    r.close()
