"""The scene side of motion on the GPU: vkrt_scene_motion_mark, vkrt_gbuffer_raycast_hits and vkrt_hit_motion against the numpy
restatement tests/np_motion.py.  Every comparison is on the 32-bit words and excuses no pixel and no record.

One sequence serves most cases (run()):
    state 0 --G-buffer with hits--> mark --> state A (nodes moved, meshes deformed, refit) --G-buffer with motion--> mark (nothing
    changed) --> state B --G-buffer with motion
on Cornell (its last two nodes move) and on a 20 k triangle atrium (a third of its nodes move, a third of its meshes carry a travelling
sine), at 72x40 and 40x72, and once each on a 1x1 image, a strip shard, a scene built with the dissolve stage and a BVH2 tree."""
import copy
import os
import sys

import numpy as np
import pytest

import np_motion
import scene_deform as sd
from conftest import ROOT
from scene_motion import apply, moved

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu
F = np.float32
DEFORM_ATTRS = ("positions", "normals", "tangents")


@pytest.fixture(scope="module")
def scenes(cornell_flat):
    import atrium

    flat, _ = atrium.build_atrium(20000, seed=4, with_textures=True)
    return {"cornell": cornell_flat, "atrium": flat}


def _camera(name, W, H):
    """(GlobalUniforms, column-major view matrix, camera origin as the kernels see it)"""
    import atrium
    import camera_np
    from vkrt_amd.flat_scene import uniforms_from_matrices

    kw = dict(atrium.DEFAULT_CAMERA) if name == "atrium" else dict(eye=(0.0, 0.0, 15.0), center=(0.0, 0.0, 0.0))
    mats = camera_np.global_uniforms(width=W, height=H, **kw)
    vm = np.asarray(camera_np.look_at(kw["eye"], kw["center"], (0, 1, 0)), F).T.reshape(-1).copy()
    return uniforms_from_matrices(*mats), vm, np.asarray(mats[1], F)[:3, 3].copy()


def _states(name, flat):
    """[state 0, state A, state B] as (FlatScene, node matrices to send, meshes to send)"""
    n = len(flat.nodes)
    if name == "cornell":
        nodes, meshes = [n - 2, n - 1], []
    else:
        nodes = sorted(np.random.default_rng(3).choice(n, n // 3, replace=False).tolist())
        meshes = sd.third_of_meshes(flat)
    out = [(flat, {}, [])]
    for seed, phase in ((11, 0.7), (12, 1.9)):
        st, mats = moved(flat, nodes, seed)
        if meshes:
            st = sd.sine(st, meshes, phase=phase)
        out.append((st, mats, meshes))
    return out


def _goto(r, state, stream=None, device=None):
    st, mats, meshes = state
    apply(r, mats, stream=stream)
    keep = sd.send(r, st, meshes, attrs=DEFORM_ATTRS, stream=stream, device=device) if meshes else []
    r.refit(stream=stream)
    return keep


def run(name, flat, W, H, options=None, shard=None, stream=None, nrd=True):
    """The sequence of the module docstring; returns torch tensors only (nothing is downloaded in between)."""
    import torch
    from vkrt_amd.renderer import Renderer

    cam, vm, _ = _camera(name, W, H)
    vm = vm if nrd else None
    states = _states(name, flat)
    r = Renderer(flat, device=0, build="ploc", options=options)
    dev = "cuda:0" if stream is not None else None  # on a stream of our own: device-sourced vertex updates (no host synchronisation)
    out, keep = {}, []
    out["plain0"] = r.gbuffer_raycast(cam, W, H, shard=shard, stream=stream, view_matrix=vm)
    out["g0"] = r.gbuffer_raycast(cam, W, H, shard=shard, stream=stream, view_matrix=vm, hits=True)
    out["cur0"], out["prev0"] = r.hit_motion(out["g0"]["hits"].view(-1, 8), stream=stream)
    r.motion_mark(stream=stream)
    keep += _goto(r, states[1], stream, dev)
    out["gA"] = r.gbuffer_raycast(cam, W, H, shard=shard, stream=stream, view_matrix=vm, motion=True)
    out["curA"], _ = r.hit_motion(out["gA"]["hits"].view(-1, 8), previous=False, stream=stream)
    r.motion_mark(stream=stream)  # nothing changed since the G-buffer: previous := current
    out["curA2"], out["prevA2"] = r.hit_motion(out["gA"]["hits"].view(-1, 8), stream=stream)
    keep += _goto(r, states[2], stream, dev)
    out["gB"] = r.gbuffer_raycast(cam, W, H, shard=shard, stream=stream, view_matrix=vm, motion=True)
    out["plainB"] = r.gbuffer_raycast(cam, W, H, shard=shard, stream=stream, view_matrix=vm)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    r.close()
    return out, states


def _np(t):
    return np.ascontiguousarray(t.cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _check_hits_and_position(g, flat):
    """cases 2 of the module: position.xyz == np_motion on the arrays of `flat` at every geometry pixel; miss records elsewhere"""
    hits = _np(g["hits"]).reshape(-1, 8)
    pos = _np(g["position"]).reshape(-1, 4)
    inst = hits.view(np.int32)[:, 3]
    geom = inst >= 0
    assert np.array_equal(np_motion.valid_records(flat, hits), geom)
    want = np_motion.hit_points(flat, hits)
    assert _same(pos[geom, :3], want[geom, :3])
    miss = np.zeros(8, F)
    miss[0] = 10000.0
    miss.view(np.int32)[3:] = -1
    assert _same(hits[~geom], np.broadcast_to(miss, hits[~geom].shape))
    assert np.all(pos[~geom] == np.array([0, 0, 0, 1], F))
    t = hits[geom, 0]
    assert np.all((t > 0.001) & (t < 10000.0)) and np.all(hits.view(np.int32)[geom, 6] >= 0)
    return hits, pos, geom


def check(out, states, min_geometry=1):
    """cases 1, 2, 4, 5 and 6 on the tensors of run()"""
    f0, fA, fB = (s[0] for s in states)
    # 1. the planes with hits are the planes without
    for a, b in (("g0", "plain0"), ("gB", "plainB")):
        for k in out[b]:
            assert _same(_np(out[a][k]), _np(out[b][k])), (a, k)
    # 2. the records are the G-buffer's surface points
    h0, p0, geom0 = _check_hits_and_position(out["g0"], f0)
    hA, pA, geomA = _check_hits_and_position(out["gA"], fA)
    hB, pB, geomB = _check_hits_and_position(out["gB"], fB)
    assert geom0.sum() >= min_geometry and geomA.sum() >= min_geometry and geomB.sum() >= min_geometry
    one = np.where(geom0, F(1), F(0))
    # 4. before any mark: current == previous == position, w = 1; misses give the zero record
    for k in ("cur0", "prev0"):
        v = _np(out[k])
        assert _same(v[geom0, :3], p0[geom0, :3]) and _same(v[:, 3], one) and not v[~geom0].any()
    # 5. mark, move, G-buffer with motion: previous on the old arrays, current is the position plane
    prevA = _np(out["gA"]["prevPosition"]).reshape(-1, 4)
    assert _same(prevA, np_motion.hit_points(f0, hA))
    curA = _np(out["curA"])
    assert _same(curA[geomA, :3], pA[geomA, :3]) and _same(curA, np_motion.hit_points(fA, hA))
    # 6. a mark with nothing changed: previous == current; then move B: previous = state A
    assert _same(_np(out["prevA2"]), _np(out["curA2"])) and _same(_np(out["curA2"]), curA)
    prevB = _np(out["gB"]["prevPosition"]).reshape(-1, 4)
    assert _same(prevB, np_motion.hit_points(fA, hB))
    moved_px = (np.abs(prevB[:, :3] - pB[:, :3]).max(-1) > 0) & geomB
    return int(moved_px.sum()), int(geomB.sum())


@pytest.mark.parametrize("W,H", [(72, 40), (40, 72)])
@pytest.mark.parametrize("name", ["cornell", "atrium"])
def test_sequence(scenes, name, W, H):
    out, states = run(name, scenes[name], W, H)
    moved_px, geom = check(out, states, min_geometry=W * H // 10)
    print(f"{name} {W}x{H}: {moved_px} of {geom} geometry pixels moved between state A and state B")
    assert moved_px > 20


def test_one_pixel_image(scenes):
    out, states = run("cornell", scenes["cornell"], 1, 1)
    check(out, states)


def test_strip_shard(scenes):
    from vkrt_amd import abi

    from vkrt_amd.sharding import shard_row_indices

    shard = abi.Shard(72, 40, 16, 2, 1)  # the second of two ranks, strips of 16 rows
    rows = np.asarray(shard_row_indices(40, 2, 1))
    out, states = run("atrium", scenes["atrium"], 72, 40, shard=shard)
    assert tuple(out["g0"]["hits"].shape) == (len(rows), 72, 8) and 0 < len(rows) < 40
    check(out, states, min_geometry=100)
    whole, _ = run("atrium", scenes["atrium"], 72, 40)
    assert _same(_np(out["gB"]["hits"]), _np(whole["gB"]["hits"])[rows]) and _same(_np(out["gB"]["prevPosition"]), _np(whole["gB"]["prevPosition"])[rows])


def test_without_the_nrd_planes(scenes):
    out, states = run("cornell", scenes["cornell"], 72, 40, nrd=False)
    assert "nrdViewZ" not in out["g0"]
    check(out, states, min_geometry=100)


def test_bvh2_layout(scenes):
    from vkrt_amd import abi

    out, states = run("atrium", scenes["atrium"], 72, 40, options={abi.VKRT_OPT_BVH_LAYOUT: 0})
    check(out, states, min_geometry=100)
    wide, _ = run("atrium", scenes["atrium"], 72, 40)
    assert _same(_np(out["gB"]["prevPosition"]), _np(wide["gB"]["prevPosition"]))


def _translucent(flat):
    """Cornell with its last box's material at alpha 0.5: with VKRT_OPT_ANYHIT_DISSOLVE its triangles' id words carry the stage's flag"""
    out = copy.copy(flat)
    out.materials = flat.materials.copy()
    m = int(flat.prim_meshes[flat.nodes[-1]["primMesh"]]["materialIndex"])
    out.materials["pbrBaseColorFactor"][m, 3] = 0.5
    return out


def test_dissolve_scene_masks_the_id_flag(scenes):
    """the raster stand-in has no dissolve stage: the planes are those of the scene built without it, and `triangle` carries no flag"""
    from vkrt_amd import abi

    flat = _translucent(scenes["cornell"])
    out, states = run("cornell", flat, 72, 40, options={abi.VKRT_OPT_ANYHIT_DISSOLVE: 1})
    check(out, states, min_geometry=100)
    tri = _np(out["gB"]["hits"]).view(np.int32)[..., 6]
    inst = _np(out["gB"]["hits"]).view(np.int32)[..., 3]
    assert (inst == len(flat.nodes) - 1).sum() > 20 and np.all(tri[inst >= 0] >= 0)
    opaque, _ = run("cornell", flat, 72, 40)
    for k in ("hits", "position", "prevPosition", "color"):
        assert _same(_np(out["gB"][k]), _np(opaque["gB"][k])), k


@pytest.mark.parametrize("name,options", [("cornell", None), ("atrium", None), ("cornell", "dissolve"), ("atrium", "bvh2")])
def test_ids_agree_with_intersect(scenes, name, options):
    """3. prim_mesh, triangle and material of the per-pixel records against Renderer.intersect: rays from the camera origin through the
    recomputed positions give a map (instance, primitive) -> (prim_mesh, triangle, material); every key the map holds must agree, and
    the map must hold at least half of the image's distinct keys (so that the check is not vacuous)."""
    import torch
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer, pack_rays

    flat = scenes[name]
    opts = None
    if options == "dissolve":
        flat, opts = _translucent(flat), {abi.VKRT_OPT_ANYHIT_DISSOLVE: 1}
    if options == "bvh2":
        opts = {abi.VKRT_OPT_BVH_LAYOUT: 0}
    W, H = 72, 40
    cam, vm, origin = _camera(name, W, H)
    state = _states(name, flat)[1]
    r = Renderer(flat, device=0, build="ploc", options=opts)
    _goto(r, state)
    g = r.gbuffer_raycast(cam, W, H, view_matrix=vm, hits=True)
    hits = _np(g["hits"]).reshape(-1, 8).view(np.int32)
    geom = hits[:, 3] >= 0
    pos = np_motion.hit_points(state[0], hits)[geom, :3]
    d = pos - origin
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = pack_rays(torch.from_numpy(np.broadcast_to(origin, d.shape).copy()).to("cuda:0"), torch.from_numpy(d.astype(F)).to("cuda:0"))
    q = _np(r.intersect(rays, ray_flags=abi.VKRT_RAY_OPAQUE).buffer).view(np.int32)
    r.close()
    q = q[q[:, 3] >= 0]
    key = lambda h: h[:, 3].astype(np.int64) << 32 | h[:, 4].astype(np.int64)  # noqa: E731
    qk, first = np.unique(key(q), return_index=True)
    table = q[first][:, 5:8]
    for k, row in zip(key(q), q[:, 5:8]):  # the map is a function
        assert np.array_equal(table[np.searchsorted(qk, k)], row)
    gk = key(hits[geom])
    at = np.clip(np.searchsorted(qk, gk), 0, len(qk) - 1)
    known = qk[at] == gk
    distinct = np.unique(gk)
    covered = np.isin(distinct, qk).mean()
    print(f"{name} {options}: the map holds {covered:.3f} of the image's {len(distinct)} distinct (instance, primitive) keys")
    assert covered >= 0.5
    assert np.array_equal(hits[geom][known][:, 5:8], table[at[known]])
    # and, independently of any ray: prim_mesh and material are the scene's own
    pm = flat.nodes["primMesh"][hits[geom][:, 3]]
    assert np.array_equal(hits[geom][:, 5], pm) and np.array_equal(hits[geom][:, 7], np.maximum(flat.prim_meshes["materialIndex"][pm], 0))


def _moved_renderer(name, flat, mark=True):
    from vkrt_amd.renderer import Renderer

    states = _states(name, flat)
    r = Renderer(flat, device=0, build="ploc")
    if mark:
        r.motion_mark()
    _goto(r, states[1])
    return r, states


def test_caller_records(scenes):
    """7. 4096 records of Renderer.intersect on random rays, with injected misses, out-of-range ids and NaN u: equal to np_motion,
    invalid ones the zero record (as vkrt_hit_surface treats them: valid = 0)"""
    import torch
    from vkrt_amd.renderer import pack_rays

    flat = scenes["atrium"]
    r, states = _moved_renderer("atrium", flat)
    o, d = sd.random_rays(states[1][0], n=4096, seed=9)
    h = r.intersect(pack_rays(torch.from_numpy(o).to("cuda:0"), torch.from_numpy(d).to("cuda:0"))).buffer
    rec = _np(h).copy()
    i32 = rec.view(np.int32)
    hit = np.nonzero(i32[:, 3] >= 0)[0]
    assert len(hit) > 2000 and len(hit) < 4096  # natural misses among them
    i32[hit[0:8], 3] = len(flat.nodes)             # instance one past the end
    i32[hit[8:16], 3] = -5
    i32[hit[16:24], 4] = 1 << 30                   # primitive far outside its mesh
    i32[hit[24:32], 4] = -1
    tris = flat.prim_meshes["indexCount"][flat.nodes["primMesh"][i32[hit[32:40], 3]]] // 3
    i32[hit[32:40], 4] = tris                      # primitive one past the end of its mesh
    rec[hit[40:48], 1] = np.nan                    # u
    rec[hit[48:56], 2] = np.inf                    # v
    dev = torch.from_numpy(rec).to("cuda:0")
    cur, prev = r.hit_motion(dev)
    surf = r.surface(dev, material=False)
    cur, prev, valid = _np(cur), _np(prev), _np(surf.valid).astype(bool)
    r.close()
    ok = np_motion.valid_records(flat, rec)
    assert np.array_equal(ok, valid) and (~ok[hit[:56]]).all() and ok[hit[56:]].all()
    assert _same(cur, np_motion.hit_points(states[1][0], rec)) and _same(prev, np_motion.hit_points(states[0][0], rec))
    assert not cur[~ok].any() and not prev[~ok].any() and np.all(cur[ok, 3] == 1) and np.all(prev[ok, 3] == 1)
    assert (np.abs(cur[ok, :3] - prev[ok, :3]).max(-1) > 0).sum() > 100


def test_attribute_updates_and_a_rebuild_keep_the_snapshot(scenes):
    """8. a normals-only vertex update leaves `previous` (and `current`) unchanged; 9. so does vkrt_accel_build after the mark"""
    import torch
    from vkrt_amd.renderer import pack_rays

    flat = scenes["atrium"]
    r, states = _moved_renderer("atrium", flat)
    o, d = sd.random_rays(states[1][0], n=4096, seed=10)
    h = r.intersect(pack_rays(torch.from_numpy(o).to("cuda:0"), torch.from_numpy(d).to("cuda:0"))).buffer
    cur, prev = (_np(t) for t in r.hit_motion(h))
    assert _same(prev, np_motion.hit_points(flat, _np(h)))
    other = sd.sine(flat, states[1][2], phase=2.5)  # other normals and tangents for the deformed meshes
    sd.send(r, other, states[1][2], attrs=("normals", "tangents"))
    cur2, prev2 = (_np(t) for t in r.hit_motion(h))
    assert _same(cur, cur2) and _same(prev, prev2)
    r.build("lbvh")
    cur3, prev3 = (_np(t) for t in r.hit_motion(h))
    assert _same(cur, cur3) and _same(prev, prev3)
    r.refit()
    assert _same(prev, _np(r.hit_motion(h, current=False)[1]))
    r.close()


def test_non_default_stream_gives_the_same_bits(scenes):
    """10. the whole sequence enqueued on a torch stream of its own, device-sourced vertex updates, no host synchronisation before the
    end: every tensor equals the default-stream run's"""
    import torch

    flat = scenes["atrium"]
    ref, _ = run("atrium", flat, 72, 40)
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        out, _ = run("atrium", flat, 72, 40, stream=s)
    for k, v in ref.items():
        for kk, a in (v.items() if isinstance(v, dict) else ((None, v),)):
            b = out[k][kk] if kk is not None else out[k]
            assert sd.digest(a) == sd.digest(b), (k, kk)
