"""Multi-hit ray queries (vkrt_intersect_multi, Renderer.intersect_multi): the first K candidates of every ray in the order (t, flattened
triangle id).

The list is defined by the candidate rule the library uses everywhere (include/vkrt.h), so every check is exact: bit-identical t, u, v
and equal ids against the oracle peeled level by level (its interval is open and its tie rule is "smallest id", so it returns the first
entry of every group of equal t), against vkrt_intersect for K = 1, and byte-identical buffers across builders, layouts, split budgets
and refits.  Scenes and hostile rays are those of test_gpu_ray_query.py."""
import copy
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

import test_gpu_ray_query as Q
import test_gpu_ray_query_visibility as V
from conftest import default_camera
from scene_motion import apply, moved

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KINDS = Q.KINDS
scenes = Q.scenes  # (the module fixture: Cornell, the small atrium, the triangle soup, each with its oracle)


def _multi(r, rays, k, **kw):
    """(records uint32 [N, K, 8], counts int32 [N]) of one call"""
    import torch

    h = r.intersect_multi(rays, k, **kw)
    torch.cuda.current_stream().synchronize()
    assert tuple(h.buffer.shape) == (rays.shape[0], k, 8) and tuple(h.count.shape) == (rays.shape[0],)
    return h.buffer.cpu().numpy().view(np.uint32).copy(), h.count.cpu().numpy().copy()


def _single(r, rays, **kw):
    import torch

    h = r.intersect(rays, **kw)
    torch.cuda.current_stream().synchronize()
    return h.buffer.cpu().numpy().view(np.uint32).copy()


def _no_faults(r):
    c = r.counters()
    assert c["traversal_faults"] == 0
    assert all(c[k] == 0 for k in ("rays_closest", "rays_shadow", "hits", "pixels", "nodes_visited", "tris_tested")), c


def _structure(buf, cnt, tmax, table=None):
    """What holds for every result: 0 <= count <= K; records behind the count are the miss record of vkrt_intersect; records before it are
    hits with strictly increasing keys (t, triangle) -- so no triangle twice -- and the attributes of their flattened id."""
    n, k, _ = buf.shape
    assert cnt.min() >= 0 and cnt.max() <= k
    j = np.arange(k)[None, :]
    live = j < cnt[:, None]
    tmax_bits = np.broadcast_to(np.asarray(tmax, np.float32), (n,)).view(np.uint32) if np.ndim(tmax) else np.full(n, np.float32(tmax)).view(np.uint32)
    miss = np.zeros((n, k, 8), np.uint32)
    miss[:, :, 0] = tmax_bits[:, None]
    miss[:, :, 3:] = 0xFFFFFFFF
    assert np.array_equal(buf[~live], miss[~live])
    t = buf[:, :, 0].view(np.float32)
    tri = buf[:, :, 6].view(np.int32)
    assert np.all(tri[live] >= 0)
    inc = (t[:, 1:] > t[:, :-1]) | ((t[:, 1:] == t[:, :-1]) & (tri[:, 1:] > tri[:, :-1]))
    assert np.all(inc[live[:, 1:]])
    if table is not None:
        ints = buf[:, :, 3:].view(np.int32)
        assert np.array_equal(ints[live][:, [0, 1, 2, 4]], table[tri[live]])


def _peel_oracle(orc, o, d, tmin, tmax, use_bvh, levels=17):
    """Per ray the oracle's answers with tmin = the t of the previous answer, until it misses (at most `levels`): one ray per call, its
    bounds are scalars.  Entries (t, u, v as uint32 bits, gid)."""
    tmin = np.broadcast_to(np.asarray(tmin, np.float32), (len(o),))
    tmax = np.broadcast_to(np.asarray(tmax, np.float32), (len(o),))
    out = []
    for i in range(len(o)):
        seq, lo = [], float(tmin[i])
        for _ in range(levels):
            t, u, v, g, _ = orc.trace_rays(o[i:i + 1], d[i:i + 1], lo, float(tmax[i]), use_bvh=use_bvh)
            if g[0] < 0:
                break
            seq.append((int(t.view(np.uint32)[0]), int(u.view(np.uint32)[0]), int(v.view(np.uint32)[0]), int(g[0])))
            lo = float(t[0])
        out.append(seq)
    return out


def _heads(buf, cnt, i):
    """indices of the entries of ray i whose t bits differ from the previous entry's"""
    return [j for j in range(int(cnt[i])) if j == 0 or buf[i, j, 0] != buf[i, j - 1, 0]]


def _assert_equals_peel(buf, cnt, seqs, gmap=None):
    """The group heads of every list equal the peeled sequence bit for bit in t, u, v and in the id, for as many as fit; a list that is
    not full is followed by a miss; the other entries carry their head's t and increasing ids (checked by _structure)."""
    k = buf.shape[1]
    groups = 0
    for i, seq in enumerate(seqs):
        heads = _heads(buf, cnt, i)
        got = [(int(buf[i, j, 0]), int(buf[i, j, 1]), int(buf[i, j, 2]), int(buf[i, j, 6])) for j in heads]
        want = seq if gmap is None else [(t, u, v, int(gmap[g])) for t, u, v, g in seq]
        if cnt[i] < k:
            assert got == want, (i, got, want)  # (the peel after the last head is a miss)
        else:
            assert len(want) >= len(got) and got == want[:len(got)], (i, got, want)
        groups += len(heads) < cnt[i]
    return groups


# ---- 1. K = 1 is vkrt_intersect ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("kind", KINDS)
def test_one_hit_is_intersect_bit_for_bit(scenes, kind, layout):
    from vkrt_amd import abi

    for name, n in (("cornell", 30001), ("soup", 30001), ("atrium_small", 60001)):
        flat, _ = scenes[name]
        r = Q._renderer(flat, kind, layout)
        r.reset_counters()
        o, d = Q._hostile_rays(flat, n, seed=61)
        rays = Q._pack(o, d, 0.001, 10000.0)
        buf, cnt = _multi(r, rays, 1)
        ref = _single(r, rays)
        assert np.array_equal(buf[:, 0], ref)
        assert np.array_equal(cnt, (ref[:, 6].view(np.int32) >= 0).astype(np.int32))
        assert cnt.mean() > 0.15
        # a mask that filters (the filtering walk) and one that does not
        masks = (np.arange(len(flat.nodes)) % 3 + 1).astype(np.uint8)
        r.set_instance_visibility(0, masks, np.zeros(len(masks), np.uint8))
        for cull in (0x1, 0x3):
            assert np.array_equal(_multi(r, rays, 1, cull_mask=cull)[0][:, 0], _single(r, rays, cull_mask=cull))
        assert np.array_equal(_multi(r, rays, 1, ray_flags=V.BACK)[0][:, 0], _single(r, rays, ray_flags=V.BACK))
        _no_faults(r)
        r.close()
    flat, _ = scenes["soup"]
    o, d = Q._hostile_rays(flat, 30001, seed=62)
    rays = Q._pack(o, d, 0.001, 10000.0)
    r = Q._renderer(flat, kind, layout, {abi.VKRT_OPT_WATERTIGHT: 1})
    assert np.array_equal(_multi(r, rays, 1)[0][:, 0], _single(r, rays))
    r.close()
    flat = Q._dissolving(scenes["cornell"][0])
    o, d = Q._hostile_rays(flat, 30001, seed=63)
    rays = Q._pack(o, d, 0.001, 10000.0)
    r = Q._renderer(flat, kind, layout, {abi.VKRT_OPT_ANYHIT_DISSOLVE: 1})
    for seed in (0, 12345):
        assert np.array_equal(_multi(r, rays, 1, seed=seed)[0][:, 0], _single(r, rays, seed=seed))
    assert np.array_equal(_multi(r, rays, 1, seed=5, ray_flags=V.OPAQUE)[0][:, 0], _single(r, rays, seed=5, ray_flags=V.OPAQUE))
    r.close()


# ---- 2. against the oracle by peeling -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "atrium_small", "soup"])
def test_lists_equal_the_oracle_peeled(scenes, name):
    flat, orc = scenes[name]
    n = 2500
    o, d = Q._hostile_rays(flat, n, seed=67)
    rays = Q._pack(o, d, 0.001, 10000.0)
    table = Q._flattened(flat)
    peels = {bvh: _peel_oracle(orc, o, d, 0.001, 10000.0, bvh) for bvh in (False, True)}
    assert peels[False] == peels[True]
    assert np.mean([len(s) for s in peels[False]]) > 0.2
    for kind, layout in (("ploc", 1), ("lbvh", 0), ("sah", 1), ("ploc", 0)):
        r = Q._renderer(flat, kind, layout)
        r.reset_counters()
        for k in (2, 5, 16):
            buf, cnt = _multi(r, rays, k)
            _structure(buf, cnt, 10000.0, table)
            for bvh in (False, True):
                _assert_equals_peel(buf, cnt, peels[bvh])
            if k == 16:
                assert (cnt >= 2).mean() > 0.02  # (lists with more than the closest hit are exercised)
        _no_faults(r)
        r.close()


# ---- 3. ties, exactly ------------------------------------------------------------------------------------------------------------
def _doubled_nodes(flat):
    out = copy.copy(flat)
    out.nodes = np.concatenate([flat.nodes, flat.nodes]).copy()
    return out


def _doubled_indices(flat):
    """the soup with every triangle listed twice in its one mesh: triangle g + T is triangle g"""
    out = copy.copy(flat)
    out.indices = np.concatenate([flat.indices, flat.indices]).astype(np.uint32)
    out.prim_meshes = flat.prim_meshes.copy()
    out.prim_meshes["indexCount"] = 2 * flat.prim_meshes["indexCount"]
    return out


def _peel_intersect(r, o, d, tmin, tmax, passes):
    """what a caller could do before: vkrt_intersect again with tmin = the t of the last hit; [passes, N, 8] records"""
    lo = np.full(len(o), tmin, np.float32)
    out = []
    for _ in range(passes):
        rec = _single(r, Q._pack(o, d, lo, tmax))
        out.append(rec)
        hit = rec[:, 6].view(np.int32) >= 0
        lo = np.where(hit, rec[:, 0].view(np.float32), np.float32(tmax)).astype(np.float32)  # (tmin = tmax: a miss without a walk)
    return np.stack(out)


@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("which", ["nodes", "indices"])
def test_coincident_triangles_both_appear(scenes, which, layout):
    import oracle_py

    flat = scenes["cornell" if which == "nodes" else "soup"][0]
    dbl = _doubled_nodes(flat) if which == "nodes" else _doubled_indices(flat)
    T = len(Q._flattened(flat))
    assert len(Q._flattened(dbl)) == 2 * T
    n = 3000
    o, d = Q._hostile_rays(flat, n, seed=71)
    rays = Q._pack(o, d, 0.001, 10000.0)
    rs, rd = Q._renderer(flat, "ploc", layout), Q._renderer(dbl, "ploc", layout)
    rd.reset_counters()
    sb, sc = _multi(rs, rays, 16)
    db, dc = _multi(rd, rays, 16)
    _structure(db, dc, 10000.0, Q._flattened(dbl))
    # the single scene's list, peeled by the oracle, with every entry twice: ids g then g + T, identical t, u, v bits.  (Two triangles
    # of the single scene at one t -- a ray through a shared edge -- sort as g1, g2, g1 + T, g2 + T: the doubled list is the single
    # list's entries and their copies, sorted by (t, id), cut at 16; every one of its entries is among the copies of the single
    # scene's first 16.)
    single_peel = _peel_oracle(scenes["cornell" if which == "nodes" else "soup"][1], o, d, 0.001, 10000.0, True)
    _assert_equals_peel(sb, sc, single_peel)
    _assert_equals_peel(db, dc, single_peel)  # the doubled scene's group heads are the single scene's, ids g
    _assert_equals_peel(db, dc, _peel_oracle(oracle_py.OracleScene(dbl), o, d, 0.001, 10000.0, False))
    def copy_of(e):  # the record of the second copy: the next instance (nodes) or the next primitive of the one mesh (indices)
        e = list(e)
        e[3 if which == "nodes" else 4] += len(flat.nodes) if which == "nodes" else T
        e[6] += T
        return tuple(e)

    pairs = 0
    for i in range(n):
        ent = [tuple(int(x) for x in sb[i, j]) for j in range(sc[i])]
        both = sorted(ent + [copy_of(e) for e in ent], key=lambda e: (e[0], e[6]))  # (t > 0: its bits order like its value)
        want = both[:16]
        got = [tuple(int(x) for x in db[i, j]) for j in range(dc[i])]
        assert got == want, (i, got[:4], want[:4])
        assert dc[i] == min(16, 2 * sc[i])
        if len(_heads(sb, sc, i)) == sc[i]:  # no tie inside the single scene: strict pairs
            for j in range(0, dc[i] - 1, 2):
                assert np.array_equal(db[i, j, :3], db[i, j + 1, :3]) and db[i, j + 1, 6] == db[i, j, 6] + T
                pairs += 1
    assert pairs > n // 4
    # the defect this call removes: peeling with vkrt_intersect returns every other entry (the first of each group of equal t)
    peel = _peel_intersect(rd, o, d, 0.001, 10000.0, 8)
    skipped = 0
    for i in range(n):
        heads = _heads(db, dc, i)
        for lvl, j in enumerate(heads[:8]):
            assert np.array_equal(peel[lvl, i], db[i, j])
        if len(heads) < 8 and dc[i] < 16:
            assert peel[len(heads), i, 6] == 0xFFFFFFFF
        skipped += dc[i] - len(heads)
        assert not any(int(peel[lvl, i, 6]) >= T and int(peel[lvl, i, 6]) != 0xFFFFFFFF for lvl in range(8))  # never a copy
    assert skipped > n // 4
    _no_faults(rd)
    rs.close()
    rd.close()


# ---- 4. split references ---------------------------------------------------------------------------------------------------------
def test_split_references_give_every_triangle_once():
    import atrium
    from vkrt_amd import abi

    flat, _ = atrium.build_atrium(60000, seed=3, variant="nonuniform")
    atrium.rotate_scene(flat, dict(atrium.DEFAULT_CAMERA), 35.0, 20.0)
    n = 60001
    o, d = Q._hostile_rays(flat, n, seed=73)
    rays = Q._pack(o, d, 0.001, 10000.0)
    table = Q._flattened(flat)
    for kind, layout in (("ploc", 1), ("lbvh", 1), ("ploc", 0)):
        out = {}
        for budget in (0, 30):
            r = Q._renderer(flat, kind, layout, {abi.VKRT_OPT_SPLIT_BUDGET: budget})
            info = r.accel_info()
            assert (info["reference_count"] > info["triangle_count"]) == (budget == 30), info
            r.reset_counters()
            out[budget] = {k: _multi(r, rays, k) for k in (4, 16)}
            _no_faults(r)
            r.close()
        for k in (4, 16):
            buf, cnt = out[30][k]
            _structure(buf, cnt, 10000.0, table)  # (strictly increasing keys: no id twice)
            tri = np.where(np.arange(k)[None, :] < cnt[:, None], buf[:, :, 6].view(np.int32), -1 - np.arange(k)[None, :])
            s = np.sort(tri, axis=1)
            assert np.all(s[:, 1:] != s[:, :-1])  # and said directly: no id occurs twice in any ray's list
            assert np.array_equal(buf, out[0][k][0]) and np.array_equal(cnt, out[0][k][1])
        assert (out[30][16][1] >= 3).mean() > 0.1


# ---- 5. tree independence -----------------------------------------------------------------------------------------------------------
def _digest(buf, cnt):
    return hashlib.sha256(buf.tobytes() + cnt.tobytes()).hexdigest()


@pytest.mark.parametrize("name", ["cornell", "atrium_small", "soup"])
def test_one_digest_over_builders_and_layouts(scenes, name):
    from vkrt_amd import abi

    flat, _ = scenes[name]
    o, d = Q._hostile_rays(flat, 60001, seed=79)
    rays = Q._pack(o, d, 0.001, 10000.0)
    got = {}
    for kind in KINDS:
        for layout in (1, 0):
            r = Q._renderer(flat, kind, layout)
            got[(kind, layout)] = tuple(_digest(*_multi(r, rays, k)) for k in (3, 8))
            r.close()
    # the scheduling options of the other queries do not reach this call either
    r = Q._renderer(flat, "ploc", 1, {abi.VKRT_OPT_WF_SHARE: 0, abi.VKRT_OPT_TRI_THRESHOLD: 0})
    got["unscheduled"] = tuple(_digest(*_multi(r, rays, k)) for k in (3, 8))
    r.close()
    assert len(set(got.values())) == 1, got


@pytest.mark.parametrize("layout", [1, 0])
def test_refit_trees_answer_like_fresh_builds_and_stale_trees_are_refused(scenes, layout):
    import torch
    from scene_deform import send, third_of_meshes, twisted
    from vkrt_amd import abi

    flat, _ = scenes["atrium_small"]
    idx = np.sort(np.random.default_rng(23).choice(len(flat.nodes), len(flat.nodes) // 3, replace=False))
    mv, mats = moved(flat, idx, 23)
    r = Q._renderer(flat, "ploc", layout)
    r.reset_counters()
    o, d = Q._hostile_rays(mv, 60001, seed=83)
    rays = Q._pack(o, d, 0.001, 10000.0)
    apply(r, mats)
    # stale: refused, nothing written
    hits = torch.full((rays.shape[0], 4, 8), 7.0, dtype=torch.float32, device="cuda:0")
    opts = abi.QueryOpts(16, 0, 0xFF, 0)
    rc = r.lib.vkrt_intersect_multi(r._h, C.c_void_p(rays.data_ptr()), rays.shape[0], C.byref(opts), 4, C.c_void_p(hits.data_ptr()), None, None)
    assert rc == abi.VKRT_ERR_NOT_BUILT and b"vkrt_scene_update_nodes" in r.lib.vkrt_last_error()
    torch.cuda.synchronize()
    assert bool((hits == 7.0).all())
    r.refit()
    fresh = Q._renderer(mv, "ploc", layout)
    a, b = _multi(r, rays, 8), _multi(fresh, rays, 8)
    assert _digest(*a) == _digest(*b)
    assert (a[1] >= 2).mean() > 0.1
    moved_digest = _digest(*a)
    fresh.close()
    # deformation on top of the motion
    meshes = third_of_meshes(mv)
    df = twisted(mv, meshes)
    send(r, df, meshes)
    assert r.lib.vkrt_intersect_multi(r._h, C.c_void_p(rays.data_ptr()), rays.shape[0], C.byref(opts), 4, C.c_void_p(hits.data_ptr()), None,
                                      None) == abi.VKRT_ERR_NOT_BUILT
    r.refit()
    fresh = Q._renderer(df, "ploc", layout)
    a, b = _multi(r, rays, 8), _multi(fresh, rays, 8)
    assert _digest(*a) == _digest(*b)
    assert _digest(*a) != moved_digest  # (the deformation is seen)
    _no_faults(r)
    r.close()
    fresh.close()


# ---- 6. filters -------------------------------------------------------------------------------------------------------------------
def _assert_sublist(full, ref, nodemap, gmap, prim_of=None):
    """full = _multi of the filtered call, ref = _multi of the sub-scene: the same lists with the sub-scene's ids mapped back"""
    (fb, fc), (rb, rc) = full, ref
    assert np.array_equal(fc, rc)
    assert np.array_equal(fb[:, :, :3], rb[:, :, :3])
    live = np.arange(fb.shape[1])[None, :] < fc[:, None]
    fi, ri = fb[:, :, 3:].view(np.int32), rb[:, :, 3:].view(np.int32)
    assert np.all(fi[~live] == -1)
    assert np.array_equal(fi[live][:, 0], nodemap[ri[live][:, 0]])
    assert np.array_equal(fi[live][:, 3], gmap[ri[live][:, 3]])
    if prim_of is None:
        assert np.array_equal(fi[live][:, [1, 2, 4]], ri[live][:, [1, 2, 4]])
    else:
        assert np.array_equal(fi[live][:, 1], prim_of[ri[live][:, 3]])
        assert np.array_equal(fi[live][:, 4], ri[live][:, 4])


@pytest.mark.parametrize("kind,layout,wt", [("ploc", 1, 0), ("lbvh", 0, 0), ("sah", 1, 1), ("ploc", 0, 1)])
def test_masks_and_facing_equal_a_sub_scene(kind, layout, wt):
    scene = V._instanced_scene()
    rays = V._ray_sets(scene, 1)
    r = V._renderer(scene, kind, layout, wt)
    r.reset_counters()
    masks, flags = V._masks(len(scene.nodes), 11)
    r.set_instance_visibility(0, masks, flags)
    for cull in (0x12, 0xA5, 0xFF):
        keep = [i for i in range(len(scene.nodes)) if masks[i] & cull]
        sub, nodemap, gmap = V._subset(scene, keep)
        rs = V._renderer(sub, wt=wt)
        for name in ("camera_tmin", "diffuse", "shadow_tmin"):
            for k in (3, 16):
                _assert_sublist(_multi(r, rays[name], k, cull_mask=cull), _multi(rs, rays[name], k), nodemap, gmap)
        rs.close()
    for name in ("camera", "diffuse_tmin"):  # cull mask 0: count 0 everywhere, miss records
        buf, cnt = _multi(r, rays[name], 4, cull_mask=0)
        assert np.all(cnt == 0)
        _structure(buf, cnt, rays[name].cpu().numpy()[:, 7])
    fl = np.random.default_rng(21).integers(0, 4, len(scene.nodes)).astype(np.uint8)
    r.set_instance_visibility(0, np.full(len(scene.nodes), 0xFF, np.uint8), fl)
    dvec = V._directions(scene, 1, 22)[0]
    par = V._parallel_rays(dvec, 23)
    for cull in (V.BACK, V.FRONT):
        sub, nodemap, gmap, prim_of = V._facing_subscene(scene, dvec, fl, cull)
        rs = V._renderer(sub, wt=wt)
        for name, ry in par.items():
            got = _multi(r, ry, 16, ray_flags=cull)
            assert (got[1] >= 2).mean() > 0.01
            _assert_sublist(got, _multi(rs, ry, 16), nodemap, gmap, prim_of)
        rs.close()
    _no_faults(r)
    r.close()


@pytest.mark.parametrize("layout", [1, 0])
def test_watertight_and_dissolve_lists_equal_their_oracles(scenes, layout):
    import oracle_py
    from vkrt_amd import abi

    n = 2000
    flat, _ = scenes["soup"]
    orc = oracle_py.OracleScene(flat)
    orc.set_watertight(True)
    o, d = Q._hostile_rays(flat, n, seed=89)
    rays = Q._pack(o, d, 0.001, 10000.0)
    r = Q._renderer(flat, "ploc", layout, {abi.VKRT_OPT_WATERTIGHT: 1})
    r.reset_counters()
    peel = _peel_oracle(orc, o, d, 0.001, 10000.0, False)
    for k in (2, 16):
        buf, cnt = _multi(r, rays, k)
        _structure(buf, cnt, 10000.0, Q._flattened(flat))
        _assert_equals_peel(buf, cnt, peel)
    _no_faults(r)
    r.close()
    flat = Q._dissolving(scenes["cornell"][0])
    orc = oracle_py.OracleScene(flat)
    orc.set_dissolve(True)
    o, d = Q._hostile_rays(flat, n, seed=97)
    rays = Q._pack(o, d, 0.001, 10000.0)
    r = Q._renderer(flat, "ploc", layout, {abi.VKRT_OPT_ANYHIT_DISSOLVE: 1})
    r.reset_counters()
    peel = _peel_oracle(orc, o, d, 0.001, 10000.0, False)  # (the oracle's payload seed is 0)
    for k in (2, 16):
        buf, cnt = _multi(r, rays, k, seed=0)
        _structure(buf, cnt, 10000.0, Q._flattened(flat))
        _assert_equals_peel(buf, cnt, peel)
    a, b, c = _multi(r, rays, 16, seed=12345), _multi(r, rays, 16, seed=12345), _multi(r, rays, 16, seed=0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], c[0])  # the seed reaches the stage
    # VKRT_RAY_OPAQUE: the lists of a scene built without the stage
    ro = Q._renderer(flat, "ploc", layout)
    want = _multi(ro, rays, 16)
    got = _multi(r, rays, 16, seed=9, ray_flags=V.OPAQUE)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert want[1].sum() > c[1].sum()  # (the stage did ignore hits)
    ro.close()
    _no_faults(r)
    r.close()


# ---- 7. per-ray bounds and edge cases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 0])
def test_per_ray_bounds(scenes, layout):
    flat, orc = scenes["soup"]
    r = Q._renderer(flat, "ploc", layout)
    pairs = [(0.001, 10000.0), (0.0, 2.5), (0.5, float("inf")), (1.0, 3.0)]
    n = 2400
    o, d = Q._hostile_rays(flat, n, seed=101)
    g = np.random.default_rng(102).integers(0, 4, n)
    tmin = np.array([pairs[k][0] for k in g], np.float32)
    tmax = np.array([pairs[k][1] for k in g], np.float32)
    rays = Q._pack(o, d, tmin, tmax)
    peel = _peel_oracle(orc, o, d, tmin, tmax, True)
    for k in (3, 16):
        buf, cnt = _multi(r, rays, k)
        _structure(buf, cnt, tmax, Q._flattened(flat))
        _assert_equals_peel(buf, cnt, peel)
        t = buf[:, :, 0].view(np.float32)
        live = np.arange(k)[None, :] < cnt[:, None]
        assert np.all((t > tmin[:, None])[live]) and np.all((t < tmax[:, None])[live])
    assert cnt.max() >= 2 and all(cnt[g == m].max() >= 1 for m in range(4))
    r.close()


@pytest.mark.parametrize("layout", [1, 0])
def test_degenerate_rays_sizes_sentinels_and_null_counts(scenes, layout):
    import torch
    from vkrt_amd import abi

    flat, orc = scenes["cornell"]
    r = Q._renderer(flat, "ploc", layout)
    r.reset_counters()
    n = 4096
    o, d = Q._hostile_rays(flat, n, seed=23)
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
    buf, cnt = _multi(r, Q._pack(o, d, tmin, tmax), 5)
    bad = kind >= 2
    assert np.all(cnt[bad] == 0)
    _structure(buf, cnt, tmax)  # (all-miss records with t = the ray's tmax bits, NaN included)
    good = ~bad
    _assert_equals_peel(buf[good], cnt[good], _peel_oracle(orc, o[good], d[good], 0.001, 10000.0, True))
    # n not a multiple of 64, n = 1; sentinels behind hits[n * K] and counts[n]; counts = NULL
    opts = abi.QueryOpts(16, 0, 0xFF, 0)
    for n, k in ((60001, 3), (1, 16), (63, 7), (65, 1)):
        o, d = Q._hostile_rays(flat, n, seed=107)
        rays = Q._pack(o, d, 0.001, 10000.0)
        hits = torch.full((n * k + 4, 8), -3.0, dtype=torch.float32, device="cuda:0")
        counts = torch.full((n + 8,), -77, dtype=torch.int32, device="cuda:0")
        h = r.intersect_multi(rays, k, out=hits[:n * k].view(n, k, 8), counts=counts[:n])
        torch.cuda.synchronize()
        assert h.buffer.data_ptr() == hits.data_ptr() and h.count.data_ptr() == counts.data_ptr()
        assert bool((hits[n * k:] == -3.0).all()) and bool((counts[n:] == -77).all())
        want = h.buffer.cpu().numpy().view(np.uint32).copy()
        wc = counts[:n].cpu().numpy().copy()
        _structure(want, wc, 10000.0, Q._flattened(flat))
        assert np.array_equal(want[:, 0], _single(r, rays))  # the first record of every list is the closest hit
        hits.fill_(-3.0)
        rc = r.lib.vkrt_intersect_multi(r._h, C.c_void_p(rays.data_ptr()), n, C.byref(opts), k, C.c_void_p(hits.data_ptr()), None, None)
        assert rc == abi.VKRT_OK
        torch.cuda.synchronize()
        assert np.array_equal(hits[:n * k].cpu().numpy().view(np.uint32).reshape(n, k, 8), want)
        assert bool((hits[n * k:] == -3.0).all())
    # misaligned and NULL arrays, n == 0
    lib, hd = r.lib, r._h
    E = abi.VKRT_ERR_INVALID_ARGUMENT
    p = lambda x: C.c_void_p(x)  # noqa: E731
    assert lib.vkrt_intersect_multi(hd, p(rays.data_ptr() + 4), 1, C.byref(opts), 2, p(hits.data_ptr()), None, None) == E
    assert lib.vkrt_intersect_multi(hd, p(rays.data_ptr()), 1, C.byref(opts), 2, p(hits.data_ptr() + 8), None, None) == E
    assert lib.vkrt_intersect_multi(hd, p(rays.data_ptr()), 1, C.byref(opts), 2, p(hits.data_ptr()), p(counts.data_ptr() + 2), None) == E
    assert b"misaligned" in lib.vkrt_last_error()
    assert lib.vkrt_intersect_multi(hd, None, 1, C.byref(opts), 2, p(hits.data_ptr()), None, None) == E
    assert lib.vkrt_intersect_multi(hd, p(rays.data_ptr()), 1, C.byref(opts), 2, None, None, None) == E
    assert lib.vkrt_intersect_multi(hd, None, 0, C.byref(opts), 2, None, None, None) == abi.VKRT_OK
    empty = r.intersect_multi(torch.empty((0, 8), dtype=torch.float32, device="cuda:0"), 4)
    assert tuple(empty.buffer.shape) == (0, 4, 8) and empty.count.numel() == 0
    _no_faults(r)
    r.close()


def test_flat_feeds_surface_without_a_copy(scenes):
    import torch

    flat, _ = scenes["cornell"]
    r = Q._renderer(flat, "ploc")
    o, d = Q._hostile_rays(flat, 5000, seed=109)
    h = r.intersect_multi(Q._pack(o, d, 0.001, 10000.0), 4)
    f = h.flat()
    assert f.buffer.data_ptr() == h.buffer.data_ptr() and tuple(f.buffer.shape) == (20000, 8)
    s = r.surface(f)
    torch.cuda.synchronize()
    valid = s.valid.view(5000, 4).cpu().numpy()
    cnt = h.count.cpu().numpy()
    assert np.array_equal(valid, (np.arange(4)[None, :] < cnt[:, None]).astype(np.int32))
    r.close()


# ---- 8. stream order and isolation ----------------------------------------------------------------------------------------------
def test_multi_queries_are_ordered_on_the_callers_stream(scenes):
    import torch
    from vkrt_amd.renderer import pack_rays

    flat, _ = scenes["atrium_small"]
    r = Q._renderer(flat, "ploc")
    n, k = 200003, 4
    side = torch.cuda.Stream(device=0)
    hits_buf = torch.empty((n, k, 8), dtype=torch.float32, device="cuda:0")
    cnt_buf = torch.empty((n,), dtype=torch.int32, device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    for rep in range(3):
        o, d = Q._hostile_rays(flat, n, seed=40 + rep)
        o_h, d_h = torch.from_numpy(o).pin_memory(), torch.from_numpy(d).pin_memory()
        with torch.cuda.stream(side):
            busy = torch.randn(2048, 2048, device="cuda:0")
            for _ in range(4):
                busy = busy @ busy * 1e-3  # work in front of the ray writes on the same stream
            rays = pack_rays(o_h.to("cuda:0", non_blocking=True) + busy[0, 0] * 0, d_h.to("cuda:0", non_blocking=True), tmin=0.001, tmax=10000.0)
            h = r.intersect_multi(rays, k, out=hits_buf, counts=cnt_buf, stream=side)
        assert h.buffer.data_ptr() == hits_buf.data_ptr() and h.count.data_ptr() == cnt_buf.data_ptr()
        side.synchronize()
        got = hits_buf.cpu().numpy().view(np.uint32).copy(), cnt_buf.cpu().numpy().copy()
        want = _multi(r, Q._pack(o, d, 0.001, 10000.0), k)  # the same rays, after everything has settled
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert (got[1] > 0).mean() > 0.15
    r.close()


def test_config1_image_unchanged_by_multi_queries(scenes):
    from vkrt_amd.flat_scene import make_push_constants

    flat, _ = scenes["cornell"]
    W = H = 256
    cam = default_camera(W, H)
    pc = make_push_constants(samples=1, depth=1, frame=0, lights_count=len(flat.lights))

    def digest(r):
        return hashlib.sha256(r.pathtrace(pc, cam, W, H, seed=0).cpu().numpy().tobytes()).hexdigest()

    r = Q._renderer(flat, "ploc")
    before = digest(r)
    o, d = Q._hostile_rays(flat, 100000, seed=59)
    rays = Q._pack(o, d, 0.001, 10000.0)
    for k in (1, 16):
        _multi(r, rays, k)
        assert digest(r) == before
    other = Q._renderer(flat, "ploc")
    assert digest(other) == before
    r.close()
    other.close()
