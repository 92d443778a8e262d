"""Morph targets on the GPU: vkrt_scene_add_morph / vkrt_scene_morph_vertices against the numpy restatement tests/np_morph.py.  No
tolerance anywhere: the morphed vertices equal np_morph in every bit, a morphed + refitted scene equals a fresh Renderer created from
the np_morph arrays by the yardstick of test_gpu_skin.py, and a morph inside a skin followed by the skin equals np_skin applied to the
np_morph result."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import np_motion
import scene_deform as sd
import scene_morph as sm
import scene_skin as ss
from conftest import ROOT, default_camera

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu
ATTRS = (("positions", "positions"), ("normals", "normals"), ("tangents", "tangents"), ("texcoords0", "texcoords0"))
F = np.float32


@pytest.fixture(scope="module")
def atrium_small():
    import atrium

    flat, _ = atrium.build_atrium(20000, seed=4, with_textures=True)
    return flat


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _add(r, m, stream=None):
    return r.add_morph(m["first"], stream=stream, **sm.deltas(m))


def _pose(r, morph, weights, device=False, stream=None):
    if device:
        import torch

        weights = torch.as_tensor(weights).to("cuda:0")
    r.morph(morph, weights, stream=stream)
    return weights


def _assert_vertices(r, flat, what=None):
    """the live vertices of the whole scene equal the arrays of `flat` in every bit"""
    got = r.read_vertices(0, len(flat.positions))
    for k, attr in ATTRS:
        assert np.array_equal(_bits(got[k]), _bits(getattr(flat, attr))), (what, k)


# ---- 1. word for word, 2. restore -------------------------------------------------------------------------------------------------------
def _word_for_word(flat, morphs, device):
    from vkrt_amd.renderer import Renderer

    r = Renderer(flat, device=0, build="ploc")
    _assert_vertices(r, flat, "as created")
    ids = [_add(r, m) for m in morphs]
    assert ids == list(range(len(morphs)))
    _assert_vertices(r, flat, "after add_morph")
    keep = [_pose(r, i, m["weights"], device=device) for i, m in zip(ids, morphs)]
    want = sm.morphed(flat, morphs)
    for m in morphs:
        sl = slice(m["first"], m["first"] + m["count"])
        for a, attr in zip(sm.ATTRS, ("positions", "normals", "tangents")):
            moved = not np.array_equal(_bits(getattr(want, attr)[sl]), _bits(getattr(flat, attr)[sl]))
            assert moved == (m[a] is not None and m["kind"] != "zero"), (m["first"], a)
    _assert_vertices(r, want, "morphed")  # (texture coordinates and every vertex outside the ranges: the created scene's)
    # a second pose starts from the captured base, not from the first: nothing accumulates
    again = [dict(m, weights=sm.weights(m["target_count"], "negative", 700 + i)) for i, m in enumerate(morphs)]
    keep += [_pose(r, i, m["weights"], device=device) for i, m in zip(ids, again)]
    _assert_vertices(r, sm.morphed(flat, again), "second pose")
    # all-zero weights (of either sign) give the created scene back in every bit
    keep += [_pose(r, i, sm.weights(m["target_count"], "zero", 0), device=device) for i, m in zip(ids, morphs)]
    _assert_vertices(r, flat, "restored")
    del keep
    r.close()


@pytest.mark.parametrize("device", [False, True])
def test_cornell_boxes_and_odd_subranges_equal_np_morph(cornell_flat, device):
    morphs = sm.cornell_cases(cornell_flat) + sm.cornell_subrange_cases(cornell_flat)
    assert [m["count"] for m in morphs[2:]] == [1, 2, 63] and all(m["first"] % 2 == 1 for m in morphs[2:])
    assert sorted(m["target_count"] for m in morphs) == [1, 2, 2, 2, 33]
    _word_for_word(cornell_flat, morphs, device)


@pytest.mark.parametrize("device", [False, True])
def test_more_targets_than_lanes_equal_np_morph(cornell_flat, device):
    morphs = sm.cornell_many_target_cases(cornell_flat)
    assert [m["target_count"] for m in morphs] == [130, 256]
    _word_for_word(cornell_flat, morphs, device)


@pytest.mark.parametrize("device", [False, True])
def test_atrium_ranges_equal_np_morph(atrium_small, device):
    morphs = sm.atrium_cases(atrium_small)
    assert [m["count"] for m in morphs[:2]] == [65, 257] and morphs[2]["first"] + morphs[2]["count"] == len(atrium_small.positions)
    assert [m["target_count"] for m in morphs] == [2, 33, 1]
    _word_for_word(atrium_small, morphs, device)


def test_updates_on_a_morphed_range_keep_texcoords_and_lose_positions(atrium_small):
    from vkrt_amd.renderer import Renderer

    flat = atrium_small
    morphs = sm.atrium_cases(flat)
    r = Renderer(flat, device=0, build="ploc")
    for m in morphs:
        _add(r, m)
    m0 = morphs[1]
    uv = np.random.default_rng(9).uniform(0, 2, (m0["count"], 2)).astype(F)
    r.update_vertices(m0["first"], positions=np.zeros((m0["count"], 3), F), texcoords0=uv)
    for i, m in enumerate(morphs):
        _pose(r, i, m["weights"])
    tex = flat.texcoords0.copy()
    tex[m0["first"]:m0["first"] + m0["count"]] = uv
    _assert_vertices(r, sd.with_arrays(sm.morphed(flat, morphs), texcoords0=tex), "update, then morph")
    r.close()


# ---- 3. the refit ----------------------------------------------------------------------------------------------------------------------
def _render(r, flat, W, H, seed=3, frames=2):
    from vkrt_amd.flat_scene import make_push_constants

    cam = default_camera(W, H)
    r.reset_counters()
    img = None
    for f in range(frames):
        img = r.pathtrace(make_push_constants(samples=2, depth=4, frame=f, lights_count=len(flat.lights)), cam, W, H, seed=seed + f, image=img)
    return sd.digest(img), r.counters()


@pytest.mark.parametrize("kind,layout", [("ploc", "wide8"), ("lbvh", "wide8"), ("sah", "bvh2")])
def test_morphed_and_refitted_equals_a_fresh_scene(cornell_flat, kind, layout):
    import torch
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer, pack_rays

    flat = cornell_flat
    morphs = sm.cornell_cases(flat)
    want = sm.morphed(flat, morphs)
    options = {abi.VKRT_OPT_BVH_LAYOUT: 0} if layout == "bvh2" else None
    r = Renderer(flat, device=0, build=kind, options=options)
    reached = r.check_accel()["nodes_reached"]
    node_count = r.accel_info()["node_count"]
    for m in morphs:
        _pose(r, _add(r, m), m["weights"])
    r.refit()
    sd.assert_sound(r.check_accel(), reached)
    assert r.accel_info()["node_count"] == node_count
    f = Renderer(want, device=0, build=kind, options=options)
    got, ref = _render(r, want, 64, 64), _render(f, want, 64, 64)
    assert got[0] == ref[0]
    for c in ("rays_closest", "rays_shadow", "pixels"):
        assert got[1][c] == ref[1][c], c
    assert got[1]["traversal_faults"] == 0 and ref[1]["traversal_faults"] == 0
    o, d = sd.random_rays(want, 4096)
    rays = pack_rays(torch.as_tensor(o, device="cuda:0"), torch.as_tensor(d, device="cuda:0"), 0.001, 1e4)
    ha, hb = r.intersect(rays), f.intersect(rays)
    a, b = ha.buffer.cpu().numpy(), hb.buffer.cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and (a.view(np.int32)[:, 3] >= 0).mean() > 0.1
    sa, sb = r.surface(ha).buffer.cpu().numpy(), f.surface(hb).buffer.cpu().numpy()
    assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
    # the refitted scene is not the unmorphed one
    g = Renderer(flat, device=0, build=kind, options=options)
    assert _render(g, flat, 64, 64)[0] != ref[0]
    for x in (r, f, g):
        x.close()


# ---- 4. morph, then skin -----------------------------------------------------------------------------------------------------------------
def _skin_and_inner_morph(flat):
    k = ss.cornell_cases(flat)[1]
    assert k["count"] >= 8
    first = k["first"] + 1 + k["first"] % 2  # an odd vertex, and an odd offset into the skin where the skin starts even
    count = k["count"] - 3 - k["first"] % 2
    m = sm.make(flat, first, count, 33, 77, kind="gaps")
    assert first % 2 == 1 and first > k["first"] and first + count < k["first"] + k["count"]
    return k, m


@pytest.mark.parametrize("device", [False, True])
def test_morph_inside_a_skin_then_skin_equals_np_skin_of_np_morph(cornell_flat, device):
    import torch
    from vkrt_amd.renderer import Renderer, pack_rays

    flat = cornell_flat
    k, m = _skin_and_inner_morph(flat)
    outer = sm.make(flat, 1, 4, 2, 78, kind="above1")  # an unskinned morph beside it
    r = Renderer(flat, device=0, build="ploc")
    o, d = sd.random_rays(flat, 2048)
    rays = pack_rays(torch.as_tensor(o, device="cuda:0"), torch.as_tensor(d, device="cuda:0"), 0.001, 1e4)
    before = r.intersect(rays).buffer.cpu().numpy()
    sk = r.add_skin(k["first"], k["joints"], k["weights"], joint_count=k["joint_count"])
    assert _add(r, m) == 0 and _add(r, outer) == 1
    keep = [_pose(r, 0, m["weights"], device=device)]
    # between the two calls: the live arrays are the created scene's and the tree is not stale
    _assert_vertices(r, flat, "after the inner morph")
    assert np.array_equal(r.intersect(rays).buffer.cpu().numpy().view(np.uint32), before.view(np.uint32))
    r.skin(sk, k["matrices"])
    want = ss.posed(flat, [k], base=sm.morphed(flat, [m]))
    assert not np.array_equal(_bits(want.positions), _bits(ss.posed(flat, [k]).positions))
    _assert_vertices(r, want, "morph, then skin")
    # the unskinned morph is independent of both
    keep.append(_pose(r, 1, outer["weights"], device=device))
    want = sm.morphed(want, [outer], base=flat)
    _assert_vertices(r, want, "and the outer morph")
    # zero weights, then the skin: the skin-only result
    keep.append(_pose(r, 0, sm.weights(33, "zero", 0), device=device))
    _assert_vertices(r, want, "zero weights before the skin call")
    r.skin(sk, k["matrices"])
    _assert_vertices(r, sm.morphed(ss.posed(flat, [k]), [outer], base=flat), "skin only")
    del keep
    r.close()


# ---- 5. refusals that need a device --------------------------------------------------------------------------------------------------
def test_overlap_straddle_two_skins_and_skin_over_morph_are_refused(cornell_flat):
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer, VkrtError

    flat = cornell_flat
    a, b = ss.cornell_cases(flat)
    assert a["first"] + a["count"] <= b["first"] and a["first"] >= 8
    r = Renderer(flat, device=0, build="ploc")
    for k in (a, b):
        r.add_skin(k["first"], k["joints"], k["weights"], joint_count=k["joint_count"])
    m0 = sm.make(flat, 1, 4, 2, 80)
    assert _add(r, m0) == 0
    end_a, end_b = a["first"] + a["count"], b["first"] + b["count"]
    cases = [((0, 2), b"overlap morph 0"), ((4, 3), b"overlap morph 0"), ((1, 4), b"overlap morph 0"),          # a morph's range
             ((a["first"] - 1, 2), b"straddle"), ((end_a - 1, 2), b"straddle"), ((a["first"] - 1, a["count"] + 2), b"straddle"),
             ((end_a - 2, b["first"] - end_a + 4), b"straddle"),                                                    # touches two skins
             ((a["first"], end_b - a["first"]), b"straddle")]
    for (first, count), word in cases:
        dp = np.zeros((1, count, 3), F)
        desc = abi.MorphDesc(C.sizeof(abi.MorphDesc), first, count, 1, dp.ctypes.data, None, None)
        out = abi.c_u(77)
        assert r.lib.vkrt_scene_add_morph(r._h, C.byref(desc), None, C.byref(out)) == abi.VKRT_ERR_INVALID_ARGUMENT
        msg = r.lib.vkrt_last_error()
        assert word in msg and b"vkrt_scene_add_morph" in msg and out.value == 77, msg
        with pytest.raises(VkrtError, match=word.decode().split()[0]):
            r.add_morph(first, position_deltas=dp)
    # the remaining refusals of the header's list that need a scene: the range, the empty range
    dp = np.zeros((1, 2, 3), F)
    for first, count, word in ((len(flat.positions) - 1, 2, b"outside the scene"), (0xFFFFFFFF, 2, b"outside the scene"), (6, 0, b"count is 0")):
        desc = abi.MorphDesc(C.sizeof(abi.MorphDesc), first, count, 1, dp.ctypes.data, None, None)
        out = abi.c_u(77)
        assert r.lib.vkrt_scene_add_morph(r._h, C.byref(desc), None, C.byref(out)) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert word in r.lib.vkrt_last_error() and out.value == 77
    # a skin over a morph
    j, w = np.zeros((2, 4), np.uint16), np.full((2, 4), 0.25, F)
    desc = abi.SkinDesc(C.sizeof(abi.SkinDesc), 4, 2, 1, j.ctypes.data, w.ctypes.data)
    out = abi.c_u(77)
    assert r.lib.vkrt_scene_add_skin(r._h, C.byref(desc), None, C.byref(out)) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"overlap morph 0" in r.lib.vkrt_last_error() and b"vkrt_scene_add_skin" in r.lib.vkrt_last_error() and out.value == 77
    with pytest.raises(VkrtError, match="overlap morph 0"):
        r.add_skin(4, j, w)
    # vkrt_scene_morph_vertices: the index, the weights
    wz = np.zeros(2, F)
    assert r.lib.vkrt_scene_morph_vertices(r._h, 1, wz.ctypes.data, abi.VKRT_MEMORY_HOST, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"morph 1" in r.lib.vkrt_last_error()
    for memory, ptr, word in ((abi.VKRT_MEMORY_HOST, None, b"weights is NULL"), (abi.VKRT_MEMORY_DEVICE, None, b"weights is NULL"),
                              (abi.VKRT_MEMORY_DEVICE, 0x1002, b"4-byte aligned")):
        assert r.lib.vkrt_scene_morph_vertices(r._h, 0, ptr, memory, None) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert word in r.lib.vkrt_last_error()
    nan = np.array([1.0, np.nan], F)
    assert r.lib.vkrt_scene_morph_vertices(r._h, 0, nan.ctypes.data, abi.VKRT_MEMORY_HOST, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"weights[1] is not finite" in r.lib.vkrt_last_error()
    _assert_vertices(r, flat, "refusals change nothing")
    assert len(r._morphs) == 1 and len(r._skins) == 2
    # the ranges next to the refused ones are free: beside the morph, inside a skin up to both of its edges
    assert r.add_morph(5, position_deltas=np.zeros((1, 2, 3), F)) == 1
    assert r.add_morph(a["first"], position_deltas=np.zeros((1, a["count"], 3), F)) == 2
    _pose(r, 0, m0["weights"])
    _assert_vertices(r, sm.morphed(flat, [m0]), "morph 0 alone")
    r.close()


# ---- 6. a stale tree, the motion snapshot ----------------------------------------------------------------------------------------------
def test_stale_tree_surface_and_motion(cornell_flat):
    import torch
    from vkrt_amd.renderer import Renderer, VkrtError, pack_rays

    flat = cornell_flat
    morphs = sm.cornell_cases(flat)
    want = sm.morphed(flat, morphs)
    r = Renderer(flat, device=0, build="ploc")
    ids = [_add(r, m) for m in morphs]
    o, d = sd.random_rays(flat, 60000)
    rays = pack_rays(torch.as_tensor(o, device="cuda:0"), torch.as_tensor(d, device="cuda:0"), 0.001, 1e4)
    hits = r.intersect(rays)  # (adding a morph moves nothing: the tree is not stale)
    h = hits.buffer.cpu().numpy()
    moved = np.isin(h.view(np.int32)[:, 3], [len(flat.nodes) - 2, len(flat.nodes) - 1])
    assert moved.sum() > 1000  # (the two boxes take about 2.4 % of rays drawn over the room's bounds)
    r.motion_mark()
    for i, m in zip(ids, morphs):
        _pose(r, i, m["weights"])
    with pytest.raises(VkrtError, match=r"\(5\)"):  # VKRT_ERR_NOT_BUILT
        r.intersect(rays)
    cur, prev = r.hit_motion(hits)
    cur, prev = cur.cpu().numpy(), prev.cpu().numpy()
    assert np.array_equal(_bits(prev), _bits(np_motion.hit_points(flat, h)))
    assert np.array_equal(_bits(cur), _bits(np_motion.hit_points(want, h)))
    assert (np.abs(cur - prev).max(-1) > 0)[moved].mean() > 0.9 and not (cur != prev)[~moved].any()
    f = Renderer(want, device=0, build="ploc")
    sa, sb = r.surface(hits).buffer.cpu().numpy(), f.surface(hits).buffer.cpu().numpy()
    assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
    r.refit()
    r.intersect(rays)
    assert r.counters()["traversal_faults"] == 0
    r.close()
    f.close()


# ---- 7. stream order -------------------------------------------------------------------------------------------------------------------
def test_device_weights_written_on_the_same_stream_just_before(cornell_flat):
    """One weight buffer, on a non-default stream: a torch op writes pose A into it, morph 0 reads it, a torch op overwrites it with pose
    B, morph 1 reads it -- enqueued back to back behind a long-running op, nothing waits on the host until the read-back."""
    import torch
    from vkrt_amd.renderer import Renderer

    flat = cornell_flat
    a, b = sm.cornell_cases(flat)
    b = sm.make(flat, b["first"], b["count"], a["target_count"], 90, kind="negative")
    r = Renderer(flat, device=0, build="ploc")
    assert [_add(r, a), _add(r, b)] == [0, 1]
    s = torch.cuda.Stream(device=0)
    wa, wb = (torch.as_tensor(m["weights"]).to("cuda:0") for m in (a, b))
    w = torch.full((a["target_count"],), 5.0, dtype=torch.float32, device="cuda:0")
    big = torch.ones((2048, 2048), device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(8):
            big = (big @ big) * (1.0 / 2048.0)
        torch.add(wa, big[0, 0] - 1.0, out=w)  # pose A (big stays all ones), available only when the products are done
        r.morph(0, w, stream=s)
        w.copy_(wb)
        r.morph(1, w, stream=s)
    s.synchronize()
    assert float(big[0, 0]) == 1.0
    _assert_vertices(r, sm.morphed(flat, [a, b]), "A into morph 0, B into morph 1")
    r.close()


# ---- 8. the C++ host layer ---------------------------------------------------------------------------------------------------------------
def test_cpp_host_morphs_a_gltf_file(tmp_path):
    """The loader's morphs + HelloVkrt's default weights at load, then morphVertices + refitAccel through the host_py hook, render the
    pixels of a fresh scene made from the np_morph arrays: as authored, and after two poses in a row, the second from the base shape."""
    import np_morph
    import test_host_morph as thm
    import test_host_skin as ths
    from vkrt_amd import abi, host_py
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Renderer

    path = ths._write(tmp_path, *thm._document())
    flat = host_py.load_gltf(path)
    morphs = host_py.load_gltf_morphs(path)
    assert len(morphs) == 3 and any(w != 0 for w in morphs[0]["weights"])
    poses = np.array([[0.5, 0.25], [1.0, -0.5]], F)
    W, H = 96, 64
    cam = dict(eye=(1.0, 1.0, 6.0), center=(1.0, 1.0, 0.0))
    kw = dict(samples=2, depth=4, frames=2, seed0=10, build=abi.VKRT_BUILD_PLOC_GPU, **cam)
    authored, count = host_py.render_gltf_morphed(path, W, H, **kw)
    posed, _ = host_py.render_gltf_morphed(path, W, H, morph=0, weights=poses, **kw)
    assert count == 3

    def want(bar_weights):
        pos, nrm, tan = flat.positions.copy(), flat.normals.copy(), flat.tangents.copy()
        for i, m in enumerate(morphs):
            sl = slice(m["first"], m["first"] + m["count"])
            w = bar_weights if i == 0 and bar_weights is not None else m["weights"]
            pos[sl], nrm[sl], tan[sl] = np_morph.morph(w, flat.positions[sl], flat.normals[sl], flat.tangents[sl], m["position_deltas"], m["normal_deltas"],
                                                       m["tangent_deltas"])
        return sd.with_arrays(flat, positions=pos, normals=nrm, tangents=tan)

    u = host_py.global_uniforms(width=W, height=H, **cam)

    def render(f):
        r = Renderer(f, device=0, build="ploc")
        out = None
        for k in range(2):
            out = r.pathtrace(make_push_constants(samples=2, depth=4, frame=k, lights_count=len(f.lights)), u, W, H, seed=10 + k, image=out)
        r.close()
        return out.cpu().numpy()

    ref_authored, ref_posed, ref_base = render(want(None)), render(want(poses[1])), render(flat)
    assert np.array_equal(authored.view(np.uint32), ref_authored.view(np.uint32))
    assert np.array_equal(posed.view(np.uint32), ref_posed.view(np.uint32))
    # (the default weights and the pose are in view)
    assert not np.array_equal(ref_authored.view(np.uint32), ref_base.view(np.uint32))
    assert not np.array_equal(ref_posed.view(np.uint32), ref_authored.view(np.uint32))
