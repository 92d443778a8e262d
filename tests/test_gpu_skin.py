"""Skinned meshes on the GPU: vkrt_scene_add_skin / vkrt_scene_skin_vertices / vkrt_debug_read_vertices against the numpy restatement
tests/np_skin.py.  No tolerance anywhere: the posed vertices equal np_skin in every bit, and a skinned + refitted scene equals a fresh
Renderer created from the np_skin arrays by the yardstick of test_gpu_vertex_update.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import np_motion
import scene_deform as sd
import scene_skin as ss
from conftest import ROOT, default_camera

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu
ATTRS = (("positions", "positions"), ("normals", "normals"), ("tangents", "tangents"), ("texcoords0", "texcoords0"))


@pytest.fixture(scope="module")
def atrium_small():
    import atrium

    flat, _ = atrium.build_atrium(20000, seed=4, with_textures=True)
    return flat


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _add(r, k, stream=None):
    return r.add_skin(k["first"], k["joints"], k["weights"], joint_count=k["joint_count"], stream=stream)


def _pose(r, skin, matrices, device=False, stream=None):
    if device:
        import torch

        matrices = torch.as_tensor(matrices).to("cuda:0")
        assert matrices.data_ptr() % 16 == 0
    r.skin(skin, matrices, stream=stream)
    return matrices


def _assert_vertices(r, flat, what=None):
    """the live vertices of the whole scene equal the arrays of `flat` in every bit"""
    got = r.read_vertices(0, len(flat.positions))
    for k, attr in ATTRS:
        assert np.array_equal(_bits(got[k]), _bits(getattr(flat, attr))), (what, k)


# ---- 1. word for word --------------------------------------------------------------------------------------------------------------------
def _word_for_word(flat, skins, device):
    from vkrt_amd.renderer import Renderer

    r = Renderer(flat, device=0, build="ploc")
    _assert_vertices(r, flat, "as created")
    ids = [_add(r, k) for k in skins]
    assert ids == list(range(len(skins)))
    _assert_vertices(r, flat, "after add_skin")
    keep = [_pose(r, i, k["matrices"], device=device) for i, k in zip(ids, skins)]
    want = ss.posed(flat, skins)
    for k in skins:
        sl = slice(k["first"], k["first"] + k["count"])
        assert not np.array_equal(want.positions[sl], flat.positions[sl]) and not np.array_equal(want.normals[sl], flat.normals[sl])
    _assert_vertices(r, want, "posed")  # (texture coordinates and every vertex outside the ranges: the created scene's)
    # a partial read, from an odd vertex, with arrays left out
    out = np.zeros((7, 3), np.float32)
    first = skins[-1]["first"] + skins[-1]["count"] - 7
    assert r.lib.vkrt_debug_read_vertices(r._h, first, 7, None, out.ctypes.data, None, None) == 0
    assert np.array_equal(_bits(out), _bits(want.normals[first:first + 7]))
    del keep
    r.close()


@pytest.mark.parametrize("device", [False, True])
def test_cornell_boxes_and_odd_subranges_equal_np_skin(cornell_flat, device):
    skins = ss.cornell_cases(cornell_flat) + ss.cornell_subrange_cases(cornell_flat)
    assert [k["count"] for k in skins[2:]] == [1, 63] and all(k["first"] % 2 == 1 for k in skins[2:])
    assert sorted(k["joint_count"] for k in skins) == [1, 2, 33, 33] and all(int(k["joints"].max()) == k["joint_count"] - 1 for k in skins)
    _word_for_word(cornell_flat, skins, device)


@pytest.mark.parametrize("device", [False, True])
def test_atrium_ranges_equal_np_skin(atrium_small, device):
    skins = ss.atrium_cases(atrium_small)
    assert [k["count"] for k in skins[:2]] == [65, 257] and skins[2]["first"] + skins[2]["count"] == len(atrium_small.positions)
    assert [k["joint_count"] for k in skins] == [1, 2, 33]
    _word_for_word(atrium_small, skins, device)


# ---- 2. the refit ----------------------------------------------------------------------------------------------------------------------
def _render(r, flat, W, H, seed=3, frames=2):
    from vkrt_amd.flat_scene import make_push_constants

    cam = default_camera(W, H)
    r.reset_counters()
    img = None
    for f in range(frames):
        img = r.pathtrace(make_push_constants(samples=2, depth=4, frame=f, lights_count=len(flat.lights)), cam, W, H, seed=seed + f, image=img)
    return sd.digest(img), r.counters()


@pytest.mark.parametrize("layout", ["wide8", "bvh2"])
@pytest.mark.parametrize("kind", ["ploc", "lbvh", "sah"])
def test_skinned_and_refitted_equals_a_fresh_scene(cornell_flat, kind, layout):
    import torch
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer, pack_rays

    flat = cornell_flat
    skins = ss.cornell_cases(flat)
    want = ss.posed(flat, skins)
    options = {abi.VKRT_OPT_BVH_LAYOUT: 0} if layout == "bvh2" else None
    r = Renderer(flat, device=0, build=kind, options=options)
    reached = r.check_accel()["nodes_reached"]
    node_count = r.accel_info()["node_count"]
    for k in skins:
        _pose(r, _add(r, k), k["matrices"])
    r.refit()
    sd.assert_sound(r.check_accel(), reached)
    assert r.accel_info()["node_count"] == node_count
    f = Renderer(want, device=0, build=kind, options=options)
    got, ref = _render(r, want, 64, 64), _render(f, want, 64, 64)
    assert got[0] == ref[0]
    for c in ("rays_closest", "rays_shadow", "pixels"):
        assert got[1][c] == ref[1][c], c
    assert got[1]["traversal_faults"] == 0 and ref[1]["traversal_faults"] == 0
    o, d = sd.random_rays(want)
    sd.assert_same_trace(r.trace_rays(o, d), f.trace_rays(o, d))
    rays = pack_rays(torch.as_tensor(o, device="cuda:0"), torch.as_tensor(d, device="cuda:0"), 0.001, 1e4)
    ha, hb = r.intersect(rays), f.intersect(rays)
    a, b = ha.buffer.cpu().numpy(), hb.buffer.cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and (a.view(np.int32)[:, 3] >= 0).mean() > 0.1
    sa, sb = r.surface(ha).buffer.cpu().numpy(), f.surface(hb).buffer.cpu().numpy()
    assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
    r.close()
    f.close()


# ---- 3. host and device matrices, poses do not accumulate, texture coordinates stay --------------------------------------------------
def test_host_and_device_matrices_second_pose_and_kept_texcoords(atrium_small):
    from vkrt_amd.renderer import Renderer

    flat = atrium_small
    skins = ss.atrium_cases(flat)
    total = len(flat.positions)
    second = [dict(k, matrices=ss.joint_matrices(k["joint_count"], 900 + i, amount=0.5)) for i, k in enumerate(skins)]
    reads = []
    for device in (False, True):
        r = Renderer(flat, device=0, build="ploc")
        keep = [_pose(r, _add(r, k), k["matrices"], device=device) for k in skins]
        first_pose = r.read_vertices(0, total)
        # texture coordinates sent to a skinned range stay through the next skin call; positions sent there are overwritten from the bind pose
        k0 = skins[1]
        uv = np.random.default_rng(9).uniform(0, 2, (k0["count"], 2)).astype(np.float32)
        r.update_vertices(k0["first"], positions=np.zeros((k0["count"], 3), np.float32), texcoords0=uv)
        keep += [_pose(r, i, k["matrices"], device=device) for i, k in enumerate(second)]
        reads.append((first_pose, r.read_vertices(0, total)))
        del keep
        r.close()
    for k, _ in ATTRS:
        assert np.array_equal(_bits(reads[0][0][k]), _bits(reads[1][0][k])) and np.array_equal(_bits(reads[0][1][k]), _bits(reads[1][1][k])), k
    want = ss.posed(flat, second)  # the second pose from the bind pose, as on a fresh scene: nothing accumulates
    tex = flat.texcoords0.copy()
    tex[k0["first"]:k0["first"] + k0["count"]] = uv
    want = sd.with_arrays(want, texcoords0=tex)
    for k, attr in ATTRS:
        assert np.array_equal(_bits(reads[0][1][k]), _bits(getattr(want, attr))), k
    assert not np.array_equal(reads[0][0]["positions"], reads[0][1]["positions"])


# ---- 4. a stale tree -------------------------------------------------------------------------------------------------------------------
def test_stale_tree_surface_and_motion(cornell_flat):
    import torch
    from vkrt_amd.renderer import Renderer, VkrtError, pack_rays

    flat = cornell_flat
    skins = ss.cornell_cases(flat)
    want = ss.posed(flat, skins)
    r = Renderer(flat, device=0, build="ploc")
    ids = [_add(r, k) for k in skins]
    o, d = sd.random_rays(flat, 60000)
    rays = pack_rays(torch.as_tensor(o, device="cuda:0"), torch.as_tensor(d, device="cuda:0"), 0.001, 1e4)
    hits = r.intersect(rays)  # (adding a skin moves nothing: the tree is not stale)
    h = hits.buffer.cpu().numpy()
    moved = np.isin(h.view(np.int32)[:, 3], [len(flat.nodes) - 2, len(flat.nodes) - 1])
    assert moved.sum() > 1000  # (the two boxes take about 2.4 % of rays drawn over the room's bounds)
    r.motion_mark()
    for i, k in zip(ids, skins):
        _pose(r, i, k["matrices"])
    with pytest.raises(VkrtError, match=r"\(5\)"):
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
    r.close()
    f.close()


# ---- 5. skin bookkeeping ---------------------------------------------------------------------------------------------------------------
def test_overlap_is_refused_and_disjoint_skins_pose_independently(cornell_flat):
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer, VkrtError

    flat = cornell_flat
    a, b = ss.cornell_cases(flat)
    r = Renderer(flat, device=0, build="ploc")
    assert _add(r, a) == 0
    # an overlap of one vertex at either end, and the same range again: refused by the library (and, before it, by the Python layer)
    for first, count in ((a["first"] - 3, 4), (a["first"] + a["count"] - 1, 2), (a["first"], a["count"])):
        j, w = np.zeros((count, 4), np.uint16), np.full((count, 4), 0.25, np.float32)
        desc = abi.SkinDesc(C.sizeof(abi.SkinDesc), first, count, 1, j.ctypes.data, w.ctypes.data)
        out = abi.c_u(77)
        assert r.lib.vkrt_scene_add_skin(r._h, C.byref(desc), None, C.byref(out)) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert b"overlap" in r.lib.vkrt_last_error() and out.value == 77
        with pytest.raises(VkrtError, match="overlap"):
            r.add_skin(first, j, w)
    assert r.lib.vkrt_scene_skin_vertices(r._h, 1, a["matrices"].ctypes.data, abi.VKRT_MEMORY_HOST, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"skin 1" in r.lib.vkrt_last_error()
    nan = a["matrices"].copy()
    nan[-1, 3] = np.nan  # (row 3 is not read, but every element is checked)
    assert r.lib.vkrt_scene_skin_vertices(r._h, 0, nan.ctypes.data, abi.VKRT_MEMORY_HOST, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"not finite" in r.lib.vkrt_last_error()
    _assert_vertices(r, flat, "refusals change nothing")
    # the adjacent ranges on both sides are free
    assert _add(r, b) == 1
    _pose(r, 1, b["matrices"])
    _assert_vertices(r, ss.posed(flat, [b]), "skin 1 alone")
    _pose(r, 0, a["matrices"])
    _assert_vertices(r, ss.posed(flat, [a, b]), "both")
    _pose(r, 1, ss.joint_matrices(b["joint_count"], 5, amount=0.3))
    _assert_vertices(r, ss.posed(flat, [a, dict(b, matrices=ss.joint_matrices(b["joint_count"], 5, amount=0.3))]), "skin 1 again")
    r.close()


# ---- 6. the C++ host layer ---------------------------------------------------------------------------------------------------------------
def test_cpp_host_skins_a_gltf_file(tmp_path):
    """The loader's skin + HelloVkrt::skinVertices + refitAccel through the host_py hook render the pixels of a fresh scene made from the
    np_skin arrays; two poses in a row, the second from the bind pose."""
    import np_skin
    import test_host_skin as ths
    from vkrt_amd import abi, host_py
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Renderer

    path = ths._write(tmp_path, *ths._document())
    flat = host_py.load_gltf(path)
    sk = host_py.load_gltf_skins(path)
    poses = np.stack([ss.joint_matrices(2, 21, amount=0.4), ss.joint_matrices(2, 22)])
    W, H = 96, 64
    cam = dict(eye=(1.5, 1.0, 6.0), center=(1.5, 1.0, 0.0))
    img, count = host_py.render_gltf_skinned(path, W, H, 0, poses, samples=2, depth=4, frames=2, seed0=10, build=abi.VKRT_BUILD_PLOC_GPU, **cam)
    assert count == 1
    pos, nrm, tan = flat.positions.copy(), flat.normals.copy(), flat.tangents.copy()
    for first, n in sk["skins"][0]["vertex_ranges"].tolist():
        sl = slice(first, first + n)
        pos[sl], nrm[sl], tan[sl] = np_skin.skin(sk["joints0"][sl], sk["weights0"][sl], poses[1], flat.positions[sl], flat.normals[sl], flat.tangents[sl])
    want = sd.with_arrays(flat, positions=pos, normals=nrm, tangents=tan)
    u = host_py.global_uniforms(width=W, height=H, **cam)

    def render(f):
        r = Renderer(f, device=0, build="ploc")
        out = None
        for k in range(2):
            out = r.pathtrace(make_push_constants(samples=2, depth=4, frame=k, lights_count=len(f.lights)), u, W, H, seed=10 + k, image=out)
        r.close()
        return out.cpu().numpy()

    ref = render(want)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert not np.array_equal(ref.view(np.uint32), render(flat).view(np.uint32))  # (the pose is in view)
