"""Moving instances without a rebuild (vkrt_scene_update_nodes + vkrt_accel_refit).  The image is a property of the triangle set, not of
the tree: a refitted tree must give exactly the pixels, ray counts and closest hits of a fresh build of the moved
scene, in every layout, builder, split setting and triangle test -- no tolerance, no new oracle."""
import ctypes as C
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


def _digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t).tobytes()).hexdigest()[:16]


@pytest.fixture(scope="module")
def cornell():
    from vkrt_amd.flat_scene import FlatScene

    return FlatScene.load_npz(os.path.join(ROOT, "tests", "golden", "cornell_flat.npz"))


@pytest.fixture(scope="module")
def atrium_small():
    import atrium

    flat, _ = atrium.build_atrium(20000, seed=4, with_textures=True)
    return flat


def _cornell_move(flat, seed=11):
    return moved(flat, [len(flat.nodes) - 2, len(flat.nodes) - 1], seed, mirror_first=False, scale=False)


def _atrium_move(flat, seed=23):
    n = len(flat.nodes)
    idx = np.sort(np.random.default_rng(seed).choice(n, n // 3, replace=False))
    return moved(flat, idx, seed)


def _render(r, flat, W, H, cam_kw=None, seed=3, frames=2, flags=0):
    from vkrt_amd.flat_scene import make_push_constants

    cam = default_camera(W, H, **(cam_kw or {}))
    r.reset_counters()
    img = None
    for f in range(frames):
        img = r.pathtrace(make_push_constants(samples=2, depth=4, frame=f, lights_count=len(flat.lights)), cam, W, H, seed=seed + f, image=img, flags=flags)
    c = r.counters()
    return _digest(img), c


def _rays(flat, n=60000, seed=5):
    rng = np.random.default_rng(seed)
    lo, hi = flat.positions.min(0), flat.positions.max(0)
    o = rng.uniform(lo - 0.5, hi + 0.5, (n, 3)).astype(np.float32)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d


def _sound(chk, node_count):
    assert chk["triangles_missing"] == 0 and chk["triangles_repeated"] == 0 and chk["box_violations"] == 0 and chk["bad_references"] == 0, chk
    assert chk["triangles_uncovered"] == 0, chk
    assert chk["nodes_reached"] == node_count, chk


def _same_trace(a, b):
    ta, ua, va, ga = a
    tb, ub, vb, gb = b
    assert np.array_equal(ga, gb)
    for x, y in ((ta, tb), (ua, ub), (va, vb)):
        assert np.array_equal(x[ga >= 0].view(np.uint32), y[gb >= 0].view(np.uint32))


def _options(mode, split, wt):
    from vkrt_amd import abi

    o = {abi.VKRT_OPT_SPLIT_BUDGET: split, abi.VKRT_OPT_WATERTIGHT: wt}
    if mode == "bvh2":
        o[abi.VKRT_OPT_BVH_LAYOUT] = 0
    if mode == "mega":
        o[abi.VKRT_OPT_MODE] = 0
    return o


def _refit_equals_fresh(flat, move, kind, options, W, H, cam_kw=None, rays=None):
    from vkrt_amd.renderer import Renderer

    mflat, mats = move
    r = Renderer(flat, device=0, build=kind, options=options)
    before = r.check_accel()
    node_count = r.accel_info()["node_count"]
    apply(r, mats)
    r.refit()
    chk = r.check_accel()
    _sound(chk, before["nodes_reached"])
    assert r.accel_info()["node_count"] == node_count
    got = _render(r, mflat, W, H, cam_kw)
    f = Renderer(mflat, device=0, build=kind, options=options)
    ref = _render(f, mflat, W, H, cam_kw)
    assert got[0] == ref[0], (kind, options)
    for k in ("rays_closest", "rays_shadow", "pixels"):
        assert got[1][k] == ref[1][k], (k, got[1][k], ref[1][k])
    assert got[1]["traversal_faults"] == 0 and ref[1]["traversal_faults"] == 0
    if rays is not None:
        _same_trace(r.trace_rays(*rays), f.trace_rays(*rays))
    r.close()
    f.close()
    return got


@pytest.mark.parametrize("mode", ["wide8", "bvh2", "mega"])
@pytest.mark.parametrize("kind", ["ploc", "lbvh", "sah"])
def test_refit_equals_fresh_build_cornell(cornell, mode, kind):
    """{wavefront wide8, wavefront BVH2, megakernel} x {PLOC, LBVH, SAH_HOST} x {split 0, -1} x {watertight 0, 1}: hash, ray counts,
    a sound tree with the built node count, and 60 k closest hits bit for bit."""
    move = _cornell_move(cornell)
    rays = _rays(move[0])
    for split in (0, -1):
        for wt in (0, 1):
            _refit_equals_fresh(cornell, move, kind, _options(mode, split, wt), 64, 64, rays=rays)


@pytest.mark.parametrize("kind", ["ploc", "lbvh"])
@pytest.mark.parametrize("split", [0, -1])
def test_refit_equals_fresh_build_atrium(atrium_small, kind, split):
    """A third of the atrium's instances rotated, translated, scaled non-uniformly, one of them mirrored (negative determinant)."""
    import atrium

    move = _atrium_move(atrium_small)
    mats = move[1]
    assert np.linalg.det(_row_major(mats[min(mats)])[:3, :3]) < 0  # the mirrored one
    _refit_equals_fresh(atrium_small, move, kind, _options("wide8", split, 0), 160, 90, atrium.DEFAULT_CAMERA, rays=_rays(move[0]))


@pytest.mark.parametrize("kind", ["ploc", "lbvh"])
def test_ten_successive_refits_and_frames_in_flight(atrium_small, kind):
    """Ten update + refit steps (each from the previous pose) and a three-frame vkrt_pathtrace_frames call equal a fresh build of the
    final pose."""
    import atrium
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Renderer

    r = Renderer(atrium_small, device=0, build=kind)
    reached = r.check_accel()["nodes_reached"]
    cur = atrium_small
    for step in range(10):
        cur, mats = moved(cur, np.sort(np.random.default_rng(100 + step).choice(len(cur.nodes), len(cur.nodes) // 3, replace=False)), 200 + step,
                          mirror_first=False)
        apply(r, mats)
        r.refit()
    _sound(r.check_accel(), reached)
    f = Renderer(cur, device=0, build=kind)
    W, H = 160, 90
    assert _render(r, cur, W, H, atrium.DEFAULT_CAMERA)[0] == _render(f, cur, W, H, atrium.DEFAULT_CAMERA)[0]
    cam = default_camera(W, H, **atrium.DEFAULT_CAMERA)
    pc = make_push_constants(samples=1, depth=4, frame=0, lights_count=len(cur.lights))
    a = r.pathtrace_frames(pc, cam, W, H, 3, seed=9)
    b = f.pathtrace_frames(pc, cam, W, H, 3, seed=9)
    assert _digest(a) == _digest(b)
    r.close()
    f.close()


@pytest.mark.parametrize("kind", ["ploc", "lbvh", "sah"])
def test_refit_without_motion_is_a_no_op(atrium_small, cornell, kind):
    """Split budget 0: refitting an unmoved scene re-encodes every node bit for bit (shared quantisation) -- the traversal visits the
    same nodes and tests the same triangles, the image and the SAH cost are those of the build.  Both layouts, every builder."""
    import atrium
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer

    # (work sharing and triangle parking make a ray's node count depend on the other rays of its wave, i.e. on the order of the
    # compacted streams: off here, so that the counts are a function of the tree alone -- the repeated render below shows it)
    opts = {abi.VKRT_OPT_SPLIT_BUDGET: 0, abi.VKRT_OPT_WF_SHARE: 0, abi.VKRT_OPT_TRI_THRESHOLD: 0}
    cases = [(layout, scene) for layout in (1, 0) for scene in ((atrium_small, atrium.DEFAULT_CAMERA, 160, 90), (cornell, {}, 64, 64))]
    for layout, (flat, kw, W, H) in cases:
        r = Renderer(flat, device=0, build=kind, options={**opts, abi.VKRT_OPT_BVH_LAYOUT: layout})
        built = _render(r, flat, W, H, kw, flags=abi.VKRT_TRACE_COUNT_TRAVERSAL)
        repeat = _render(r, flat, W, H, kw, flags=abi.VKRT_TRACE_COUNT_TRAVERSAL)
        assert repeat[1]["nodes_visited"] == built[1]["nodes_visited"] and repeat[1]["tris_tested"] == built[1]["tris_tested"]
        sah = r.accel_info()["sah_cost"]
        r.refit()
        again = _render(r, flat, W, H, kw, flags=abi.VKRT_TRACE_COUNT_TRAVERSAL)
        assert again[0] == built[0]
        for k in ("nodes_visited", "tris_tested", "rays_closest", "rays_shadow"):
            assert again[1][k] == built[1][k], (k, again[1][k], built[1][k])
        info = r.accel_info()
        assert abs(info["sah_cost"] - sah) <= 1e-5 * sah, (layout, info["sah_cost"], sah)
        r.close()


def test_moved_cornell_matches_the_oracle(cornell):
    import camera_np
    import oracle_py
    from vkrt_amd.flat_scene import make_push_constants, uniforms_from_matrices
    from vkrt_amd.renderer import Renderer

    mflat, mats = _cornell_move(cornell)
    W = H = 64
    cam = uniforms_from_matrices(*camera_np.global_uniforms(width=W, height=H))
    pc = make_push_constants(samples=2, depth=3, frame=0, lights_count=len(mflat.lights))
    ref, _ = oracle_py.OracleScene(mflat).render(pc, cam, W, H, seed=7)
    for kind in ("ploc", "lbvh", "sah"):
        r = Renderer(cornell, device=0, build=kind)
        apply(r, mats)
        r.refit()
        img = r.pathtrace(pc, cam, W, H, seed=7).cpu().numpy()
        assert np.mean(np.any(img.view(np.uint32) != ref.view(np.uint32), axis=-1)) < 1e-4
        assert float(np.sqrt(np.mean((img[..., :3].astype(np.float64) - ref[..., :3]) ** 2))) < 1e-3
        r.close()


def test_hybrid_after_refit_equals_fresh_scene(atrium_small):
    """Shading reads o2w / w2o: the G-buffer and the hybrid trace see the updated instance records."""
    import atrium
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Renderer

    mflat, mats = _atrium_move(atrium_small)
    W, H = 160, 90
    cam = default_camera(W, H, **atrium.DEFAULT_CAMERA)
    out = []
    for which in ("refit", "fresh"):
        if which == "refit":
            r = Renderer(atrium_small, device=0, build="ploc")
            apply(r, mats)
            r.refit()
        else:
            r = Renderer(mflat, device=0, build="ploc")
        g = r.gbuffer_raycast(cam, W, H)
        pc = make_push_constants(samples=1, depth=3, frame=0, lights_count=len(mflat.lights))
        pc.useShadows, pc.useAO, pc.useGI = 1, 1, 1
        acc = r.hybrid_trace(pc, cam, W, H, g, seed=4)
        out.append([_digest(g[k]) for k in ("color", "position", "normal", "roughMetal")] + [_digest(acc)])
        r.close()
    assert out[0] == out[1]


def test_update_contract(cornell):
    import torch
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer, VkrtError

    mflat, mats = _cornell_move(cornell)
    W = H = 64
    fresh = Renderer(mflat, device=0, build="ploc")
    want = _render(fresh, mflat, W, H)[0]
    fresh.close()

    # refit before any build
    r = Renderer(cornell, device=0, build=None)
    with pytest.raises(VkrtError, match=r"\(5\)"):
        r.refit()
    r.close()

    r = Renderer(cornell, device=0, build="ploc")
    unmoved = _render(r, cornell, W, H)[0]
    apply(r, mats)
    # stale between update and refit: every tracing entry point refuses
    from vkrt_amd.flat_scene import make_push_constants

    pc = make_push_constants(samples=1, depth=2, frame=0, lights_count=len(cornell.lights))
    cam = default_camera(W, H)
    for call in (lambda: r.pathtrace(pc, cam, W, H), lambda: r.gbuffer_raycast(cam, W, H), lambda: r.trace_rays(*_rays(cornell, 16)),
                 r.read_accel):
        with pytest.raises(VkrtError, match=r"\(5\)"):
            call()
    info = r.accel_info()
    nb, tb = int(info["node_bytes"]), int(info["triangle_bytes"])
    nodes, tris, root = np.zeros(nb // 4 + 1, np.uint32), np.zeros(tb // 4 + 1, np.float32), C.c_int32(7)
    assert r.lib.vkrt_debug_read_accel(r._h, nodes.ctypes.data, nb, tris.ctypes.data, tb, C.byref(root)) == 5 and root.value == 7
    # a full build after update_nodes builds the moved scene
    r.build("ploc")
    assert _render(r, mflat, W, H)[0] == want
    # refused: a changed primMesh, a NaN matrix -- the scene is unchanged and usable
    bad = abi.Node()
    bad.worldMatrix[:] = list(mats[max(mats)])
    bad.primMesh = (int(cornell.nodes[max(mats)]["primMesh"]) + 1) % len(cornell.prim_meshes)
    assert r.lib.vkrt_scene_update_nodes(r._h, max(mats), 1, C.byref(bad), None) == 1
    assert b"primMesh" in r.lib.vkrt_last_error()
    nan = mats[max(mats)].copy()
    nan[5] = np.nan
    with pytest.raises(VkrtError, match=r"\(1\).*not finite"):
        r.update_nodes(max(mats), nan[None])
    ok = abi.Node()
    ok.worldMatrix[:] = list(mats[max(mats)])
    ok.primMesh = int(cornell.nodes[max(mats)]["primMesh"])
    assert r.lib.vkrt_scene_update_nodes(r._h, len(cornell.nodes), 1, C.byref(ok), None) == 1  # range outside the scene
    assert _render(r, mflat, W, H)[0] == want
    # vkrt_debug_read_accel takes exactly the tree's byte counts and non-NULL buffers
    info = r.accel_info()
    nb, tb = int(info["node_bytes"]), int(info["triangle_bytes"])
    nodes, tris, root = np.zeros(nb // 4 + 1, np.uint32), np.zeros(tb // 4 + 1, np.float32), C.c_int32(7)
    for args in ((nb + 4, tb), (nb - 4, tb), (nb, tb + 48), (nb, tb - 48)):
        assert r.lib.vkrt_debug_read_accel(r._h, nodes.ctypes.data, args[0], tris.ctypes.data, args[1], C.byref(root)) == 1, args
    assert r.lib.vkrt_debug_read_accel(r._h, None, nb, tris.ctypes.data, tb, C.byref(root)) == 1
    assert r.lib.vkrt_debug_read_accel(r._h, nodes.ctypes.data, nb, None, tb, C.byref(root)) == 1
    assert r.lib.vkrt_debug_read_accel(r._h, nodes.ctypes.data, nb, tris.ctypes.data, tb, None) == 1
    assert root.value == 7
    assert r.lib.vkrt_debug_read_accel(r._h, nodes.ctypes.data, nb, tris.ctypes.data, tb, C.byref(root)) == 0 and root.value == 0
    # a zero scale (a hidden instance) is accepted, as at vkrt_scene_create
    r.update_nodes(0, np.zeros((1, 16), np.float32))
    r.refit()
    assert _render(r, mflat, W, H)[1]["traversal_faults"] == 0
    r.close()

    # update, refit and trace enqueued on one non-default stream without synchronising in between: stream order is all it takes (the
    # library's internal lane streams fork from and join to the caller's stream)
    r = Renderer(cornell, device=0, build="ploc")
    s = torch.cuda.Stream(device=0)
    img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        first = r.pathtrace(pc, cam, W, H, seed=1, stream=s).clone()  # reads the old transforms
        apply(r, mats, stream=s)
        r.refit(stream=s)
        for f in range(2):
            r.pathtrace(make_push_constants(samples=2, depth=4, frame=f, lights_count=len(cornell.lights)), cam, W, H, seed=3 + f, image=img, stream=s)
    s.synchronize()
    assert _digest(img) == want
    r2 = Renderer(cornell, device=0, build="ploc")
    assert _digest(first) == _digest(r2.pathtrace(pc, cam, W, H, seed=1))
    assert unmoved != want
    r.close()
    r2.close()


def test_cpp_host_update_and_refit_match_python(tmp_path):
    """HelloVkrt::updateNodeTransforms + refitAccel (the reference's buildTlas(..., update) role) through the C++ host layer give the
    image the Python Renderer gives for the same glTF, motion, camera and seeds."""
    import atrium
    import gltf_export
    import gltf_flatten
    from vkrt_amd import abi, host_py
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Renderer

    flat0, _ = atrium.build_atrium(2000, seed=5, with_textures=True)
    path = str(tmp_path / "atrium.gltf")
    gltf_export.export_gltf(flat0, path)
    flat = gltf_flatten.load_gltf(path)
    first, count = 3, 4
    steps = []
    cur = flat
    for k in range(2):
        cur, mats = moved(cur, list(range(first, first + count)), 40 + k, mirror_first=(k == 0))
        steps.append(np.stack([mats[i] for i in range(first, first + count)]))
    W, H = 160, 90
    cam = atrium.DEFAULT_CAMERA
    img = host_py.render_gltf_moved(path, W, H, first, np.stack(steps), samples=2, depth=4, frames=3, seed0=10, build=abi.VKRT_BUILD_PLOC_GPU, **cam)
    r = Renderer(flat, device=0, build="ploc")
    for m in steps:
        r.update_nodes(first, m)
        r.refit()
    u = host_py.global_uniforms(width=W, height=H, **cam)
    ref = None
    for f in range(3):
        ref = r.pathtrace(make_push_constants(samples=2, depth=4, frame=f, lights_count=len(flat.lights)), u, W, H, seed=10 + f, image=ref)
    assert np.array_equal(img.view(np.uint32), ref.cpu().numpy().view(np.uint32))
    r.close()
