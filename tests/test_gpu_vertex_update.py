"""Deforming meshes of a live scene (vkrt_scene_update_vertices + vkrt_accel_refit).  The yardstick is the one of test_gpu_refit.py, with
no tolerance anywhere: a Renderer created from the undeformed FlatScene, updated and refitted, against a fresh Renderer created from
the deformed FlatScene -- image digest after two progressive frames, ray counts, no traversal faults, a sound tree with the built node
count, and 60 k random closest hits bit for bit."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

import scene_deform as sd
from conftest import default_camera
from scene_motion import apply, moved

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KINDS = ("ploc", "lbvh", "sah")


@pytest.fixture(scope="module")
def cornell():
    from vkrt_amd.flat_scene import FlatScene

    return FlatScene.load_npz(os.path.join(ROOT, "tests", "golden", "cornell_flat.npz"))


@pytest.fixture(scope="module")
def atrium_small():
    import atrium

    flat, _ = atrium.build_atrium(20000, seed=4, with_textures=True)
    return flat


def _boxes(flat):
    """the primitive-meshes of Cornell's two boxes (its last two nodes, the ones test_gpu_refit.py moves)"""
    return sorted({int(flat.nodes[-2]["primMesh"]), int(flat.nodes[-1]["primMesh"])})


def _options(mode="wide8", split=-1, wt=0):
    from vkrt_amd import abi

    o = {abi.VKRT_OPT_SPLIT_BUDGET: split, abi.VKRT_OPT_WATERTIGHT: wt}
    if mode == "bvh2":
        o[abi.VKRT_OPT_BVH_LAYOUT] = 0
    if mode == "mega":
        o[abi.VKRT_OPT_MODE] = 0
    return o


def _render(r, flat, W, H, cam_kw=None, seed=3, frames=2, stream=None, image=None):
    from vkrt_amd.flat_scene import make_push_constants

    cam = default_camera(W, H, **(cam_kw or {}))
    r.reset_counters()
    img = image
    for f in range(frames):
        img = r.pathtrace(make_push_constants(samples=2, depth=4, frame=f, lights_count=len(flat.lights)), cam, W, H, seed=seed + f, image=img,
                          stream=stream)
    return sd.digest(img), r.counters()


def _same_frames(got, ref, what=None):
    assert got[0] == ref[0], what
    for k in ("rays_closest", "rays_shadow", "pixels"):
        assert got[1][k] == ref[1][k], (what, k, got[1][k], ref[1][k])
    assert got[1]["traversal_faults"] == 0 and ref[1]["traversal_faults"] == 0, what


def _update_equals_fresh(flat, dflat, meshes, kind, options, W, H, cam_kw=None, attrs=sd.ATTRS, ranges=None):
    """updated + refitted == fresh, by every measure of the module docstring"""
    from vkrt_amd.renderer import Renderer

    r = Renderer(flat, device=0, build=kind, options=options)
    reached = r.check_accel()["nodes_reached"]
    node_count = r.accel_info()["node_count"]
    sd.send(r, dflat, meshes, ranges=ranges, attrs=attrs)
    r.refit()
    sd.assert_sound(r.check_accel(), reached)
    assert r.accel_info()["node_count"] == node_count
    f = Renderer(dflat, device=0, build=kind, options=options)
    _same_frames(_render(r, dflat, W, H, cam_kw), _render(f, dflat, W, H, cam_kw), (kind, options))
    rays = sd.random_rays(dflat)
    sd.assert_same_trace(r.trace_rays(*rays), f.trace_rays(*rays))
    r.close()
    f.close()


# ---- 1. Cornell, its two boxes twisted: every layout, builder, split setting and triangle test ------------------------------------------
@pytest.mark.parametrize("mode", ["wide8", "bvh2", "mega"])
@pytest.mark.parametrize("kind", KINDS)
def test_twisted_boxes_equal_a_fresh_scene(cornell, mode, kind):
    meshes = _boxes(cornell)
    dflat = sd.twisted(cornell, meshes)
    assert not np.array_equal(dflat.positions, cornell.positions) and not np.array_equal(dflat.normals, cornell.normals)
    for split in (0, -1):
        for wt in (0, 1):
            _update_equals_fresh(cornell, dflat, meshes, kind, _options(mode, split, wt), 64, 64)


# ---- 2. the small atrium: a third of its meshes under a sine displacement, an instanced one among them --------------------------------------
@pytest.mark.parametrize("kind", ["ploc", "lbvh"])
@pytest.mark.parametrize("split", [0, -1])
def test_sine_on_a_third_of_the_atrium(atrium_small, kind, split):
    import atrium

    meshes = sd.third_of_meshes(atrium_small)
    uses = np.bincount(atrium_small.nodes["primMesh"], minlength=len(atrium_small.prim_meshes))
    assert max(uses[m] for m in meshes) > 1  # a mesh that several nodes instance deforms in all of them
    dflat = sd.sine(atrium_small, meshes, phase=0.7)
    _update_equals_fresh(atrium_small, dflat, meshes, kind, _options("wide8", split, 0), 160, 90, atrium.DEFAULT_CAMERA,
                         attrs=("positions", "normals", "tangents"))


# ---- 3. device source == host source ---------------------------------------------------------------------------------------------------
def test_device_source_equals_host_source(atrium_small):
    import atrium
    import torch
    from vkrt_amd.renderer import Renderer

    meshes = sd.third_of_meshes(atrium_small)
    dflat = sd.sine(atrium_small, meshes, phase=1.9)
    W, H = 160, 90
    out = []
    for source in ("host", "device", "device_unaligned"):
        r = Renderer(atrium_small, device=0, build="ploc")
        if source == "device_unaligned":
            # one buffer, every array at a 4-byte offset from the 16-byte aligned block before it: the alignment the header promises to take
            for m in meshes:
                first, count = sd.mesh_range(dflat, m)
                buf = torch.zeros(12 * count + 8, dtype=torch.float32, device="cuda:0")
                kw, at = {}, 1
                for k, w in (("positions", 3), ("normals", 3), ("tangents", 4), ("texcoords0", 2)):
                    kw[k] = buf[at:at + w * count].view(count, w)
                    kw[k].copy_(torch.as_tensor(getattr(dflat, k)[first:first + count]))
                    at += w * count
                assert kw["positions"].data_ptr() % 16 == 4
                r.update_vertices(first, **kw)
        else:
            sd.send(r, dflat, meshes, device="cuda:0" if source == "device" else None)
        r.refit()
        out.append((sd.accel_bytes(r), _render(r, dflat, W, H, atrium.DEFAULT_CAMERA)[0]))
        r.close()
    assert out[0] == out[1] == out[2]


# ---- 4. partial ranges and kept attributes ---------------------------------------------------------------------------------------------
def test_partial_range_and_kept_attributes(atrium_small):
    import atrium
    from vkrt_amd.renderer import Renderer

    W, H = 160, 90
    m = int(np.argmax(np.bincount(atrium_small.nodes["primMesh"])))  # a column or an arch: in view many times
    full = sd.sine(atrium_small, [m], phase=0.3, amplitude=0.2)
    first, count = sd.mesh_range(atrium_small, m)
    assert count >= 12
    lo, n = first + count // 4, count // 2  # a sub-range strictly inside the mesh, positions only: normals, tangents, uv kept
    pos = atrium_small.positions.copy()
    pos[lo:lo + n] = full.positions[lo:lo + n]
    mixed = sd.with_arrays(atrium_small, positions=pos)
    _update_equals_fresh(atrium_small, mixed, None, "ploc", _options(), W, H, atrium.DEFAULT_CAMERA, attrs=("positions",), ranges=[(lo, n)])

    # normals and texture coordinates alone: the tree is not stale, no refit, and the shading reads them (hybrid G-buffer planes)
    rng = np.random.default_rng(3)
    nrm = atrium_small.normals.copy()
    uv = atrium_small.texcoords0.copy()
    v = rng.standard_normal((count, 3))
    nrm[first:first + count] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    uv[first:first + count] = rng.uniform(0, 3, (count, 2)).astype(np.float32)
    shaded = sd.with_arrays(atrium_small, normals=nrm, texcoords0=uv)
    cam = default_camera(W, H, **atrium.DEFAULT_CAMERA)
    r = Renderer(atrium_small, device=0, build="ploc")
    before = sd.accel_bytes(r)
    plain = r.gbuffer_raycast(cam, W, H)
    sd.send(r, shaded, ranges=[(first, count)], attrs=("normals",))
    sd.send(r, shaded, ranges=[(first, count)], attrs=("texcoords0",))
    got = r.gbuffer_raycast(cam, W, H)  # (no refit in between: NOT_BUILT here would fail the test)
    assert sd.accel_bytes(r) == before
    f = Renderer(shaded, device=0, build="ploc")
    ref = f.gbuffer_raycast(cam, W, H)
    for k in ("normal", "color", "position", "roughMetal"):
        assert sd.digest(got[k]) == sd.digest(ref[k]), k
    assert sd.digest(got["normal"]) != sd.digest(plain["normal"]) and sd.digest(got["color"]) != sd.digest(plain["color"])
    _same_frames(_render(r, shaded, W, H, atrium.DEFAULT_CAMERA), _render(f, shaded, W, H, atrium.DEFAULT_CAMERA))
    r.close()
    f.close()


# ---- 5. degenerate and back ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("split", [0, -1])
def test_collapse_to_a_point_and_back(cornell, kind, split):
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer

    m = _boxes(cornell)[0]
    dflat = sd.collapsed(cornell, m)
    for mode in ("wide8", "bvh2"):
        opts = _options(mode, split, 0)
        _update_equals_fresh(cornell, dflat, [m], kind, opts, 64, 64, attrs=("positions",))
        r = Renderer(cornell, device=0, build=kind, options=opts)
        built = sd.accel_bytes(r)
        if r.get_option(abi.VKRT_INFO_SPLIT_BUDGET) != 0:
            # (a refit gives a split reference its whole triangle's box: the tree to return to is the no-op refit of the build)
            r.refit()
            built = sd.accel_bytes(r)
        sd.send(r, dflat, [m], attrs=("positions",))
        r.refit()
        assert sd.accel_bytes(r) != built
        sd.send(r, cornell, [m], attrs=("positions",))
        r.refit()
        assert sd.accel_bytes(r) == built, (kind, mode, split)
        r.close()


# ---- 6. exact boxes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["wide8", "bvh2"])
def test_deformed_boxes_and_cost_are_exact(cornell, atrium_small, layout):
    """After a deformation + refit the node words are the float64 restatement of the installed topology and sah_cost its cost, by the
    rules (and the code) of test_gpu_bvh_bounds.py."""
    import test_gpu_bvh_bounds as bounds
    from vkrt_amd.renderer import Renderer

    cases = [(cornell, sd.twisted(cornell, _boxes(cornell)), _boxes(cornell), k, wt) for k in KINDS for wt in (0, 1)]
    am = sd.third_of_meshes(atrium_small)
    cases += [(atrium_small, sd.sine(atrium_small, am, phase=0.7), am, k, 0) for k in ("ploc", "lbvh")]
    for flat, dflat, meshes, kind, wt in cases:
        for split in (0, -1):
            r = Renderer(flat, device=0, build=kind, options=bounds._options(layout, wt, split))
            cost0 = r.accel_info()["sah_cost"]
            sd.send(r, dflat, meshes)
            r.refit()
            _, info = bounds.check_exact(r, wt, f"deformed {kind} {layout} split={split} wt={wt}")
            assert info["sah_cost"] != cost0
            r.close()


# ---- 7. with the other live-scene calls ------------------------------------------------------------------------------------------------
def test_with_node_updates_visibility_and_ray_queries(atrium_small):
    import atrium
    import oracle_py
    import torch
    from vkrt_amd.renderer import Renderer, pack_rays

    W, H = 160, 90
    meshes = sd.third_of_meshes(atrium_small)
    n = len(atrium_small.nodes)
    mflat, mats = moved(atrium_small, np.sort(np.random.default_rng(5).choice(n, n // 4, replace=False)), 77)
    dflat = sd.sine(mflat, meshes, phase=2.4, base=mflat)
    r = Renderer(atrium_small, device=0, build="ploc")
    masks = np.where(np.arange(n) % 3 == 0, 1, 2).astype(np.uint8)
    r.set_instance_visibility(0, masks)
    table = r.read_node_masks().copy()
    # node and vertex updates, interleaved, before ONE refit
    apply(r, {k: v for k, v in list(mats.items())[::2]})
    sd.send(r, dflat, meshes)
    apply(r, {k: v for k, v in list(mats.items())[1::2]})
    r.refit()
    f = Renderer(dflat, device=0, build="ploc")
    _same_frames(_render(r, dflat, W, H, atrium.DEFAULT_CAMERA), _render(f, dflat, W, H, atrium.DEFAULT_CAMERA))
    # visibility set before the deformation survives it
    assert np.array_equal(r.read_node_masks(), table) and np.array_equal(r.instance_visibility()[0], masks)
    o, d = sd.random_rays(dflat, 60000, seed=8)
    rays = pack_rays(torch.as_tensor(o, device="cuda:0"), torch.as_tensor(d, device="cuda:0"), 0.001, 1e4)
    keep = np.nonzero(masks == 1)[0]
    sub = copy.copy(dflat)
    sub.nodes = dflat.nodes[keep].copy()
    cnt = np.array([int(dflat.prim_meshes[nd["primMesh"]]["indexCount"]) // 3 for nd in dflat.nodes], np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)])
    gmap = np.concatenate([np.arange(off[i], off[i + 1]) for i in keep])
    s = Renderer(sub, device=0, build="ploc")
    a = r.intersect(rays, cull_mask=1).buffer.cpu().numpy()
    b = s.intersect(rays).buffer.cpu().numpy()
    assert np.array_equal(a[:, :3].view(np.uint32), b[:, :3].view(np.uint32))
    ai, bi = a[:, 3:].view(np.int32), b[:, 3:].view(np.int32)
    hit = bi[:, 3] >= 0
    assert hit.mean() > 0.1 and np.array_equal(ai[:, 3] >= 0, hit)
    assert np.array_equal(ai[hit, 0], keep[bi[hit, 0]]) and np.array_equal(ai[hit, 3], gmap[bi[hit, 3]])
    assert np.array_equal(ai[hit][:, [1, 2, 4]], bi[hit][:, [1, 2, 4]])
    s.close()
    # the one direct comparison with the oracle: closest hits and occlusion of the deformed scene
    orc = oracle_py.OracleScene(dflat)
    t, u, v, gid, _ = orc.trace_rays(o, d, 0.001, 1e4, use_bvh=True)
    h = r.intersect(rays)
    occ = r.occluded(rays).cpu().numpy()
    hb = h.buffer.cpu().numpy()
    tri = hb[:, 3:].view(np.int32)[:, 3]
    assert np.array_equal(tri, gid) and (gid >= 0).mean() > 0.15
    hitm = gid >= 0
    for k, x in enumerate((t, u, v)):
        assert np.array_equal(hb[hitm, k].view(np.uint32), np.ascontiguousarray(x[hitm], np.float32).view(np.uint32)), k
    _, _, _, any_gid, _ = orc.trace_rays(o, d, 0.001, 1e4, any_hit=True, use_bvh=True)
    assert np.array_equal(occ, (any_gid >= 0).astype(np.int32))
    r.close()
    f.close()


# ---- 8. stale and rebuild ----------------------------------------------------------------------------------------------------------------
def test_stale_until_refit_and_rebuild_with_every_builder(cornell):
    import torch
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Renderer, VkrtError, pack_rays

    W = H = 64
    meshes = _boxes(cornell)
    dflat = sd.twisted(cornell, meshes)
    pc = make_push_constants(samples=1, depth=2, frame=0, lights_count=len(cornell.lights))
    cam = default_camera(W, H)
    o, d = sd.random_rays(cornell, 256)
    rays = pack_rays(torch.as_tensor(o, device="cuda:0"), torch.as_tensor(d, device="cuda:0"))
    r = Renderer(cornell, device=0, build="ploc")
    # an unbuilt scene takes updates and does not become stale; count 0 and all-NULL updates are no-ops on a built one
    u = Renderer(cornell, device=0, build=None)
    sd.send(u, dflat, meshes)
    u.build("ploc")
    f = Renderer(dflat, device=0, build="ploc")
    assert sd.accel_bytes(u) == sd.accel_bytes(f)
    u.close()
    r.update_vertices(0)
    r.update_vertices(3, positions=np.zeros((0, 3), np.float32))
    r.pathtrace(pc, cam, W, H)
    g = r.gbuffer_raycast(cam, W, H)
    sd.send(r, dflat, meshes, attrs=("positions",))
    for call in (lambda: r.pathtrace(pc, cam, W, H), lambda: r.gbuffer_raycast(cam, W, H), lambda: r.trace_rays(o, d), r.read_accel,
                 lambda: r.intersect(rays), lambda: r.occluded(rays), r.check_accel,
                 lambda: r.hybrid_trace(pc, cam, W, H, g)):
        with pytest.raises(VkrtError, match=r"\(5\)"):
            call()
    # refused updates change nothing: the scene is still stale with the deformed positions, and a refit gives the deformed scene
    nan = dflat.positions[:4].copy()
    nan[2, 1] = np.inf
    with pytest.raises(VkrtError, match=r"\(1\).*not finite"):
        r.update_vertices(0, positions=nan)
    bad = abi.VertexUpdate(C.sizeof(abi.VertexUpdate), len(cornell.positions) - 1, 2, abi.VKRT_MEMORY_HOST, nan.ctypes.data, None, None, None)
    assert r.lib.vkrt_scene_update_vertices(r._h, bad, None) == 1 and b"outside" in r.lib.vkrt_last_error()
    r.refit()
    sd.send(r, dflat, meshes, attrs=("normals", "tangents", "texcoords0"))
    _same_frames(_render(r, dflat, W, H), _render(f, dflat, W, H))
    f.close()
    r.close()
    # build() instead of refit(): the fresh build's bytes with every builder, after a host-sourced and after a device-sourced update
    for kind in KINDS:
        for layout in ("wide8", "bvh2"):
            opts = _options(layout, 0, 0)
            f = Renderer(dflat, device=0, build=kind, options=opts)
            want = sd.accel_bytes(f), f.accel_info()["sah_cost"], f.get_option(abi.VKRT_INFO_ANYHIT_ORDER), _render(f, dflat, W, H)[0]
            f.close()
            for device in (None, "cuda:0"):
                r = Renderer(cornell, device=0, build=kind, options=opts)
                keep = sd.send(r, dflat, meshes, device=device)
                r.build(kind)
                got = sd.accel_bytes(r), r.accel_info()["sah_cost"], r.get_option(abi.VKRT_INFO_ANYHIT_ORDER), _render(r, dflat, W, H)[0]
                assert got == want, (kind, layout, device)
                del keep
                r.close()


# ---- 9. stream order ---------------------------------------------------------------------------------------------------------------------
def test_stream_order_without_host_synchronisation(cornell):
    """trace A, update + refit, trace B, update back + refit, trace C, enqueued back to back on a non-default stream from device arrays."""
    import torch
    from vkrt_amd.renderer import Renderer

    W = H = 64
    meshes = _boxes(cornell)
    dflat = sd.twisted(cornell, meshes)
    want = []
    for flat in (cornell, dflat):
        f = Renderer(flat, device=0, build="ploc")
        want.append(_render(f, flat, W, H)[0])
        f.close()
    assert want[0] != want[1]
    r = Renderer(cornell, device=0, build="ploc")
    r.refit()  # (the first refit of a build allocates and synchronises: done before the sequence)
    s = torch.cuda.Stream(device=0)
    imgs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    there = {m: {k: torch.as_tensor(np.ascontiguousarray(getattr(dflat, k)[slice(*_span(dflat, m))]), device="cuda:0") for k in sd.ATTRS} for m in meshes}
    back = {m: {k: torch.as_tensor(np.ascontiguousarray(getattr(cornell, k)[slice(*_span(cornell, m))]), device="cuda:0") for k in sd.ATTRS} for m in meshes}
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        _frames_only(r, cornell, W, H, s, imgs[0])
        for m in meshes:
            r.update_vertices(sd.mesh_range(dflat, m)[0], stream=s, **there[m])
        r.refit(stream=s)
        _frames_only(r, dflat, W, H, s, imgs[1])
        for m in meshes:
            r.update_vertices(sd.mesh_range(cornell, m)[0], stream=s, **back[m])
        r.refit(stream=s)
        _frames_only(r, cornell, W, H, s, imgs[2])
    s.synchronize()
    assert [sd.digest(i) for i in imgs] == [want[0], want[1], want[0]]
    assert r.counters()["traversal_faults"] == 0
    r.close()


def _span(flat, m):
    first, count = sd.mesh_range(flat, m)
    return first, first + count


def _frames_only(r, flat, W, H, stream, image):
    """two progressive frames into `image`, nothing that waits for the device (no counter read)"""
    from vkrt_amd.flat_scene import make_push_constants

    cam = default_camera(W, H)
    for f in range(2):
        r.pathtrace(make_push_constants(samples=2, depth=4, frame=f, lights_count=len(flat.lights)), cam, W, H, seed=3 + f, image=image, stream=stream)


# ---- 10. the C++ host layer ----------------------------------------------------------------------------------------------------------------
def test_cpp_host_update_vertices_and_refit(tmp_path):
    """HelloVkrt::updateVertices + refitAccel through the host_py hook render the pixels of a fresh scene made from the deformed arrays."""
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
    m = int(np.argmax(flat.prim_meshes["vertexCount"]))
    first, count = sd.mesh_range(flat, m)
    steps = [sd.sine(flat, [m], phase=p, amplitude=0.25) for p in (0.4, 1.1)]
    W, H = 160, 90
    cam = atrium.DEFAULT_CAMERA
    sl = slice(first, first + count)
    img = host_py.render_gltf_deformed(path, W, H, first, np.stack([s.positions[sl] for s in steps]), normals=np.stack([s.normals[sl] for s in steps]),
                                       tangents=np.stack([s.tangents[sl] for s in steps]), samples=2, depth=4, frames=3, seed0=10,
                                       build=abi.VKRT_BUILD_PLOC_GPU, **cam)
    r = Renderer(steps[-1], device=0, build="ploc")
    u = host_py.global_uniforms(width=W, height=H, **cam)
    ref = None
    for f in range(3):
        ref = r.pathtrace(make_push_constants(samples=2, depth=4, frame=f, lights_count=len(flat.lights)), u, W, H, seed=10 + f, image=ref)
    assert np.array_equal(img.view(np.uint32), ref.cpu().numpy().view(np.uint32))
    plain = Renderer(flat, device=0, build="ploc")
    assert sd.digest(plain.pathtrace(make_push_constants(samples=2, depth=4, frame=0, lights_count=len(flat.lights)), u, W, H, seed=10)) != \
        sd.digest(r.pathtrace(make_push_constants(samples=2, depth=4, frame=0, lights_count=len(flat.lights)), u, W, H, seed=10))
    r.close()
    plain.close()
