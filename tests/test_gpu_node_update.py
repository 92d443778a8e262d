"""Moving instances from device memory (vkrt_scene_update_node_transforms).  A device update must be bit for bit a host update of the same
matrices: the instance records are compared byte for byte with a twin scene moved through the host's vkrt_scene_update_nodes, and what
follows from them -- refitted and rebuilt trees, ray queries with visibility, motion -- with fresh scenes.  No tolerances."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from conftest import default_camera
from scene_instances import NODES, instances_scene, rays_from_above
from scene_motion import apply, moved

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIRRORED = 0x10000  # VKRT_VIS_MIRRORED
NOT_BUILT = r"\(5\)"


def _digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t).tobytes()).hexdigest()[:16]


def _bytes(rec):
    return np.ascontiguousarray(rec).view(np.uint8).reshape(len(rec), -1)


def _device(a, dtype=None):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to("cuda:0")


def _stack(mats, nodes):
    return np.stack([mats[int(i)] for i in nodes]).astype(np.float32)


@pytest.fixture(scope="module")
def flat():
    return instances_scene()


@pytest.fixture(scope="module")
def cornell():
    from vkrt_amd.flat_scene import FlatScene

    return FlatScene.load_npz(os.path.join(ROOT, "tests", "golden", "cornell_flat.npz"))


@pytest.fixture(scope="module")
def cornell_move(cornell):
    """(moved scene, {node: matrix}, first, (2, 16) matrices): the last two nodes moved, as test_gpu_refit.py moves them"""
    n = len(cornell.nodes)
    mflat, mats = moved(cornell, [n - 2, n - 1], 11, mirror_first=False, scale=False)
    return mflat, mats, n - 2, _stack(mats, (n - 2, n - 1))


def _render(r, flat, W=64, H=48, stream=None):
    """(image digest, counters) of 2 frames, 2 spp, depth 4"""
    from vkrt_amd.flat_scene import make_push_constants

    cam = default_camera(W, H)
    r.reset_counters(stream=stream)
    img = None
    for f in range(2):
        img = r.pathtrace(make_push_constants(samples=2, depth=4, frame=f, lights_count=len(flat.lights)), cam, W, H, seed=3 + f, image=img, stream=stream)
    if stream is not None:
        stream.synchronize()
    c = r.counters()
    assert c["traversal_faults"] == 0
    return _digest(img), {k: c[k] for k in ("rays_closest", "rays_shadow", "hits", "pixels", "traversal_faults")}


@pytest.fixture(scope="module")
def cornell_fresh(cornell_move):
    """digest and counters of fresh builds of the moved Cornell box, per (builder, layout)"""
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer

    out = {}
    for kind, layout in (("ploc", 1), ("ploc", 0), ("lbvh", 1), ("sah", 1)):
        f = Renderer(cornell_move[0], device=0, build=kind, options={abi.VKRT_OPT_BVH_LAYOUT: layout})
        out[kind, layout] = _render(f, cornell_move[0])
        if (kind, layout) == ("ploc", 1):
            out["split"] = f.split_references(30)
        f.close()
    return out


# ---- 1. records ------------------------------------------------------------------------------------------------------------------------
def test_dense_device_updates_write_the_hosts_records(flat):
    """Ranges of 1, 63, 64, 65 and all 300 nodes (below, at and above a wave; more than one workgroup), each holding a mirrored matrix,
    the larger ones a zero scale too: after each, all 300 records equal the host-path twin's, and those outside the range are untouched."""
    from vkrt_amd.renderer import Renderer

    r, twin = Renderer(flat, device=0, build=None), Renderer(flat, device=0, build=None)
    assert np.array_equal(_bytes(r.read_instances(0, NODES)), _bytes(twin.read_instances(0, NODES)))
    for step, (first, count) in enumerate(((0, 1), (5, 63), (7, 64), (3, 65), (0, NODES))):
        nodes = list(range(first, first + count))
        _, mats = moved(flat, nodes, 50 + step, mirror_first=True)  # (each step from the first pose: the range's first node is mirrored)
        if count > 2:
            mats[first + 2] = np.zeros(16, np.float32)  # a zero scale: a hidden instance, a singular matrix
            mats[first + 2][12:15] = (1.0, 2.0, 3.0 + step)
        before = r.read_instances(0, NODES)
        r.update_nodes(first, _device(_stack(mats, nodes)))
        twin.update_nodes(first, _stack(mats, nodes))
        got, want = r.read_instances(0, NODES), twin.read_instances(0, NODES)
        assert np.array_equal(_bytes(got), _bytes(want)), (first, count, np.flatnonzero((_bytes(got) != _bytes(want)).any(1))[:8])
        outside = np.ones(NODES, bool)
        outside[first:first + count] = False
        assert np.array_equal(_bytes(got)[outside], _bytes(before)[outside])
        assert (_bytes(got)[~outside] != _bytes(before)[~outside]).any(1).all()  # every node of the range did move
        assert got["vis"][first] & MIRRORED and np.array_equal(got["primMesh"], flat.nodes["primMesh"]) and not got["pad"].any()
        if count > 2:
            assert np.isnan(got["w2o"][first + 2]).all() and not got["o2w"][first + 2][[0, 1, 2, 4, 5, 6, 8, 9, 10]].any()
    r.close()
    twin.close()


# ---- 2. sparse ---------------------------------------------------------------------------------------------------------------------------
def test_sparse_updates_device_and_host(flat):
    """130 distinct indices in random order plus three entries that name no node (skipped); then the host's sparse form; its refusal"""
    import torch
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer

    rng = np.random.default_rng(8)
    nodes = rng.choice(NODES, 130, replace=False)
    mflat, mats = moved(flat, nodes, 61, mirror_first=True)
    M = _stack(mats, nodes)
    idx = np.concatenate([nodes[:40], [NODES], nodes[40:90], [1000, -1], nodes[90:]]).astype(np.int64)  # -1: 0xffffffff
    junk = np.full((1, 16), 7.0, np.float32)
    M_all = np.concatenate([M[:40], junk, M[40:90], junk, junk, M[90:]])
    twin = Renderer(flat, device=0, build=None)
    apply(twin, mats)
    want = twin.read_instances(0, NODES)
    r = Renderer(flat, device=0, build=None)
    before = r.read_instances(0, NODES)
    r.update_nodes(0, _device(M_all), indices=_device(idx.astype(np.int32)))
    got = r.read_instances(0, NODES)
    assert np.array_equal(_bytes(got), _bytes(want))
    untouched = np.ones(NODES, bool)
    untouched[nodes] = False
    assert np.array_equal(_bytes(got)[untouched], _bytes(before)[untouched]) and untouched.sum() == NODES - 130
    r.close()
    # the sparse host form, and duplicates applied in order: the last entry of a node wins
    h = Renderer(flat, device=0, build=None)
    dup = np.concatenate([nodes[:3], nodes])
    h.update_nodes(0, np.concatenate([junk, junk, junk, M]), indices=dup)
    assert np.array_equal(_bytes(h.read_instances(0, NODES)), _bytes(want))
    # refused: an index out of range changes nothing (the library's own check; Renderer.update_nodes refuses it earlier)
    bad_idx = np.array([nodes[0], NODES, nodes[1]], np.uint32)
    other = np.ascontiguousarray(M[5:8] + 1.0)
    u = abi.NodeUpdate(C.sizeof(abi.NodeUpdate), 0, 3, abi.VKRT_MEMORY_HOST, other.ctypes.data, bad_idx.ctypes.data)
    assert h.lib.vkrt_scene_update_node_transforms(h._h, C.byref(u), None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"node_indices[1] is 300, outside the scene's 300 nodes" in h.lib.vkrt_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_bytes(h.read_instances(0, NODES)), _bytes(want))
    h.close()
    twin.close()


# ---- 3. refit equals fresh ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 0], ids=["wide8", "bvh2"])
def test_device_update_and_refit_equal_a_fresh_build(cornell, cornell_move, cornell_fresh, layout):
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer

    mflat, _, first, M = cornell_move
    r = Renderer(cornell, device=0, build="ploc", options={abi.VKRT_OPT_BVH_LAYOUT: layout})
    unmoved = _render(r, cornell)
    r.update_nodes(first, _device(M))
    r.refit()
    assert _render(r, mflat) == cornell_fresh["ploc", layout]
    assert unmoved[0] != cornell_fresh["ploc", layout][0]
    r.close()


# ---- 4. rebuild after a device update ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ploc", "lbvh", "sah"])
def test_a_rebuild_after_a_device_update_builds_the_moved_scene(cornell, cornell_move, cornell_fresh, kind):
    """every builder and the scene bounds read the host copy of the matrices: the build downloads it first"""
    from vkrt_amd.renderer import Renderer

    mflat, _, first, M = cornell_move
    r = Renderer(cornell, device=0, build=kind)
    r.update_nodes(first, _device(M))
    r.build(kind)
    assert _render(r, mflat) == cornell_fresh[kind, 1]
    r.close()


def test_split_references_after_a_device_update_are_the_moved_scenes(cornell, cornell_move, cornell_fresh):
    from vkrt_amd.renderer import Renderer, VkrtError

    _, _, first, M = cornell_move
    r = Renderer(cornell, device=0, build=None)
    r.update_nodes(first, _device(M))
    got, want = r.split_references(30), cornell_fresh["split"]
    assert got["ref_count"] == want["ref_count"] > 0
    for k in ("prio", "scale", "ref_tri", "ref_box"):
        assert np.array_equal(np.asarray(got[k]).view(np.uint32), np.asarray(want[k]).view(np.uint32)), k
    # a matrix that is not finite came through the device path unseen: the build refuses it and builds nothing; a correct update repairs
    bad = M.copy()
    bad[1, 13] = np.inf
    r.update_nodes(first, _device(bad))
    with pytest.raises(VkrtError, match=r"\(1\).*node %d: worldMatrix\[13\] is not finite" % (first + 1)):
        r.build("ploc")
    with pytest.raises(VkrtError, match=NOT_BUILT):
        r.accel_info()
    r.update_nodes(first + 1, _device(M[1:]))
    r.build("ploc")
    assert _render(r, cornell_move[0]) == cornell_fresh["ploc", 1]
    r.close()


# ---- 5. visibility after a device update ---------------------------------------------------------------------------------------------------
def test_visibility_after_a_device_update_keeps_the_transform(flat):
    import torch
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer, pack_rays

    i, j = 44, 131  # a quad that gets mask 1, a box that is moved and keeps its visibility
    mflat, mats = moved(flat, [i, j], 71, mirror_first=True)
    r = Renderer(flat, device=0, build="ploc")
    r.update_nodes(0, _device(_stack(mats, (i, j))), indices=_device(np.array([i, j], np.int32)))
    r.set_instance_visibility(i, [1], [0])
    r.refit()
    f = Renderer(mflat, device=0, build="ploc")
    f.set_instance_visibility(i, [1], [0])
    got, want = r.read_instances(0, NODES), f.read_instances(0, NODES)
    assert np.array_equal(_bytes(got), _bytes(want))
    assert got["vis"][i] == (MIRRORED | 1) and got["vis"][j] == 0xFF | (abi.VKRT_INSTANCE_FACING_CULL_DISABLE << 8)
    rays = pack_rays(*(_device(a) for a in rays_from_above()))
    on_i = {}
    for cull_mask, ray_flags in ((0xFF, 0), (1, 0), (0xFE, 0), (0xFF, abi.VKRT_RAY_CULL_BACK_FACING), (0xFF, abi.VKRT_RAY_CULL_FRONT_FACING)):
        a, b = r.intersect(rays, cull_mask=cull_mask, ray_flags=ray_flags), f.intersect(rays, cull_mask=cull_mask, ray_flags=ray_flags)
        torch.cuda.synchronize()
        assert torch.equal(a.buffer.view(torch.int32), b.buffer.view(torch.int32)), (cull_mask, ray_flags)
        on_i[cull_mask, ray_flags] = int((a.instance == i).sum())
    # the device-moved quad is seen from above and below, is hidden from a mask without bit 0, and -- no FACING_CULL_DISABLE any more --
    # is culled by facing: each of its hits falls to exactly one of the two flags (nothing lies above or below it)
    back, front = on_i[0xFF, abi.VKRT_RAY_CULL_BACK_FACING], on_i[0xFF, abi.VKRT_RAY_CULL_FRONT_FACING]
    assert on_i[0xFF, 0] == on_i[1, 0] > 4 and on_i[0xFE, 0] == 0
    assert back > 0 and front > 0 and back + front == on_i[0xFF, 0]
    for x in (r, f):
        assert x.counters()["traversal_faults"] == 0
        x.close()


# ---- 6. motion ---------------------------------------------------------------------------------------------------------------------------
def test_motion_after_a_device_update_equals_the_host_paths(flat):
    import torch
    from vkrt_amd.renderer import Renderer, pack_rays

    nodes = list(range(90, 170))
    _, mats = moved(flat, nodes, 81, mirror_first=True)
    rays = pack_rays(*(_device(a) for a in rays_from_above(8000)))
    out = []
    for device in (True, False):
        r = Renderer(flat, device=0, build="ploc")
        hits = r.intersect(rays)
        r.motion_mark()
        r.update_nodes(nodes[0], _device(_stack(mats, nodes)) if device else _stack(mats, nodes))
        cur, prev = r.hit_motion(hits)  # (needs no tree: the live records and the snapshot)
        torch.cuda.synchronize()
        out.append((hits.buffer.cpu().numpy().view(np.uint32), cur.cpu().numpy().view(np.uint32), prev.cpu().numpy().view(np.uint32)))
        r.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    inst = out[0][0].view(np.int32)[:, 3]
    moving = (inst >= nodes[0]) & (inst <= nodes[-1])
    assert moving.sum() > 100 and (out[0][1][moving] != out[0][2][moving]).any(1).all()  # hits on moved nodes were elsewhere before
    still = (inst >= 0) & ~moving
    assert still.sum() > 100 and np.array_equal(out[0][1][still], out[0][2][still])


# ---- 7. stream order ---------------------------------------------------------------------------------------------------------------------
def test_update_refit_and_trace_in_stream_order_without_a_wait(cornell, cornell_move, cornell_fresh):
    """the matrices come out of a torch op on the same stream; update, refit and trace follow with no synchronisation in between"""
    import torch
    from vkrt_amd.renderer import Renderer

    mflat, _, first, M = cornell_move
    r = Renderer(cornell, device=0, build="ploc")
    base = _device(M)
    x = torch.rand((1 << 22,), device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=0)
    with torch.cuda.stream(s):
        mats = base + 0 * (x.sort().values[:32].reshape(2, 16))  # some work in front of the values
        r.update_nodes(first, mats, stream=s)
        r.refit(stream=s)
        got = _render(r, mflat, stream=s)
    assert got == cornell_fresh["ploc", 1]
    r.close()


# ---- 8. errors with a scene ----------------------------------------------------------------------------------------------------------------
def test_refusals_with_a_scene_and_the_stale_tree(cornell, cornell_move, cornell_fresh):
    import torch
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Renderer, VkrtError, pack_rays

    mflat, _, first, M = cornell_move
    n = len(cornell.nodes)
    r = Renderer(cornell, device=0, build="ploc")
    lib, fn = r.lib, r.lib.vkrt_scene_update_node_transforms
    unmoved = _render(r, cornell)
    before = r.read_instances(0, n)
    dev, didx = _device(np.concatenate([M, M])), _device(np.array([first, first + 1, 0, 0], np.int32))
    nan, idx = M.copy(), np.array([first, n], np.uint32)
    nan[1, 6] = np.nan
    HOST, DEVICE = abi.VKRT_MEMORY_HOST, abi.VKRT_MEMORY_DEVICE

    def refused(text, first_, count, memory, matrices, indices=None):
        u = abi.NodeUpdate(C.sizeof(abi.NodeUpdate), first_, count, memory, matrices, indices)
        assert fn(r._h, C.byref(u), None) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert text in lib.vkrt_last_error(), lib.vkrt_last_error()

    # each refusal with the later ones behind it: the range, NULL matrices, alignment (device), an index, a value (host)
    refused(b"nodes [%d, %d) outside the scene's %d nodes" % (first, n + 1, n), first, 3, HOST, None)
    refused(b"nodes [%d, %d) outside" % (n + 1, n + 1), n + 1, 0, DEVICE, None)
    refused(b"outside", 0xFFFFFFFF, 2, DEVICE, dev.data_ptr() + 4)
    refused(b"world_matrices is NULL", 0, 2, DEVICE, None, didx.data_ptr() + 2)
    refused(b"world_matrices is NULL", first, 2, DEVICE, None)
    refused(b"world_matrices is NULL", 0, 2, HOST, None, idx.ctypes.data)
    refused(b"is not 16-byte aligned", first, 2, DEVICE, dev.data_ptr() + 4)
    refused(b"world_matrices", 0, 2, DEVICE, dev.data_ptr() + 8, didx.data_ptr() + 2)
    refused(b"node_indices", 0, 2, DEVICE, dev.data_ptr(), didx.data_ptr() + 2)
    refused(b"node_indices[1] is %d" % n, 0, 2, HOST, nan.ctypes.data, idx.ctypes.data)
    refused(b"world_matrices[22] (entry 1, node %d) is not finite" % (first + 1), first, 2, HOST, nan.ctypes.data)
    refused(b"world_matrices[22] (entry 1, node 0) is not finite", 0, 2, HOST, nan.ctypes.data, np.array([first, 0], np.uint32).ctypes.data)
    # count == 0: accepted, nothing enqueued, the tree stays usable (NULL arrays, either memory, either form)
    for memory, ix in ((HOST, None), (DEVICE, None), (DEVICE, didx.data_ptr()), (HOST, idx.ctypes.data)):
        u = abi.NodeUpdate(C.sizeof(abi.NodeUpdate), 0 if ix else n, 0, memory, None, ix)
        assert fn(r._h, C.byref(u), None) == abi.VKRT_OK
    torch.cuda.synchronize()
    assert np.array_equal(_bytes(r.read_instances(0, n)), _bytes(before))
    assert _render(r, cornell) == unmoved
    # vkrt_debug_read_instances: its own refusals
    out = np.zeros(n + 1, np.dtype((np.uint8, 96)))
    for args in ((0, n + 1, out.ctypes.data, 96 * (n + 1)), (n, 1, out.ctypes.data, 96), (0, n, out.ctypes.data, 96 * n - 4), (0, n, out.ctypes.data, 96 * n + 96),
                 (0, n, None, 96 * n), (0xFFFFFFFF, 2, out.ctypes.data, 192)):
        assert lib.vkrt_debug_read_instances(r._h, *args) == abi.VKRT_ERR_INVALID_ARGUMENT, args
    assert lib.vkrt_debug_read_instances(r._h, n, 0, out.ctypes.data, 0) == abi.VKRT_OK and not out.any()
    # an accepted update makes the tree stale: traces and queries refuse until the refit; surface and motion reads need no tree
    rays = pack_rays(*(_device(a) for a in (np.array([[0.0, 1.0, 5.0]], np.float32), np.array([[0.0, 0.0, -1.0]], np.float32))))
    hits = r.intersect(rays)
    r.update_nodes(first, dev[:2])
    pc, cam = make_push_constants(samples=1, depth=2, frame=0, lights_count=len(cornell.lights)), default_camera(64, 48)
    for call in (lambda: r.pathtrace(pc, cam, 64, 48), lambda: r.gbuffer_raycast(cam, 64, 48), lambda: r.intersect(rays), lambda: r.occluded(rays),
                 lambda: r.intersect(rays, cull_mask=1), r.read_accel):
        with pytest.raises(VkrtError, match=NOT_BUILT):
            call()
    r.surface(hits)
    r.hit_motion(hits)
    # a host update of the other nodes in between: primMesh is still checked against the host copy, the device-moved nodes stay
    r.update_nodes(0, np.stack([cornell.nodes[k]["worldMatrix"] for k in range(first)]))
    wrong = abi.Node()
    wrong.worldMatrix[:] = [float(v) for v in M[0]]
    wrong.primMesh = (int(cornell.nodes[first]["primMesh"]) + 1) % len(cornell.prim_meshes)
    assert lib.vkrt_scene_update_nodes(r._h, first, 1, C.byref(wrong), None) == abi.VKRT_ERR_INVALID_ARGUMENT and b"primMesh" in lib.vkrt_last_error()
    r.refit()
    assert _render(r, mflat) == cornell_fresh["ploc", 1]
    r.build("sah")  # (the download still happens: the host update covered other nodes)
    assert _render(r, mflat) == cornell_fresh["sah", 1]
    r.close()
