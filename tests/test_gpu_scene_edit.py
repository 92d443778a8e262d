"""Editing a live scene's lights, materials and textures (vkrt_scene_update_lights / _materials / _texture).  Scene A is created from the
base data of scene_edit_scenes.py and updated to the target; scene B is a fresh scene created from the target.  Everything that can be
read or rendered must then be equal bit for bit: the three tables, every mip level and footprint record, frames in both execution modes,
the hybrid planes, surfaces, alpha-tested queries; in stream order, with no refit and no rebuild.  No tolerances."""
import ctypes as C

import numpy as np
import pytest

from conftest import default_camera
from scene_edit_scenes import NOISE, base_scene, target_images, target_scene
from test_texture_lod import CAMERA

pytestmark = pytest.mark.gpu

NOT_BUILT = r"\(5\)"
W, H = 48, 32


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t).view(np.uint8)


@pytest.fixture(scope="module")
def base():
    return base_scene()


@pytest.fixture(scope="module")
def target(base):
    return target_scene(base)


def _edit(r, target, memory="device", stream=None, textures=None):
    """lights, materials and textures of `r` to the target's; lights and materials in two ranges each, the second ending at the table's end"""
    lights = target.lights
    if memory == "device":
        import torch

        dl = _dev(lights.view(np.float32).reshape(-1, 8))
        images = [_dev(t["rgba8"]) for t in target.textures]
        torch.cuda.synchronize()
        r.update_lights(1, dl[1:], stream=stream)  # (row 1 of an (n, 8) float32 tensor: 32-byte offset, 16-byte aligned)
        r.update_lights(0, dl[:1], stream=stream)
    else:
        images = [t["rgba8"] for t in target.textures]
        r.update_lights(1, lights[1:], stream=stream)
        r.update_lights(0, lights[:1], stream=stream)
    r.update_materials(2, target.materials[2:], stream=stream)
    r.update_materials(0, target.materials[:2], stream=stream)
    for ti in (range(len(images)) if textures is None else textures):
        r.update_texture(ti, images[ti], stream=stream)
    return images, (dl if memory == "device" else None)


def _tables(r, flat, quads=True):
    """every byte the readers give: lights, material records, every level of every texture, every footprint record"""
    out = {"lights": _bits(r.read_lights(0, len(flat.lights))), "materials": _bits(r.read_materials(0, len(flat.materials)))}
    for ti, t in enumerate(flat.textures):
        h, w = t["rgba8"].shape[:2]
        levels = int(np.floor(np.log2(max(w, h)))) + 1
        for L in range(levels):
            if L == 0 and quads:
                out[f"texture {ti} level 0"], out[f"texture {ti} quads"] = r.read_texture(ti, 0, quads=True)
            else:
                out[f"texture {ti} level {L}"] = r.read_texture(ti, L)
    return out


def _same(got, want):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


# ---- 5. tables -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("memory", ["host", "device"])
def test_an_edited_scene_holds_the_tables_of_a_fresh_one(base, target, memory):
    from vkrt_amd.renderer import Renderer

    a, b = Renderer(base, device=0, build=None), Renderer(target, device=0, build=None)
    try:
        before, want = _tables(a, base), _tables(b, target)
        assert any(not np.array_equal(before[k], want[k]) for k in want if k.startswith("texture")) and not np.array_equal(before["lights"], want["lights"])
        keep = _edit(a, target, memory)
        _same(_tables(a, base), want)
        # level 0 is the image itself, the quads its REPEAT neighbourhoods, the alpha modes are untouched
        for ti, t in enumerate(target.textures):
            assert np.array_equal(want[f"texture {ti} level 0"], t["rgba8"])
        rec = a.read_materials(0, 4)
        assert (rec["alphaMode"] == 0).all() and (rec["alphaCutoff"] == np.float32(0.5)).all() and rec["m"].tobytes() == target.materials.tobytes()
        # and back again, texture by texture: an update reaches its own texture only
        for ti, t in enumerate(base.textures):
            a.update_texture(ti, t["rgba8"] if memory == "host" else _dev(t["rgba8"]))
            got = _tables(a, base)
            for tj in range(len(base.textures)):
                src = before if tj <= ti else want
                for k in src:
                    if k.startswith(f"texture {tj} "):
                        assert np.array_equal(got[k], src[k]), (ti, k)
        del keep
    finally:
        a.close()
        b.close()


def test_alpha_modes_survive_a_material_update(base, target):
    from vkrt_amd.renderer import Renderer

    a = Renderer(base, device=0, build=None)
    try:
        a.set_material_alpha(0, [1, 0, 1, 1], [0.25, 0.5, 0.75, 0.125])
        a.update_materials(0, target.materials)
        rec = a.read_materials(0, 4)
        assert list(rec["alphaMode"]) == [1, 0, 1, 1] and list(rec["alphaCutoff"]) == [0.25, 0.5, 0.75, 0.125]
        assert rec["m"].tobytes() == target.materials.tobytes() and not rec["pad"].any()
    finally:
        a.close()


def test_without_a_footprint_pool_the_pools_are_equal_and_quads_unsupported(base, target, monkeypatch):
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer, VkrtError

    monkeypatch.setenv("VKRT_TEX_QUADS", "0")
    a, b = Renderer(base, device=0, build=None), Renderer(target, device=0, build=None)
    try:
        _edit(a, target, "device")
        _same(_tables(a, base, quads=False), _tables(b, target, quads=False))
        for r in (a, b):
            with pytest.raises(VkrtError, match=rf"\({abi.VKRT_ERR_UNSUPPORTED}\).*no footprint pool"):
                r.read_texture(NOISE, 0, quads=True)
        offsets = a.read_materials(0, 4)["ref"][:, 1::2] & 0x7FFFFFFF
        assert offsets.max() > 0 and np.array_equal(a.read_materials(0, 4)["tex"][:, :, 3], np.zeros((4, 4), np.uint32))
    finally:
        a.close()
        b.close()


def test_refusals_with_a_scene_come_in_the_headers_order_and_change_nothing(base):
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import MAT_DTYPE
    from vkrt_amd.renderer import Renderer

    a = Renderer(base, device=0, build=None)
    lib, h, BAD = a.lib, a._h, abi.VKRT_ERR_INVALID_ARGUMENT
    try:
        before = _tables(a, base)

        def refused(rc, text, code=BAD):
            assert rc == code and text in lib.vkrt_last_error(), (rc, lib.vkrt_last_error())

        lights = np.ones(2, base.lights.dtype)
        lu = lambda **k: C.byref(abi.LightUpdate(24, k.get("first", 0), k.get("count", 2), k.get("memory", 0), k.get("lights", lights.ctypes.data)))  # noqa: E731
        refused(lib.vkrt_scene_update_lights(h, lu(first=1, lights=None), None), b"lights [1, 3) outside the scene's 2 lights")  # the range before the NULL array
        refused(lib.vkrt_scene_update_lights(h, lu(first=3, count=0), None), b"lights [3, 3) outside")
        refused(lib.vkrt_scene_update_lights(h, lu(lights=None, memory=1), None), b"lights is NULL")
        refused(lib.vkrt_scene_update_lights(h, lu(lights=0x1008, memory=1), None), b"not 16-byte aligned")
        assert lib.vkrt_scene_update_lights(h, lu(first=2, count=0, lights=None), None) == abi.VKRT_OK  # an empty range at the end
        mats = np.zeros(2, MAT_DTYPE)
        mats["pbrBaseColorTexture"][1] = 7
        refused(lib.vkrt_scene_update_materials(h, 3, 2, mats.ctypes.data, None), b"materials[1]: texture index 7 out of range")  # before the range
        mats["pbrBaseColorTexture"][1] = -1
        refused(lib.vkrt_scene_update_materials(h, 3, 2, mats.ctypes.data, None), b"materials [3, 5) outside the scene's 4 materials")
        refused(lib.vkrt_scene_update_materials(h, 3, 2, None, None), b"materials is NULL")
        assert lib.vkrt_scene_update_materials(h, 4, 0, None, None) == abi.VKRT_OK
        img = np.zeros((21, 37, 4), np.uint8)
        tu = lambda **k: C.byref(abi.TextureUpdate(32, k.get("texture", 0), k.get("width", 37), k.get("height", 21), k.get("memory", 0),  # noqa: E731
                                                   k.get("rgba8", img.ctypes.data)))
        refused(lib.vkrt_scene_update_texture(h, tu(texture=7, width=1, rgba8=None), None), b"texture 7 outside the scene's 7 textures")
        refused(lib.vkrt_scene_update_texture(h, tu(width=21, height=37, rgba8=None), None), b"21x37: texture 0 is 37x21")
        refused(lib.vkrt_scene_update_texture(h, tu(rgba8=None, memory=1), None), b"rgba8 is NULL")
        refused(lib.vkrt_scene_update_texture(h, tu(rgba8=0x1004, memory=1), None), b"not 16-byte aligned")
        out = np.zeros(4096, np.uint8)
        refused(lib.vkrt_debug_read_lights(h, 0, 2, out.ctypes.data, 63), b"bytes 63")
        refused(lib.vkrt_debug_read_materials(h, 2, 3, out.ctypes.data, 576), b"outside the scene's 4 materials")
        refused(lib.vkrt_debug_read_texture(h, 0, 6, out.ctypes.data, 4, None, 0), b"level 6 outside texture 0's 6 levels")
        refused(lib.vkrt_debug_read_texture(h, 0, 5, out.ctypes.data, 8, None, 0), b"texel_bytes 8")
        refused(lib.vkrt_debug_read_texture(h, 0, 5, out.ctypes.data, 4, out.ctypes.data, 16), b"quads with level 5")
        _same(_tables(a, base), before)
    finally:
        a.close()


# ---- 6. frames and samples -------------------------------------------------------------------------------------------------------------
def _rays(n=24):
    """a grid of rays from the camera of test_texture_lod.py over both floor strips and both walls"""
    import torch
    from vkrt_amd.renderer import pack_rays

    x, y = np.meshgrid(np.linspace(-3.4, 3.4, n), np.linspace(-1.0, 4.5, n))
    eye = np.array(CAMERA["eye"], np.float32)
    d = np.stack([x.ravel(), y.ravel(), np.full(x.size, -10.0)], 1).astype(np.float32) - eye
    return pack_rays(torch.from_numpy(np.tile(eye, (d.shape[0], 1))).to("cuda:0"), torch.from_numpy(d).to("cuda:0"))


def _frames(r, flat, stream=None, image=None):
    """two path-traced frames (4 spp, depth 3) accumulated into one image"""
    from vkrt_amd.flat_scene import make_push_constants

    cam = default_camera(W, H, **CAMERA)
    for f in range(2):
        image = r.pathtrace(make_push_constants(samples=4, depth=3, frame=f, lights_count=len(flat.lights)), cam, W, H, seed=11 + f, image=image, stream=stream)
    return image


def _everything(r, flat):
    """what a scene renders and samples: the two frames with their ray counters, the G-buffer with mips and the hybrid accumulation plane,
    the surfaces at the hits of a ray grid"""
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants

    cam = default_camera(W, H, **CAMERA)
    out = {}
    r.reset_counters()
    out["image"] = _bits(_frames(r, flat))
    c = r.counters()
    assert c["traversal_faults"] == 0
    out["counters"] = np.array([c[k] for k in ("rays_closest", "rays_shadow", "hits", "diffuse_hits", "pixels")], np.uint64)
    assert r.get_option(abi.VKRT_OPT_GBUFFER_MIPS) == 1
    g = r.gbuffer_raycast(cam, W, H, lights_count=len(flat.lights))
    for k, v in g.items():
        out["gbuffer " + k] = _bits(v)
    pc = make_push_constants(samples=2, depth=3, frame=0, lights_count=len(flat.lights))
    out["hybrid"] = _bits(r.hybrid_trace(pc, cam, W, H, g, seed=5))
    hits = r.intersect(_rays())
    assert int((hits.instance >= 0).sum()) > 300
    out["hits"] = _bits(hits.buffer)
    out["surface"] = _bits(r.surface(hits, material=True).buffer)
    return out


@pytest.mark.parametrize("mode", [1, 0], ids=["wavefront", "megakernel"])
def test_an_edited_scene_renders_and_samples_like_a_fresh_one(base, target, mode):
    """no refit and no rebuild after the updates, and no call answers VKRT_ERR_NOT_BUILT (any would raise)"""
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer

    a = Renderer(base, device=0, build="ploc", options={abi.VKRT_OPT_MODE: mode})
    b = Renderer(target, device=0, build="ploc", options={abi.VKRT_OPT_MODE: mode})
    try:
        before, want = _everything(a, base), _everything(b, target)
        for k in ("image", "gbuffer color", "hybrid", "surface"):
            assert not np.array_equal(before[k], want[k]), k  # the edit is visible in each of them
        assert np.array_equal(before["hits"], want["hits"])  # and the geometry is the same
        keep = _edit(a, target, "device")
        _same(_everything(a, base), want)
        del keep
    finally:
        a.close()
        b.close()


# ---- 7. stream order -------------------------------------------------------------------------------------------------------------------
def test_updates_are_ordered_on_the_callers_stream(base, target):
    """trace, all three updates, trace again on one non-default stream with no host wait in between; the host arrays are overwritten as
    soon as their calls return"""
    import torch
    from vkrt_amd.renderer import Renderer

    a, fresh_a, fresh_b = (Renderer(f, device=0, build="ploc") for f in (base, base, target))
    try:
        want_first, want_second = _bits(_frames(fresh_a, base)), _bits(_frames(fresh_b, target))
        assert not np.array_equal(want_first, want_second)
        images = [_dev(t["rgba8"]) for t in target.textures]
        first, second = (torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(2))
        lights, mats = target.lights.copy(), target.materials.copy()
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device="cuda:0")
        _frames(a, base, stream=s, image=first)
        a.update_lights(0, lights, stream=s)
        lights[:] = np.zeros(1, lights.dtype)[0]
        a.update_materials(0, mats, stream=s)
        mats[:] = np.zeros(1, mats.dtype)[0]
        for ti, img in enumerate(images):
            a.update_texture(ti, img, stream=s)
        _frames(a, target, stream=s, image=second)
        s.synchronize()
        assert np.array_equal(_bits(first), want_first)
        assert np.array_equal(_bits(second), want_second)
    finally:
        for r in (a, fresh_a, fresh_b):
            r.close()


# ---- 8. alpha test ---------------------------------------------------------------------------------------------------------------------
def test_a_new_alpha_channel_changes_alpha_tested_queries_without_a_refit(base):
    """every material VKRT_ALPHA_MASK; the base-colour textures get the target's texels, alpha channel included"""
    import copy
    from vkrt_amd.renderer import Renderer

    images = target_images(base)
    fresh = copy.deepcopy(base)
    for t, img in zip(fresh.textures, images):
        t["rgba8"] = img
    a, b = Renderer(base, device=0, build="ploc"), Renderer(fresh, device=0, build="ploc")
    try:
        rays = _rays(40)
        for r in (a, b):
            r.set_material_alpha(0, [1, 1, 1, 1], 0.5)
        before = _bits(a.intersect(rays).buffer), _bits(a.occluded(rays))
        want = _bits(b.intersect(rays).buffer), _bits(b.occluded(rays))
        assert not np.array_equal(before[0], want[0]) and not np.array_equal(before[1], want[1])
        for ti, img in enumerate(images):
            a.update_texture(ti, _dev(img))
        got = _bits(a.intersect(rays).buffer), _bits(a.occluded(rays))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        opaque = _bits(a.intersect(rays, ray_flags=1).buffer)  # VKRT_RAY_OPAQUE: the test is what makes the difference
        assert not np.array_equal(opaque, got[0])
    finally:
        a.close()
        b.close()


# ---- 9. dissolve -----------------------------------------------------------------------------------------------------------------------
def _with_alpha(flat, alphas):
    import copy

    f = copy.deepcopy(flat)
    for k, a in enumerate(alphas):
        f.materials[k]["pbrBaseColorFactor"][3] = a
    return f


def test_dissolve_needs_a_rebuild_only_when_a_material_turns_non_opaque(base):
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer, VkrtError

    opts = {abi.VKRT_OPT_ANYHIT_DISSOLVE: 1}
    start, lower, turned = _with_alpha(base, [0.5, 1, 1, 1]), _with_alpha(base, [0.25, 1, 1, 1]), _with_alpha(base, [0.25, 0.5, 1, 1])
    rays = _rays(40)

    def queries(r):
        return _bits(r.intersect(rays, seed=9).buffer), _bits(r.occluded(rays, seed=9))

    a = Renderer(start, device=0, build="ploc", options=opts)
    try:
        want = {}
        for name, flat in (("start", start), ("lower", lower), ("turned", turned)):
            f = Renderer(flat, device=0, build="ploc", options=opts)
            want[name] = queries(f)
            f.close()
        assert not np.array_equal(want["start"][0], want["lower"][0]) and not np.array_equal(want["lower"][0], want["turned"][0])
        # 0.5 -> 0.25: the triangles carry the flag already
        a.update_materials(0, lower.materials[:1])
        got = queries(a)
        assert np.array_equal(got[0], want["lower"][0]) and np.array_equal(got[1], want["lower"][1])
        # 1.0 -> 0.5: their triangles do not
        a.update_materials(1, turned.materials[1:2])
        for call in (lambda: a.intersect(rays, seed=9), lambda: a.occluded(rays, seed=9), a.refit, lambda: _frames(a, turned)):
            with pytest.raises(VkrtError, match=NOT_BUILT + ".*vkrt_scene_update_materials"):
                call()
        a.update_materials(1, start.materials[1:2])  # opaque again: still refused, the rule looks at updates, not at the current state
        with pytest.raises(VkrtError, match=NOT_BUILT):
            a.intersect(rays, seed=9)
        a.update_materials(1, turned.materials[1:2])
        a.build("ploc")
        got = queries(a)
        assert np.array_equal(got[0], want["turned"][0]) and np.array_equal(got[1], want["turned"][1])
        # the opposite direction needs nothing
        a.update_materials(0, _with_alpha(base, [1, 0.5, 1, 1]).materials[:1])
        f = Renderer(_with_alpha(base, [1, 0.5, 1, 1]), device=0, build="ploc", options=opts)
        fresh = queries(f)
        f.close()
        got = queries(a)
        assert np.array_equal(got[0], fresh[0]) and np.array_equal(got[1], fresh[1])
    finally:
        a.close()
    # built without the option, the same update needs nothing
    a, f = Renderer(start, device=0, build="ploc"), Renderer(turned, device=0, build="ploc")
    try:
        a.update_materials(0, turned.materials)
        got, fresh = queries(a), queries(f)
        assert np.array_equal(got[0], fresh[0]) and np.array_equal(got[1], fresh[1])
        assert np.array_equal(_bits(_frames(a, turned)), _bits(_frames(f, turned)))
    finally:
        a.close()
        f.close()
