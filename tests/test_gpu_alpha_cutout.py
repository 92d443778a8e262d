"""Alpha-tested ray queries (vkrt_scene_set_material_alpha; include/vkrt.h "alpha-tested materials"): a candidate on a MASK material is
ignored inside the walk when !(alpha >= cutoff).

The reference of every comparison is the machinery the library had before the stage, on a renderer whose materials are all opaque:
intersect_multi(rays, 16, VKRT_RAY_OPAQUE) lists every candidate in order, surface() gives each one's alpha, and the first entry that
is not MASK or has alpha >= cutoff is the expected closest hit (its existence the expected occlusion).  A ray whose list is full
without an admitted entry cannot be judged and is left out; the tests bound how many may be."""
import copy
import hashlib
import os
import sys

import numpy as np
import pytest

import test_gpu_hit_surface as S
import test_gpu_ray_query as Q
from scene_motion import apply, moved

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

F = np.float32
OPAQUE_FLAG, BACK = 0x1, 0x10  # VKRT_RAY_OPAQUE, VKRT_RAY_CULL_BACK_FACING
MASK = 1
CONFIGS = [(k, lay) for k in Q.KINDS for lay in (1, 0)]
KMAX = 16


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def _sync():
    import torch

    torch.cuda.current_stream().synchronize()


def _candidates(r, rays, seed=0, dissolve_of=None, **kw):
    """Every candidate of every ray in order, from a renderer that ignores nothing (VKRT_RAY_OPAQUE): records uint32 [N, 16, 8], counts,
    alpha float32 [N, 16] of surface().  dissolve_of: the scene's materials when the dissolve rule of tests/test_oracle.py applies too
    (ignored iff factor.a < 1 and (factor.a == 0 or rnd(tea(triangle id, seed)) > factor.a)) -> also `dissolved` bool [N, 16]."""
    flags = kw.pop("ray_flags", 0) | OPAQUE_FLAG
    h = r.intersect_multi(rays, KMAX, seed=seed, ray_flags=flags, **kw)
    s = r.surface(h.flat())
    _sync()
    buf = h.buffer.cpu().numpy().view(np.uint32).copy()
    cnt = h.count.cpu().numpy().copy()
    alpha = s.alpha.cpu().numpy().reshape(buf.shape[0], KMAX).copy()
    dissolved = np.zeros(alpha.shape, bool)
    if dissolve_of is not None:
        import np_pathtrace

        gid = buf[:, :, 6].view(np.int32)
        live = gid >= 0
        a = dissolve_of["pbrBaseColorFactor"][np.maximum(buf[:, :, 7].view(np.int32), 0), 3].astype(F)
        st = np_pathtrace.tea(np.where(live, gid, 0).astype(np.uint32).ravel(), np.full(gid.size, seed, np.uint32))
        _, rn = np_pathtrace.rnd(st)
        dissolved = live & (a < 1.0) & ((a == 0.0) | (rn.reshape(gid.shape) > a))
    return buf, cnt, alpha, dissolved


def _expected(cand, modes, cutoffs, tmax):
    """From the candidate lists: (admitted bool [N, 16], judged bool [N], expected vkrt_hit words uint32 [N, 8], expected occlusion)."""
    buf, cnt, alpha, dissolved = cand
    n = buf.shape[0]
    mat = np.maximum(buf[:, :, 7].view(np.int32), 0)
    live = np.arange(KMAX)[None, :] < cnt[:, None]
    masked = np.asarray(modes)[mat] == MASK
    with np.errstate(invalid="ignore"):
        admitted = live & ~dissolved & (~masked | (alpha >= np.asarray(cutoffs, F)[mat]))
    any_adm = admitted.any(1)
    judged = any_adm | (cnt < KMAX)
    first = np.argmax(admitted, 1)
    want = np.zeros((n, 8), np.uint32)
    want[:, 0] = np.broadcast_to(np.asarray(tmax, F), (n,)).view(np.uint32)
    want[:, 3:] = 0xFFFFFFFF
    want[any_adm] = buf[np.arange(n), first][any_adm]
    return admitted, judged, want, any_adm.astype(np.int32)


def _expected_multi(cand, admitted, k, tmax):
    """The first k admitted entries of every list with their count; judged where the list was not full or held k admitted entries."""
    buf, cnt = cand[0], cand[1]
    n = buf.shape[0]
    want = np.zeros((n, k, 8), np.uint32)
    want[:, :, 0] = np.broadcast_to(np.asarray(tmax, F), (n,)).view(np.uint32)[:, None]
    want[:, :, 3:] = 0xFFFFFFFF
    rank = np.cumsum(admitted, 1) - 1
    for j in range(KMAX):
        sel = admitted[:, j] & (rank[:, j] < k)
        want[sel, rank[sel, j]] = buf[sel, j]
    num = admitted.sum(1)
    return want, np.minimum(num, k).astype(np.int32), (cnt < KMAX) | (num >= k)


def _queries(r, rays, k=4, **kw):
    h = r.intersect(rays, **kw)
    occ = r.occluded(rays, **kw)
    m = r.intersect_multi(rays, k, **kw)
    _sync()
    return (h.buffer.cpu().numpy().view(np.uint32).copy(), occ.cpu().numpy().copy(), m.buffer.cpu().numpy().view(np.uint32).copy(),
            m.count.cpu().numpy().copy())


def _assert_stage(r, rays, cand, modes, cutoffs, tmax, max_left_out, k=4, **kw):
    """intersect / occluded / intersect_multi(k) of r equal the reference, bit for bit on all eight words, on every judged ray."""
    admitted, judged, want, want_occ = _expected(cand, modes, cutoffs, tmax)
    wm, wc, judged_m = _expected_multi(cand, admitted, k, tmax)
    print(f"left out: {int((~judged).sum())} of {len(judged)} rays (closest hit / occlusion), {int((~judged_m).sum())} (multi-hit K = {k})")
    # (a multi-hit list also needs its k admitted entries among the 16: twice the cap, still none where every list is complete)
    assert (~judged).mean() <= max_left_out and (~judged_m).mean() <= 2 * max_left_out
    hit, occ, mb, mc = _queries(r, rays, k, **kw)
    bad = np.nonzero(judged & np.any(hit != want, 1))[0]
    assert bad.size == 0, (bad[:5], hit[bad[:2]], want[bad[:2]])
    assert np.array_equal(occ[judged], want_occ[judged])
    assert np.array_equal(mc[judged_m], wc[judged_m]) and np.array_equal(mb[judged_m], wm[judged_m])
    return admitted, judged, want


# ---- scene 1: the layer stack -------------------------------------------------------------------------------------------------------
# (material, what it is) from the top layer (z = 0) down, 0.1 apart.  The solid layers sit in the middle so that rays from above and
# from below both pass several cut-out layers first.
NOISE, NPOT, ONE, LINEAR = 0, 1, 2, 3  # textures
LAYERS = [
    dict(tex=NOISE, a=1.0, mode=MASK, cutoff=0.5),    # 0: 64 x 64 noise alpha, sRGB-flagged
    dict(tex=NPOT, a=1.0, mode=MASK, cutoff=0.5),     # 1: 5 x 3
    dict(tex=ONE, a=1.0, mode=MASK, cutoff=0.5),      # 2: 1 x 1, alpha 100 / 255 < 0.5: wholly invisible
    dict(tex=-1, a=0.2, mode=MASK, cutoff=0.5),       # 3: no texture, factor.a < cutoff: wholly invisible
    dict(tex=NPOT, a=1.0, mode=MASK, cutoff=0.25),    # 4
    dict(tex=-1, a=0.9, mode=MASK, cutoff=0.5),       # 5: no texture, factor.a >= cutoff: wholly solid
    dict(tex=NOISE, a=1.0, mode=0, cutoff=0.5),       # 6: the noise texture again, OPAQUE
    dict(tex=ONE, a=1.0, mode=MASK, cutoff=0.25),     # 7: 100 / 255 >= 0.25: solid
    dict(tex=-1, a=0.2, mode=MASK, cutoff=0.0),       # 8: a cutoff of 0 admits everything
    dict(tex=NPOT, a=1.0, mode=MASK, cutoff=0.0),     # 9: the same over a texture
    dict(tex=NOISE, a=0.7, mode=MASK, cutoff=0.25),   # 10: factor.a times the tap
    dict(tex=LINEAR, a=1.0, mode=MASK, cutoff=0.5),   # 11: the linear copy of the noise texture
]
INVISIBLE, SOLID, PARTIAL = (2, 3), (5, 6, 7, 8, 9), (0, 1, 4, 10, 11)


def _layer_stack():
    from vkrt_amd.flat_scene import LIGHT_DTYPE, MAT_DTYPE, NODE_DTYPE, PRIM_DTYPE, FlatScene

    n = len(LAYERS)
    rng = np.random.default_rng(17)
    quad = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], F)
    quv = np.array([[-1.5, -1.5], [2.5, -1.5], [2.5, 2.5], [-1.5, 2.5]], F)  # REPEAT wraps negative and positive
    pos = np.concatenate([quad + F([0, 0, -0.1 * k]) for k in range(n)])
    uv = np.concatenate([quv + F([0.013 * k, -0.007 * k]) for k in range(n)])
    idx = np.tile(np.uint32([0, 1, 2, 0, 2, 3]), n)
    pm = np.zeros(n, PRIM_DTYPE)
    nodes = np.zeros(n, NODE_DTYPE)
    mats = np.zeros(n, MAT_DTYPE)
    for k, L in enumerate(LAYERS):
        pm[k] = (6 * k, 6, 4 * k, 4, k)
        nodes[k] = (np.eye(4, dtype=F).reshape(-1), k)
        mats[k]["pbrBaseColorFactor"] = (0.8, 0.7, 0.6, L["a"])
        mats[k]["metallicFactor"], mats[k]["roughnessFactor"] = 0.0, 0.8
        for t in ("metallicRoughnessTexture", "normalTexture", "emissiveTexture"):
            mats[k][t] = -1
        mats[k]["pbrBaseColorTexture"] = L["tex"]
    noise = rng.integers(0, 256, (64, 64, 4), dtype=np.uint8)
    npot = rng.integers(0, 256, (3, 5, 4), dtype=np.uint8)
    one = np.array([[[200, 150, 100, 100]]], np.uint8)
    tex = [dict(rgba8=noise, is_srgb=True), dict(rgba8=npot, is_srgb=False), dict(rgba8=one, is_srgb=True), dict(rgba8=noise.copy(), is_srgb=False)]
    lights = np.zeros(1, LIGHT_DTYPE)
    lights[0] = ((0, 0, 3), (1, 1, 1), 10.0, 0)
    flat = FlatScene(pos, np.tile(F([0, 0, 1]), (4 * n, 1)), np.tile(F([1, 0, 0, 1]), (4 * n, 1)), uv, idx, pm, mats, lights, nodes, tex)
    return flat, np.array([L["mode"] for L in LAYERS], np.uint32), np.array([L["cutoff"] for L in LAYERS], F)


def _stack_rays(per_ray_tmin=False):
    """A perpendicular grid from above and from below and two oblique grids through the stack (some rays pass beside it): 40 000 rays.
    One tmin for all of them takes the shared walk of the wide layout; per-ray tmin takes the lane walk."""
    g = np.linspace(-1.05, 1.05, 100).astype(F)
    x, y = (a.ravel() for a in np.meshgrid(g, g + F(0.003)))  # (off the quads' diagonals: a ray on a shared edge hits both triangles)
    sets = []
    for z0, d in ((1.0, (0, 0, -1)), (-2.1, (0, 0, 1)), (1.0, (0.35, 0.2, -1)), (-2.1, (-0.15, 0.45, 1))):
        d = np.asarray(d, np.float64)
        d = (d / np.linalg.norm(d)).astype(F)
        o = np.stack([x - d[0] / abs(d[2]) * 1.5 * (d[0] != 0), y - d[1] / abs(d[2]) * 1.5 * (d[1] != 0), np.full(x.shape, z0, F)], 1).astype(F)
        sets.append((o, np.tile(d, (len(x), 1))))
    o = np.concatenate([s[0] for s in sets])
    d = np.concatenate([s[1] for s in sets])
    tmin = (0.001 + 1e-5 * (np.arange(len(o)) % 7)).astype(F) if per_ray_tmin else 0.001
    return Q._pack(o, d, tmin, 100.0)


@pytest.fixture(scope="module")
def stack():
    """The layer stack, its modes, a renderer whose materials are all opaque, the two ray sets and their candidate lists."""
    flat, modes, cutoffs = _layer_stack()
    ref = Q._renderer(flat, "ploc", 1)
    rays = {lane: _stack_rays(lane) for lane in (False, True)}
    cand = {lane: _candidates(ref, rays[lane]) for lane in (False, True)}
    yield dict(flat=flat, modes=modes, cutoffs=cutoffs, ref=ref, rays=rays, cand=cand)
    ref.close()


def _masked(flat, kind, layout, modes, cutoffs, options=None):
    r = Q._renderer(flat, kind, layout, options)
    r.set_material_alpha(0, modes, cutoffs)
    return r


@pytest.mark.parametrize("kind,layout", CONFIGS)
def test_layer_stack_equals_the_filtered_candidate_lists(stack, kind, layout):
    flat, modes, cutoffs = stack["flat"], stack["modes"], stack["cutoffs"]
    r = _masked(flat, kind, layout, modes, cutoffs)
    r.reset_counters()
    assert np.array_equal(r.material_alpha()[0], modes) and np.array_equal(r.material_alpha()[1], cutoffs)
    for lane in (False, True):
        cand = stack["cand"][lane]
        assert len(LAYERS) <= cand[1].max() < KMAX  # every list is complete: no ray may be left out
        admitted, judged, want = _assert_stage(r, stack["rays"][lane], cand, modes, cutoffs, 100.0, max_left_out=0.0)
        assert judged.all()
        # the stage is really exercised: the reference differs from the opaque answer on at least a quarter of the rays
        opaque = _expected(cand, np.zeros_like(modes), cutoffs, 100.0)[2]
        assert np.any(want != opaque, 1).mean() >= 0.25
        # layer by layer: invisible, solid, OPAQUE and cutoff-0 layers behave as named; alpha never goes through the sRGB curve
        layer = np.maximum(cand[0][:, :, 7].view(np.int32), 0)
        live = np.arange(KMAX)[None, :] < cand[1][:, None]
        for k in INVISIBLE:
            assert not admitted[live & (layer == k)].any()
        for k in SOLID:
            assert admitted[live & (layer == k)].all()
        for k in PARTIAL:
            share = admitted[live & (layer == k)].mean()
            assert 0.05 < share < 0.95, (k, share)
    assert r.counters()["traversal_faults"] == 0
    r.close()


def test_srgb_flag_does_not_touch_alpha(stack):
    """The sRGB-flagged noise texture and its linear copy, on the same coordinates, cut the same holes."""
    flat, modes, cutoffs = stack["flat"], stack["modes"], stack["cutoffs"]
    twin = copy.copy(flat)
    twin.texcoords0 = flat.texcoords0.copy()
    twin.texcoords0[44:48] = flat.texcoords0[0:4]  # layer 11 (the linear copy) takes layer 0's coordinates
    ref = Q._renderer(twin, "ploc", 1)
    rays = stack["rays"][False][:10000]  # the perpendicular grid from above
    cand = _candidates(ref, rays)
    layer = np.maximum(cand[0][:, :, 7].view(np.int32), 0)
    live = np.arange(KMAX)[None, :] < cand[1][:, None]
    a0, a11 = cand[2][live & (layer == 0)], cand[2][live & (layer == 11)]
    assert a0.size == a11.size > 5000 and np.array_equal(a0.view(np.uint32), a11.view(np.uint32)) and 0.2 < (a0 >= 0.5).mean() < 0.8
    r = _masked(twin, "ploc", 1, modes, cutoffs)
    _assert_stage(r, rays, cand, modes, cutoffs, 100.0, max_left_out=0.0)
    r.close()
    ref.close()


def test_cutoff_is_compared_exactly(stack):
    """cutoff = the bits of an alpha observed through surface(): that hit is admitted; one ulp more and it is ignored."""
    flat, modes, cutoffs = stack["flat"], stack["modes"], stack["cutoffs"]
    rays = stack["rays"][False][:10000]
    buf, cnt, alpha, _ = (a[:10000] for a in stack["cand"][False])
    first_layer = buf[:, 0, 7].view(np.int32)
    pick = np.nonzero((cnt > 0) & (first_layer == 0) & (alpha[:, 0] > 0.3) & (alpha[:, 0] < 0.7))[0][::97][:24]
    assert pick.size == 24
    for layout in (1, 0):
        r = _masked(flat, "ploc", layout, modes, cutoffs)
        for i in pick:
            a = alpha[i, 0]
            one = rays[i:i + 1].clone()
            for cut, kept in ((a, True), (np.nextafter(a, F(np.inf)), False), (np.nextafter(a, F(-np.inf)), True)):
                r.set_material_alpha(0, [MASK], float(cut))
                assert r.material_alpha()[1][0] == cut
                hit, occ, _, _ = _queries(r, one, 1)
                assert (hit[0, 7] == 0) == kept, (i, a, cut)
                if kept:
                    assert np.array_equal(hit[0], buf[i, 0])
        r.close()


# ---- scene 2: the small atrium, shared walk and lane walk, both stages together -----------------------------------------------------------
def _hash_alpha(h, w, block, salt):
    """A blocky hash pattern: alpha is constant over block x block texels, so the cut-outs have edges and interiors."""
    y, x = np.mgrid[0:h, 0:w]
    v = ((x // block).astype(np.uint64) * np.uint64(73856093)) ^ ((y // block).astype(np.uint64) * np.uint64(19349663)) ^ np.uint64(salt * 83492791)
    v = (v * np.uint64(2654435761)) >> np.uint64(7)
    return (v & np.uint64(255)).astype(np.uint8)


@pytest.fixture(scope="module")
def cutout_atrium():
    """atrium_small with every textured material MASK over copies of its textures whose alpha channel is a hash pattern."""
    import atrium

    flat, info = atrium.build_atrium(20000, seed=4, with_textures=True)
    flat = copy.copy(flat)
    flat.textures = [dict(rgba8=np.ascontiguousarray(t["rgba8"]).copy(), is_srgb=t["is_srgb"]) for t in flat.textures]
    for i, t in enumerate(flat.textures):
        t["rgba8"][:, :, 3] = _hash_alpha(t["rgba8"].shape[0], t["rgba8"].shape[1], 16 << (i % 3), i + 1)
    textured = flat.materials["pbrBaseColorTexture"] >= 0
    modes = textured.astype(np.uint32)
    cutoffs = np.where(np.arange(len(modes)) % 2 == 0, 0.5, 0.25).astype(F)
    assert 8 <= modes.sum() < len(modes)
    # camera rays share one tmin (the shared walk); hostile random rays have per-ray tmin (the lane walk).  The bounds (tmax = 40 and 12)
    # keep the rays that have 16 candidates at all far below the cap of unjudgeable rays (the oracle's peel: see the test's docstring)
    W, H = 200, 100
    co, cd = S._camera_rays(W, H, info)
    ho, hd = Q._hostile_rays(flat, 20000, seed=131)
    tmin = np.random.default_rng(7).uniform(0.001, 0.01, len(ho)).astype(F)
    return dict(flat=flat, info=info, modes=modes, cutoffs=cutoffs, cam=(co, cd, 0.001, 40.0), hostile=(ho, hd, tmin, 12.0))


_ATRIUM_CONFIGS = [("ploc", 1), ("lbvh", 0), ("sah", 1)]


def _atrium_case(A, flat, options, configs, seed=0, dissolve=False, **kw):
    ref = Q._renderer(flat, "ploc", 1, options)
    sets = {}
    for name in ("cam", "hostile"):
        o, d, tmin, tmax = A[name]
        rays = Q._pack(o, d, tmin, tmax)
        sets[name] = (rays, _candidates(ref, rays, seed=seed, dissolve_of=flat.materials if dissolve else None, **kw), tmax)
    ref.close()
    for kind, layout in configs:
        r = _masked(flat, kind, layout, A["modes"], A["cutoffs"], options)
        r.reset_counters()
        for name, (rays, cand, tmax) in sets.items():
            admitted, judged, want = _assert_stage(r, rays, cand, A["modes"], A["cutoffs"], tmax, max_left_out=0.005, seed=seed, **kw)
            opaque = _expected((cand[0], cand[1], cand[2], np.zeros_like(cand[3])), np.zeros_like(A["modes"]), A["cutoffs"], tmax)[2]
            # the stage decides a share of these rays (about a third of the hostile rays hit anything, two thirds of the materials are MASK
            # and cut 25-50 % of their area away: some 5 %, more among the camera rays; a stage that never acted would give 0)
            changed = np.any(want != opaque, 1)[judged].mean()
            print(f"{name}: the stage changes {changed:.4f} of the judged rays")
            assert changed > 0.02, name
        assert r.counters()["traversal_faults"] == 0
        r.close()


def test_atrium_cutouts_shared_walk_and_lane_walk(cutout_atrium):
    """Camera rays (one tmin: the shared walk on the wide layout) and hostile rays (per-ray tmin: the lane walk) equal the reference.
    Unjudgeable rays (16 candidates, none admitted) are capped at 0.5 %.  The oracle's peel (test_gpu_multihit._peel_oracle) of these
    rays finds 16 or more surfaces along 1 of the 20 000 camera rays (tmax = 40; 2.9 surfaces on average) and along 19 of the 20 000
    hostile rays (tmax = 12; with tmax = 40 it would be 56), so at most 0.1 % can be unjudgeable."""
    _atrium_case(cutout_atrium, cutout_atrium["flat"], None, _ATRIUM_CONFIGS)


def test_atrium_cutouts_watertight(cutout_atrium):
    from vkrt_amd import abi

    _atrium_case(cutout_atrium, cutout_atrium["flat"], {abi.VKRT_OPT_WATERTIGHT: 1}, [("ploc", 1), ("lbvh", 0)])


def test_atrium_cutouts_beside_the_dissolve_stage(cutout_atrium):
    """Both stages active: a candidate is ignored if either says so.  Two materials get factor.a = 0.5: a MASK one over a texture (both
    stages judge its triangles) and an untextured opaque one (the dissolve stage alone)."""
    from vkrt_amd import abi

    A = cutout_atrium
    flat = copy.copy(A["flat"])
    flat.materials = A["flat"].materials.copy()
    masked, plain = np.nonzero(A["modes"] == MASK)[0], np.nonzero(A["modes"] == 0)[0]
    flat.materials["pbrBaseColorFactor"][masked[1], 3] = 0.5
    flat.materials["pbrBaseColorFactor"][plain[0], 3] = 0.5
    for seed in (0, 4242):
        _atrium_case(A, flat, {abi.VKRT_OPT_ANYHIT_DISSOLVE: 1}, [("ploc", 1), ("lbvh", 0)], seed=seed, dissolve=True)


def test_atrium_cutouts_after_the_cull_mask_and_facing_filter(cutout_atrium):
    """A cull mask and VKRT_RAY_CULL_BACK_FACING: the filtered candidate list comes first, the alpha rule acts on it."""
    A = cutout_atrium
    flat = A["flat"]
    masks = (np.arange(len(flat.nodes)) % 3 + 1).astype(np.uint8)
    ref = Q._renderer(flat, "ploc", 1)
    ref.set_instance_visibility(0, masks, np.zeros(len(masks), np.uint8))
    o, d, tmin, tmax = A["hostile"]
    rays = Q._pack(o, d, tmin, tmax)
    kw = dict(cull_mask=0x1, ray_flags=BACK)
    cand = _candidates(ref, rays, **kw)
    unfiltered = _candidates(ref, rays)
    assert cand[1].sum() < 0.6 * unfiltered[1].sum()  # the filter does remove candidates
    ref.close()
    for kind, layout in (("ploc", 1), ("sah", 0)):
        r = _masked(flat, kind, layout, A["modes"], A["cutoffs"])
        r.set_instance_visibility(0, masks, np.zeros(len(masks), np.uint8))
        _assert_stage(r, rays, cand, A["modes"], A["cutoffs"], tmax, max_left_out=0.005, **kw)
        r.close()


# ---- 3. VKRT_RAY_OPAQUE and the untouched paths -----------------------------------------------------------------------------------------
def test_opaque_flag_and_the_other_entry_points_ignore_the_modes(cutout_atrium):
    import torch
    from vkrt_amd.flat_scene import make_push_constants

    A = cutout_atrium
    flat, info = A["flat"], A["info"]
    o, d, tmin, tmax = A["hostile"]
    rays = Q._pack(o, d, tmin, tmax)
    W, H = 64, 36
    cam = S._camera(W, H, info)[0]
    pc = make_push_constants(samples=1, depth=3, frame=0, lights_count=len(flat.lights))
    pts = torch.as_tensor(o[:5000], device="cuda:0")

    def untouched(r):
        cp = r.closest_point(pts, radius=3.0)
        hits = r.intersect(rays, ray_flags=OPAQUE_FLAG)
        surf = r.surface(hits)
        img = r.pathtrace(pc, cam, W, H, seed=3)
        gb = r.gbuffer_raycast(cam, W, H)
        _sync()
        tr = r.trace_rays(o[:5000], d[:5000], 0.001, 12.0)
        return dict(closest_point=cp.buffer.cpu().numpy().view(np.uint32).copy(), surface=surf.buffer.cpu().numpy().view(np.uint32).copy(),
                    pathtrace=hashlib.sha256(img.cpu().numpy().tobytes()).hexdigest(),
                    gbuffer=hashlib.sha256(b"".join(gb[k].cpu().numpy().tobytes() for k in sorted(gb))).hexdigest(),
                    trace_rays=[np.asarray(a).copy() for a in tr])

    for kind, layout in (("ploc", 1), ("lbvh", 0)):
        plain = Q._renderer(flat, kind, layout)
        want_q = _queries(plain, rays, 4)
        want_u = untouched(plain)
        plain.close()
        r = _masked(flat, kind, layout, A["modes"], A["cutoffs"])
        r.reset_counters()
        got_q = _queries(r, rays, 4, ray_flags=OPAQUE_FLAG)
        for a, b in zip(got_q, want_q):
            assert np.array_equal(a, b)
        assert not np.array_equal(_queries(r, rays, 4)[0], want_q[0])  # (without the flag the modes do act)
        got_u = untouched(r)
        for key in ("closest_point", "surface"):
            assert np.array_equal(got_u[key], want_u[key]), key
        assert got_u["pathtrace"] == want_u["pathtrace"] and got_u["gbuffer"] == want_u["gbuffer"]
        for a, b in zip(got_u["trace_rays"], want_u["trace_rays"]):
            assert np.array_equal(a.view(np.uint32) if a.dtype == F else a, b.view(np.uint32) if b.dtype == F else b)
        assert r.counters()["traversal_faults"] == 0
        r.close()


# ---- 4. liveness ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 0])
def test_modes_are_live_stream_ordered_and_survive_refit_and_build(stack, layout):
    import torch
    from vkrt_amd import abi
    from vkrt_amd.renderer import VkrtError

    flat, modes, cutoffs = stack["flat"], stack["modes"], stack["cutoffs"]
    rays, cand = stack["rays"][False], stack["cand"][False]
    want = _expected(cand, modes, cutoffs, 100.0)[2]
    opaque = _expected(cand, np.zeros_like(modes), cutoffs, 100.0)[2]
    r = Q._renderer(flat, "ploc", layout)
    # every material starts as {OPAQUE, 0.5}; a range outside the scene's materials is refused and changes nothing
    m0, c0 = r.material_alpha()
    assert not m0.any() and np.all(c0 == F(0.5))
    arr = (abi.MaterialAlpha * 2)(abi.MaterialAlpha(1, 0.25), abi.MaterialAlpha(1, 0.25))
    assert r.lib.vkrt_scene_set_material_alpha(r._h, len(modes) - 1, 2, arr, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert r.lib.vkrt_scene_get_material_alpha(r._h, len(modes), 1, arr) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert r.lib.vkrt_scene_set_material_alpha(r._h, len(modes), 0, None, None) == abi.VKRT_OK
    with pytest.raises(VkrtError):
        r.set_material_alpha(len(modes), [1])
    assert not r.material_alpha()[0].any()
    # on the caller's stream between two queries: the second sees the modes, the first does not
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        first = r.intersect(rays, stream=s)
        r.set_material_alpha(0, modes, cutoffs, stream=s)
        second = r.intersect(rays, stream=s)
    s.synchronize()
    assert np.array_equal(first.buffer.cpu().numpy().view(np.uint32), opaque)
    assert np.array_equal(second.buffer.cpu().numpy().view(np.uint32), want)
    # a node move + refit, then a fresh build: the modes stay (the moved scene's own reference)
    mflat, mats = moved(flat, [1, 4, 9], seed=5, mirror_first=False, scale=False)
    apply(r, mats)
    r.refit()
    ref = Q._renderer(mflat, "ploc", 1)
    mcand = _candidates(ref, rays)
    ref.close()
    _assert_stage(r, rays, mcand, modes, cutoffs, 100.0, max_left_out=0.0)
    r.build("lbvh")
    _assert_stage(r, rays, mcand, modes, cutoffs, 100.0, max_left_out=0.0)
    assert np.array_equal(r.material_alpha()[0], modes)
    # texture coordinates alone: no refit, the tree is not stale, the next query reads the shifted coordinates
    shifted = (mflat.texcoords0 + F([0.37, -0.21])).astype(F)
    r.update_vertices(0, texcoords0=shifted)
    sflat = copy.copy(mflat)
    sflat.texcoords0 = shifted
    ref = Q._renderer(sflat, "ploc", 1)
    scand = _candidates(ref, rays)
    ref.close()
    _, _, swant = _assert_stage(r, rays, scand, modes, cutoffs, 100.0, max_left_out=0.0)
    assert np.any(swant != _expected(mcand, modes, cutoffs, 100.0)[2], 1).mean() > 0.1  # (the shift did move the holes)
    # back to OPAQUE: the opaque answers bit for bit
    r.set_material_alpha(0, np.zeros_like(modes), cutoffs)
    plain = _expected(scand, np.zeros_like(modes), cutoffs, 100.0)
    hit, occ, _, _ = _queries(r, rays, 1)
    assert np.array_equal(hit, plain[2]) and np.array_equal(occ, plain[3])
    assert r.counters()["traversal_faults"] == 0
    r.close()


# ---- 5. one digest ----------------------------------------------------------------------------------------------------------------------
def test_one_digest_over_builders_layouts_split_and_sharing(stack):
    from vkrt_amd import abi

    flat, modes, cutoffs = stack["flat"], stack["modes"], stack["cutoffs"]
    digests = set()
    for kind in Q.KINDS:
        for layout in (1, 0):
            for budget in (0, 30):
                for share in (0, 16):
                    r = _masked(flat, kind, layout, modes, cutoffs, {abi.VKRT_OPT_SPLIT_BUDGET: budget, abi.VKRT_OPT_WF_SHARE: share})
                    h = hashlib.sha256()
                    for lane in (False, True):
                        for part in _queries(r, stack["rays"][lane], 4):
                            h.update(np.ascontiguousarray(part).tobytes())
                    digests.add(h.hexdigest())
                    r.close()
    assert len(digests) == 1
