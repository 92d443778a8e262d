"""VKRT_OPT_ALPHA_TEST: the frame entry points (vkrt_pathtrace*, vkrt_gbuffer_raycast*, vkrt_hybrid_trace*) run the alpha test of
VKRT_ALPHA_MASK materials on every ray they trace (include/vkrt.h "alpha-tested materials").

Every comparison is bit for bit on uint32 views.  Two references:
  * whole cut-outs: a triangle whose material admits nothing is, for every ray, a triangle that is not there, so the CPU oracle -- which
    knows no alpha mode -- renders the expected image from the same scene with the invisible instances' nodes given an all-zero matrix
    (a zero scale hides an instance and keeps every flattened triangle id, so the dissolve stage's tea(id, seed) draws stay the same);
  * texel-resolved cut-outs: the integrator of tests/test_gpu_hit_surface.py, whose rays are vkrt_intersect / vkrt_occluded -- they
    already run the stage -- and whose hits are shaded by the oracle's shadeSurface."""
import copy
import hashlib
import os
import sys

import numpy as np
import pytest

import test_gpu_alpha_cutout as A
import test_gpu_hit_surface as S
import test_gpu_ray_query as Q
from scene_motion import apply, moved
from test_gpu_alpha_cutout import cutout_atrium  # noqa: F401  (the fixture, instantiated once for this module)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

F = np.float32
MASK = 1
COUNTERS = ("rays_closest", "rays_shadow", "hits", "diffuse_hits", "pixels")
RAY_COUNTERS = ("rays_closest", "rays_shadow", "pixels")  # what the wavefront pipeline counts without VKRT_TRACE_COUNT_TRAVERSAL


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _np(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _opts(extra=None, alpha=1):
    from vkrt_amd import abi

    o = {abi.VKRT_OPT_ALPHA_TEST: alpha}
    o.update(extra or {})
    return o


def _renderer(flat, kind, layout, modes, cutoffs, options=None, alpha=1):
    r = Q._renderer(flat, kind, layout, _opts(options, alpha))
    if modes is not None:
        r.set_material_alpha(0, modes, cutoffs)
    return r


def _zero_scaled(flat, nodes):
    out = copy.copy(flat)
    out.nodes = flat.nodes.copy()
    for i in nodes:
        out.nodes[i]["worldMatrix"] = 0.0
    return out


def _changed(a, b):
    return float(np.any(_u32(a) != _u32(b), axis=-1).mean())


def _assert_same(got, want, what):
    bad = np.argwhere(np.any(_u32(got).reshape(want.shape[0], want.shape[1], -1) != _u32(want).reshape(want.shape[0], want.shape[1], -1), axis=-1))
    print(f"{what}: {len(bad)} of {want.shape[0] * want.shape[1]} pixels differ")
    assert len(bad) == 0, (what, bad[:5])


# ---- test 1: whole cut-outs of the layer stack against the oracle ---------------------------------------------------------------------
STACK_CAMERA = {"camera": dict(eye=(0.7, 0.5, 2.2), center=(0.0, 0.0, -0.5), up=(0.0, 1.0, 0.0), fov=60.0)}
STACK_WH = (64, 36)
DISSOLVING_LAYER = 6  # the solid OPAQUE layer that gets factor alpha 0.5 for the runs with VKRT_OPT_ANYHIT_DISSOLVE


def _whole_cutout_stack(dissolve):
    """The layer stack with the two wholly invisible layers (2 and 3) moved above layer 0, the PARTIAL layers OPAQUE.  The solid OPAQUE
    layer 6 sits between them and layer 0, so that with dissolve -- its factor alpha is 0.5 then -- the camera's rays meet both stages."""
    flat, modes, cutoffs = A._layer_stack()
    flat = copy.copy(flat)
    flat.positions = np.array(flat.positions, F)
    flat.materials = flat.materials.copy()
    for k, z in zip(A.INVISIBLE, (0.2, 0.1)):
        flat.positions[4 * k:4 * k + 4, 2] = F(z)
    flat.positions[4 * DISSOLVING_LAYER:4 * DISSOLVING_LAYER + 4, 2] = F(0.05)
    modes = modes.copy()
    modes[list(A.PARTIAL)] = 0
    if dissolve:
        assert modes[DISSOLVING_LAYER] == 0 and DISSOLVING_LAYER in A.SOLID
        flat.materials["pbrBaseColorFactor"][DISSOLVING_LAYER, 3] = 0.5
    return flat, modes, cutoffs


@pytest.fixture(scope="module")
def stack_reference():
    """The oracle's images and counters of the stack with the invisible layers zero-scaled, per (watertight, dissolve, frame), made once."""
    import oracle_py
    from vkrt_amd.flat_scene import make_push_constants

    W, H = STACK_WH
    cam = S._camera(W, H, STACK_CAMERA)[0]
    old = np.random.default_rng(5).random((H, W, 4)).astype(F)
    cache = {}

    def get(wt, dissolve, frame):
        key = (wt, dissolve, frame)
        if key not in cache:
            flat, modes, cutoffs = _whole_cutout_stack(dissolve)
            orc = oracle_py.OracleScene(_zero_scaled(flat, A.INVISIBLE))
            orc.set_watertight(wt)
            orc.set_dissolve(dissolve)
            pc = make_push_constants(samples=2, depth=4, frame=frame, lights_count=len(flat.lights))
            cache[key] = (flat, modes, cutoffs, pc) + orc.render(pc, cam, W, H, seed=21, image=old.copy())
        return cache[key]

    return dict(get=get, cam=cam, old=old)


@pytest.mark.parametrize("kind,layout", A.CONFIGS)
def test_whole_cutouts_of_the_layer_stack_equal_the_oracle(stack_reference, kind, layout):
    import torch
    from vkrt_amd import abi

    W, H = STACK_WH
    cam, old = stack_reference["cam"], stack_reference["old"]
    for wt in (0, 1):
        for dissolve in (0, 1):
            flat, modes, cutoffs = _whole_cutout_stack(dissolve)
            r = _renderer(flat, kind, layout, modes, cutoffs, {abi.VKRT_OPT_WATERTIGHT: wt, abi.VKRT_OPT_ANYHIT_DISSOLVE: dissolve})
            for frame in (0, 3):
                _, _, _, pc, want, cnt = stack_reference["get"](wt, dissolve, frame)
                r.set_option(abi.VKRT_OPT_ALPHA_TEST, 1)
                # the plain launch counts rays and pixels; the instrumented one (other kernels) every tally
                for flags, names in ((0, RAY_COUNTERS), (abi.VKRT_TRACE_COUNT_TRAVERSAL, COUNTERS)):
                    r.reset_counters()
                    got = _np(r.pathtrace(pc, cam, W, H, seed=21, flags=flags, image=torch.as_tensor(old.copy(), device="cuda:0")))
                    c = r.counters()
                    _assert_same(got, want, f"{kind} layout {layout} watertight {wt} dissolve {dissolve} frame {frame} flags {flags}")
                    assert {k: c[k] for k in names} == {k: cnt[k] for k in names}
                r.set_option(abi.VKRT_OPT_ALPHA_TEST, 0)
                off = _np(r.pathtrace(pc, cam, W, H, seed=21, image=torch.as_tensor(old.copy(), device="cuda:0")))
                share = _changed(got, off)
                print(f"  the option changes {share:.3f} of the pixels")
                assert share > 0.02
            assert r.counters()["traversal_faults"] == 0
            r.close()


# ---- test 2: texture-driven whole cut-outs (the shutters), all three frame modes -----------------------------------------------------
SHUTTER_GRID = 8     # 8 x 8 quads
TEXTURE_SIDE, BLOCK = 64, 8
SHUTTER_CAMERA = {"camera": dict(eye=(0.4, 0.3, 4.0), center=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=45.0)}
SHUTTER_WH = (64, 36)


def _shutter_scene():
    """A floor and a back wall (one opaque material) and, in front of them, 8 x 8 small quads, each a node and primitive-mesh of its own,
    all of one MASK material whose base-colour texture has alpha 0 or 255 in 8 x 8-texel blocks.  Quad (i, j) takes its coordinates from
    inside block (i, j), at least 2 texels from the block's border, shifted by whole turns (negative and > 1: REPEAT).
    Returns (flat, modes, cutoffs, invisible bool [64] by node order, first shutter node)."""
    from vkrt_amd.flat_scene import LIGHT_DTYPE, MAT_DTYPE, NODE_DTYPE, PRIM_DTYPE, FlatScene

    rng = np.random.default_rng(41)
    G, T, Bk = SHUTTER_GRID, TEXTURE_SIDE, BLOCK
    block_alpha = np.where(rng.random((G, G)) < 0.5, 0, 255).astype(np.uint8)  # [row j (v), column i (u)]
    tex = rng.integers(0, 256, (T, T, 4), dtype=np.uint8)
    tex[:, :, 3] = np.kron(block_alpha, np.ones((Bk, Bk), np.uint8))
    pos, uv, idx, pm, nodes = [], [], [], [], []
    # floor (y = -1.2) and back wall (z = -1.5)
    pos += [[-4, -1.2, -1.5], [4, -1.2, -1.5], [4, -1.2, 3], [-4, -1.2, 3], [-4, -1.2, -1.5], [4, -1.2, -1.5], [4, 3, -1.5], [-4, 3, -1.5]]
    uv += [[0, 0], [1, 0], [1, 1], [0, 1]] * 2
    idx += [0, 2, 1, 0, 3, 2, 0, 1, 2, 0, 2, 3]
    pm += [(0, 6, 0, 4, 0), (6, 6, 4, 4, 0)]
    nodes += [0, 1]
    nrm = [[0, 1, 0]] * 4 + [[0, 0, 1]] * 4
    invisible = []
    for j in range(G):
        for i in range(G):
            k = j * G + i
            x0, y0 = -1.6 + 0.4 * i, -0.9 + 0.225 * j
            v0 = len(pos)
            pos += [[x0, y0, 0], [x0 + 0.36, y0, 0], [x0 + 0.36, y0 + 0.2, 0], [x0, y0 + 0.2, 0]]
            nrm += [[0, 0, 1]] * 4
            turn_u, turn_v = (k % 5) - 2, ((k // 5) % 4) - 1  # whole turns: -2 .. 2 and -1 .. 2
            lo_u, hi_u = (Bk * i + 2 + (k % 3) * 0.5) / T + turn_u, (Bk * i + 6 - (k % 2) * 0.5) / T + turn_u
            lo_v, hi_v = (Bk * j + 2 + (k % 2) * 0.75) / T + turn_v, (Bk * j + 6 - (k % 3) * 0.25) / T + turn_v
            uv += [[lo_u, lo_v], [hi_u, lo_v], [hi_u, hi_v], [lo_u, hi_v]]
            i0 = len(idx)
            idx += [0, 1, 2, 0, 2, 3]
            pm.append((i0, 6, v0, 4, 1))
            nodes.append(len(pm) - 1)
            invisible.append(block_alpha[j, i] == 0)
    n = len(pos)
    pms = np.zeros(len(pm), PRIM_DTYPE)
    for k, p in enumerate(pm):
        pms[k] = p
    nd = np.zeros(len(nodes), NODE_DTYPE)
    for k, m in enumerate(nodes):
        nd[k] = (np.eye(4, dtype=F).reshape(-1), m)
    mats = np.zeros(2, MAT_DTYPE)
    for k, (col, t) in enumerate((((0.7, 0.7, 0.75, 1.0), -1), ((0.9, 0.8, 0.5, 1.0), 0))):
        mats[k]["pbrBaseColorFactor"] = col
        mats[k]["metallicFactor"], mats[k]["roughnessFactor"] = 0.0, 0.7
        for name in ("metallicRoughnessTexture", "normalTexture", "emissiveTexture"):
            mats[k][name] = -1
        mats[k]["pbrBaseColorTexture"] = t
    lights = np.zeros(2, LIGHT_DTYPE)
    lights[0] = ((0.5, 1.5, 3.5), (1, 1, 1), 30.0, 0)
    lights[1] = ((-1.0, 0.5, 2.5), (1, 0.9, 0.8), 15.0, 0)
    flat = FlatScene(np.array(pos, F), np.array(nrm, F), np.tile(F([1, 0, 0, 1]), (n, 1)), np.array(uv, F), np.array(idx, np.uint32), pms, mats, lights, nd,
                     [dict(rgba8=tex, is_srgb=True)])
    return flat, np.array([0, MASK], np.uint32), np.array([0.5, 0.5], F), np.array(invisible), 2


def _footprint_is_one_block(flat, first):
    """numpy: the bilinear LOD-0 REPEAT footprint of every point of every shutter stays inside one alpha block, 2 texels from its border"""
    T, Bk = TEXTURE_SIDE, BLOCK
    alpha = flat.textures[0]["rgba8"][:, :, 3]
    out = []
    for k in range(SHUTTER_GRID ** 2):
        q = flat.texcoords0[8 + 4 * k:8 + 4 * k + 4].astype(np.float64) * T  # texel units (a quad's coordinates are bilinear in its corners)
        lo, hi = q.min(0), q.max(0)
        assert np.all(np.floor(lo / Bk) == np.floor((hi - 1e-9) / Bk)), k                          # one block ...
        assert np.all(lo - np.floor(lo / Bk) * Bk >= 2.0) and np.all(np.ceil(hi / Bk) * Bk - hi >= 2.0), k  # ... 2 texels inside it
        xs = np.arange(int(np.floor(lo[0] - 0.5)), int(np.floor(hi[0] - 0.5)) + 2) % T
        ys = np.arange(int(np.floor(lo[1] - 0.5)), int(np.floor(hi[1] - 0.5)) + 2) % T
        vals = np.unique(alpha[np.ix_(ys, xs)])
        assert vals.size == 1 and vals[0] in (0, 255), k
        out.append(vals[0] == 0)
    uvs = flat.texcoords0[8:]
    assert (uvs < 0).any() and (uvs > 1).any()  # REPEAT on both sides
    return np.array(out)


def _view_matrix(c):
    import camera_np

    return np.asarray(camera_np.look_at(c["eye"], c["center"], c["up"]), F).T.reshape(-1).copy()


@pytest.fixture(scope="module")
def shutters():
    import oracle_py
    from vkrt_amd.flat_scene import make_push_constants

    flat, modes, cutoffs, invisible, first = _shutter_scene()
    assert np.array_equal(_footprint_is_one_block(flat, first), invisible)
    assert 0.25 <= invisible.mean() <= 0.75, invisible.mean()
    W, H = SHUTTER_WH
    cam, vi, pi = S._camera(W, H, SHUTTER_CAMERA)
    vm = _view_matrix(SHUTTER_CAMERA["camera"])
    L = len(flat.lights)
    orc = oracle_py.OracleScene(_zero_scaled(flat, first + np.nonzero(invisible)[0]))
    pc = make_push_constants(samples=2, depth=4, frame=0, lights_count=L)
    image, cnt = orc.render(pc, cam, W, H, seed=13)
    g = orc.gbuffer_nrd(cam, vm, W, H, lights_count=L)
    hpc = make_push_constants(samples=1, depth=4, frame=0, lights_count=L)
    hpc.useShadows, hpc.useAO, hpc.useGI = 1, 1, 1
    return dict(flat=flat, modes=modes, cutoffs=cutoffs, invisible=invisible, first=first, cam=cam, vm=vm, pc=pc, hpc=hpc, image=image, cnt=cnt, g=g, orc=orc)


def test_shutter_alpha_is_the_blocks_constant(shutters):
    """surface() at random points of every shutter: an invisible one has alpha exactly 0; a visible one 1 up to the rounding of the
    blend of four equal texels ((1 - a) + a and the two products: within 2 ulp of 1), far above the cutoff."""
    flat, inv, first = shutters["flat"], shutters["invisible"], shutters["first"]
    rng = np.random.default_rng(3)
    n_each = 40
    o, d, owner = [], [], []
    for k in range(SHUTTER_GRID ** 2):
        p = flat.positions[8 + 4 * k:8 + 4 * k + 4]
        s, t = rng.uniform(0.02, 0.98, n_each), rng.uniform(0.02, 0.98, n_each)
        pts = p[0] + np.outer(s, p[1] - p[0]) + np.outer(t, p[3] - p[0])
        o.append(pts + F([0, 0, 1.0]))
        d.append(np.tile(F([0, 0, -1]), (n_each, 1)))
        owner += [k] * n_each
    r = Q._renderer(flat, "ploc", 1)
    hits = r.intersect(Q._pack(np.concatenate(o).astype(F), np.concatenate(d), 0.001, 10.0), ray_flags=A.OPAQUE_FLAG)
    surf = r.surface(hits)
    inst = _np(hits.buffer).view(np.int32)[:, 3]
    alpha = _np(surf.alpha).reshape(-1)
    owner = np.array(owner)
    assert np.array_equal(inst, owner + first)
    assert np.all(alpha[inv[owner]] == 0.0)
    assert np.all(np.abs(alpha[~inv[owner]] - 1.0) <= 2.0 ** -22)
    assert r.counters()["traversal_faults"] == 0
    r.close()


@pytest.mark.parametrize("layout", [1, 0])
def test_shutters_in_pathtrace_gbuffer_and_hybrid_equal_the_oracle(shutters, layout):
    from vkrt_amd import abi

    Sh = shutters
    flat, W, H = Sh["flat"], SHUTTER_WH[0], SHUTTER_WH[1]
    cam, L = Sh["cam"], len(Sh["flat"].lights)
    r = _renderer(flat, "ploc", layout, Sh["modes"], Sh["cutoffs"])
    for flags, names in ((0, RAY_COUNTERS), (abi.VKRT_TRACE_COUNT_TRAVERSAL, COUNTERS)):
        r.reset_counters()
        got = _np(r.pathtrace(Sh["pc"], cam, W, H, seed=13, flags=flags))
        c = r.counters()
        _assert_same(got, Sh["image"], f"pathtrace layout {layout} flags {flags}")
        assert {k: c[k] for k in names} == {k: Sh["cnt"][k] for k in names}
    # the primary hits of the opaque scene: which pixels see an invisible shutter first
    co, cd = S._camera_rays(W, H, SHUTTER_CAMERA)
    inst = _np(r.intersect(Q._pack(co, cd, 0.001, 10000.0), ray_flags=A.OPAQUE_FLAG).buffer).view(np.int32)[:, 3].reshape(H, W)
    through = (inst >= Sh["first"]) & Sh["invisible"][np.clip(inst - Sh["first"], 0, len(Sh["invisible"]) - 1)]
    assert through.mean() > 0.05
    g_plain = r.gbuffer_raycast(cam, W, H, lights_count=L)
    g_nrd = r.gbuffer_raycast(cam, W, H, lights_count=L, view_matrix=Sh["vm"])
    for k in ("color", "position", "normal", "roughMetal"):
        _assert_same(_np(g_plain[k]), Sh["g"][k], f"gbuffer {k} layout {layout}")
        _assert_same(_np(g_nrd[k]), Sh["g"][k], f"gbuffer_nrd {k} layout {layout}")
    for k in ("nrdNormalRoughness", "nrdViewZ"):
        want = Sh["g"][k] if Sh["g"][k].ndim == 3 else Sh["g"][k][..., None]
        _assert_same(_np(g_nrd[k]).reshape(want.shape), want, f"gbuffer_nrd {k} layout {layout}")
    assert not _np(g_nrd["nrdRadianceHitDist"]).any()
    r.set_option(abi.VKRT_OPT_ALPHA_TEST, 0)
    g_off = r.gbuffer_raycast(cam, W, H, lights_count=L)
    moved_px = np.any(_u32(_np(g_off["position"])) != _u32(_np(g_plain["position"])), axis=-1)
    assert np.all(moved_px[through])
    r.set_option(abi.VKRT_OPT_ALPHA_TEST, 1)
    gnp = {k: _np(v) for k, v in g_nrd.items()}
    want, cnt = Sh["orc"].hybrid(Sh["hpc"], cam, W, H, gnp, seed=17)
    want_nrd, rad = Sh["orc"].hybrid_nrd(Sh["hpc"], cam, W, H, gnp, seed=17)
    r.reset_counters()
    acc = _np(r.hybrid_trace(Sh["hpc"], cam, W, H, g_plain, seed=17))
    c = r.counters()
    _assert_same(acc, want, f"hybrid layout {layout}")
    print(f"hybrid rays: closest {c['rays_closest']} (oracle {cnt['rays_closest']}), shadow {c['rays_shadow']} (oracle {cnt['rays_shadow']})")
    assert (c["rays_closest"], c["rays_shadow"], c["pixels"]) == (cnt["rays_closest"], cnt["rays_shadow"], cnt["pixels"])
    acc_nrd = _np(r.hybrid_trace(Sh["hpc"], cam, W, H, g_nrd, seed=17))
    _assert_same(acc_nrd, want_nrd, f"hybrid_nrd layout {layout}")
    _assert_same(_np(g_nrd["nrdRadianceHitDist"]), rad, f"hybrid_nrd radiance / hit distance layout {layout}")
    # the option does act in the hybrid pass: on the option-on G-buffer, the accumulation with the stage off differs
    r.set_option(abi.VKRT_OPT_ALPHA_TEST, 0)
    assert _changed(_np(r.hybrid_trace(Sh["hpc"], cam, W, H, g_plain, seed=17)), acc) > 0.02
    assert r.counters()["traversal_faults"] == 0
    r.close()


# ---- test 3: texel-resolved cut-outs against the query integrator ---------------------------------------------------------------------
ATRIUM_WH = (64, 36)
ATRIUM_CASES = [(0, 1, 4), (3, 2, 6)]  # (frame, samples, depth)


def _atrium_frame(r, A_, frame, samples, depth, seed=11, **kw):
    import torch
    from vkrt_amd.flat_scene import make_push_constants

    W, H = ATRIUM_WH
    cam = S._camera(W, H, A_["info"])[0]
    pc = make_push_constants(samples=samples, depth=depth, frame=frame, lights_count=len(A_["flat"].lights))
    old = np.random.default_rng(3).random((H, W, 4)).astype(F)
    return _np(r.pathtrace(pc, cam, W, H, seed=seed, image=torch.as_tensor(old.copy(), device="cuda:0"), **kw))


def _integrator_image(r, flat, info, W, H, frame, samples, depth, monkeypatch, seed=11):
    import np_pathtrace as P
    from vkrt_amd.flat_scene import make_push_constants

    _, vi, pi = S._camera(W, H, info)
    pc = make_push_constants(samples=samples, depth=depth, frame=frame, lights_count=len(flat.lights))
    old = np.random.default_rng(3).random((H, W, 4)).astype(F)
    sc = S._query_pathtracer(r, flat, monkeypatch)
    ys, xs = np.mgrid[0:H, 0:W]
    got = P.pathtrace_pixels(sc, pc, vi, pi, W, H, seed, xs.ravel(), ys.ravel(), old=old.reshape(-1, 4)).reshape(H, W, 4)
    return got, sc


@pytest.mark.parametrize("frame,samples,depth", ATRIUM_CASES)
def test_atrium_cutouts_equal_the_query_integrator(cutout_atrium, monkeypatch, frame, samples, depth):  # noqa: F811
    from vkrt_amd import abi

    A_ = cutout_atrium
    W, H = ATRIUM_WH
    r = _renderer(A_["flat"], "ploc", 1, A_["modes"], A_["cutoffs"])
    r.reset_counters()
    own = _atrium_frame(r, A_, frame, samples, depth)
    c = r.counters()
    want, sc = _integrator_image(r, A_["flat"], A_["info"], W, H, frame, samples, depth, monkeypatch)
    print(f"frame {frame} spp {samples} depth {depth}: closest rays {c['rays_closest']} (integrator {sc.rays_closest}), shadow rays {c['rays_shadow']} "
          f"(integrator {sc.rays_shadow})")
    _assert_same(own, want, "pathtrace against the query integrator")
    assert (c["rays_closest"], c["rays_shadow"]) == (sc.rays_closest, sc.rays_shadow)
    r.set_option(abi.VKRT_OPT_ALPHA_TEST, 0)
    share = _changed(own, _atrium_frame(r, A_, frame, samples, depth))
    print(f"  the option changes {share:.3f} of the pixels")
    assert share > 0.02
    assert r.counters()["traversal_faults"] == 0
    r.close()


def test_full_layer_stack_equals_the_query_integrator(monkeypatch):
    """All twelve layers with their own modes: partial cut-outs over the 64 x 64 noise, the 5 x 3 texture and the factor-only materials."""
    import torch
    from vkrt_amd.flat_scene import make_push_constants

    flat, modes, cutoffs = A._layer_stack()
    W, H = STACK_WH
    cam = S._camera(W, H, STACK_CAMERA)[0]
    for layout in (1, 0):
        r = _renderer(flat, "lbvh", layout, modes, cutoffs)
        pc = make_push_constants(samples=1, depth=4, frame=0, lights_count=len(flat.lights))
        old = np.random.default_rng(3).random((H, W, 4)).astype(F)
        r.reset_counters()
        own = _np(r.pathtrace(pc, cam, W, H, seed=11, image=torch.as_tensor(old.copy(), device="cuda:0")))
        c = r.counters()
        want, sc = _integrator_image(r, flat, STACK_CAMERA, W, H, 0, 1, 4, monkeypatch)
        _assert_same(own, want, f"layer stack layout {layout}")
        assert (c["rays_closest"], c["rays_shadow"]) == (sc.rays_closest, sc.rays_shadow)
        assert r.counters()["traversal_faults"] == 0
        r.close()


# ---- test 4: one digest over every schedule -------------------------------------------------------------------------------------------
DIGEST_CASE = (3, 2, 6)  # (frame, samples, depth) of the test-3 atrium image


def _digest(img):
    return hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def atrium_digest(cutout_atrium):  # noqa: F811
    """the digest of the default configuration (ploc, wide8), which test 3 compares with the query integrator"""
    A_ = cutout_atrium
    r = _renderer(A_["flat"], "ploc", 1, A_["modes"], A_["cutoffs"])
    out = _digest(_atrium_frame(r, A_, *DIGEST_CASE))
    r.close()
    return out


def _schedules():
    from vkrt_amd import abi

    out = [(f"{kind}-layout{layout}", kind, layout, {}, 0) for kind in Q.KINDS for layout in (1, 0)]
    for name, option, values in (("split", abi.VKRT_OPT_SPLIT_BUDGET, (0, 30)), ("share", abi.VKRT_OPT_WF_SHARE, (0, 16)),
                                 ("threshold", abi.VKRT_OPT_TRI_THRESHOLD, (0, 32)), ("lend", abi.VKRT_OPT_WF_TRI_LEND, (0, 1)),
                                 ("sample-sync", abi.VKRT_OPT_WF_SAMPLE_SYNC, (0, 1)), ("camera-rounds", abi.VKRT_OPT_WF_CAMERA_ROUNDS, (0, 1)),
                                 ("subframes", abi.VKRT_OPT_WF_SUBFRAMES, (1, 3))):
        out += [(f"{name}{v}", "ploc", 1, {option: v}, 0) for v in values]
    out.append(("megakernel", "ploc", 1, {abi.VKRT_OPT_MODE: 0}, 0))
    out.append(("count", "ploc", 1, {}, abi.VKRT_TRACE_COUNT_TRAVERSAL))
    out.append(("count-bvh2", "ploc", 0, {}, abi.VKRT_TRACE_COUNT_TRAVERSAL))
    out.append(("count-megakernel", "ploc", 1, {abi.VKRT_OPT_MODE: 0}, abi.VKRT_TRACE_COUNT_TRAVERSAL))
    out.append(("watertight-lend", "ploc", 1, {abi.VKRT_OPT_WATERTIGHT: 1, abi.VKRT_OPT_WF_TRI_LEND: 1}, -1))  # compared with lend 0 below
    return out


@pytest.mark.parametrize("name,kind,layout,options,flags", _schedules(), ids=[c[0] for c in _schedules()])
def test_one_digest_over_builders_layouts_and_schedules(cutout_atrium, atrium_digest, name, kind, layout, options, flags):  # noqa: F811
    from vkrt_amd import abi

    A_ = cutout_atrium
    r = _renderer(A_["flat"], kind, layout, A_["modes"], A_["cutoffs"], options)
    got = _digest(_atrium_frame(r, A_, *DIGEST_CASE, flags=max(flags, 0)))
    assert r.counters()["traversal_faults"] == 0
    r.close()
    if flags >= 0:
        assert got == atrium_digest
    else:  # the watertight image is another image: lending must not change it (alpha + watertight keeps VKRT_OPT_WF_TRI_LEND effective)
        r = _renderer(A_["flat"], kind, layout, A_["modes"], A_["cutoffs"], {**options, abi.VKRT_OPT_WF_TRI_LEND: 0})
        assert got == _digest(_atrium_frame(r, A_, *DIGEST_CASE))
        r.close()


def test_shards_and_frames_in_flight_render_the_same_image(cutout_atrium, atrium_digest):  # noqa: F811
    import torch
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.sharding import shard_row_indices

    A_ = cutout_atrium
    flat, modes, cutoffs = A_["flat"], A_["modes"], A_["cutoffs"]
    W, H = ATRIUM_WH
    frame, samples, depth = DIGEST_CASE
    cam = S._camera(W, H, A_["info"])[0]
    # two shards against one
    pc = make_push_constants(samples=samples, depth=depth, frame=frame, lights_count=len(flat.lights))
    old = np.random.default_rng(3).random((H, W, 4)).astype(F)
    r = _renderer(flat, "ploc", 1, modes, cutoffs)
    whole = np.zeros((H, W, 4), F)
    for rank in range(2):
        rows = shard_row_indices(H, 2, rank, 8)
        part = r.pathtrace(pc, cam, W, H, seed=11, shard=abi.Shard(W, H, 8, 2, rank), image=torch.as_tensor(old[rows].copy(), device="cuda:0"))
        whole[rows] = _np(part)
    assert r.counters()["traversal_faults"] == 0
    r.close()
    assert _digest(whole) == atrium_digest
    # vkrt_pathtrace_frames, 1 and 3 frames in flight, against single calls (frames 0 .. 2, seeds 11 .. 13)
    frames = {}
    for name, in_flight in (("single calls", None), ("1 in flight", 1), ("3 in flight", 3)):
        r = _renderer(flat, "ploc", 1, modes, cutoffs, None if in_flight is None else {abi.VKRT_OPT_WF_FRAMES_IN_FLIGHT: in_flight})
        img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        pc0 = make_push_constants(samples=1, depth=4, frame=0, lights_count=len(flat.lights))
        if in_flight is None:
            for f in range(3):
                pc0.frame = f
                r.pathtrace(pc0, cam, W, H, seed=11 + f, image=img)
        else:
            r.pathtrace_frames(pc0, cam, W, H, 3, seed=11, image=img)
        frames[name] = _digest(_np(img))
        assert r.counters()["traversal_faults"] == 0
        r.close()
    assert len(set(frames.values())) == 1, frames


# ---- test 5: liveness and gating --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 0])
def test_the_stage_is_live_and_gated(layout):
    import torch
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import VkrtError

    flat, modes, cutoffs = A._layer_stack()
    W, H = STACK_WH
    cam = S._camera(W, H, STACK_CAMERA)[0]
    pc = make_push_constants(samples=1, depth=4, frame=0, lights_count=len(flat.lights))

    def frame(r):
        return _np(r.pathtrace(pc, cam, W, H, seed=9))

    def fresh(f, with_modes=True, alpha=1):
        q = _renderer(f, "ploc", layout, modes if with_modes else None, cutoffs, alpha=alpha)
        out = frame(q)
        q.close()
        return out

    opaque = fresh(flat, with_modes=False, alpha=0)
    cut = fresh(flat)
    assert _changed(cut, opaque) > 0.02
    r = _renderer(flat, "ploc", layout, None, None)
    # the option on and no MASK material: the option-off image; the modes with the option off: unchanged as well
    assert np.array_equal(_u32(frame(r)), _u32(opaque))
    r.set_option(abi.VKRT_OPT_ALPHA_TEST, 0)
    r.set_material_alpha(0, modes, cutoffs)
    assert np.array_equal(_u32(frame(r)), _u32(opaque))
    rays = A._stack_rays()[:5000]
    o, d = _np(rays)[:, 0:3].copy(), _np(rays)[:, 4:7].copy()
    debug_off = [np.asarray(a).copy() for a in r.trace_rays(o, d, 0.001, 100.0)]
    r.set_option(abi.VKRT_OPT_ALPHA_TEST, 1)
    assert r.get_option(abi.VKRT_OPT_ALPHA_TEST) == 1
    for a, b in zip(debug_off, r.trace_rays(o, d, 0.001, 100.0)):  # the debug hook never takes the stage
        assert np.array_equal(a.view(np.uint32) if a.dtype == F else a, np.asarray(b).view(np.uint32) if a.dtype == F else np.asarray(b))
    assert np.array_equal(_u32(frame(r)), _u32(cut))
    # on the caller's stream, with no build in between: OPAQUE again, then MASK again
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r.set_material_alpha(0, np.zeros_like(modes), cutoffs, stream=s)
        first = r.pathtrace(pc, cam, W, H, seed=9, stream=s, image=torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0"))
        r.set_material_alpha(0, modes, cutoffs, stream=s)
        second = r.pathtrace(pc, cam, W, H, seed=9, stream=s, image=torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0"))
    s.synchronize()
    assert np.array_equal(_u32(_np(first)), _u32(opaque)) and np.array_equal(_u32(_np(second)), _u32(cut))
    # texture coordinates alone move the holes: no refit, the tree is not stale
    shifted = (flat.texcoords0 + F([0.37, -0.21])).astype(F)
    r.update_vertices(0, texcoords0=shifted)
    sflat = copy.copy(flat)
    sflat.texcoords0 = shifted
    want = fresh(sflat)
    assert np.array_equal(_u32(frame(r)), _u32(want)) and _changed(want, cut) > 0.02
    # node moves + refit: a fresh build's image; the option and the modes survive the refit and a rebuild
    mflat, mats = moved(sflat, [1, 4, 9], seed=5, mirror_first=False, scale=False)
    apply(r, mats)
    r.refit()
    want = fresh(mflat)
    assert np.array_equal(_u32(frame(r)), _u32(want))
    r.build("lbvh")
    assert np.array_equal(_u32(frame(r)), _u32(want))
    # 128-thread traversal workgroups: refused while the stage is active, rendered as before while it is not
    r.set_option(abi.VKRT_OPT_WF_TRAV_BLOCK, 128)
    with pytest.raises(VkrtError) as e:
        frame(r)
    assert f"({abi.VKRT_ERR_UNSUPPORTED})" in str(e.value) and "VKRT_OPT_ALPHA_TEST" in str(e.value)
    with pytest.raises(VkrtError):
        r.gbuffer_raycast(cam, W, H)
    r.set_material_alpha(0, np.zeros_like(modes), cutoffs)
    wide_blocks = frame(r)
    r.set_option(abi.VKRT_OPT_WF_TRAV_BLOCK, 64)
    assert np.array_equal(_u32(wide_blocks), _u32(frame(r)))
    assert r.counters()["traversal_faults"] == 0
    r.close()
