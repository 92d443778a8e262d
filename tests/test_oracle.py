"""Pins the CPU oracle (oracle/oracle.cpp): integer KATs, cross-restatement agreement, brute force
vs BVH, analytic images.  The reference ships no golden vectors, so these are the
pins the oracle has ("parity unpinned" w.r.t. the Vulkan reference itself)."""
import json
import os

import numpy as np
import pytest

import oracle_py
from conftest import GOLDEN, default_camera
from vkrt_amd.flat_scene import make_push_constants


def test_prng_known_answers():
    kat = json.load(open(os.path.join(GOLDEN, "prng_kat.json")))
    for a, b, want in kat["tea"] + kat["survey_appendix_c"]["tea"]:
        assert oracle_py.tea(a, b) == want
    for rec in kat["lcg"]:
        got = oracle_py.lcg_sequence(rec["start"], len(rec["seq"]))
        for (s, bits, r), (ws, wb) in zip(got, rec["seq"]):
            assert (s, bits) == (ws, wb)
            assert r == wb / 16777216.0  # exact: 24-bit integer / 2^24
    sv = kat["survey_appendix_c"]
    got = oracle_py.lcg_sequence(0, 3)
    assert [[g[0], g[1]] for g in got] == sv["lcg_from_0"]
    chain = [g[2] for g in oracle_py.lcg_sequence(oracle_py.tea(0, 0), 4)]
    assert chain == sv["rnd_chain_from_tea00"]


def test_seed_index_collisions_match_survey():
    """raytrace.rgen:27 uses y*x + x: only 283,600 distinct indices at 1280x720."""
    kat = json.load(open(os.path.join(GOLDEN, "prng_kat.json")))["survey_appendix_c"]["distinct_seed_indices"]
    for (w, h), want in (((1280, 720), kat["1280x720"]), ((256, 256), kat["256x256"])):
        y, x = np.mgrid[0:h, 0:w].astype(np.uint64)
        assert len(np.unique((y * x + x) & 0xFFFFFFFF)) == want


def test_sincos_profile_accuracy():
    """The profile's sin/cos stay within 2 ulp-ish of the true functions over the sampled range."""
    x = (np.arange(0, 1 << 24, 37, dtype=np.float64) / 16777216.0 * 6.2831855).astype(np.float32)
    s, c = oracle_py.eval_math(0, x), oracle_py.eval_math(1, x)
    assert np.max(np.abs(s - np.sin(x.astype(np.float64)))) < 2.5e-7
    assert np.max(np.abs(c - np.cos(x.astype(np.float64)))) < 2.5e-7
    xs = np.linspace(0, 1, 1001, dtype=np.float32)
    p = oracle_py.eval_math(4, xs)
    assert np.allclose(p, xs.astype(np.float64) ** 5, rtol=3e-7, atol=1e-30)


def test_shading_agrees_with_numpy_restatement():
    """The generator's own records (the `default` stratum of tests/shade_records.py): discrete outputs exact, and every record within
    four times the measured maximum difference (tests/test_shade_records.py holds the other strata and the binary64 twin)."""
    import np_shading
    import shade_records

    rec, a, b, _ = shade_records.evaluate("default")
    assert rec.shape[0] == 20000
    # discrete outputs are exact: lobe choice, PRNG state, ray origin
    assert np.array_equal(a[:, 12], b[:, 12])
    assert np.array_equal(a[:, 17].view(np.uint32), np_shading.out_seed(b))
    assert np.array_equal(a[:, 3:6], b[:, 3:6])
    assert np.isfinite(a[:, :17]).all() and np.isfinite(b[:, :17]).all()
    shade_records.check_parity("default")  # no quantile: the bar holds for every record
    for lo, hi, name in ((0, 3, "hitValue"), (6, 9, "rayDirection"), (9, 12, "weight"), (13, 14, "lightDist"), (14, 17, "shadowRayDir")):
        x, y = a[:, lo:hi].astype(np.float64), b[:, lo:hi].astype(np.float64)
        scale = np.maximum(np.abs(x), np.abs(y)).max(axis=1, keepdims=True) + 1e-3
        err = np.abs(x - y) / scale
        assert err.max() < 2e-4, (name, float(err.max()))
        assert np.median(err) < 2e-6, (name, float(np.median(err)))


def test_camera_ray_matches_numpy():
    import camera_np

    W, H = 1280, 720
    vp, vi, pi = camera_np.global_uniforms(width=W, height=H)
    cam = default_camera(W, H)
    for (x, y) in ((0, 0), (W - 1, H - 1), (640, 360), (17, 700)):
        o, d = oracle_py.camera_ray(cam, x, y, W, H)
        ndc = np.array([(x + 0.5) / W * 2 - 1, (y + 0.5) / H * 2 - 1, 1.0, 1.0])
        tgt = pi.astype(np.float64) @ ndc
        dd = vi.astype(np.float64) @ np.append(tgt[:3] / np.linalg.norm(tgt[:3]), 0.0)
        assert np.allclose(o, [0, 0, 15], atol=1e-5)
        assert np.allclose(d, dd[:3], atol=2e-6)
    # row 0 is the top of the image (perspectiveVK flips Y)
    _, d_top = oracle_py.camera_ray(cam, 640, 0, W, H)
    assert d_top[1] > 0


def test_bruteforce_equals_bvh_config1(cornell_oracle, cornell_flat):
    """BASELINE config 1 (cornell 256x256, 1 spp, depth 1): BVH-independent result."""
    W = H = 256
    cam = default_camera(W, H)
    pc = make_push_constants(samples=1, depth=1, frame=0, lights_count=1)
    a, ca = cornell_oracle.render(pc, cam, W, H, seed=0, use_bvh=True)
    rows = np.arange(0, H, 4, dtype=np.uint32)  # every 4th row by brute force (time bound)
    b, cb = cornell_oracle.render(pc, cam, W, H, seed=0, use_bvh=False, rows=rows)
    assert np.array_equal(a[rows].view(np.uint32), b.view(np.uint32))
    assert not np.isnan(a).any()
    # depth-1 analytic structure: alpha forced to 1, background = clearColor*0.8
    assert np.all(a[..., 3] == 1.0)
    assert np.all(a[0, 0, :3] == np.float32(0.8))
    assert ca["rays_closest"] == W * H and ca["pixels"] == W * H
    assert ca["rays_shadow"] == ca["diffuse_hits"]


def test_bruteforce_equals_bvh_multibounce(cornell_oracle):
    W, H = 96, 64
    cam = default_camera(W, H)
    pc = make_push_constants(samples=3, depth=4, frame=2, lights_count=1)
    img0 = np.full((H, W, 4), 0.25, np.float32)
    a, _ = cornell_oracle.render(pc, cam, W, H, seed=11, image=img0.copy(), use_bvh=True)
    b, _ = cornell_oracle.render(pc, cam, W, H, seed=11, image=img0.copy(), use_bvh=False)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_ray_queries_bruteforce_equals_bvh(cornell_oracle):
    rng = np.random.default_rng(3)
    o = rng.uniform(-4.5, 4.5, (3000, 3)).astype(np.float32)
    d = rng.standard_normal((3000, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t0, u0, v0, g0, _ = cornell_oracle.trace_rays(o, d, use_bvh=True)
    t1, u1, v1, g1, _ = cornell_oracle.trace_rays(o, d, use_bvh=False)
    assert np.array_equal(g0, g1) and np.array_equal(t0.view(np.uint32), t1.view(np.uint32))
    _, _, _, a0, _ = cornell_oracle.trace_rays(o, d, tmax=2.5, any_hit=True, use_bvh=True)
    _, _, _, a1, _ = cornell_oracle.trace_rays(o, d, tmax=2.5, any_hit=True, use_bvh=False)
    assert np.array_equal(a0, a1)


def test_miss_only_image(cornell_oracle):
    """raytrace.rmiss:15 -- looking away from the scene every pixel is clearColor*0.8."""
    W, H = 40, 30
    cam = default_camera(W, H, eye=(0, 0, 15), center=(0, 0, 30))
    pc = make_push_constants(samples=2, depth=4, frame=0, lights_count=1, clear_color=(0.25, 0.5, 1.0, 1.0))
    img, c = cornell_oracle.render(pc, cam, W, H, seed=1)
    want = np.array([np.float32(0.25) * np.float32(0.8), np.float32(0.5) * np.float32(0.8), np.float32(0.8), 1.0], np.float32)
    assert np.all(img == want)
    assert c["rays_closest"] == W * H * 2 and c["hits"] == 0 and c["rays_shadow"] == 0


def test_frame_accumulation_is_mix(cornell_oracle):
    """raytrace.rgen:136-141: frame>0 blends new into old with a = 1/(frame+1)."""
    W, H = 32, 24
    cam = default_camera(W, H)
    pc1 = make_push_constants(samples=1, depth=2, frame=3, lights_count=1)
    old = np.full((H, W, 4), 0.5, np.float32)
    a, _ = cornell_oracle.render(pc1, cam, W, H, seed=4, image=old.copy())
    zero = np.zeros((H, W, 4), np.float32)
    b, _ = cornell_oracle.render(pc1, cam, W, H, seed=4, image=zero.copy())  # = new * a
    al = np.float32(1.0) / np.float32(4.0)
    want = old[..., :3] * (np.float32(1) - al) + (b[..., :3] / al) * al
    assert np.allclose(a[..., :3], want, rtol=1e-6, atol=1e-7)


def test_texture_sampler_bilinear_repeat_srgb(cornell_flat):
    import copy

    flat = copy.copy(cornell_flat)
    rng = np.random.default_rng(0)
    tex = rng.integers(0, 256, (4, 8, 4), dtype=np.uint8)
    flat.textures = [dict(rgba8=tex, is_srgb=False), dict(rgba8=tex, is_srgb=True)]
    s = oracle_py.OracleScene(flat, build_bvh=False)
    # texel centres reproduce the texel; REPEAT wraps
    uv = np.array([[(2 + 0.5) / 8, (1 + 0.5) / 4], [(2 + 0.5) / 8 + 3.0, (1 + 0.5) / 4 - 2.0]], np.float32)
    out = s.sample_texture(0, uv)
    assert np.allclose(out[0], tex[1, 2] / 255.0, atol=1e-6) and np.allclose(out[1], out[0], atol=1e-5)
    # halfway between two texels = their mean
    mid = s.sample_texture(0, np.array([[3.0 / 8, 1.5 / 4]], np.float32))[0]
    assert np.allclose(mid, (tex[1, 2].astype(np.float64) + tex[1, 3]) / 2 / 255.0, atol=1e-6)
    # sRGB decode on rgb, linear alpha
    c = tex[1, 2].astype(np.float64) / 255.0
    lin = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    o = s.sample_texture(1, uv[:1])[0]
    assert np.allclose(o[:3], lin[:3], atol=1e-6) and np.isclose(o[3], c[3], atol=1e-6)
    # out-of-range texture index -> 1x1 white dummy
    assert np.all(s.sample_texture(7, uv[:1]) == 1.0)


def test_full_sweep_sah_tree_is_valid(cornell_oracle):
    info = cornell_oracle.bvh_info()
    assert info["leaves"] == info["nodes"] + 1
    assert info["max_depth"] < 64
    v, ids = cornell_oracle.triangles()
    assert len(v) == 16732 and np.array_equal(ids[:, 0], np.arange(16732))


def test_bruteforce_equals_bvh_on_flat_axis_aligned_geometry():
    """Regression for the slab-test margins: the atrium is full of axis-aligned, zero-thickness boxes (floor and wall quads).
    With only the far side padded by 2 ulp (Ize 2013) one pixel in ~1e5 differed between the BVH and the brute-force walk --
    the triangle test accepts rays that graze an edge from just outside the box.  Rows chosen to include the pixel that
    exposed it (row 119 of the 384x216 view, frames 0 and 1)."""
    import os, sys

    import numpy as np

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import atrium
    import camera_np
    import oracle_py
    from vkrt_amd.flat_scene import make_push_constants, uniforms_from_matrices

    flat, _ = atrium.build_atrium(20000, seed=3)
    orc = oracle_py.OracleScene(flat)
    W, H = 384, 216
    cam = uniforms_from_matrices(*camera_np.global_uniforms(width=W, height=H, **atrium.DEFAULT_CAMERA))
    rows = np.array([40, 118, 119, 120, 200], np.uint32)
    a = np.zeros((len(rows), W, 4), np.float32)
    b = np.zeros((len(rows), W, 4), np.float32)
    for f in range(2):
        pc = make_push_constants(samples=2, depth=6, frame=f, lights_count=len(flat.lights))
        orc.render(pc, cam, W, H, seed=40 + f, rows=rows, image=a)
        orc.render(pc, cam, W, H, seed=40 + f, rows=rows, image=b, use_bvh=False)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_fallback_light_tables_are_independent_copies_that_agree():
    """hello_vulkan.cpp:255-326 is transcribed three times (oracle/gltf_flatten.py, vkrt_amd.flat_scene, host/gltf_loader.cpp
    through the C++ loader): a typo in one of them must show."""
    import gltf_flatten
    from vkrt_amd.flat_scene import fallback_lights

    a, b = gltf_flatten.reference_fallback_lights(), fallback_lights()
    assert a.shape == b.shape == (8,)
    for k in ("position", "color", "intensity", "type"):
        assert np.array_equal(a[k], b[k]), k
    assert gltf_flatten.reference_fallback_lights is not fallback_lights


# ---- watertight ray/triangle test (VKRT_OPT_WATERTIGHT; what traceRayEXT is by the Vulkan specification) ------------------------
def test_watertight_test_closes_the_cornell_wall_diagonal(cornell_flat):
    """Config 1's camera rays through pixels (x, 255 - x) run exactly through the diagonal shared by the back wall's two triangles.
    Binary32 Moeller-Trumbore rejects them in both (the known deviation of DESIGN.md section 2) and they reach the outer shell 0.1
    behind the wall; the watertight test gives each of them to one of the two triangles, as the float64 restatement and a conformant
    driver do.  Everywhere else the two tests agree on the triangle."""
    import np_pathtrace

    W = H = 256
    cam = default_camera(W, H)
    orc = oracle_py.OracleScene(cornell_flat)
    yy, xx = np.mgrid[0:H, 0:W]
    od = np.array([np.concatenate(oracle_py.camera_ray(cam, int(x), int(y), W, H)) for x, y in zip(xx.ravel(), yy.ravel())], np.float32)
    o, d = od[:, :3], od[:, 3:]
    t_mt, _, _, g_mt, _ = orc.trace_rays(o, d)
    orc.set_watertight(True)
    t_wt, u_wt, v_wt, g_wt, _ = orc.trace_rays(o, d)
    t_wb, _, _, g_wb, _ = orc.trace_rays(o, d, use_bvh=False)
    assert np.array_equal(g_wt, g_wb) and np.array_equal(t_wt.view(np.uint32), t_wb.view(np.uint32))  # tree walk == loop over all triangles
    leak = np.nonzero(np.abs(t_mt - t_wt) > 1e-3)[0]
    assert 1 <= len(leak) <= 16 and np.all(xx.ravel()[leak] + yy.ravel()[leak] == 255)
    assert np.all(t_mt[leak] - t_wt[leak] > 0.05)  # Moeller-Trumbore: through the wall, onto the shell behind it
    # (elsewhere a ray on a shared edge may be given to the other of the two triangles -- a different id at the same distance)
    t64, tri64, _, _ = np_pathtrace.NpScene(cornell_flat).closest(o[leak], d[leak])
    assert np.allclose(t64, t_wt[leak], rtol=0, atol=1e-4)  # float64: the wall
    assert np.all((u_wt[leak] == 0.0) | (v_wt[leak] == 0.0) | (np.abs(u_wt[leak] + v_wt[leak] - 1.0) < 1e-6))  # hits ON the shared edge
    rest = np.ones(t_mt.shape[0], bool); rest[leak] = False
    assert np.abs(t_mt[rest] - t_wt[rest]).max() < 2e-5 and np.mean(g_mt[rest] != g_wt[rest]) < 2e-3


def test_watertight_test_has_no_leaks_along_shared_edges_and_vertices():
    """Rays aimed at points ON the interior edges and vertices of a randomly rotated, finely tessellated sheet (end points of the
    edges are float32 vertices; targets are float32 combinations of them, so they sit within rounding of an edge, on either side).
    A sheet is closed along those edges: every such ray must hit.  The watertight test never misses; Moeller-Trumbore on the same
    rays does."""
    from vkrt_amd.flat_scene import LIGHT_DTYPE, MAT_DTYPE, NODE_DTYPE, PRIM_DTYPE, FlatScene

    rng = np.random.default_rng(11)
    g = 24
    xs = np.linspace(-1, 1, g + 1)
    gx, gz = np.meshgrid(xs, xs)
    P = np.stack([gx.ravel(), 0.05 * np.sin(3 * gx.ravel()) * np.cos(2 * gz.ravel()), gz.ravel()], -1)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    P = (P @ Q.T * 3.7 + rng.uniform(-2, 2, 3)).astype(np.float32)
    idx = []
    for j in range(g):
        for i in range(g):
            a = j * (g + 1) + i
            idx += [a, a + g + 1, a + 1, a + 1, a + g + 1, a + g + 2]
    idx = np.array(idx, np.uint32)
    V = P.shape[0]
    pm = np.zeros(1, PRIM_DTYPE); pm[0] = (0, idx.size, 0, V, 0)
    mats = np.zeros(1, MAT_DTYPE)
    mats[0]["pbrBaseColorFactor"] = [0.8, 0.8, 0.8, 1.0]
    mats[0]["pbrBaseColorTexture"] = mats[0]["metallicRoughnessTexture"] = mats[0]["normalTexture"] = mats[0]["emissiveTexture"] = -1
    nodes = np.zeros(1, NODE_DTYPE); nodes[0]["worldMatrix"] = np.eye(4, dtype=np.float32).ravel()
    lights = np.zeros(1, LIGHT_DTYPE); lights[0] = ((0.0, 5.0, 0.0), (1, 1, 1), 10.0, 0)
    flat = FlatScene(P, np.tile(np.array([0, 1, 0], np.float32), (V, 1)), np.tile(np.array([1, 0, 0, 1], np.float32), (V, 1)), np.zeros((V, 2), np.float32),
                     idx, pm, mats, lights, nodes, [])
    orc = oracle_py.OracleScene(flat)
    tri = idx.reshape(-1, 3)
    # interior edges: the diagonal of every quad and the edges between quads; targets = vertices and points along those edges
    n = 40000
    t = tri[rng.integers(0, tri.shape[0], n)]
    e = rng.integers(0, 3, n)
    a, b = P[t[np.arange(n), e]], P[t[np.arange(n), (e + 1) % 3]]
    s = rng.choice([0.0, 1.0, 0.5, 0.25, 1.0 / 3.0], n) * (rng.random(n) < 0.5) + rng.random(n) * 0.5
    s = np.clip(s, 0, 1).astype(np.float32)[:, None]
    target = (a * (1 - s) + b * s).astype(np.float32)
    cen = P.mean(0)
    keep = np.linalg.norm((target - cen) @ Q, axis=1, ord=np.inf) < 3.7 * 0.95  # stay away from the sheet's outer boundary
    nrm = Q[:, 1]
    o = (target + nrm * rng.uniform(2, 6, (n, 1)) + rng.normal(0, 1.0, (n, 3))).astype(np.float32)
    d = (target - o).astype(np.float32)
    o, d = o[keep], d[keep]
    _, _, _, g_mt, _ = orc.trace_rays(o, d, tmin=0.0, tmax=1e9, use_bvh=False)
    orc.set_watertight(True)
    _, _, _, g_wt, _ = orc.trace_rays(o, d, tmin=0.0, tmax=1e9, use_bvh=False)
    _, _, _, g_wt_tree, _ = orc.trace_rays(o, d, tmin=0.0, tmax=1e9)
    assert o.shape[0] > 30000
    assert (g_wt < 0).sum() == 0, int((g_wt < 0).sum())
    assert np.array_equal(g_wt, g_wt_tree)
    assert (g_mt < 0).sum() > 0  # the default test does leak on these rays


# ---- any-hit alpha / dissolve stage (VKRT_OPT_ANYHIT_DISSOLVE; raytrace_rahit_todo.glsl:23-37, inert in the reference) ----------------
def _cornell_with_alpha(cornell_flat, alphas):
    import copy

    flat = copy.deepcopy(cornell_flat)
    for m, a in alphas.items():
        flat.materials["pbrBaseColorFactor"][m, 3] = a
    return flat


def test_dissolve_stage_is_inert_for_opaque_materials_and_tree_independent(cornell_flat):
    W, H = 96, 64
    cam = default_camera(W, H)
    pc = make_push_constants(samples=2, depth=4, frame=0, lights_count=1)
    assert abs(float(cornell_flat.materials["pbrBaseColorFactor"][7, 3]) - 0.05) < 1e-6  # the asset itself carries one non-opaque material
    orc = oracle_py.OracleScene(_cornell_with_alpha(cornell_flat, {7: 1.0}))
    base, c0 = orc.render(pc, cam, W, H, seed=5)
    orc.set_dissolve(True)
    same, c1 = orc.render(pc, cam, W, H, seed=5)
    assert np.array_equal(base.view(np.uint32), same.view(np.uint32)) and c0["rays_shadow"] == c1["rays_shadow"]  # every alpha is 1
    # materials 0..8 of the Cornell file; make three of them translucent and one invisible (7 keeps the file's 0.05)
    flat = _cornell_with_alpha(cornell_flat, {1: 0.5, 3: 0.25, 4: 0.0, 6: 0.9})
    o2 = oracle_py.OracleScene(flat)
    opaque, _ = o2.render(pc, cam, W, H, seed=5)
    assert np.array_equal(opaque.view(np.uint32), base.view(np.uint32))  # stage off: alpha is not looked at
    o2.set_dissolve(True)
    tree, ct = o2.render(pc, cam, W, H, seed=5)
    brute, cb = o2.render(pc, cam, W, H, seed=5, use_bvh=False)
    assert np.array_equal(tree.view(np.uint32), brute.view(np.uint32)) and ct["rays_closest"] == cb["rays_closest"]
    assert np.mean(np.any(tree.view(np.uint32) != base.view(np.uint32), axis=-1)) > 0.05  # and it does change the picture


def test_dissolve_stage_passes_the_expected_fraction_of_rays():
    """A screen of material alpha in front of a backdrop: the fraction of rays that reach the backdrop is 1 - alpha (each ray decides per
    triangle from rnd(tea(triangle id, seed)); seed 0 rays differ by triangle only, so a finely tessellated screen is used)."""
    from vkrt_amd.flat_scene import LIGHT_DTYPE, MAT_DTYPE, NODE_DTYPE, PRIM_DTYPE, FlatScene

    g = 40
    xs = np.linspace(-1, 1, g + 1, dtype=np.float32)
    gx, gy = np.meshgrid(xs, xs)
    screen = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size, np.float32)], -1)
    idx = []
    for j in range(g):
        for i in range(g):
            a = j * (g + 1) + i
            idx += [a, a + 1, a + g + 1, a + 1, a + g + 2, a + g + 1]
    back = np.array([[-3, -3, -1], [3, -3, -1], [3, 3, -1], [-3, 3, -1]], np.float32)
    pos = np.concatenate([screen, back]).astype(np.float32)
    V = pos.shape[0]
    idx_all = np.concatenate([np.array(idx, np.uint32), np.array([0, 1, 2, 0, 2, 3], np.uint32)])
    pm = np.zeros(2, PRIM_DTYPE)
    pm[0] = (0, len(idx), 0, screen.shape[0], 0)
    pm[1] = (len(idx), 6, screen.shape[0], 4, 1)
    nodes = np.zeros(2, NODE_DTYPE)
    for k in range(2):
        nodes[k]["worldMatrix"] = np.eye(4, dtype=np.float32).ravel(); nodes[k]["primMesh"] = k
    lights = np.zeros(1, LIGHT_DTYPE); lights[0] = ((0.0, 0.0, 5.0), (1, 1, 1), 10.0, 0)
    rng = np.random.default_rng(4)
    n = 20000
    o = np.concatenate([rng.uniform(-0.95, 0.95, (n, 2)), np.full((n, 1), 2.0)], 1).astype(np.float32)
    d = np.tile(np.array([[0, 0, -1]], np.float32), (n, 1))
    for alpha in (0.0, 0.3, 0.75, 1.0):
        mats = np.zeros(2, MAT_DTYPE)
        for m in mats:
            m["pbrBaseColorFactor"] = [0.8, 0.8, 0.8, 1.0]
            m["pbrBaseColorTexture"] = m["metallicRoughnessTexture"] = m["normalTexture"] = m["emissiveTexture"] = -1
        mats[0]["pbrBaseColorFactor"][3] = alpha
        flat = FlatScene(pos, np.tile(np.array([0, 0, 1], np.float32), (V, 1)), np.tile(np.array([1, 0, 0, 1], np.float32), (V, 1)), np.zeros((V, 2), np.float32),
                         idx_all, pm, mats, lights, nodes, [])
        orc = oracle_py.OracleScene(flat)
        orc.set_dissolve(True)
        t, _, _, gid, _ = orc.trace_rays(o, d)
        through = float(np.mean(gid >= len(idx) // 3))  # hit the backdrop (its two triangles come last)
        assert abs(through - (1.0 - alpha)) < 0.03, (alpha, through)
        # ray by ray against an independent statement of the rule (numpy tea / lcg of oracle/np_pathtrace.py): the screen triangle
        # under the ray (opaque query) is ignored iff alpha == 0 or rnd(tea(triangle id, payload seed = 0)) > alpha
        import np_pathtrace

        orc.set_dissolve(False)
        _, _, _, under, _ = orc.trace_rays(o, d)
        orc.set_dissolve(True)
        assert np.all(under < len(idx) // 3)
        st = np_pathtrace.tea(under.astype(np.uint32), np.zeros_like(under, dtype=np.uint32))
        _, r = np_pathtrace.rnd(st)
        expect_ignored = (r > np.float32(alpha)) | (alpha == 0.0)
        assert np.array_equal(gid >= len(idx) // 3, expect_ignored)
        _, _, _, anyh, _ = orc.trace_rays(o, d, tmin=0.001, tmax=2.5, any_hit=True)  # shadow-type query that ends before the backdrop
        assert abs(float(np.mean(anyh < 0)) - (1.0 - alpha)) < 0.03
