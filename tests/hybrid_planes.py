"""Synthetic G-buffer planes that reach every branch of the hybrid pass (raytraceHybrid.rgen: k_hybrid, k_hy_gi_init / k_wf_shade_hybrid,
csrc/hybrid_gi.h), and the oracle's answers for them.

numpy and the oracle only, deterministic in the seed.  The G-buffer is caller-owned memory in the ABI (vkrt_gbuffer, vkrt_nrd_planes):
a host that rasterises its own hands the library whatever it has.  So the planes here are not what vkrt_gbuffer_raycast leaves for an
ordinary camera: every pixel has a KIND (kept in an integer plane, so that a failure is reported by kind), a VARIANT inside the kind,
and every 8x8 tile a LAYOUT that says which of its lanes are shaded at all.

Kinds (KINDS): clear (position and normal all zero, some zeros written as -0.0, .w = 1 or anything), half_clear (position exactly
zero, unit normal: shaded, at the origin), surface (a uniform point of a random triangle, in float32 from the flat arrays, lifted off
along the geometric normal by 0, 1e-4, 1e-2 or 0.2; normal geometric, flipped, tilted by 0-90 degrees, or of length 0.5 or 2),
terminator (normal perpendicular to the float32 direction to light 0, and that normal nudged by +-1..4 ulp in its largest component),
near_light (0.05, float32(0.1), 0.1000001, 0.2, 0.5 from light 0: lightDistance - 0.1 negative, zero, tiny), free_space (inside the
padded scene bounds, outside them, 2e4 away), material (surface points with (roughness, metalness) on a grid that holds (0, 0.8) and
(0.2f, 1) and their float32 neighbours on both sides, with and without the rg16f round trip, roughness 0, 1, 1.5, albedo channels from
{0, 0.5, 1, 4, -0.25}), view_depth (nrdViewZ from {0, -0.5, -30, 30, 6e4}), outward (a point outside the scene whose normal looks away
from it: its GI path misses at depth 1) and degenerate (NaN / infinity in a position, normal, roughness or viewZ, the position exactly
at the light, a zero normal with a non-zero position) -- the last only in the case named "degenerate", which nothing else depends on.

Layouts (LAYOUTS), per 8x8 tile, the tiles of an image taking them in turn: none, one lane (corner, edge, middle), all but one, all,
checkerboard, one row; one_lit (all shaded, one lane's normal faces light 0 and the others' look away: one lane alone wants a shadow
ray), one_mirror (one mirror-like lane among diffuse ones) and one_deep (one surface lane among `outward` lanes: with depth 8 it alone
is still active at depth 7)."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

F = np.float32
KINDS = ("clear", "half_clear", "surface", "terminator", "near_light", "free_space", "material", "view_depth", "outward", "degenerate")
K = {k: i for i, k in enumerate(KINDS)}
LAYOUTS = ("none", "one_corner", "one_edge", "one_middle", "all_but_one", "all", "checkerboard", "one_row", "one_lit", "one_mirror", "one_deep")
PLAIN = LAYOUTS[:8]
SIZES = ((1, 1), (8, 8), (13, 11), (72, 40), (40, 72))
ALBEDO_SET = np.array([0.0, 0.5, 1.0, 4.0, -0.25], F)
VIEWZ_SET = np.array([0.0, -0.5, -30.0, 30.0, 6e4], F)
NEAR_SET = np.array([0.05, F(0.1), 0.1000001, 0.2, 0.5], F)
LIFT_SET = np.array([0.0, 1e-4, 1e-2, 0.2], F)
# kind mix of the shaded lanes of a plain tile (terminator and near_light only where light 0 is the light: lightsCount == 1)
MIX = (("surface", 0.26), ("terminator", 0.10), ("near_light", 0.10), ("free_space", 0.12), ("material", 0.26), ("view_depth", 0.08),
       ("half_clear", 0.03), ("outward", 0.05))

# name -> scene, (W, H), (useShadows, useAO, useGI), depth, frame, lights (1 or "all"), seed of the trace call, row-major seed index,
# layouts the tiles take in turn, seed of the planes.  About a dozen; every toggle triple, depth 0 1 2 5 8, frame 0 1 7.
CASES = {
    "cornell-all": dict(scene="cornell", size=(72, 40), toggles=(1, 1, 1), depth=5, frame=0, lights=1, seed=11, row_major=0, layouts=PLAIN, pseed=101),
    "cornell-deep": dict(scene="cornell", size=(40, 72), toggles=(1, 1, 1), depth=8, frame=7, lights=1, seed=12, row_major=1,
                         layouts=("one_mirror", "one_deep", "one_lit", "all", "one_deep", "checkerboard", "one_mirror"), pseed=102),
    "cornell-shadow": dict(scene="cornell", size=(13, 11), toggles=(1, 0, 0), depth=2, frame=1, lights=1, seed=13, row_major=0, layouts=("all", "one_lit", "checkerboard"), pseed=103),
    "cornell-ao": dict(scene="cornell", size=(8, 8), toggles=(0, 1, 0), depth=1, frame=0, lights=1, seed=14, row_major=1, layouts=("all",), pseed=104),
    "cornell-gi": dict(scene="cornell", size=(72, 40), toggles=(0, 0, 1), depth=2, frame=0, lights=1, seed=15, row_major=1, layouts=PLAIN[1:], pseed=105),
    "cornell-none": dict(scene="cornell", size=(13, 11), toggles=(0, 0, 0), depth=0, frame=1, lights=1, seed=16, row_major=0, layouts=("all", "checkerboard"), pseed=106),
    "cornell-1x1": dict(scene="cornell", size=(1, 1), toggles=(1, 1, 0), depth=5, frame=0, lights=1, seed=17, row_major=0, layouts=("all",), pseed=107),
    "atrium-all": dict(scene="atrium", size=(72, 40), toggles=(1, 1, 1), depth=5, frame=0, lights="all", seed=18, row_major=0, layouts=PLAIN, pseed=108),
    "atrium-L1": dict(scene="atrium", size=(40, 72), toggles=(1, 0, 1), depth=8, frame=1, lights=1, seed=19, row_major=1,
                      layouts=("all", "one_deep", "one_mirror", "one_lit", "all_but_one", "one_row"), pseed=109),
    "atrium-aogi": dict(scene="atrium", size=(13, 11), toggles=(0, 1, 1), depth=1, frame=0, lights="all", seed=20, row_major=0, layouts=("all", "all_but_one"), pseed=110),
    "all-clear": dict(scene="cornell", size=(72, 40), toggles=(1, 1, 1), depth=5, frame=0, lights=1, seed=21, row_major=0, layouts=("none",), pseed=111),
    "single": dict(scene="cornell", size=(13, 11), toggles=(1, 1, 1), depth=5, frame=0, lights=1, seed=22, row_major=0, layouts=("single",), pseed=112),
    "degenerate": dict(scene="cornell", size=(72, 40), toggles=(1, 1, 1), depth=5, frame=0, lights=1, seed=23, row_major=1, layouts=("all", "checkerboard", "all_but_one"),
                       pseed=113, degenerate=True),
}
NON_DEGENERATE = tuple(n for n in CASES if n != "degenerate")
SHARDED = ("cornell-all", (16, 3, 1))  # abi.Shard(W, H, 16, 3, 1) on 72x40: the rows of the whole-frame result
DISSOLVE = ("cornell-all", "cornell-deep")  # the two Cornell cases with all toggles on, under VKRT_OPT_ANYHIT_DISSOLVE
DISSOLVE_ALPHA = {1: 0.5, 3: 0.25, 4: 0.0, 6: 0.9}  # material -> alpha, as tests/test_gpu_parity.py sets them for the stage


def quantize_half(x):
    """the rg16f / r16f round trip (quantizeHalf): float32 -> binary16 (RNE) -> float32"""
    with np.errstate(over="ignore"):
        return np.asarray(x, F).astype(np.float16).astype(F)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def scene(name, dissolve=False):
    return _scene(name, bool(dissolve))


@functools.lru_cache(maxsize=None)
def _scene(name, dissolve):
    """(flat scene, OracleScene, camera keywords) of "cornell" (tests/golden/cornell_flat.npz) or "atrium" (the textured one of
    tests/test_hybrid.py); dissolve: Cornell with translucent and invisible materials, the oracle's any-hit stage on"""
    import copy

    import oracle_py
    from vkrt_amd.flat_scene import FlatScene

    if name == "cornell":
        flat, camkw = FlatScene.load_npz(os.path.join(HERE, "golden", "cornell_flat.npz")), {}
        if dissolve:
            flat = copy.deepcopy(flat)
            for m, a in DISSOLVE_ALPHA.items():
                flat.materials["pbrBaseColorFactor"][m, 3] = a
    else:
        import atrium

        flat, _ = atrium.build_atrium(6000, seed=3, with_textures=True, variant="emissive_mixed_lights")
        camkw = dict(atrium.DEFAULT_CAMERA)
    orc = oracle_py.OracleScene(flat)
    if dissolve:
        orc.set_dissolve(True)
    return flat, orc, camkw


def camera(name, W, H):
    import camera_np
    from vkrt_amd.flat_scene import uniforms_from_matrices

    return uniforms_from_matrices(*camera_np.global_uniforms(width=W, height=H, **scene(name)[2]))


@functools.lru_cache(maxsize=None)
def world_triangles(name):
    """[T, 3, 3] float32 world-space corners of every instanced triangle, from the flat arrays (hello_vulkan.cpp:1035-1043)"""
    flat = scene(name)[0]
    pos = np.asarray(flat.positions, F).reshape(-1, 3)
    out = []
    for nd in flat.nodes:
        M = np.asarray(nd["worldMatrix"], F).reshape(4, 4).T
        pm = flat.prim_meshes[int(nd["primMesh"])]
        n = int(pm["indexCount"]) // 3
        idx = np.asarray(flat.indices[int(pm["firstIndex"]): int(pm["firstIndex"]) + 3 * n], np.int64).reshape(n, 3) + int(pm["vertexOffset"])
        out.append((pos[idx] @ M[:3, :3].T + M[:3, 3]).astype(F))
    return np.concatenate(out)


# ---- small float32 vector helpers -------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-300)


def _random_unit(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def _perpendicular(rng, a):
    """a random unit vector perpendicular to each row of a (float64)"""
    r = _random_unit(rng, a.shape[0])
    p = np.cross(a, r)
    bad = np.linalg.norm(p, axis=-1) < 1e-3
    p[bad] = np.cross(a[bad], np.roll(r[bad], 1, axis=-1) + 0.5)
    return _unit(p)


def _light_dir32(light, pos):
    """normalize(light - pos) as the shader computes it: binary32, sum of squares left to right, x / sqrt(.)"""
    d = (light.astype(F) - pos.astype(F)).astype(F)
    s = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + d[:, 2] * d[:, 2]).astype(F)
    return (d / np.sqrt(s, dtype=F)[:, None]).astype(F)


def _nudge(v, ulps):
    """v with its largest component moved by ulps[i] float32 steps"""
    v = np.ascontiguousarray(v, F).copy()
    k = np.argmax(np.abs(v), axis=1)
    r = np.arange(v.shape[0])
    bits = v[r, k].view(np.int32).astype(np.int64)
    bits = bits + np.where(v[r, k] >= 0, ulps, -ulps)  # one step up in magnitude = one step up in the integer
    v[r, k] = bits.astype(np.int32).view(F)
    return v


# ---- material grid ------------------------------------------------------------------------------------------------------------------
def material_grid():
    """[(roughness, metalness, side)] float32.  side: 0 none, 1..3 = below / at / above the 0.8 boundary by varying the metalness around
    (0, 0.8), 4..6 = above / at / below it by varying the roughness around (0.2f, 1): metal * (1 - rough) falls as the roughness rises"""
    m8, r2, one = F(0.8), F(0.2), F(1.0)
    g = [(F(0), np.nextafter(m8, F(0)), 1), (F(0), m8, 2), (F(0), np.nextafter(m8, one), 3),
         (np.nextafter(r2, F(0)), one, 4), (r2, one, 5), (np.nextafter(r2, one), one, 6)]
    for r in (0.0, 0.05, 0.19, 0.21, 0.5, 1.0, 1.5):
        for m in (0.0, 0.5, 0.79, 0.81, 1.0):
            g.append((F(r), F(m), 0))
            g.append((quantize_half(r), quantize_half(m), 0))  # ... and after the rg16f round trip
    return g


def mirror_like(rm):
    """ratio >= 0.8 in binary32 (giFirstRay): a condition on the inputs"""
    rm = np.asarray(rm, F)
    return ~((rm[..., 1] * (F(1.0) - rm[..., 0])).astype(F) < F(0.8))


# ---- the planes ---------------------------------------------------------------------------------------------------------------------
def _tile_mask(layout, rng):
    m = np.zeros((8, 8), bool)
    if layout == "one_corner":
        m[7, 7] = True
    elif layout == "one_edge":
        m[0, 3] = True
    elif layout in ("one_middle", "single"):
        m[3, 4] = True
    elif layout == "all_but_one":
        m[:] = True
        m[rng.integers(8), rng.integers(8)] = False
    elif layout == "checkerboard":
        m[::2, ::2] = m[1::2, 1::2] = True
    elif layout == "one_row":
        m[5] = True
    elif layout != "none":
        m[:] = True
    return m


def make_planes(name):
    """dict: color, position, normal [H,W,4], roughMetal [H,W,2], nrdViewZ [H,W] float32 (nrdNormalRoughness too, zeros: the pass does
    not read it), kind, variant, layout [H,W] int32, degenerate [H,W] bool"""
    c = CASES[name]
    W, H = c["size"]
    rng = np.random.default_rng(c["pseed"])
    flat = scene(c["scene"])[0]
    tris = world_triangles(c["scene"])
    light0 = np.asarray(flat.lights["position"][0], F)
    lo, hi = tris.reshape(-1, 3).min(0).astype(np.float64), tris.reshape(-1, 3).max(0).astype(np.float64)
    ext, mid = hi - lo, 0.5 * (lo + hi)
    n = W * H
    ys, xs = np.divmod(np.arange(n), W)
    # layout of each pixel's tile and whether the lane is shaded
    tiles_x = (W + 7) // 8
    tile = (ys // 8) * tiles_x + xs // 8
    names = c["layouts"]
    single = names == ("single",)
    tile_layout = [names[t % len(names)] for t in range(tile.max() + 1)]
    if single:
        tile_layout = ["single"] + ["none"] * (len(tile_layout) - 1)
    if W * H == 1:
        masks = [np.ones((8, 8), bool)]
    else:
        masks = [_tile_mask(l, rng) for l in tile_layout]
    shaded = np.array([masks[t][y % 8, x % 8] for t, x, y in zip(tile, xs, ys)])
    layout = np.array([LAYOUTS.index("one_middle" if tile_layout[t] == "single" else tile_layout[t]) for t in tile], np.int32)
    special = np.array([tile_layout[t] for t in tile])
    # the one lane of a special tile: a fixed lane per tile
    lane = (ys % 8) * 8 + xs % 8
    chosen_lane = np.array([(7 * t + 19) % 64 for t in range(tile.max() + 1)])[tile]
    in_tile_w, in_tile_h = np.minimum(8, W - (xs // 8) * 8), np.minimum(8, H - (ys // 8) * 8)
    chosen_lane = (chosen_lane // 8 % in_tile_h) * 8 + chosen_lane % 8 % in_tile_w  # (inside a partial tile)
    is_chosen = lane == chosen_lane

    # kind of every shaded lane
    mix = [(k, w) for k, w in MIX if c["lights"] == 1 or k not in ("terminator", "near_light")]
    kind = rng.choice([K[k] for k, _ in mix], size=n, p=np.array([w for _, w in mix]) / sum(w for _, w in mix))
    kind = np.where((special == "one_lit") | (special == "single"), K["surface"], kind)
    kind = np.where(special == "one_mirror", K["material"], kind)
    kind = np.where(special == "one_deep", np.where(is_chosen, K["surface"], K["outward"]), kind)
    kind = np.where(shaded, kind, K["clear"]).astype(np.int32)
    variant = np.zeros(n, np.int32)

    # a surface sample for every pixel
    t = rng.integers(0, tris.shape[0], n)
    u, v = rng.uniform(size=n), rng.uniform(size=n)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    A, B, C_ = tris[t, 0].astype(np.float64), tris[t, 1].astype(np.float64), tris[t, 2].astype(np.float64)
    P = A + u[:, None] * (B - A) + v[:, None] * (C_ - A)
    Ng = _unit(np.cross(B - A, C_ - A))
    lift = rng.integers(0, 4, n)
    pos = P + LIFT_SET[lift].astype(np.float64)[:, None] * Ng
    nvar = rng.integers(0, 5, n)  # geometric, flipped, tilted, half length, double length
    angle = rng.uniform(0, np.pi / 2, n)
    tilted = np.cos(angle)[:, None] * Ng + np.sin(angle)[:, None] * _perpendicular(rng, Ng)
    nrm = np.select([(nvar == 0)[:, None], (nvar == 1)[:, None], (nvar == 2)[:, None], (nvar == 3)[:, None]], [Ng, -Ng, tilted, 0.5 * Ng], 2.0 * Ng)
    variant = np.where(np.isin(kind, (K["surface"], K["material"], K["view_depth"])), nvar * 4 + lift, variant)
    # default material: a handful of half-quantised pairs, albedo in [0, 1)
    rm = quantize_half(np.stack([rng.choice([0.0, 0.3, 0.55, 1.0], n), rng.choice([0.0, 0.2, 1.0], n)], -1))
    albedo = rng.uniform(0, 1, (n, 3)).astype(F)
    view_z = quantize_half(-rng.uniform(1.0, 40.0, n))

    # free space: 0 inside the padded bounds, 1 outside them, 2 at distance 2e4
    m = kind == K["free_space"]
    fv = rng.integers(0, 3, n)
    inside = mid + (rng.uniform(-0.55, 0.55, (n, 3))) * ext
    outside = mid + _random_unit(rng, n) * np.linalg.norm(ext) * rng.uniform(1.5, 3.0, n)[:, None]
    far = _random_unit(rng, n) * 2e4
    fpos = np.select([(fv == 0)[:, None], (fv == 1)[:, None]], [inside, outside], far)
    pos, nrm = np.where(m[:, None], fpos, pos), np.where(m[:, None], _random_unit(rng, n), nrm)
    variant = np.where(m, fv, variant)
    # outward: outside the bounds, the normal looking away from the scene (every ray of its hemisphere misses)
    m = kind == K["outward"]
    out_dir = _random_unit(rng, n)
    pos, nrm = np.where(m[:, None], mid + out_dir * np.linalg.norm(ext) * 1.2, pos), np.where(m[:, None], out_dir, nrm)
    # half clear: position exactly zero, unit normal
    m = kind == K["half_clear"]
    pos, nrm = np.where(m[:, None], 0.0, pos), np.where(m[:, None], _random_unit(rng, n), nrm)
    # near light: at NEAR_SET from light 0, the normal towards the light (the shadow ray is wanted; its tmax is <= tmin up to 0.2)
    m = kind == K["near_light"]
    nv = rng.integers(0, len(NEAR_SET), n)
    ndir = _random_unit(rng, n)
    pos = np.where(m[:, None], light0.astype(np.float64) + NEAR_SET[nv].astype(np.float64)[:, None] * ndir, pos)
    nrm = np.where(m[:, None], -ndir, nrm)
    variant = np.where(m, nv, variant)
    # view depth
    m = kind == K["view_depth"]
    zv = rng.integers(0, len(VIEWZ_SET), n)
    view_z = np.where(m, quantize_half(VIEWZ_SET[zv]), view_z)
    # material sweep: grid point + albedo channels from ALBEDO_SET
    m = kind == K["material"]
    grid = material_grid()
    gi = rng.integers(0, len(grid), n)
    gi = np.where(rng.uniform(size=n) < 0.45, rng.integers(0, 6, n), gi)  # the six sides of the boundary often enough
    grm = np.array([(r, mm) for r, mm, _ in grid], F)[gi]
    gside = np.array([s for _, _, s in grid], np.int32)[gi]
    rm = np.where(m[:, None], grm, rm)
    albedo = np.where(m[:, None], ALBEDO_SET[rng.integers(0, len(ALBEDO_SET), (n, 3))], albedo)
    variant = np.where(m, gside * 100 + variant, variant)
    # one_mirror tiles: the chosen lane mirror-like (0, 1), the others diffuse; geometric normals so that the paths stay inside
    m = (special == "one_mirror") & shaded
    rm = np.where(m[:, None], np.where(is_chosen[:, None], np.array([0.0, 1.0], F), np.array([1.0, 0.0], F)), rm)
    nrm = np.where(m[:, None], Ng, nrm)
    albedo = np.where(m[:, None], rng.uniform(0.2, 1, (n, 3)).astype(F), albedo)
    variant = np.where(m, np.where(is_chosen, 1, 0), variant)

    pos32, nrm32 = pos.astype(F), nrm.astype(F)
    # terminator: normal perpendicular to the float32 light direction of the float32 position, then nudged by 0, +-1 .. +-4 ulp
    m = kind == K["terminator"]
    L32 = _light_dir32(light0, pos32)
    tn = _perpendicular(rng, L32.astype(np.float64)).astype(F)
    ul = rng.integers(-4, 5, n)
    nrm32 = np.where(m[:, None], _nudge(tn, ul), nrm32)
    variant = np.where(m, ul, variant)
    # one_lit tiles: the chosen lane's normal towards light 0, the others' away from it
    m = (special == "one_lit") & shaded
    toward = (L32.astype(np.float64) * 0.8 + 0.6 * _perpendicular(rng, L32.astype(np.float64))).astype(F)
    nrm32 = np.where(m[:, None], np.where(is_chosen[:, None], toward, -toward), nrm32)
    variant = np.where(m, np.where(is_chosen, 1, 0), variant)
    # one_deep tiles: the chosen lane a diffuse surface point with its geometric normal
    m = (special == "one_deep") & is_chosen & shaded
    nrm32 = np.where(m[:, None], Ng.astype(F), nrm32)
    pos32 = np.where(m[:, None], (P + 1e-2 * Ng).astype(F), pos32)
    rm = np.where(m[:, None], np.array([1.0, 0.0], F), rm)

    degenerate = np.zeros(n, bool)
    if c.get("degenerate"):
        degenerate = shaded & (rng.uniform(size=n) < 0.12)
        dv = rng.integers(0, 8, n)
        nan, inf = F(np.nan), F(np.inf)
        comp = rng.integers(0, 3, n)
        r = np.arange(n)
        for code, (arr, val) in enumerate(((pos32, nan), (pos32, inf), (nrm32, nan), (nrm32, -inf))):
            mm = degenerate & (dv == code)
            arr[r[mm], comp[mm]] = val
        rm[degenerate & (dv == 4), 0] = nan
        view_z[degenerate & (dv == 5)] = np.where(rng.uniform(size=int((degenerate & (dv == 5)).sum())) < 0.5, nan, inf)
        pos32[degenerate & (dv == 6)] = light0
        nrm32[degenerate & (dv == 7)] = 0.0
        kind = np.where(degenerate, K["degenerate"], kind).astype(np.int32)
        variant = np.where(degenerate, dv, variant)

    # clear lanes: zeros, some of them -0.0, .w = 1 or anything
    clear = kind == K["clear"]
    zero = np.where(rng.uniform(size=(n, 6)) < 0.3, F(-0.0), F(0.0)).astype(F)
    pos32, nrm32 = np.where(clear[:, None], zero[:, :3], pos32), np.where(clear[:, None], zero[:, 3:], nrm32)
    w_other = rng.uniform(-2, 2, (n, 3)).astype(F)
    wsel = rng.uniform(size=n) < 0.5
    albedo = np.where(clear[:, None], np.where(wsel[:, None], F(1.0), w_other), albedo).astype(F)
    variant = np.where(clear, wsel.astype(np.int32), variant)

    g = {"color": np.concatenate([rng.uniform(0, 1, (n, 3)).astype(F), albedo[:, 0:1]], 1),
         "position": np.concatenate([pos32, albedo[:, 1:2]], 1), "normal": np.concatenate([nrm32, albedo[:, 2:3]], 1)}
    g = {k: np.ascontiguousarray(v.reshape(H, W, 4), F) for k, v in g.items()}
    g["roughMetal"] = np.ascontiguousarray(rm.reshape(H, W, 2), F)
    g["nrdViewZ"] = np.ascontiguousarray(np.asarray(view_z, F).reshape(H, W))
    g["nrdNormalRoughness"] = np.zeros((H, W, 4), F)
    meta = dict(kind=kind.reshape(H, W), variant=variant.reshape(H, W).astype(np.int32), layout=layout.reshape(H, W), degenerate=degenerate.reshape(H, W))
    return g, meta


def shaded_mask(g):
    """loadGbufferPixel's rule: not all six of position.xyz, normal.xyz compare equal to 0 (-0.0 does; NaN does not)"""
    return ~(np.all(g["position"][..., :3] == 0, -1) & np.all(g["normal"][..., :3] == 0, -1))


def prefill(W, H):
    """what nrdRadianceHitDist holds before the call: the device must leave these words alone where GI did not run"""
    return np.random.default_rng(5).uniform(100.0, 200.0, (H, W, 4)).astype(F)


def old_accum(name):
    """the accumulation plane before a frame > 0: random values in [-2, 50]"""
    c = CASES[name]
    W, H = c["size"]
    return np.random.default_rng(c["pseed"] + 1000).uniform(-2.0, 50.0, (H, W, 4)).astype(F)


def push_constants(name, frame=None):
    from vkrt_amd.flat_scene import make_push_constants

    c = CASES[name]
    L = 1 if c["lights"] == 1 else len(scene(c["scene"])[0].lights)
    pc = make_push_constants(samples=1, depth=c["depth"], frame=c["frame"] if frame is None else frame, lights_count=L)
    pc.useShadows, pc.useAO, pc.useGI = c["toggles"]
    return pc


def bits(x):
    """float words as uint32 with every NaN folded to one pattern (tests/test_gpu_shade_records.py: IEEE pins neither sign nor payload)"""
    b = np.ascontiguousarray(x, F).view(np.uint32).copy()
    b[(b & 0x7FFFFFFF) > 0x7F800000] = 0x7FC00000
    return b


def oracle_run(name, use_bvh=True, frame=None, dissolve=False):
    """The oracle over a case: dict accum, rad (nrdRadianceHitDist, 0 where GI did not run: the wrapper hands zeros in), counters"""
    c = CASES[name]
    W, H = c["size"]
    _, orc, _ = scene(c["scene"], dissolve)
    g, _ = planes(name)
    pc = push_constants(name, frame)
    cam = camera(c["scene"], W, H)
    old = old_accum(name) if pc.frame > 0 else None
    acc, cnt = orc.hybrid(pc, cam, W, H, g, seed=c["seed"], flags=c["row_major"], accum=None if old is None else old.copy(), use_bvh=use_bvh)
    acc2, rad = orc.hybrid_nrd(pc, cam, W, H, g, seed=c["seed"], flags=c["row_major"], accum=None if old is None else old.copy(), use_bvh=use_bvh)
    assert np.array_equal(bits(acc), bits(acc2)), name  # the two entry points of the oracle are one function
    return dict(accum=acc, rad=rad, counters=cnt)


@functools.lru_cache(maxsize=None)
def planes(name):
    return make_planes(name)


def reference(name, dissolve=False):
    return _reference(name, bool(dissolve))


@functools.lru_cache(maxsize=None)
def _reference(name, dissolve):
    """planes, meta and the oracle's answer (tree walk; tests/test_hybrid_planes.py shows brute force gives the same words on Cornell),
    computed once and shared read-only: dict g, meta, shaded, gi (where GI ran), accum, rad, counters"""
    g, meta = planes(name)
    r = oracle_run(name, dissolve=dissolve)
    sh = shaded_mask(g)
    return dict(g=g, meta=meta, shaded=sh, gi=sh & (CASES[name]["toggles"][2] == 1), **r)


def by_kind(mask, meta):
    """{kind name: pixels of mask} without the zeros"""
    return {KINDS[k]: int((mask & (meta["kind"] == k)).sum()) for k in range(len(KINDS)) if (mask & (meta["kind"] == k)).any()}


def half_neighbours(a, b):
    """a, b binary16-representable float32 values: equal, or adjacent binary16 values (same sign or across zero)"""
    ha, hb = np.asarray(a, F).astype(np.float16).view(np.int16).astype(np.int32), np.asarray(b, F).astype(np.float16).view(np.int16).astype(np.int32)
    ka, kb = np.where(ha < 0, -(ha & 0x7FFF), ha), np.where(hb < 0, -(hb & 0x7FFF), hb)
    return np.abs(ka - kb) <= 1


# ---- k_post / oracle_py.post ---------------------------------------------------------------------------------------------------------
def post_inputs(n):
    """(main, rt) [n, 4] float32: zeros, negatives, infinities and values up to 1e4"""
    rng = np.random.default_rng(77)
    pool = np.concatenate([[0.0, -0.0, 1.0, 1e4, np.inf, -np.inf, -1.0, -1e-3, 0.5, 2.2, 1e-30, 65504.0], rng.uniform(0, 1, 40), rng.uniform(0, 1e4, 20),
                           -rng.uniform(0, 3, 8)]).astype(F)
    m, r = pool[rng.integers(0, len(pool), (n, 4))], pool[rng.integers(0, len(pool), (n, 4))]
    m[0], r[0] = 0.0, 0.0  # (a texel that is zero on every arm)
    return m, r


POST_ARMS = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 1, 1)]  # (rtMode, viewAccumulated, useGI): post.frag's six arms


def post_float64(m, r, rt_mode, view_accumulated, use_gi):
    """post.frag:36-58 with the composite in binary32 (one rounding per operation, as both sides do) and the gamma in float64"""
    m, r = np.asarray(m, F).copy(), np.asarray(r, F)
    with np.errstate(invalid="ignore", over="ignore"):
        if rt_mode == 0:
            if view_accumulated == 0:
                m = np.concatenate([(m[:, :3] * r[:, 3:4]).astype(F) + r[:, :3], np.ones((m.shape[0], 1), F)], 1).astype(F)
            elif use_gi == 1:
                m[:, :3] = (r[:, :3] * r[:, 3:4]).astype(F)
            else:
                m[:, :3] = r[:, 3:4]
        return np.power(m.astype(np.float64), 1.0 / 2.2)


def assert_post(out, want):
    """2e-5 relative + 1e-6 absolute (the bar of tests/test_hybrid.py), NaN at exactly the reference's texels, infinities equal"""
    out = np.asarray(out, np.float64)
    assert np.array_equal(np.isnan(out), np.isnan(want))
    fin = np.isfinite(want)
    assert np.array_equal(out[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    assert np.all(np.abs(out[fin] - want[fin]) <= 2e-5 * np.abs(want[fin]) + 1e-6)
