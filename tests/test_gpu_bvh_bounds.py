"""Tree boxes and SAH costs against an exact host recomputation (tests/np_bvh.py).  vkrt_debug_check_accel proves a tree sound -- every
triangle inside its ancestors' boxes -- which a box one cell too loose, or a refit that never shrinks, passes; the images are
tree-independent by design.  Here the installed node words (vkrt_debug_read_accel) must be, bit for bit, what the layout headers' rules
give for the tree's own topology and records, and vkrt_accel_info.sah_cost must be the float64 cost of those boxes: every builder, both
layouts, both triangle tests, after builds and after refits."""
import os
import sys

import numpy as np
import pytest

import np_bvh
from scene_motion import _col_major, _row_major, apply, moved

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KINDS = ("sah", "lbvh", "ploc")
SAH_REL = 2e-6


def _options(layout, wt, split=0):
    from vkrt_amd import abi

    return {abi.VKRT_OPT_BVH_LAYOUT: 1 if layout == "wide8" else 0, abi.VKRT_OPT_WATERTIGHT: wt, abi.VKRT_OPT_SPLIT_BUDGET: split}


def _triangle_scene(pos, world=None):
    """A one-instance FlatScene of the triangles pos [3n, 3] (world: column-major node matrix, default identity)."""
    from vkrt_amd.flat_scene import LIGHT_DTYPE, MAT_DTYPE, NODE_DTYPE, PRIM_DTYPE, FlatScene

    pos = np.ascontiguousarray(pos, np.float32)
    m = pos.shape[0]
    idx = np.arange(m, dtype=np.uint32)
    pm = np.zeros(1, PRIM_DTYPE)
    pm[0] = (0, m, 0, m, 0)
    mats = np.zeros(1, MAT_DTYPE)
    mats[0]["pbrBaseColorFactor"] = [0.8, 0.8, 0.8, 1.0]
    mats[0]["pbrBaseColorTexture"] = mats[0]["metallicRoughnessTexture"] = mats[0]["normalTexture"] = mats[0]["emissiveTexture"] = -1
    mats[0]["roughnessFactor"] = 1.0
    nodes = np.zeros(1, NODE_DTYPE)
    nodes[0]["worldMatrix"] = np.eye(4, dtype=np.float32).ravel() if world is None else world
    lights = np.zeros(1, LIGHT_DTYPE)
    lights[0] = ((0.3, 0.3, 2.0), (1, 1, 1), 10.0, 0)
    return FlatScene(pos, np.tile(np.array([0, 0, 1], np.float32), (m, 1)), np.tile(np.array([1, 0, 0, 1], np.float32), (m, 1)),
                     np.zeros((m, 2), np.float32), idx, pm, mats, lights, nodes, [])


def _soup(n=3000, seed=7):
    """Needles (1 / sin of the corner from 2 to 1e5: the slop is non-zero for most of them), slivers and ordinary triangles."""
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(-10, 10, (n, 3))
    d1 = rng.standard_normal((n, 3))
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    t = rng.standard_normal((n, 3))
    t -= (t * d1).sum(1, keepdims=True) * d1
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    phi = np.arcsin(1.0 / np.exp(rng.uniform(np.log(2.0), np.log(1e5), n)))
    l1, l2 = np.exp(rng.uniform(-3, 2, (2, n)))
    p1 = p0 + l1[:, None] * d1
    p2 = p0 + l2[:, None] * (np.cos(phi)[:, None] * d1 + np.sin(phi)[:, None] * t)
    return np.stack([p0, p1, p2], 1).reshape(-1, 3)


@pytest.fixture(scope="module")
def scenes():
    import atrium
    from vkrt_amd.flat_scene import FlatScene

    cornell = FlatScene.load_npz(os.path.join(ROOT, "tests", "golden", "cornell_flat.npz"))
    atrium_small, _ = atrium.build_atrium(20000, seed=4, with_textures=False)
    soup = _soup()
    far = np.diag([1e-4, 1e-4, 1e-4, 1.0])
    far[:3, 3] = 1e5
    pile = np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), (3000, 1))
    line = np.zeros((3 * 8, 3), np.float32)  # degenerate triangles along the x axis: a root box of zero area (cost 0)
    line[:, 0] = np.arange(3 * 8) * 0.25
    return {"cornell": cornell, "atrium_small": atrium_small, "soup": _triangle_scene(soup), "soup_far": _triangle_scene(soup, _col_major(far)),
            "pile": _triangle_scene(pile), "line": _triangle_scene(line)}


def _same_floats(got, want, what):
    """Bitwise equality of float words; +0 and -0 count as one value (the sign of a zero bound does not change a box, and min / max
    of equal zeros may return either)."""
    g = np.ascontiguousarray(got, np.float32)
    w = np.ascontiguousarray(want, np.float32)
    bad = (g.view(np.uint32) != w.view(np.uint32)) & ~((g == 0) & (w == 0))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first at {np.argwhere(bad)[:4].tolist()}: {g[bad][:4]} vs {w[bad][:4]}"


def _assert_sah(got, want, what):
    assert abs(float(got) - want) <= SAH_REL * abs(want), (what, float(got), want)


def check_exact(r, wt, what, slot_boxes=None):
    """The installed tree is the exact restatement of its topology: leaf boxes = unions of their records' whole-triangle boxes (or of
    slot_boxes = (lo, hi) per slot: the boxes of a pre-split tree's references), nodes quantised by the header's rule (wide8) or stored
    as floats (BVH2), and sah_cost the float64 cost of those boxes.  Returns the tree."""
    a = r.read_accel()
    info = r.accel_info()
    rlo, rhi = np_bvh.record_bounds(a["tris"], wt) if slot_boxes is None else slot_boxes
    if a["layout"] == 1:
        exp, _, _, slo, shi, d = np_bvh.exact_wide8(a["nodes"], rlo, rhi)
        levels = np_bvh.wide8_levels(d)
        assert sum(l.size for l in levels) == a["nodes"].shape[0] == info["node_count"], what
        _same_floats(a["nodes"][:, 0:3].view(np.float32), exp[:, 0:3].view(np.float32), f"{what}: wide8 origins")
        bad = np.argwhere(a["nodes"][:, 3:] != exp[:, 3:])
        assert bad.size == 0, f"{what}: {len(bad)} exponent / plane words differ, first (node, word - 3) {bad[:4].tolist()}"
        want = np_bvh.sah_wide8(a["nodes"], slo, shi, levels)
    else:
        exp, levels = np_bvh.exact_bvh2(a["nodes"], a["root_ref"], rlo, rhi)
        reached = np.concatenate(levels) if levels else np.zeros(0, np.int64)
        if r.build_kind == "sah":  # (device BVH2 arrays also hold the radix nodes inside collapsed leaves)
            assert reached.size == info["node_count"], what
        _same_floats(a["nodes"][reached, 0:12], exp[reached].reshape(-1, 12), f"{what}: BVH2 child boxes")
        want = np_bvh.sah_bvh2(a["nodes"], a["root_ref"], levels=levels)
    _assert_sah(info["sah_cost"], want, what)
    return a, info


def _reached_words(a):
    if a["layout"] == 1:
        return a["nodes"].view(np.uint32)
    _, refs = np_bvh.decode_bvh2(a["nodes"])
    levels = np_bvh.bvh2_levels(refs, a["root_ref"])
    return a["nodes"][np.sort(np.concatenate(levels))].view(np.uint32) if levels else a["nodes"][:0].view(np.uint32)


@pytest.mark.parametrize("name", ["cornell", "atrium_small", "soup", "soup_far", "pile", "line"])
def test_built_boxes_and_cost_are_exact_and_reproducible(scenes, name):
    """Split budget 0, {sah, lbvh, ploc} x {wide8, BVH2} x {Moeller-Trumbore, watertight}: every node word as restated, sah_cost within 2e-6
    of the float64 cost, and a second build of the scene gives the same node words, records and sah_cost bits."""
    from vkrt_amd.renderer import Renderer

    flat = scenes[name]
    for layout in ("wide8", "bvh2"):
        for wt in (0, 1):
            for kind in KINDS:
                what = f"{name} {kind} {layout} wt={wt}"
                r = Renderer(flat, device=0, build=kind, options=_options(layout, wt))
                a, info = check_exact(r, wt, what)
                assert a["layout"] == (1 if layout == "wide8" else 0), what
                r.build(kind)
                b = r.read_accel()
                again = r.accel_info()
                assert b["root_ref"] == a["root_ref"] and np.array_equal(_reached_words(a), _reached_words(b)), f"{what}: node words differ"
                assert np.array_equal(a["tris"].view(np.uint32), b["tris"].view(np.uint32)), f"{what}: records differ"
                assert np.float32(again["sah_cost"]).view(np.uint32) == np.float32(info["sah_cost"]).view(np.uint32), (what, again["sah_cost"],
                                                                                                                        info["sah_cost"])
                r.close()


def test_bench_scene_boxes_and_cost(scenes):
    """The 262 k-triangle bench atrium, device builders, wide8: exact words, exact cost, reproducible cost (the float cost sum of the
    device BVH2 that the collapse starts from used to be an atomic sum in arbitrary order)."""
    import atrium
    from vkrt_amd.renderer import Renderer

    flat, _ = atrium.build_atrium(262144, seed=1, with_textures=False)
    for kind in ("ploc", "lbvh"):
        r = Renderer(flat, device=0, build=kind, options=_options("wide8", 0))
        a, info = check_exact(r, 0, f"bench {kind}")
        r.build(kind)
        b = r.read_accel()
        assert np.array_equal(a["nodes"], b["nodes"]) and np.array_equal(a["tris"].view(np.uint32), b["tris"].view(np.uint32)), kind
        assert r.accel_info()["sah_cost"] == info["sah_cost"], kind
        r.close()
    # the device BVH2 of the same scene (what the automatic split decision compares when VKRT_OPT_BVH_LAYOUT = 0)
    for kind in ("ploc", "lbvh"):
        r = Renderer(flat, device=0, build=kind, options=_options("bvh2", 0))
        _, info = check_exact(r, 0, f"bench {kind} bvh2")
        r.build(kind)
        assert np.float32(r.accel_info()["sah_cost"]).view(np.uint32) == np.float32(info["sah_cost"]).view(np.uint32), kind
        r.close()


def _scaled(flat, nodes, factor):
    """Every node of `nodes` scaled by `factor` about its own centre (boxes must shrink for factor < 1)."""
    import copy

    from scene_motion import _centre

    out = copy.copy(flat)
    out.nodes = flat.nodes.copy()
    mats = {}
    for i in nodes:
        c = _centre(flat, i)
        S = np.diag([factor, factor, factor, 1.0])
        T0, T1 = np.eye(4), np.eye(4)
        T0[:3, 3], T1[:3, 3] = -c, c
        mats[int(i)] = _col_major(T1 @ S @ T0 @ _row_major(flat.nodes[i]["worldMatrix"]))
        out.nodes[i]["worldMatrix"] = mats[int(i)]
    return out, mats


@pytest.mark.parametrize("layout", ["wide8", "bvh2"])
@pytest.mark.parametrize("split", [0, -1])
def test_refit_boxes_and_cost_are_exact(scenes, layout, split):
    """Mirrored and scaled rigid motions, then a scale-down step: after each refit every node is the restatement (leaf boxes = unions of
    their records' whole-triangle boxes, k_rf_w8 / k_rf_b2) and sah_cost its float64 cost.  Moving back and refitting an unsplit tree
    restores the build's words bit for bit."""
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer

    cases = [("cornell", k, wt) for k in KINDS for wt in (0, 1)] + [("atrium_small", k, 0) for k in ("ploc", "lbvh")]
    for name, kind, wt in cases:
        flat = scenes[name]
        what = f"{name} {kind} {layout} split={split} wt={wt}"
        r = Renderer(flat, device=0, build=kind, options=_options(layout, wt, split))
        built = r.read_accel()
        n = len(flat.nodes)
        idx = [n - 2, n - 1] if name == "cornell" else list(np.sort(np.random.default_rng(23).choice(n, n // 3, replace=False)))
        cur, mats = moved(flat, idx, 31)
        apply(r, mats)
        r.refit()
        check_exact(r, wt, what + " moved")
        area0 = np_bvh.area64(*np_bvh.record_bounds(r.read_accel()["tris"], wt)).sum()
        cur, mats = _scaled(cur, idx, 0.5)
        apply(r, mats)
        r.refit()
        a, _ = check_exact(r, wt, what + " scaled down")
        assert np_bvh.area64(*np_bvh.record_bounds(a["tris"], wt)).sum() < area0, what
        apply(r, {int(i): np.asarray(flat.nodes[i]["worldMatrix"], np.float32) for i in idx})
        r.refit()
        back, _ = check_exact(r, wt, what + " moved back")
        if r.get_option(abi.VKRT_INFO_SPLIT_BUDGET) == 0:
            assert np.array_equal(_reached_words(back), _reached_words(built)), f"{what}: moved back, words differ from the build"
            assert np.array_equal(back["tris"].view(np.uint32), built["tris"].view(np.uint32)), what
        r.close()


@pytest.fixture(scope="module")
def rotated_building():
    import atrium

    flat, _ = atrium.build_atrium(60000, seed=3, variant="nonuniform")
    atrium.rotate_scene(flat, dict(atrium.DEFAULT_CAMERA), 35.0, 20.0)
    return flat


@pytest.mark.parametrize("budget", [30, 100])
def test_split_tree_boxes_are_bounded(rotated_building, budget):
    """Pre-split trees before any refit, from the installed words alone: upper bounds -- a leaf child inside the tightest quantisation
    of its records' whole-triangle boxes, an internal child inside the tightest quantisation (on the parent's grid) of its own
    children's decoded boxes -- and sah_cost at most the cost those decoded boxes give (wide8) or the cost of the stored boxes (BVH2,
    float boxes: exact).  The references' clipped boxes themselves are shown by vkrt_debug_split_references: held exactly in
    test_split_tree_boxes_are_exact below, and to the restated splitter in tests/test_gpu_split_refs.py."""
    from vkrt_amd.renderer import Renderer

    for layout in ("wide8", "bvh2"):
        for kind in ("ploc", "lbvh"):
            what = f"rotated {kind} {layout} budget={budget}"
            r = Renderer(rotated_building, device=0, build=kind, options=_options(layout, 0, budget))
            a = r.read_accel()
            info = r.accel_info()
            assert info["reference_count"] > info["triangle_count"], what
            rlo, rhi = np_bvh.record_bounds(a["tris"], 0)
            if a["layout"] == 1:
                _split_wide8(a["nodes"], rlo, rhi, info["sah_cost"], what)
            else:
                _split_bvh2(a, rlo, rhi, info["sah_cost"], what)
            r.close()


@pytest.mark.parametrize("name", ["grid8", "rotated_small"])
def test_split_tree_boxes_are_exact(name):
    """Budget 30, {ploc, lbvh} x {wide8, BVH2}: with the box of every reference in its slot (vkrt_debug_split_references; which reference
    sits in which slot: np_bvh.slot_references) the installed words are those of exact_wide8 / exact_bvh2, word for word, and sah_cost is
    within 2e-6 of the float64 cost of those boxes -- what test_built_boxes_and_cost_are_exact_and_reproducible holds unsplit trees to."""
    from test_gpu_split_refs import flat_scene
    from vkrt_amd.renderer import Renderer

    flat = flat_scene(name)
    for layout in ("wide8", "bvh2"):
        for kind in ("ploc", "lbvh"):
            what = f"{name} {kind} {layout} budget=30"
            r = Renderer(flat, device=0, build=kind, options=_options(layout, 0, 30))
            a = r.read_accel()
            d = r.split_references(30)
            assert r.accel_info()["reference_count"] == d["ref_count"] > r.accel_info()["triangle_count"], what
            wlo, whi = np_bvh.record_bounds(a["tris"], 0)  # every triangle owns a slot: the scene bounds of the whole triangles
            ref = np_bvh.slot_references(a, r.read_triangle_ids(), d["ref_tri"], d["ref_box"][:, 0:3], d["ref_box"][:, 3:6], wlo.min(axis=0),
                                         whi.max(axis=0))
            box = d["ref_box"][ref]
            assert np.all(box[:, 0:3] >= wlo) and np.all(box[:, 3:6] <= whi), f"{what}: a reference's box outside its triangle's"
            check_exact(r, 0, what, (np.ascontiguousarray(box[:, 0:3]), np.ascontiguousarray(box[:, 3:6])))
            r.close()


def _split_wide8(nodes, rlo, rhi, sah_cost, what):
    d = np_bvh.decode_wide8(nodes)
    levels = np_bvh.wide8_levels(d)
    dlo, dhi = np_bvh.decoded_wide8_boxes(d)  # [N, 8, 3] float64
    occ = d["meta"] != 0
    ulo = np.where(occ[:, :, None], dlo, np.inf).min(axis=1)  # union of each node's decoded slots
    uhi = np.where(occ[:, :, None], dhi, -np.inf).max(axis=1)
    reached = np.concatenate(levels)
    leaf, cnt, first = np_bvh._leaf_slots(d, reached)
    im = d["imask"][reached]
    for s in range(8):
        blo = np.full((reached.size, 3), np.inf)
        bhi = np.full((reached.size, 3), -np.inf)
        internal = ((im >> s) & 1).astype(bool)
        child = d["childBase"][reached] + np_bvh._popcount(im & ((1 << s) - 1))
        blo[internal], bhi[internal] = ulo[child[internal]], uhi[child[internal]]
        for k in range(3):
            use = leaf[:, s] & (cnt[:, s] > k)
            blo[use] = np.minimum(blo[use], rlo[first[use, s] + k])
            bhi[use] = np.maximum(bhi[use], rhi[first[use, s] + k])
        on = occ[reached, s]
        ql, qh = np_bvh.quantise_on_grid(d["origin"][reached][on], d["eb"][reached][on], blo[on], bhi[on])
        assert np.all(d["qlo"][reached[on], :, s] >= ql) and np.all(d["qhi"][reached[on], :, s] <= qh), (
            what, s, int((d["qlo"][reached[on], :, s] < ql).sum()), int((d["qhi"][reached[on], :, s] > qh).sum()))
    # cost: decoded boxes contain the float boxes (larger numerator); the root's float box is at least (origin, the largest slot hi minus
    # one cell) -- the smallest box the root's words allow
    sc = np.ldexp(1.0, d["eb"][0] - 127)
    o = d["origin"][0].astype(np.float64)
    hi_min = (o[None, :] + np.maximum(d["qhi"][0].T - 1, 0) * sc[None, :])[occ[0]].max(axis=0)
    bound = np_bvh.sah_wide8(nodes, dlo, dhi, levels, root_area=np_bvh.area64(o, hi_min))
    assert float(sah_cost) <= bound * (1 + SAH_REL), (what, float(sah_cost), bound)


def _split_bvh2(a, rlo, rhi, sah_cost, what):
    box, refs = np_bvh.decode_bvh2(a["nodes"])
    levels = np_bvh.bvh2_levels(refs, a["root_ref"])
    reached = np.concatenate(levels)
    for c in range(2):
        r = refs[reached, c]
        got = box[reached, c]
        blo = np.full((reached.size, 3), np.inf, np.float32)
        bhi = np.full((reached.size, 3), -np.inf, np.float32)
        internal = r >= 0
        ch = box[r[internal]]
        blo[internal] = np.minimum(ch[:, 0, 0:3], ch[:, 1, 0:3])
        bhi[internal] = np.maximum(ch[:, 0, 3:6], ch[:, 1, 3:6])
        f, n = np_bvh.leaf_code(r)
        for k in range(8):
            use = ~internal & (n > k)
            blo[use] = np.minimum(blo[use], rlo[f[use] + k])
            bhi[use] = np.maximum(bhi[use], rhi[f[use] + k])
        assert np.all(got[:, 0:3] >= blo) and np.all(got[:, 3:6] <= bhi), (what, c)
    _assert_sah(sah_cost, np_bvh.sah_bvh2(a["nodes"], a["root_ref"], levels=levels), what)
