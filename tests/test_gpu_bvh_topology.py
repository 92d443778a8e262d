"""The trees the device builders install against the exact host restatement of their algorithms (tests/np_bvh_build.py, whose own witnesses
are in tests/test_np_bvh_build.py).  vkrt_debug_check_accel proves a tree sound and tests/test_gpu_bvh_bounds.py proves its boxes exact for
whatever topology was installed; the images do not depend on the tree.  So a builder that sorts on 20 bits, splits one position off,
searches a shorter window or collapses short of its optimum passes all of that and only loses a few percent of ray rate.  Here the order of
the leaves, every node of the binary trees and the structure and cost of the wide trees must be what the algorithms give.

The scenes are built with VKRT_OPT_SPLIT_BUDGET = 0; `grid8` and `rotated_small` run with a budget of 30 as well: the leaves are then the
references vkrt_debug_split_references shows, with their clipped boxes (held to the restated splitter in tests/test_gpu_split_refs.py),
their keys taken inside the scene bounds of the whole triangles.  The host `sah` builder is not part of the wide checks: the BVH2 it installs has leaves of up to 4 triangles, the tree its collapse consumes is a second build with one triangle
per leaf, which no entry point shows."""
import os
import sys

import numpy as np
import pytest

import np_bvh
import np_bvh_build as nb
from scene_motion import _col_major
from test_gpu_bvh_bounds import _options, _soup, _triangle_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SOUP_SIZES = (2, 3, 5, 255, 256, 257, 513, 1000)  # the workgroup (256) and window (16) borders of k_ploc_nn
SMALL = tuple(f"soup{n}" for n in SOUP_SIZES) + ("pile", "line", "soup_far", "cornell")
BVH2_STACK_WORDS = 64  # per lane: a BVH2 deeper than 62 is refused at install (VKRT_ERR_UNSUPPORTED)
LARGE = ("soup4200", "atrium_small")  # above 4096 triangles: the upper-level pass, on its full-sweep path and on its binned path
SCENES = SMALL + LARGE
SPLIT = ("grid8", "rotated_small")  # the scenes that also run pre-split, budget 30
CASES = [(n, 0) for n in SCENES] + [(n, 30) for n in SPLIT]
IDS = list(SCENES) + [f"{n}-split30" for n in SPLIT]


@pytest.fixture(scope="module")
def scenes():
    import atrium
    from vkrt_amd.flat_scene import FlatScene

    out = {f"soup{n}": _triangle_scene(_soup(n)) for n in SOUP_SIZES + (4200,)}
    out["pile"] = _triangle_scene(np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), (600, 1)))  # all codes tie
    line = np.zeros((3 * 8, 3), np.float32)  # a root box of zero extent on two axes
    line[:, 0] = np.arange(3 * 8) * 0.25
    out["line"] = _triangle_scene(line)
    far = np.diag([1e-4, 1e-4, 1e-4, 1.0])  # 2 mm of soup at 1e5: many centres share a cell
    far[:3, 3] = 1e5
    out["soup_far"] = _triangle_scene(_soup(1000), _col_major(far))
    out["cornell"] = FlatScene.load_npz(os.path.join(ROOT, "tests", "golden", "cornell_flat.npz"))
    out["atrium_small"], _ = atrium.build_atrium(20000, seed=4, with_textures=False)
    from test_gpu_split_refs import flat_scene

    for n in SPLIT:
        out[n] = flat_scene(n)
    return out


def _build(flat, kind, layout, budget=0):
    from vkrt_amd.renderer import Renderer

    r = Renderer(flat, device=0, build=kind, options=_options(layout, 0, budget))
    a = r.read_accel()
    a["ids"] = r.read_triangle_ids()
    a["info"] = r.accel_info()
    if budget:
        a["refs"] = r.split_references(budget)
    r.close()
    assert a["layout"] == (1 if layout == "wide8" else 0)
    return a


class Restated:
    """One scene: the device's BVH2 builds (read once) and everything the restatement derives from the installed records."""

    def __init__(self, name, flat, budget=0):
        self.name, self.flat, self.budget = name, flat, budget
        self.device = {}
        self.trees = {}
        a = self.built("lbvh", "bvh2")
        ids = a["ids"].astype(np.int64)
        rlo, rhi = np_bvh.record_bounds(a["tris"], 0)  # per slot
        if budget == 0:
            self.T = T = ids.size
            assert T == flat.instanced_triangle_count and np.array_equal(np.sort(ids), np.arange(T)), f"{name}: slot ids are not a permutation"
            self.lo, self.hi = np.zeros((T, 3), np.float32), np.zeros((T, 3), np.float32)
            self.lo[ids], self.hi[ids] = rlo, rhi  # back to the order of the flattened ids
            self.tri_of = np.arange(T)
            self.bounds = nb.scene_bounds(self.lo, self.hi)
            self.keys = nb.morton_keys(self.lo, self.hi)
        else:  # the leaves are the references of the pre-split stage, in emission order, with their clipped boxes
            d = a["refs"]
            self.T = T = d["ref_count"]
            assert T == ids.size == a["info"]["reference_count"] > flat.instanced_triangle_count, f"{name}: {T} references, {ids.size} slots"
            self.lo, self.hi = np.ascontiguousarray(d["ref_box"][:, 0:3]), np.ascontiguousarray(d["ref_box"][:, 3:6])
            self.tri_of = d["ref_tri"].astype(np.int64)
            self.bounds = nb.scene_bounds(rlo, rhi)  # of the whole triangles: every triangle owns a slot
            self.keys = nb.morton_keys(self.lo, self.hi, *self.bounds)
        self.order = nb.sorted_order(self.keys)
        self.slot_ids = self.tri_of[self.order]  # the triangle every leaf position holds
        self.slo, self.shi = self.lo[self.order], self.hi[self.order]  # leaf boxes by position

    def built(self, kind, layout, metric=None, monkeypatch=None):
        """The installed tree of one build (read once per module).  metric: the merge cost of the clustering, through the library's
        VKRT_PLOC_METRIC hook, set for the build alone."""
        key = (kind, layout, metric)
        if key not in self.device:
            if metric is not None:
                monkeypatch.setenv("VKRT_PLOC_METRIC", str(metric))
            try:
                self.device[key] = _build(self.flat, kind, layout, self.budget)
            finally:
                if metric is not None:
                    monkeypatch.delenv("VKRT_PLOC_METRIC")
        return self.device[key]

    def tree(self, kind, metric=2):
        """The binary hierarchy (unit leaves) of a builder, boxes included."""
        key = (kind, metric)
        if key not in self.trees:
            if kind == "lbvh":
                h = nb.fit_boxes(nb.karras(self.keys[self.order]), self.slo, self.shi)
                F = 0
            else:
                h = nb.ploc(self.slo, self.shi, metric)
                F = 0
                if self.T > nb.TOP_MIN_TRIANGLES:
                    h, F = nb.top_levels_sah(h, self.slo, self.shi)
            nb.check_hierarchy(h, self.T)
            h["frontier"] = F
            self.trees[key] = h
        return self.trees[key]


@pytest.fixture(scope="module")
def restated(scenes):
    cache = {}

    def get(name, budget=0):
        if (name, budget) not in cache:
            cache[name, budget] = Restated(name, scenes[name], budget)
        return cache[name, budget]

    return get


def _assert_same_bvh2(a, root, refs, what):
    """Every node a walk from root_ref reaches holds the restated pair of references; the reached set is the restated set."""
    assert a["root_ref"] == root, f"{what}: root reference {a['root_ref']}, restated {root}"
    _, dev = np_bvh.decode_bvh2(a["nodes"])
    levels = np_bvh.bvh2_levels(dev, a["root_ref"])
    reached = np.sort(np.concatenate(levels)) if levels else np.zeros(0, np.int64)
    want = np.array(sorted(refs), np.int64)
    if not np.array_equal(reached, want):
        raise AssertionError(f"{what}: {reached.size} nodes reached, {want.size} restated; only on the device "
                             f"{np.setdiff1d(reached, want)[:8].tolist()}, only restated {np.setdiff1d(want, reached)[:8].tolist()}")
    exp = np.array([refs[int(n)] for n in want], np.int64).reshape(-1, 2)
    bad = np.flatnonzero((dev[want] != exp).any(axis=1))
    assert bad.size == 0, (f"{what}: {bad.size} of {want.size} nodes differ, first node {int(want[bad[0]])}: device "
                           f"{dev[want[bad[0]]].tolist()}, restated {exp[bad[0]].tolist()}")


@pytest.mark.parametrize("name,budget", CASES, ids=IDS)
def test_leaf_order_is_the_stable_morton_sort(restated, name, budget):
    """lbvh and ploc, BVH2: slot k holds the k-th triangle of the stable sort of (63-bit key, flattened id) -- pre-split: the triangle of
    the k-th reference of the stable sort of (key, reference number)."""
    s = restated(name, budget)
    k = s.keys[s.order]
    assert np.all(k[1:] >= k[:-1]) and np.all((k[1:] > k[:-1]) | (s.order[1:] > s.order[:-1]))
    for kind in ("lbvh", "ploc"):
        ids = s.built(kind, "bvh2")["ids"].astype(np.int64)
        bad = np.flatnonzero(ids != s.slot_ids)
        assert bad.size == 0, (f"{name} {kind}: {bad.size} of {s.T} slots differ, first slot {int(bad[0])}: device id {int(ids[bad[0]])}" +
                               (f" (key {int(s.keys[ids[bad[0]]]):#x})" if budget == 0 else "") +
                               f", restated id {int(s.slot_ids[bad[0]])} (key {int(s.keys[s.order[bad[0]]]):#x})")
    if name in ("pile", "soup_far"):
        assert np.unique(s.keys).size < s.T // 2, f"{name}: the scene is here for its tied keys"
    if name == "pile":
        assert np.array_equal(s.order, np.arange(s.T))


@pytest.mark.parametrize("name,budget", CASES, ids=IDS)
def test_lbvh_is_the_karras_tree(restated, name, budget):
    """BVH2 layout: the radix tree with position tie-breaks, subtrees of <= 4 triangles as leaves ~((first << 3) | (count - 1))."""
    s = restated(name, budget)
    root, refs = nb.emit(s.tree("lbvh"), s.T, 4)
    _assert_same_bvh2(s.built("lbvh", "bvh2"), root, refs, f"{name} lbvh")


@pytest.mark.parametrize("name,budget", CASES, ids=IDS)
def test_ploc_is_the_restated_clustering(restated, name, budget, monkeypatch):
    """BVH2 layout, one triangle per leaf.  Up to 1000 triangles: the pure clustering under all three merge costs (T = 257 also with
    the hook that makes every search pass barren).  Above 4096: the default cost with the SAH pass over the upper levels."""
    from vkrt_amd.renderer import VkrtError

    s = restated(name, budget)
    metrics = (2,) if s.T > nb.TOP_MIN_TRIANGLES else (0, 1, 2) + ((98,) if name == "soup257" else ())
    for metric in metrics:
        what = f"{name} ploc metric {metric}"
        hook = None if metric == 2 else metric
        h = s.tree("ploc", metric)
        root, refs = nb.emit(h, s.T, 1)
        depth = nb.depth_of(h)
        if depth + 2 > BVH2_STACK_WORDS:
            # the union-area costs chain clusters; the library does not install a BVH2 its lane stack cannot walk.  The refusal names
            # the depth, which must be the restated one, and the same clustering is held to the restated tree through its collapse
            with pytest.raises(VkrtError, match=rf"\(6\): BVH depth {depth} needs"):
                s.built("ploc", "bvh2", hook, monkeypatch)
            _assert_wide_is_optimal_cut(s, h, s.built("ploc", "wide8", hook, monkeypatch), what + " wide8")
            print(f"{what}: restated depth {depth}, refused as a BVH2, held to the restated tree through its wide8 collapse")
            continue
        a = s.built("ploc", "bvh2", hook, monkeypatch)
        _assert_same_bvh2(a, root, refs, what)
        assert a["info"]["max_depth"] == depth, (what, a["info"]["max_depth"], depth)
        assert np.array_equal(a["ids"], s.slot_ids), f"{name} ploc metric {metric}: leaf order"
    if name in LARGE and budget == 0:  # (also asserted on the CPU, on boxes without slop: tests/test_np_bvh_build.py)
        F = s.tree("ploc")["frontier"]
        assert (F > nb.TOP_SWEEP_MAX) == (name == "atrium_small") and F >= 2, (name, F)


def _wide_against_binary(a, s, h, what):
    """The wide tree's children as leaf sets of the binary hierarchy h.  Returns (SAH sum of the wide tree on h's boxes in float64,
    the wide tree as nb.collapse_cuts writes one: {binary node of a wide node: (sorted child references, sorted leaf-child references)})."""
    T = s.T
    d = np_bvh.decode_wide8(a["nodes"])
    levels = np_bvh.wide8_levels(d)
    assert sum(l.size for l in levels) == a["nodes"].shape[0] == a["info"]["node_count"], what
    ids = a["ids"].astype(np.int64)
    if s.budget == 0:
        assert ids.size == T and np.array_equal(np.sort(ids), np.arange(T)), f"{what}: a triangle is missing or repeated among the slots"
    else:  # the slots of a triangle hold the same record: which of its references each one is, from the leaf boxes (np_bvh.slot_references)
        ids = np_bvh.slot_references(a, ids, s.tri_of, s.lo, s.hi, *s.bounds)
    pos_of = np.empty(T, np.int64)
    pos_of[s.order] = np.arange(T)
    pos = pos_of[ids]  # leaf position of every wide-tree slot
    # the leaf set of a node as (sum of two random 64-bit words per leaf, count): equal sets give equal keys, and 128 random bits keep
    # unequal ones apart
    rng = np.random.default_rng(1234)
    word = rng.integers(0, 1 << 63, (T, 2), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    ch = h["children"]
    hsum = np.zeros((T - 1, 2), np.uint64)
    for lvl in reversed(nb.levels_of(ch)):
        for c in range(2):
            r = ch[lvl, c]
            hsum[lvl] += np.where((r < 0)[:, None], word[np.where(r < 0, ~r, 0)], hsum[np.maximum(r, 0)])
    area_n = np_bvh.area64(h["lo"], h["hi"])
    area_l = np_bvh.area64(s.slo, s.shi)
    lookup = {(int(hsum[n, 0]), int(hsum[n, 1]), int(h["count"][n])): (n, float(area_n[n])) for n in range(T - 1)}
    assert len(lookup) == T - 1
    for p in range(T):
        lookup[(int(word[p, 0]), int(word[p, 1]), 1)] = (~p, float(area_l[p]))
    assert len(lookup) == 2 * T - 1
    # slot sets of the wide tree, bottom-up
    N = a["nodes"].shape[0]
    slot_sum = np.zeros((N, 8, 2), np.uint64)
    slot_cnt = np.zeros((N, 8), np.int64)
    seen = np.zeros(T, np.int64)
    for idx in reversed(levels):
        leaf, cnt, first = np_bvh._leaf_slots(d, idx)
        assert cnt.max() <= 3, f"{what}: a leaf child of {int(cnt.max())} triangles"
        im = d["imask"][idx]
        for sl in range(8):
            internal = ((im >> sl) & 1).astype(bool)
            child = d["childBase"][idx] + np_bvh._popcount(im & ((1 << sl) - 1))
            acc = np.zeros((idx.size, 2), np.uint64)
            acc[internal] = slot_sum[child[internal]].sum(axis=1, dtype=np.uint64)
            n = np.where(internal, 0, cnt[:, sl])
            n[internal] = slot_cnt[child[internal]].sum(axis=1)
            for k in range(3):
                use = leaf[:, sl] & (cnt[:, sl] > k)
                t = first[use, sl] + k
                assert t.size == 0 or t.max() < T, f"{what}: leaf slot outside the triangle records"
                acc[use] += word[pos[t]]
                np.add.at(seen, t, 1)
            slot_sum[idx, sl] = acc
            slot_cnt[idx, sl] = n
    assert np.all(seen == 1), f"{what}: {int((seen != 1).sum())} triangle slots are not in exactly one leaf child"
    # the root stands for the binary root; every child for one node of the binary tree (so an internal child's own children partition
    # that node's set: their sum is its key, and every triangle is in one leaf only)
    root_key = (int(slot_sum[0].sum(axis=0, dtype=np.uint64)[0]), int(slot_sum[0].sum(axis=0, dtype=np.uint64)[1]), int(slot_cnt[0].sum()))
    assert root_key == (int(hsum[0, 0]), int(hsum[0, 1]), T), f"{what}: the root's children do not partition the scene"
    total = float(area_n[0])
    occ = d["meta"] != 0
    internal = ((d["imask"][:, None] >> np.arange(8)) & 1).astype(bool)
    stands_for = np.zeros(N, np.int64)  # (node 0: the binary root)
    kids = [([], []) for _ in range(N)]
    for n, sl in np.argwhere(occ):  # (ascending n: a node's parent comes before it, the numbering is breadth-first)
        key = (int(slot_sum[n, sl, 0]), int(slot_sum[n, sl, 1]), int(slot_cnt[n, sl]))
        assert key in lookup, f"{what}: child {int(sl)} of wide node {int(n)} ({key[2]} triangles) is no node of the binary tree"
        ref, area = lookup[key]
        total += area * (1 if internal[n, sl] else key[2])
        kids[n][0].append(ref)
        if internal[n, sl]:
            stands_for[d["childBase"][n] + np_bvh._popcount(d["imask"][n] & ((1 << int(sl)) - 1))] = ref
        else:
            kids[n][1].append(ref)
    cuts = {int(stands_for[n]): (tuple(sorted(kids[n][0])), tuple(sorted(kids[n][1]))) for n in range(N)}
    assert len(cuts) == N, what
    return total, cuts


@pytest.mark.parametrize("kind", ["lbvh", "ploc"])
@pytest.mark.parametrize("name,budget", CASES, ids=IDS)
def test_wide_collapse_cuts_the_binary_tree_at_its_optimum(restated, name, budget, kind):
    """wide8 layout.  Structure: every child of every wide node holds the leaf set of one node of the restated binary tree, the
    children of a node partition the node they came from, no leaf child holds more than 3 triangles, each triangle appears once.
    Optimum: the float64 SAH sum of the wide tree on the binary tree's float32 boxes equals the optimum of the recurrences in the header
    of wide_collapse.hip, evaluated in float64, within (3 x depth + 3) x 2^-24: three float32 roundings per level of the device's dynamic
    programme (a sum of two child costs, the area term, the leaf product) and nothing else.
    Choice: among cuts of equal cost the tree is the one the same recurrences give in float32 with the lowest k on equal sums, the leaf
    form when it costs no more, and no extra slot unless strictly cheaper -- wide node for wide node, child for child."""
    s = restated(name, budget)
    _assert_wide_is_optimal_cut(s, s.tree(kind), s.built(kind, "wide8"), f"{name} {kind} wide8")


def _assert_wide_is_optimal_cut(s, h, a, what):
    got, cuts = _wide_against_binary(a, s, h, what)
    N = len(cuts)
    want = nb.collapse_optimum(h, s.slo, s.shi)
    depth = nb.depth_of(h)
    tol = (3 * depth + 3) * 2.0 ** -24
    if want == 0.0:
        assert got == 0.0, f"{what}: cost {got} on a tree whose optimum is 0"
    else:
        ratio = got / want
        assert abs(ratio - 1.0) <= tol, (f"{what}: wide SAH sum {got!r} / optimum {want!r} = {ratio!r}, tolerance {tol:.3e} (binary depth "
                                         f"{depth}, {N} wide nodes)" + (": below the optimum -- the restatement is wrong" if ratio < 1 else ""))
    restated_cuts = nb.collapse_cuts(h, nb.collapse_tables(h, s.slo, s.shi, np.float32))
    if cuts != restated_cuts:
        both = sorted(set(cuts) & set(restated_cuts))
        diff = [n for n in both if cuts[n] != restated_cuts[n]]
        first = f"first at binary node {diff[0]}: device {cuts[diff[0]]}, restated {restated_cuts[diff[0]]}" if diff else "no common node differs"
        raise AssertionError(f"{what}: {N} wide nodes, {len(restated_cuts)} restated, {len(diff)} of the {len(both)} common ones with other "
                             f"children; {first}")


def test_triangle_ids_entry_sizes_and_errors(scenes):
    """vkrt_debug_read_triangle_ids on a live scene: one id per slot in both layouts and for the host builder, exact byte counts only,
    NULL refused, a stale tree refused with VKRT_ERR_NOT_BUILT, and the ids are the records' id words."""
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer, VkrtError

    flat = scenes["cornell"]
    T = flat.instanced_triangle_count
    for kind in ("sah", "lbvh", "ploc"):
        for layout in ("wide8", "bvh2"):
            r = Renderer(flat, device=0, build=kind, options=_options(layout, 0))
            ids = r.read_triangle_ids()
            assert ids.dtype == np.uint32 and np.array_equal(np.sort(ids), np.arange(T)), (kind, layout)
            words = r.read_accel()["tris"].view(np.uint32)[:, 9]
            assert np.array_equal(ids, words & 0x7FFFFFFF), (kind, layout)
            r.close()
    r = Renderer(flat, device=0, build="ploc", options=_options("wide8", 0))
    buf = np.full(T + 2, 7, np.uint32)
    fn = r.lib.vkrt_debug_read_triangle_ids
    for nbytes in (4 * T + 4, 4 * T - 4, 0, 48 * T):
        assert fn(r._h, buf.ctypes.data, nbytes) == abi.VKRT_ERR_INVALID_ARGUMENT, nbytes
        assert b"vkrt_debug_read_triangle_ids" in r.lib.vkrt_last_error()
    assert fn(r._h, None, 4 * T) == abi.VKRT_ERR_INVALID_ARGUMENT and fn(None, buf.ctypes.data, 4 * T) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert np.all(buf == 7)
    assert fn(r._h, buf.ctypes.data, 4 * T) == abi.VKRT_OK and np.all(buf[T:] == 7) and np.array_equal(np.sort(buf[:T]), np.arange(T))
    r.update_nodes(0, np.asarray(flat.nodes[0]["worldMatrix"], np.float32)[None])  # stale until the refit
    assert fn(r._h, buf.ctypes.data, 4 * T) == abi.VKRT_ERR_NOT_BUILT
    with pytest.raises(VkrtError, match=r"\(5\)"):
        r.read_triangle_ids()
    r.refit()
    assert np.array_equal(r.read_triangle_ids(), buf[:T])
    r.close()
