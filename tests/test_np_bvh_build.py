"""Witnesses of tests/np_bvh_build.py, the restatement that tests/test_gpu_bvh_topology.py holds the device builders to: every vectorised
piece against the plainest statement of its rule (a recursion, a scalar loop, an enumeration), on inputs small enough to enumerate."""
import os
import sys
import time

import numpy as np
import pytest

import np_bvh_build as nb

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _random_boxes(rng, n, size=(0.01, 1.0), span=10.0):
    lo = rng.uniform(-span, span, (n, 3)).astype(F32)
    hi = (lo + np.exp(rng.uniform(np.log(size[0]), np.log(size[1]), (n, 3))).astype(F32)).astype(F32)
    return lo, hi


def _same_tree(a, b, what):
    for k in ("children", "count"):
        assert np.array_equal(a[k], b[k]), (what, k, np.argwhere(a[k] != b[k])[:4].tolist())
    for k in ("lo", "hi"):
        if k in a and k in b:
            assert np.array_equal(a[k], b[k]), (what, k)


def test_morton_keys_interleave_21_bits_x_lowest():
    lo = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [0.5, 0.25, 0.75]], F32)
    cells = nb.morton_cells(lo, lo, lo.min(0), lo.max(0))
    top = 2097151
    assert cells.tolist() == [[0, 0, 0], [top, 0, 0], [0, top, 0], [0, 0, top], [top, top, top], [1 << 20, 1 << 19, 3 << 19]]
    keys = nb.morton_keys(lo, lo)
    every = sum(1 << (3 * b) for b in range(21))
    assert [int(k) for k in keys[:5]] == [0, every, every << 1, every << 2, (1 << 63) - 1]
    assert int(keys[5]) == (1 << 60) | (1 << 58) | (1 << 62) | (1 << 59)  # x: bit 20 -> 60; y: bit 19 -> 58; z: bits 20, 19 -> 62, 59
    # an axis without extent gives cell 0, whatever the centre
    flat = np.array([[3, 5, 1], [3, 6, 2]], F32)
    assert nb.morton_cells(flat, flat, flat.min(0), flat.max(0))[:, 0].tolist() == [0, 0]
    # ties keep the order of the flattened ids
    assert nb.sorted_order(np.array([5, 1, 5, 1, 0], np.uint64)).tolist() == [4, 1, 3, 0, 2]


@pytest.mark.parametrize("distinct", [1, 3, 40, 1 << 62])
def test_karras_is_the_recursive_radix_tree(distinct):
    """T = 2 .. 300, keys with many duplicates (one distinct key: every split is decided by position alone)."""
    rng = np.random.default_rng(distinct % 1000)
    for T in range(2, 301):
        keys = np.sort(rng.integers(0, distinct, T, dtype=np.uint64) << np.uint64(int(rng.integers(0, 2)) * 20))
        a, b = nb.karras(keys), nb.karras_recursive(keys)
        for k in ("children", "count", "first"):
            assert np.array_equal(a[k], b[k]), (T, k)
        nb.check_hierarchy(a, T)
        # a subtree is a run of positions: what lets k_emit write a collapsed leaf as (first, count)
        root, refs = nb.emit(a, T, 4)
        got = sorted(p for r in ([root] if root < 0 else [x for pair in refs.values() for x in pair if x < 0])
                     for p in range((~r) >> 3, ((~r) >> 3) + ((~r) & 7) + 1))
        assert got == list(range(T)), T


def _ploc_cases():
    rng = np.random.default_rng(5)
    cases = {}
    for T in (2, 3, 17, 33, 34, 200):
        cases[f"random{T}"] = _random_boxes(rng, T)
    pile = (np.zeros((151, 3), F32), np.ones((151, 3), F32))
    cases["pile"] = pile
    n = 200  # areas from 1e-6 to 1e6 side by side: the cancellation the forced pass exists for
    lo = rng.uniform(-1, 1, (n, 3)).astype(F32)
    hi = (lo + np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (n, 1))).astype(F32)).astype(F32)
    cases["wide_range"] = (lo, hi)
    return cases


@pytest.mark.parametrize("metric", [0, 1, 2, 98])
def test_vectorised_ploc_is_the_scalar_loop(metric):
    for name, (lo, hi) in _ploc_cases().items():
        a, b = nb.ploc(lo, hi, metric), nb.ploc_scalar(lo, hi, metric)
        _same_tree(a, b, (name, metric))
        assert a["passes"] == b["passes"], name
        T = lo.shape[0]
        nb.check_hierarchy(a, T)
        if name == "pile" and metric != 98:
            assert a["passes"][0] == (T, T // 2, False), a["passes"][0]  # every i / i ^ 1 pair merges at once
        if metric == 98:
            assert all(p[2] == (k % 2 == 1) and (p[1] > 0) == p[2] for k, p in enumerate(a["passes"])), a["passes"]
        # boxes are the unions, ids go down from T - 2 pass by pass
        fit = nb.fit_boxes({"children": a["children"]}, lo, hi)
        assert np.array_equal(fit["lo"], a["lo"]) and np.array_equal(fit["hi"], a["hi"]), name


def test_ploc_pass_without_a_mutual_pair_is_followed_by_a_forced_pass():
    """Boxes with areas from 1e-6 to 1e6 under the area-increase cost (not symmetric in i and j): a pass in which nobody's pick picks
    back.  The next pass pairs neighbours, and the search resumes after it."""
    n = 200
    rng = np.random.default_rng(1)
    lo = rng.uniform(-1, 1, (n, 3)).astype(F32)
    hi = (lo + np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (n, 1))).astype(F32)).astype(F32)
    h = nb.ploc(lo, hi, 1)
    nb.check_hierarchy(h, n)
    _same_tree(h, nb.ploc_scalar(lo, hi, 1), "wide range")
    barren = [k for k, p in enumerate(h["passes"]) if p[1] == 0]
    assert barren and all(h["passes"][k + 1] == (h["passes"][k][0], h["passes"][k][0] // 2, True) for k in barren), h["passes"]
    assert not h["passes"][barren[0] + 2][2]
    # the hook makes every search pass barren, whatever the boxes
    h = nb.ploc(lo, hi, 98)
    assert h["passes"][0] == (n, 0, False) and h["passes"][1] == (n, n // 2, True)


def _random_binary_tree(rng, leaves):
    """A random hierarchy over `leaves` leaves with ids as the library numbers them (0 the root)."""
    items = [~p for p in range(leaves)]
    rng.shuffle(items)
    children = np.zeros((leaves - 1, 2), np.int64)
    nid = leaves - 2
    while len(items) > 1:
        k = int(rng.integers(0, len(items) - 1))
        children[nid] = (items[k], items[k + 1])
        items[k:k + 2] = [nid]
        nid -= 1
    h = {"children": children, "first": np.full(leaves - 1, -1, np.int64)}
    lv = nb.levels_of(children)
    cnt = np.zeros(leaves - 1, np.int64)
    for lvl in reversed(lv):
        r = children[lvl]
        cnt[lvl] = np.where(r < 0, 1, cnt[np.maximum(r, 0)]).sum(axis=1)
    h["count"] = cnt
    return h


def _brute_optimum(h, leaf_lo, leaf_hi):
    """Every wide tree the binary tree allows, by enumeration of the cuts below every node."""
    ch, cnt = h["children"], h["count"]
    area = 2.0 * nb._half_area(h["lo"].astype(np.float64), h["hi"].astype(np.float64))
    larea = 2.0 * nb._half_area(leaf_lo.astype(np.float64), leaf_hi.astype(np.float64))

    def cuts(r):  # all antichains that cover the subtree of reference r
        if r < 0:
            return [(r,)]
        return [(r,)] + [a + b for a in cuts(int(ch[r, 0])) for b in cuts(int(ch[r, 1]))]

    def as_node(r):  # r's subtree under a wide node of its own
        return area[r] + min(sum(child(c) for c in cut) for cut in cuts(r) if 2 <= len(cut) <= 8)

    def child(r):  # the cheapest child of a wide node that covers r's subtree: a leaf of <= 3 triangles or a wide node
        if r < 0:
            return larea[~r]
        return min(area[r] * cnt[r] if cnt[r] <= 3 else np.inf, as_node(r))

    leaf = area[0] * cnt[0] if cnt[0] <= 3 else np.inf
    return area[0] + leaf if leaf <= as_node(0) else as_node(0)


def test_collapse_recurrences_reach_the_enumerated_optimum():
    rng = np.random.default_rng(11)
    for leaves in list(range(2, 13)) * 3:
        h = _random_binary_tree(rng, leaves)
        lo, hi = _random_boxes(rng, leaves, size=(0.05, 3.0), span=3.0)
        nb.fit_boxes(h, lo, hi)
        nb.check_hierarchy(h, leaves)
        got, want = nb.collapse_optimum(h, lo, hi), _brute_optimum(h, lo, hi)
        assert abs(got - want) <= 1e-12 * want, (leaves, got, want)
        # the tree read off the tables is a tree over every leaf, and it costs what the tables promise -- in float32 tables as well
        for dtype in (np.float64, np.float32):
            t = nb.collapse_tables(h, lo, hi, dtype)
            assert t["C"].dtype == dtype
            cuts = nb.collapse_cuts(h, t)
            cost, seen = 0.0, []
            for root, (kids, leaf_kids) in cuts.items():
                assert (len(kids) <= 8 and set(leaf_kids) <= set(kids) and all(k in cuts for k in kids if k not in leaf_kids)) or leaves <= 3
                cost += float(t["area"][root])
                for k in leaf_kids:
                    n = 1 if k < 0 else int(h["count"][k])
                    assert n <= 3
                    cost += float(t["leaf_area"][~k] if k < 0 else t["area"][k]) * n
                    seen += _leaves_below(h, k)
            assert sorted(seen) == list(range(leaves))
            promised = float(t["area"][0] + t["C"][0, 1]) if t["leaf_form"][0] else float(t["C"][0, 1])
            assert abs(cost - promised) <= (1e-12 if dtype is np.float64 else 40 * 2.0 ** -24) * promised, (leaves, dtype, cost, promised)
    # more than 8 leaves under the root of a comb: the optimum needs a second wide node
    h = _random_binary_tree(np.random.default_rng(1), 12)
    lo, hi = _random_boxes(rng, 12)
    nb.fit_boxes(h, lo, hi)
    t = nb.collapse_tables(h, lo, hi)
    assert not t["leaf_form"][0] and t["C"][0, 1] == t["area"][0] + t["D8"][0] and np.all(np.diff(t["C"][:, 1:], axis=1) <= 0)
    assert len(nb.collapse_cuts(h, t)) >= 2


def test_collapse_ties_take_the_lowest_k_and_the_leaf_form():
    """Eight coincident unit boxes under a balanced tree: sums tie wherever a slot more gains nothing.  Every D(n, j) names the lowest k
    of its minimum, a pair of triangles is a leaf (2 A, against A + 2 A as a node), and the root's cut is what those choices give."""
    ch = np.array([[1, 2], [3, 4], [5, 6], [~0, ~1], [~2, ~3], [~4, ~5], [~6, ~7]], np.int64)
    h = {"children": ch, "count": np.array([8, 4, 4, 2, 2, 2, 2]), "first": np.full(7, -1)}
    lo, hi = np.zeros((8, 3), F32), np.ones((8, 3), F32)
    nb.fit_boxes(h, lo, hi)
    t = nb.collapse_tables(h, lo, hi, np.float32)
    assert t["leaf_form"].tolist() == [False, False, False, True, True, True, True]  # 2 A as a leaf <= A + 2 A as a node
    # D(0, 8): k = 1 gives C(1, 1) + C(2, 7) = 30 + 24, k = 2 .. 6 give 24 + 24: the lowest of them
    assert t["k8"].tolist() == [2, 1, 1, 1, 1, 1, 1] and not t["k"][3:].any()
    # node 1: one slot = a node of its own (A + 4 A); two slots = its two leaf pairs (4 A): strictly cheaper, k = 1; no gain beyond
    assert t["C"][1].tolist()[1:] == [30.0, 24.0, 24.0, 24.0, 24.0, 24.0, 24.0] and t["k"][1].tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    assert nb.collapse_cuts(h, t) == {0: ((3, 4, 5, 6), (3, 4, 5, 6))}


def _leaves_below(h, ref):
    if ref < 0:
        return [~ref]
    return _leaves_below(h, int(h["children"][ref, 0])) + _leaves_below(h, int(h["children"][ref, 1]))


def _brute_sweep(ref, cnt, lo, hi):
    """The best sweep split by trying every (axis, k) with boxes recomputed from scratch, in the order and with the tie rule the pass
    states: a cheaper split wins, an equal one only if nearer the middle."""
    n = ref.size
    best, best_off, best_left = F32(np.inf), abs(1 - n // 2), None
    for axis in range(3):
        order = sorted(range(n), key=lambda e: (float(lo[e, axis] + hi[e, axis]), int(ref[e])))
        if best_left is None:
            best_left = order[:1]
        for k in range(1, n):
            L, R = order[:k], order[k:]
            c = (nb._half_area(lo[L].min(0), hi[L].max(0)) * F32(cnt[L].sum()) + nb._half_area(lo[R].min(0), hi[R].max(0)) * F32(cnt[R].sum()))
            off = abs(k - n // 2)
            if c < best or (c == best and off < best_off):
                best, best_off, best_left = c, off, L
    return best_left


def test_top_builder_sweep_finds_the_best_split():
    rng = np.random.default_rng(3)
    for n in (2, 3, 7, 16, 33, 64):
        for kind in ("random", "grid", "same"):
            lo, hi = _random_boxes(rng, n)
            if kind == "grid":  # many equal centres and equal costs
                lo = np.floor(lo / 4).astype(F32) * 4
                hi = lo + 1
            if kind == "same":
                lo[:], hi[:] = 0, 1
            ref = rng.permutation(np.concatenate([~np.arange(n // 2), np.arange(100, 100 + n - n // 2)])).astype(np.int64)
            ref = np.sort(ref)
            cnt = rng.integers(1, 17, n)
            tb = nb._TopBuilder(ref, cnt, lo, hi, np.arange(n))
            split = tb._sweep(0, n)
            want = _brute_sweep(ref, cnt, lo, hi)
            assert tb.ref[:split].tolist() == [int(ref[e]) for e in want], (n, kind)
            if kind == "same":
                assert split == n // 2  # equal costs must not peel one entry per level


def _world_boxes(flat):
    """Triangle boxes of a FlatScene in flattened order (float64 transform rounded once: near the device's boxes, which is all the
    sizes below need)."""
    lo, hi = [], []
    for node in flat.nodes:
        pm = flat.prim_meshes[node["primMesh"]]
        idx = flat.indices[pm["firstIndex"]:pm["firstIndex"] + pm["indexCount"]].astype(np.int64) + int(pm["vertexOffset"])
        M = np.asarray(node["worldMatrix"], np.float64).reshape(4, 4).T
        p = (flat.positions[idx].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).reshape(-1, 3, 3)
        lo.append(p.min(axis=1))
        hi.append(p.max(axis=1))
    return np.concatenate(lo).astype(F32), np.concatenate(hi).astype(F32)


@pytest.fixture(scope="module")
def large_scenes():
    import atrium
    from test_gpu_bvh_bounds import _soup

    p = _soup(4200).reshape(-1, 3, 3)
    atrium_small, _ = atrium.build_atrium(20000, seed=4, with_textures=False)
    return {"soup4200": (p.min(axis=1).astype(F32), p.max(axis=1).astype(F32)), "atrium_small": _world_boxes(atrium_small)}


@pytest.mark.parametrize("name", ["soup4200", "atrium_small"])
def test_upper_level_pass_on_the_scenes_of_the_gpu_module(large_scenes, name):
    """The two scenes above 4096 triangles take the two paths of the pass (full sweep up to 1024 entries, bins above), the rebuilt tree
    is a tree with the same ids and the same frontier subtrees, and its SAH cost does not rise.  Prints the restatement's time."""
    lo, hi = large_scenes[name]
    T = lo.shape[0]
    t0 = time.perf_counter()
    order = nb.sorted_order(nb.morton_keys(lo, hi))
    slo, shi = lo[order], hi[order]
    h = nb.ploc(slo, shi)
    t1 = time.perf_counter()
    top, F = nb.top_levels_sah(h, slo, shi)
    t2 = time.perf_counter()
    print(f"{name}: T = {T}, clustering {t1 - t0:.2f} s in {len(h['passes'])} passes, frontier {F}, upper levels {t2 - t1:.2f} s")
    assert (F > nb.TOP_SWEEP_MAX) == (name == "atrium_small"), F
    nb.check_hierarchy(h, T)
    nb.check_hierarchy(top, T)
    K, ids, fr = nb.top_frontier(h, T)
    assert fr.size == F == ids.size + 1 and ids[0] == 0
    # the rebuilt levels are a binary tree over the same frontier that uses the same ids
    inner = np.zeros(T - 1, bool)
    inner[ids] = True
    kids = top["children"][ids].reshape(-1)
    is_inner = (kids >= 0) & inner[np.maximum(kids, 0)]
    assert np.array_equal(np.sort(kids[is_inner]), ids[1:]) and np.array_equal(np.sort(kids[~is_inner]), fr)
    below = np.setdiff1d(np.arange(T - 1), ids)
    _same_tree({k: h[k][below] for k in ("children", "count", "lo", "hi")}, {k: top[k][below] for k in ("children", "count", "lo", "hi")}, name)
    fit = nb.fit_boxes({"children": top["children"]}, slo, shi)
    assert np.array_equal(fit["lo"], top["lo"]) and np.array_equal(fit["hi"], top["hi"])

    def cost(t):
        return float(nb._half_area(t["lo"].astype(np.float64), t["hi"].astype(np.float64)).sum())

    assert cost(top) <= cost(h), (cost(top), cost(h))
    assert t2 - t0 < 60.0


def test_emit_leaf_codes_and_reached_nodes():
    keys = np.array([0, 0, 0, 0, 1, 2, 3, 4 << 60, 5 << 60], np.uint64)
    h = nb.karras(keys)
    root, refs = nb.emit(h, 9, 4)
    # [0..6] | [7, 8], node 6 over [0..6] = [0..4] | [5, 6], node 4 over [0..4] = [0..3] | [4]: runs of <= 4 positions are leaves
    assert root == 0 and refs == {0: (6, ~((7 << 3) | 1)), 6: (4, ~((5 << 3) | 1)), 4: (~((0 << 3) | 3), ~(4 << 3))}
    root, refs = nb.emit(h, 9, 1)
    assert len(refs) == 8 and all(r >= 0 or ((~r) & 7) == 0 for pair in refs.values() for r in pair)
    assert nb.emit(nb.karras(keys[:3]), 3, 4) == (~2, {})
