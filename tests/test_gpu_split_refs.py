"""Triangle pre-splitting (lbvh.hip: k_split_priority, k_split_budget, k_split_refs<false / true>) against its exact host restatement
(tests/np_split.py, whose own witnesses -- and the wrong splitters these checks tell from the right one -- are in tests/test_np_split.py).
vkrt_debug_check_accel samples a split triangle on a 45-point lattice and the images are tree-independent by design, so a piece box
that is too small in a sliver, a cut at the wrong plane or a budget spent on the wrong triangles used to pass everything.  Here
vkrt_debug_split_references shows the priorities, the scale D and the references, and

  a  the priorities are zero exactly where the rules say so and elsewhere the cube root of the restated binary32 argument;
  b  every piece's box contains the triangle clipped to the piece's cell, in rational arithmetic (hand-made scenes) -- with the
     partition witness of tests/test_np_split.py: no point of a triangle is left uncovered;
  c  D, the piece counts and every box word are the restatement's, bit for bit, each stage fed the device's output of the stage before;
  d  the counting and the emitting instantiation agree: no padding repeats, no merged boxes;
  e  the hook shows what a build uses, leaves the installed tree alone and refuses what its contract refuses.

VKRT_SPLIT_PARITY_JSON=<file>: the measured figures go there (how profiles/split_refs_parity.json was taken)."""
import json
import os
import sys

import numpy as np
import pytest

import np_split as ns
import split_scenes
from scene_motion import _col_major
from test_gpu_bvh_bounds import _options, _same_floats, _triangle_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
F32 = np.float32
PROFILE = os.path.join(ROOT, "profiles", "split_refs_parity.json")
ULP_CAP = 4.0  # a larger distance is a finding about the cube root's argument, not about cbrtf

CASES = tuple((name, wt) for name in split_scenes.HAND_MADE for wt in ((0, 1) if name in split_scenes.BOTH_TESTS else (0,))) + (("rotated_small", 0),)
IDS = [f"{n}-wt{w}" for n, w in CASES]


def budgets_of(name):
    return (30,) if name == "rotated_small" else split_scenes.BUDGETS


def flat_scene(name):
    if name == "rotated_small":
        import atrium

        flat, _ = atrium.build_atrium(20000, seed=4, with_textures=False)
        atrium.rotate_scene(flat, dict(atrium.DEFAULT_CAMERA), 35.0, 20.0)
        return flat
    pos, world = split_scenes.HAND_MADE[name]()
    return _triangle_scene(pos, None if world is None else _col_major(world))


def id_order_records(r, T):
    """The installed records of an unsplit build, back in the order of the flattened ids."""
    a = r.read_accel()
    ids = r.read_triangle_ids().astype(np.int64)
    assert ids.size == T and np.array_equal(np.sort(ids), np.arange(T))
    rec = np.zeros((T, 12), F32)
    rec[ids] = a["tris"].reshape(-1, 12)
    return rec


class Case:
    """One scene and triangle test: the hook's output for every budget, and the restatement of each stage fed the device's output of
    the stage before it."""

    def __init__(self, name, wt):
        from vkrt_amd.renderer import Renderer

        self.name, self.wt = name, wt
        flat = flat_scene(name)
        r = Renderer(flat, device=0, build="lbvh", options=_options("bvh2", wt, 0))
        self.T = T = flat.instanced_triangle_count
        self.sc = ns.Scene(id_order_records(r, T), wt)
        self.dev = {b: r.split_references(b) for b in budgets_of(name)}
        r.close()
        self.x, self.zero, self.p64 = ns.priority(self.sc)
        self.restated = {}

    def pieces(self, b):
        """(splits, counts, boxes, cells) restated from the device's priorities and D."""
        if b not in self.restated:
            d = self.dev[b]
            s = ns.split_counts(d["prio"], d["scale"])
            self.restated[b] = (s,) + ns.all_pieces(self.sc, s)
        return self.restated[b]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(name, wt):
        if (name, wt) not in cache:
            cache[name, wt] = Case(name, wt)
        return cache[name, wt]

    return get


def _record(key, entry):
    path = os.environ.get("VKRT_SPLIT_PARITY_JSON")
    if not path:
        return
    data = json.load(open(path)) if os.path.exists(path) else {"cases": {}}
    data["cases"].setdefault(key, {}).update(entry)
    ulps = [c["max_priority_ulp"] for c in data["cases"].values() if "max_priority_ulp" in c]
    data["max_priority_ulp"] = max(ulps) if ulps else 0.0
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("name,wt", CASES, ids=IDS)
def test_priorities(cases, name, wt):
    """The device's zero set is the restated one; elsewhere p is cbrt(float64(x)) of the restated binary32 x within the accuracy of the
    device library's cbrtf plus half an ulp for rounding the reference.  The ROCm documentation installed with the compiler states no
    bound for cbrtf, so the bound is the largest distance measured over all scenes (profiles/split_refs_parity.json: max_priority_ulp)
    plus one ulp, and never more than 4 ulp."""
    c = cases(name, wt)
    for b in budgets_of(name):
        prio = c.dev[b]["prio"]
        assert prio.dtype == np.float32 and prio.shape == (c.T,)
        assert np.array_equal(prio.view(np.uint32), c.dev[budgets_of(name)[0]]["prio"].view(np.uint32)), "the priorities depend on the budget"
    assert np.all(np.isfinite(prio)) and np.all(prio >= 0)
    wrong = np.flatnonzero((prio == 0) != c.zero)
    assert wrong.size == 0, (f"{name} wt={wt}: {wrong.size} triangles are zero on one side only, first {wrong[:8].tolist()}: device "
                             f"{prio[wrong[:8]].tolist()}, restated x {c.x[wrong[:8]].tolist()}")
    live = ~c.zero
    ulp = np.zeros(c.T)
    ulp[live] = np.abs(prio[live].astype(np.float64) - c.p64[live]) / np.spacing(c.p64[live].astype(F32)).astype(np.float64)
    worst = float(ulp.max()) if live.any() else 0.0
    print(f"{name} wt={wt}: {int(live.sum())} of {c.T} priorities positive, largest distance from cbrt(float64(x)) {worst:.3f} ulp")
    for b in budgets_of(name):
        _record(f"{name}-wt{wt}-b{b}", dict(max_priority_ulp=worst))
    measured = json.load(open(PROFILE))["max_priority_ulp"] if os.path.exists(PROFILE) else ULP_CAP - 1.0
    bound = min(measured + 1.0, ULP_CAP)
    assert worst <= bound, (name, wt, worst, bound, int(np.argmax(ulp)), float(c.x[np.argmax(ulp)]))


@pytest.mark.parametrize("name,wt", CASES, ids=IDS)
def test_scale_counts_and_boxes_bit_for_bit(cases, name, wt):
    """budget_scale(device priorities) is the device's D in every bit; pieces() with s = min(unsigned(D x prio), 255) from the device's
    values gives the device's box words in emission order for every triangle; ref_tri is the run-length expansion of the counts;
    ref_count is their sum and T < ref_count <= T + budget."""
    c = cases(name, wt)
    for b in budgets_of(name):
        d = c.dev[b]
        what = f"{name} wt={wt} budget={b}"
        budget = c.T * b // 100
        D = ns.budget_scale(d["prio"], budget)
        assert F32(D).view(np.uint32) == F32(d["scale"]).view(np.uint32), (what, float(D), float(d["scale"]))
        s, counts, boxes, _ = c.pieces(b)
        assert s.sum() <= budget, what
        R = d["ref_count"]
        assert c.T < R <= c.T + budget, (what, R)
        assert d["ref_tri"].shape == (R,) and d["ref_box"].shape == (R, 6)
        dev_counts = np.bincount(d["ref_tri"], minlength=c.T)
        assert np.array_equal(d["ref_tri"], np.repeat(np.arange(c.T), dev_counts)), f"{what}: the pieces of a triangle are not contiguous in id order"
        bad = np.flatnonzero(dev_counts != counts)
        assert bad.size == 0, (f"{what}: {bad.size} triangles with another number of pieces, first {bad[:6].tolist()}: device "
                               f"{dev_counts[bad[:6]].tolist()}, restated {counts[bad[:6]].tolist()} (splits {s[bad[:6]].tolist()})")
        assert R == counts.sum(), what
        _same_floats(d["ref_box"], boxes, f"{what}: reference boxes (row = reference, column = lo3 hi3)")
        _record(f"{name}-wt{wt}-b{b}", dict(T=int(c.T), ref_count=int(R), triangles_split=int((dev_counts > 1).sum()), scale=float(d["scale"]),
                                             splits_without_a_piece=int(s.sum() - (R - c.T))))


@pytest.mark.parametrize("name,wt", [k for k in CASES if k[0] != "rotated_small"], ids=[i for i in IDS if not i.startswith("rotated")])
def test_pieces_are_conservative_exactly(cases, name, wt):
    """Every vertex of the triangle clipped to a piece's cell (Sutherland-Hodgman in Fractions on the binary32 vertices) lies inside the
    DEVICE's box of that piece; an unsplit triangle's vertices lie inside its one box.  No tolerance.  With the partition witness of
    tests/test_np_split.py the pieces leave no point of the triangle uncovered.  The smallest slack of a computed cut-point coordinate
    goes to the profile: the margin the 8-ulp pad really has (information)."""
    c = cases(name, wt)
    for b in budgets_of(name):
        d = c.dev[b]
        what = f"{name} wt={wt} budget={b}"
        s, counts, _, cells = c.pieces(b)
        dev_counts = np.bincount(d["ref_tri"], minlength=c.T)
        assert np.array_equal(dev_counts, counts), f"{what}: piece counts differ (see test_scale_counts_and_boxes_bit_for_bit): cells cannot be paired"
        off = np.concatenate([[0], np.cumsum(counts)])
        whole = np.flatnonzero(s == 0)
        box = d["ref_box"][off[whole]]
        v = c.sc.v[whole]
        assert np.all(v >= box[:, None, 0:3]) and np.all(v <= box[:, None, 3:6]), f"{what}: an unsplit triangle's vertex outside its box"
        slack, empty = float("inf"), 0
        for g in np.flatnonzero(s > 0):
            bad, sl = ns.violations(c.sc.v[g], cells[g], d["ref_box"][off[g]:off[g + 1]])
            assert bad == 0, f"{what}: triangle {int(g)} ({int(counts[g])} pieces): {bad} coordinates of its clipped pieces outside their boxes"
            slack = min(slack, sl)
            empty += sum(1 for cell in cells[g] if len(ns.clip_exact(c.sc.v[g], cell)) == 0)
        print(f"{what}: smallest slack of a computed coordinate {slack:.3e}; {empty} pieces hold no part of their triangle")
        _record(f"{name}-wt{wt}-b{b}", dict(min_exact_slack=slack, empty_pieces=empty))


@pytest.mark.parametrize("name,wt", CASES, ids=IDS)
def test_counting_and_emitting_instantiations_agree(cases, name, wt):
    """The emitting instantiation is held to the slots the counting one claimed: a divergence shows as trailing pieces that repeat one
    another bit for bit (the padding loop) or as a last box that is a union.  No triangle's pieces repeat unless the restatement emits
    the same repeat, and the last box of every triangle is the restatement's last box."""
    c = cases(name, wt)
    for b in budgets_of(name):
        d = c.dev[b]
        s, counts, boxes, _ = c.pieces(b)
        if d["ref_count"] != counts.sum():
            pytest.fail(f"{name} wt={wt} budget={b}: {d['ref_count']} references, {int(counts.sum())} restated")

        def repeats(bx, tri):
            w = np.ascontiguousarray(bx, F32).view(np.uint32)
            same = np.all(w[1:] == w[:-1], axis=1) & (tri[1:] == tri[:-1])
            return np.flatnonzero(same)

        tri = np.repeat(np.arange(c.T), counts)
        got, want = repeats(d["ref_box"], d["ref_tri"]), repeats(boxes, tri)
        assert np.array_equal(got, want), (name, wt, b, got[:8].tolist(), want[:8].tolist())
        last = np.cumsum(counts) - 1
        _same_floats(d["ref_box"][last], boxes[last], f"{name} wt={wt} budget={b}: the last piece of every triangle")


@pytest.mark.parametrize("name", ["grid8", "soup257", "rotated_small"])
def test_hook_shows_what_the_build_uses(cases, name):
    """Builds with the same budget: reference_count is the hook's ref_count and the installed slots hold the hook's triangles, as
    multisets; the hook leaves the installed tree's words and records unchanged; two calls give the same bytes."""
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer

    c = cases(name, 0)
    flat = flat_scene(name)
    b = 30
    d = c.dev[b]
    for kind in ("ploc", "lbvh"):
        for layout in ("wide8", "bvh2"):
            what = f"{name} {kind} {layout}"
            r = Renderer(flat, device=0, build=kind, options=_options(layout, 0, b))
            assert r.accel_info()["reference_count"] == d["ref_count"], what
            assert r.get_option(abi.VKRT_INFO_SPLIT_BUDGET) == b
            assert np.array_equal(np.sort(r.read_triangle_ids()), np.sort(d["ref_tri"])), what
            before = r.read_accel()
            one, two = r.split_references(b), r.split_references(b)
            after = r.read_accel()
            for k in ("prio", "ref_tri", "ref_box"):
                assert one[k].tobytes() == two[k].tobytes() == d[k].tobytes(), (what, k)
            assert F32(one["scale"]).tobytes() == F32(two["scale"]).tobytes() == F32(d["scale"]).tobytes() and one["ref_count"] == two["ref_count"]
            assert before["root_ref"] == after["root_ref"] and before["nodes"].tobytes() == after["nodes"].tobytes(), what
            assert before["tris"].tobytes() == after["tris"].tobytes(), what
            r.close()


def test_hook_contract():
    """Needs no tree; the identity list with the whole-triangle boxes when nothing is split; the option decides the record format;
    capacity below T + T x percent / 100, a percent outside 1..100 and NULL pointers are VKRT_ERR_INVALID_ARGUMENT and write nothing."""
    import ctypes as C

    import np_bvh
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer

    flat = flat_scene("grid8")
    T = flat.instanced_triangle_count
    r = Renderer(flat, device=0, build=None, options=_options("bvh2", 0, 0))
    got = r.split_references(30)  # before any build
    assert got["ref_count"] > T
    r.build("lbvh")
    assert np.array_equal(r.split_references(30)["ref_box"].view(np.uint32), got["ref_box"].view(np.uint32))
    rec = id_order_records(r, T)
    one = r.split_references(1)  # T * 1 / 100 == 0 splits: nothing is split, no priority is computed
    lo, hi = np_bvh.record_bounds(rec, 0)
    assert one["ref_count"] == T and np.array_equal(one["ref_tri"], np.arange(T)) and one["scale"] == 0 and not one["prio"].any()
    _same_floats(one["ref_box"], np.concatenate([lo, hi], 1), "identity list: whole-triangle boxes")
    fn = r.lib.vkrt_debug_split_references
    cap = T + T * 30 // 100
    tri, box, n = np.full(cap + 1, 7, np.uint32), np.full((cap + 1, 6), 7, F32), C.c_uint32(7)
    for percent, capacity in ((30, cap - 1), (30, 0), (100, 2 * T - 1), (0, cap), (101, 3 * T)):
        assert fn(r._h, percent, None, None, tri.ctypes.data, box.ctypes.data, capacity, C.byref(n)) == abi.VKRT_ERR_INVALID_ARGUMENT, (percent, capacity)
        assert b"vkrt_debug_split_references" in r.lib.vkrt_last_error()
    assert fn(None, 30, None, None, tri.ctypes.data, box.ctypes.data, cap, C.byref(n)) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert fn(r._h, 30, None, None, None, box.ctypes.data, cap, C.byref(n)) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert fn(r._h, 30, None, None, tri.ctypes.data, None, cap, C.byref(n)) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert fn(r._h, 30, None, None, tri.ctypes.data, box.ctypes.data, cap, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert np.all(tri == 7) and np.all(box == 7) and n.value == 7
    # NULL prio / scale are skipped; an exact capacity is enough
    assert fn(r._h, 30, None, None, tri.ctypes.data, box.ctypes.data, cap, C.byref(n)) == abi.VKRT_OK and n.value == got["ref_count"]
    assert np.array_equal(tri[: n.value], got["ref_tri"]) and np.all(tri[cap:] == 7)
    # the option as it stands now decides which vertices the splitter sees; the installed (Moeller-Trumbore) tree is not touched
    before = r.read_accel()
    r.set_option(abi.VKRT_OPT_WATERTIGHT, 1)
    wt = r.split_references(100)
    r.set_option(abi.VKRT_OPT_WATERTIGHT, 0)
    sc = ns.Scene(ns.records(split_scenes.grid8()[0], 1), 1)
    counts, boxes, _ = ns.all_pieces(sc, ns.split_counts(wt["prio"], wt["scale"]))
    assert wt["ref_count"] == counts.sum()
    _same_floats(wt["ref_box"], boxes, "watertight records through the option alone")
    assert r.read_accel()["tris"].tobytes() == before["tris"].tobytes()
    r.close()
