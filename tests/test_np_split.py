"""Witnesses of tests/np_split.py, the restatement that tests/test_gpu_split_refs.py holds the pre-splitting kernels to, on the hand-made
scenes of tests/split_scenes.py (records made on the host the way k_flatten makes them; the priority's cube root is numpy's here -- on
the device it is the device's, and everything after it is fed the device's values).  No GPU.

The pieces of a triangle partition it (exact areas), their number and the budget's scale stay inside their bounds, nothing depends on
the unit of length, and five subtly wrong splitters -- the mutants of np_split.MUTANTS -- are each told from the right one by the two
checks the device is held to: exact containment of every clipped piece in its box, and bitwise equality of the boxes."""
from fractions import Fraction

import numpy as np
import pytest

import np_split as ns
import split_scenes

F32 = np.float32
NAMES = tuple(split_scenes.HAND_MADE)


class Case:
    """One scene and triangle test: the restated stages with numpy's cube root standing in for the device's."""

    def __init__(self, name, wt, scale=1.0):
        pos, world = split_scenes.HAND_MADE[name]()
        if world is None:
            pos = (pos * F32(scale)).astype(F32)
        else:
            world = world.copy()
            world[:3] *= scale
        self.sc = ns.Scene(ns.records(pos, wt, world), wt)
        self.x, self.zero, p64 = ns.priority(self.sc)
        self.prio = p64.astype(F32)
        self._split = {}

    def split(self, percent):
        if percent not in self._split:
            budget = self.sc.T * percent // 100
            D = ns.budget_scale(self.prio, budget)
            s = ns.split_counts(self.prio, D)
            counts, boxes, cells = ns.all_pieces(self.sc, s)
            self._split[percent] = (budget, D, s, counts, boxes, cells)
        return self._split[percent]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(name, wt=0, scale=1.0):
        if (name, wt, scale) not in cache:
            cache[name, wt, scale] = Case(name, wt, scale)
        return cache[name, wt, scale]

    return get


def _tests_of(name):
    return (0, 1) if name in split_scenes.BOTH_TESTS else (0,)


def _interval(cell, box):
    """The cell inside the triangle's own box as closed intervals [3][2] of exact binary32 values."""
    iv = [[float(box[k]), float(box[3 + k])] for k in range(3)]
    for axis, pos, side in cell:
        if side < 0:
            iv[axis][1] = min(iv[axis][1], float(pos))
        else:
            iv[axis][0] = max(iv[axis][0], float(pos))
    return iv


@pytest.mark.parametrize("name", NAMES)
def test_pieces_partition_the_triangle(cases, name):
    """Every split triangle, every budget: the cells are boxes with disjoint interiors inside the triangle's box (planes are binary32
    values: plain comparisons are exact), and the exact polygons of the pieces have the triangle's area -- as vector areas, Fraction
    equality; for a triangle of zero area (a segment) the extents of the pieces on every axis sum to the segment's.  So the cells leave
    no part of the triangle out.  1 <= pieces <= s + 1, and on these scenes every split makes a piece (but on `far`): no box runs out of
    planes, and the "box shrinks to one side" step is never taken.  In exact arithmetic it cannot be: a plane strictly inside a
    piece's box has part of the triangle on either side of it, and the intervals that bound that part and the box on another axis
    meet pairwise, hence all together.  It is restated all the same, and a device that took it would show in the bitwise comparison."""
    seen_segment = 0
    for wt in _tests_of(name):
        c = cases(name, wt)
        for percent in split_scenes.BUDGETS:
            budget, D, s, counts, boxes, cells = c.split(percent)
            assert np.all(counts >= 1) and np.all(counts <= s + 1), (name, percent)
            assert counts.sum() > c.sc.T and s.sum() <= budget, (name, percent, int(counts.sum()), int(s.sum()), budget)
            if name != "far":  # (at 1e5 a piece a few binary32 steps across has no plane strictly inside its box left)
                assert np.array_equal(counts, s + 1), (name, percent, np.flatnonzero(counts != s + 1)[:8].tolist())
            for g in np.flatnonzero(s > 0):
                v = c.sc.v[g]
                b0 = np.concatenate([v.min(0), v.max(0)])
                ivs = [_interval(cell, b0) for cell in cells[g]]
                for i in range(len(ivs)):
                    for j in range(i):
                        assert any(ivs[i][k][1] <= ivs[j][k][0] or ivs[j][k][1] <= ivs[i][k][0] for k in range(3)), (name, percent, int(g), i, j)
                polys = [ns.clip_exact(v, cell) for cell in cells[g]]
                whole = ns.vector_area_exact(ns.clip_exact(v, ()))
                if any(whole):
                    total = [sum(ns.vector_area_exact(p)[k] for p in polys) for k in range(3)]
                    assert total == whole, (name, percent, int(g), [float(t) for t in total], [float(w) for w in whole])
                else:
                    seen_segment += 1
                    for k in range(3):
                        ext = sum((max(q[k] for q in p) - min(q[k] for q in p)) for p in polys if p)
                        assert ext == Fraction(float(b0[3 + k])) - Fraction(float(b0[k])), (name, percent, int(g), k)
    if name == "needles_and_lines":
        assert seen_segment > 0, "no collinear triangle was split"


@pytest.mark.parametrize("name", NAMES)
def test_every_piece_is_inside_its_box(cases, name):
    """The restatement is conservative on the host scenes: what tests/test_gpu_split_refs.py then proves of the device's boxes."""
    for wt in _tests_of(name):
        c = cases(name, wt)
        for percent in split_scenes.BUDGETS:
            _, _, s, counts, boxes, cells = c.split(percent)
            off = np.concatenate([[0], np.cumsum(counts)])
            for g in np.flatnonzero(s > 0):
                bad, _ = ns.violations(c.sc.v[g], cells[g], boxes[off[g]:off[g + 1]])
                assert bad == 0, (name, wt, percent, int(g), bad)


def test_the_scenes_reach_the_arms_they_are_here_for(cases):
    c = cases("one_giant")
    _, _, s, counts, _, _ = c.split(100)
    assert s.max() == ns.MAX_PER_TRI and counts.max() == ns.MAX_PER_TRI + 1, (int(s.max()), int(counts.max()))
    c = cases("needles_and_lines")
    assert (c.sc.slop > 0).sum() >= 30 and np.all(c.prio[c.sc.slop > 0] == 0)
    _, _, s, counts, _, _ = c.split(100)
    assert np.all(counts[c.sc.slop > 0] == 1)
    c = cases("flat")
    assert c.sc.gext[2] == 0 and (c.prio > 0).sum() > 100
    c = cases("grid8")
    assert c.sc.glo.tolist() == [0, 0, 0] and c.sc.gext.tolist() == [8, 8, 8]
    _, _, s, _, _, _ = c.split(100)
    print("grid8 splits at 100 %:", s[s > 0].tolist())
    assert int(np.argmax(c.prio)) == 12 and s[12] == s.max(), "the diagonal triangle (id 12) leads"
    c = cases("far")
    assert (c.prio > 0).sum() == 3 and c.sc.glo.min() > 9e4
    # the overflow rule of the piece stack: with room for 4 items a cut is refused once 3 are waiting, and the piece goes out whole
    c = cases("one_giant")
    g = int(np.argmax(c.prio))
    deep, _ = ns.pieces(c.sc.v[g], c.sc.full[g], c.sc.slop[g], c.sc.grid, 255)
    shallow, cells = ns.pieces(c.sc.v[g], c.sc.full[g], c.sc.slop[g], c.sc.grid, 255, stack_size=4)
    assert 1 < shallow.shape[0] < deep.shape[0]
    assert ns.violations(c.sc.v[g], cells, shallow)[0] == 0


@pytest.mark.parametrize("name", NAMES)
def test_budget_scale_fills_the_budget(cases, name):
    """count(D) <= budget < count(nextafter(D, inf) x (1 + 2^-20)) whenever some priority is positive -- and the budget can be passed at
    all: where every triangle with a positive priority at the cap of 255 splits stays within the budget, no scale passes it, and D must
    then put each of them at the cap."""
    c = cases(name)
    assert (c.prio > 0).any()
    for percent in split_scenes.BUDGETS:
        budget = c.sc.T * percent // 100
        D = ns.budget_scale(c.prio, budget)
        assert ns.count(c.prio, D) <= budget, (name, percent)
        reachable = int((c.prio > 0).sum()) * ns.MAX_PER_TRI > budget
        if reachable:
            up = F32(np.nextafter(D, F32(np.inf)) * F32(1 + 2.0 ** -20))
            assert ns.count(c.prio, up) > budget, (name, percent, float(D), ns.count(c.prio, up), budget)
        else:
            assert np.all(ns.split_counts(c.prio, D)[c.prio > 0] == ns.MAX_PER_TRI), (name, percent)
    assert ns.budget_scale(c.prio, 0) == 0 and ns.budget_scale(np.zeros(5, F32), 3) == 0


def test_budget_sum_is_the_kernels_order():
    """Thread t adds g = t, t + 1024, ... in sequence, then the tree reduction: against the scalar statement, on values whose float64 sum
    depends on the order."""
    rng = np.random.default_rng(5)
    a = (rng.uniform(0, 1, 3000) * 10.0 ** rng.integers(-12, 6, 3000)).astype(F32)
    red = [0.0] * 1024
    for t in range(1024):
        for g in range(t, a.size, 1024):
            red[t] += float(a[g])
    off = 512
    while off:
        for t in range(off):
            red[t] += red[t + off]
        off >>= 1
    assert ns._strided_sum64(a) == red[0]


@pytest.mark.parametrize("name", NAMES)
def test_scale_invariance(cases, name):
    """The scene scaled by 2^-10 and by 2^10 (exact in binary32): bit-identical x, hence priorities, and the same piece counts."""
    base = cases(name)
    for scale in (2.0 ** -10, 2.0 ** 10):
        other = cases(name, 0, scale)
        assert np.array_equal(base.x.view(np.uint32), other.x.view(np.uint32)) and np.array_equal(base.zero, other.zero), (name, scale)
        for percent in (30, 100):
            assert np.array_equal(base.split(percent)[3], other.split(percent)[3]), (name, scale, percent)


# the scene (at a 100 % budget) on which each wrong splitter is told from the right one, and by which of the device test's two checks
KILLED_BY = {
    "no_pad": ("far", "containment"),           # the cut-point pad set to 0: cut points rounded inwards leave their box
    "no_snap": ("one_giant", "bitwise"),        # the p[axis] = pos line dropped
    "no_clamp": ("one_giant", "bitwise"),       # the clamp to the parent box dropped: conservative still, but boxes as large as the triangle
    "short_axis": ("grid8", "bitwise"),         # the tie between axes going to the shorter axis
    "half_and_half": ("one_giant", "bitwise"),  # s dealt half and half
    # what the kernel did before this test existed: a plane on the box's face ends the search on its axis, so a left half is never cut
    # again on the axis it came from and the giant triangle's 255 splits make 83 pieces
    "face_ends_axis": ("one_giant", "bitwise"),
}


@pytest.mark.parametrize("mutant", ns.MUTANTS)
def test_mutant_is_killed(cases, mutant):
    scene, how = KILLED_BY[mutant]
    c = cases(scene)
    _, _, s, counts, boxes, _ = c.split(100)
    mc, mb, mcells = ns.all_pieces(c.sc, s, mutant)
    off = np.concatenate([[0], np.cumsum(mc)])
    bad = sum(ns.violations(c.sc.v[g], mcells[g], mb[off[g]:off[g + 1]])[0] for g in np.flatnonzero(s > 0))
    differs = not (np.array_equal(mc, counts) and np.array_equal(mb.view(np.uint32), boxes.view(np.uint32)))
    print(f"{mutant} on {scene}: {bad} coordinates outside their box, boxes {'differ' if differs else 'are the same'}")
    if how == "containment":
        assert bad > 0, f"{mutant}: the exact containment check reports nothing on {scene}"
    else:
        assert differs, f"{mutant}: the boxes on {scene} are bit for bit those of the right splitter"
