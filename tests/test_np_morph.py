"""tests/np_morph.py, the numpy restatement the GPU morph tests compare bits with: the vectorised form against a scalar Python loop (one
float32 operation at a time, the header's formula as written) in every bit on every case of test_gpu_morph.py, all-zero weights giving
the base bits back, and the four plausible wrong readings of the formula told apart on inputs where each changes at least one bit."""
import os
import sys

import numpy as np
import pytest

import np_morph
import scene_morph as sm
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
F = np.float32
U = 2.0 ** -24  # unit roundoff of binary32


@pytest.fixture(scope="module")
def cases(cornell_flat):
    """(FlatScene, morph) of every GPU case of test_gpu_morph.py"""
    import atrium

    flat, _ = atrium.build_atrium(20000, seed=4, with_textures=True)
    out = [(cornell_flat, m) for m in sm.cornell_cases(cornell_flat) + sm.cornell_subrange_cases(cornell_flat) + sm.cornell_many_target_cases(cornell_flat)]
    return out + [(flat, m) for m in sm.atrium_cases(flat)]


def _base(flat, m):
    sl = slice(m["first"], m["first"] + m["count"])
    return flat.positions[sl], flat.normals[sl], flat.tangents[sl]


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_the_cases_are_the_ones_the_issue_names(cases):
    counts = [m["count"] for _, m in cases]
    assert {1, 63, 65, 257} <= set(counts)
    assert all(m["first"] % 2 == 1 for _, m in cases if m["count"] in (1, 63, 65, 257))
    flat, m = cases[-1]
    assert m["first"] + m["count"] == len(flat.positions)
    assert sorted({m["target_count"] for _, m in cases}) == [1, 2, 33, 130, 256]
    w = [m["weights"] for _, m in cases if m["target_count"] == 130][0]
    assert w[63] != 0 and w[64] != 0 and w[129] != 0 and not w[[62, 65, 128]].any()  # in use on both sides of a 64-weight boundary
    assert sm.disjoint([m for f, m in cases if f is cases[0][0]])
    kinds = {m["kind"] for _, m in cases}
    assert kinds == {"zero", "negative", "above1", "gaps"}
    for _, m in cases:
        w = m["weights"]
        assert w.dtype == F and w.shape == (m["target_count"],)
        for a in sm.ATTRS:
            assert m[a] is None or (m[a].dtype == F and m[a].shape == (m["target_count"], m["count"], 3))
        if m["kind"] == "zero":
            assert not w.any() and np.signbit(w).any()
        if m["kind"] == "negative":
            assert (w < 0).all()
        if m["kind"] == "above1":
            assert (w > 1).all()
    g = [m["weights"] for _, m in cases if m["kind"] == "gaps" and m["target_count"] == 33][0]
    z = np.flatnonzero(g == 0)
    assert len(z) >= 5 and g[0] != 0 and g[-1] != 0 and all(g[i - 1] != 0 and g[i + 1] != 0 for i in z)  # zeros between non-zeros
    have = {tuple(a for a in sm.ATTRS if m[a] is not None) for _, m in cases}
    assert ("position_deltas",) in have and ("normal_deltas",) in have and sm.ATTRS in have


def test_vectorised_equals_the_scalar_loop_in_every_bit(cases):
    for flat, m in cases:
        p, n, t = _base(flat, m)
        got = np_morph.morph(m["weights"], p, n, t, **sm.deltas(m))
        ref = np_morph.morph_scalar(m["weights"], p, n, t, **sm.deltas(m))
        for a, b, name in zip(got, ref, ("positions", "normals", "tangents")):
            assert a.dtype == F and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (m["first"], name)
        assert np.array_equal(_bits(got[2][:, 3]), _bits(t[:, 3]))
        # an attribute without deltas comes back as the base, in every bit
        for a, b, attr in zip(got, (p, n, t), sm.ATTRS):
            if m[attr] is None:
                assert np.array_equal(_bits(a), _bits(b)), (m["first"], attr)
        if m["kind"] != "zero":
            assert not np.array_equal(_bits(got[0]), _bits(p)) or m["position_deltas"] is None


def test_float64_evaluation_within_the_rounding_bound(cases):
    """P is the base plus K = (number of non-zero weights) terms, each with one rounding of its product and one of its addition; every
    partial sum is bounded by S = |p| + sum |w dP| (1 + u)^(2K), so |P - exact| <= gamma_2K * S with gamma_m = m u / (1 - m u)."""
    for flat, m in cases:
        if m["position_deltas"] is None:
            continue
        p, n, t = _base(flat, m)
        w = m["weights"].astype(np.float64)
        d = m["position_deltas"].astype(np.float64)
        K = int((w != 0).sum())
        exact = p.astype(np.float64) + np.einsum("k,kvc->vc", w, d)
        S = np.abs(p.astype(np.float64)) + np.einsum("k,kvc->vc", np.abs(w), np.abs(d))
        g = 2 * K * U / (1 - 2 * K * U)
        got = np_morph.morph(m["weights"], p, n, t, **sm.deltas(m))[0]
        assert np.all(np.abs(got.astype(np.float64) - exact) <= g * S), m["first"]


def test_zero_weights_return_the_base_bits_with_negative_zero():
    rng = np.random.default_rng(1)
    p = np.array([[-0.0, 1.0, -0.0], [0.0, -0.0, 2.5]], F)
    n = np.array([[0.0, 3.0, -0.0], [-0.0, -0.0, -0.0]], F)  # (not unit, and a zero normal: neither is normalised)
    t = np.array([[2.0, -0.0, 0.0, -1.0], [-0.0, 0.5, 0.0, 1.0]], F)
    d = [np.ascontiguousarray(rng.uniform(0.5, 1.0, (3, 2, 3)), F) for _ in range(3)]
    for w in (np.zeros(3, F), np.array([0.0, -0.0, 0.0], F), np.full(3, -0.0, F)):
        for fn in (np_morph.morph, np_morph.morph_scalar):
            got = fn(w, p, n, t, d[0], d[1], d[2])
            assert _same(got, (p, n, t)), (w, fn.__name__)
    # some weight not zero: the normal is normalised even where its own sum did not move
    got = np_morph.morph(np.array([0.0, 1.0, 0.0], F), p, n, t, d[0], np.zeros_like(d[1]), None)
    assert np.array_equal(got[1][0], np.array([0.0, 1.0, -0.0], F)) and np.array_equal(_bits(got[2]), _bits(t))
    assert not got[1][1].any()  # (the guard: a zero normal stays)


def _crafted():
    """inputs on which every wrong variant below changes a bit (e = 2^-12)
    x: a base of -0 and deltas of 1: "multiply by zero" gives -0 + 0 * 1 = +0, the skip keeps -0
    y: base -(1 + 2e), target 0 has w = d = 1 + e: w * d = 1 + 2e + e^2 rounds to 1 + 2e (a tie, to even), so the stated sum is 0; a
       fused multiply-add keeps the e^2 = 2^-24
    z: base 1, deltas 2^-24, 2^-24, -1: in index order (1 + 2^-24) + 2^-24 stays 1 (ties to even) and ends at 0; reversed, 1 - 1 = 0
       and the two small terms survive: 2^-23"""
    e = F(2.0 ** -12)
    p = np.array([[-0.0, -(1.0 + 2.0 * float(e)), 1.0]], F)
    n = np.array([[0.0, 3.0, 4.0]], F)  # length 5: "always normalise" shows with zero weights
    t = np.array([[1.0, 0.0, 0.0, -1.0]], F)
    dP = np.array([[[1.0, 1.0 + e, 2.0 ** -24]], [[1.0, 0.0, 2.0 ** -24]], [[0.0, 0.0, -1.0]]], F)
    return p, n, t, dP


def test_the_wrong_variants_each_differ_in_a_bit():
    p, n, t, dP = _crafted()
    e = F(2.0 ** -12)
    dN = np.zeros_like(dP)
    right = lambda w, **kw: np_morph.morph(w, p, n, t, dP, dN, None, **kw)  # noqa: E731
    # a fused multiply-add: y = -(1 + 2e) + (1 + e)(1 + e); the rounded product drops e^2, the fused sum sees it
    w = np.array([1.0 + e, 0.0, 0.0], F)
    a, b = right(w), right(w, fused=True)
    assert not np.array_equal(_bits(a[0]), _bits(b[0]))
    assert _same(a, np_morph.morph_scalar(w, p, n, t, dP, dN, None))
    assert float(a[0][0, 1]) == 0.0 and float(b[0][0, 1]) == 2.0 ** -24
    # a reversed target order: z = ((1 + 2^-24) + 2^-24) - 1 = 0 against ((1 - 1) + 2^-24) + 2^-24 = 2^-23
    w = np.ones(3, F)
    a, b = right(w), right(w, reverse=True)
    assert float(a[0][0, 2]) == 0.0 and float(b[0][0, 2]) == 2.0 ** -23
    assert _same(a, np_morph.morph_scalar(w, p, n, t, dP, dN, None))
    # "always normalise": with all-zero weights the length-5 normal stays as it is
    w = np.zeros(3, F)
    a, b = right(w), right(w, always_normalize=True)
    assert np.array_equal(_bits(a[1]), _bits(n)) and not np.array_equal(_bits(a[1]), _bits(b[1]))
    # "multiply by zero instead of skipping": -0 + 0 * 1 = +0, the skip keeps -0
    a, b = right(w), right(w, multiply_zero=True)
    assert np.signbit(a[0][0, 0]) and not np.signbit(b[0][0, 0]) and not np.array_equal(_bits(a[0]), _bits(b[0]))
    assert _same(a, (p, n, t))
