"""tests/np_skin.py, the numpy restatement the GPU skinning tests compare bits with, held to two independent evaluations on every vertex
of those tests' cases: a scalar Python loop (one float32 operation at a time, the header's formula as written) in every bit, and a
float64 evaluation within a bound derived from the number of roundings."""
import os
import sys

import numpy as np
import pytest

import np_skin
import scene_skin as ss
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
F = np.float32
U = 2.0 ** -24  # unit roundoff of binary32


@pytest.fixture(scope="module")
def cases(cornell_flat):
    """(FlatScene, skin) of every GPU case of test_gpu_skin.py"""
    import atrium

    flat, _ = atrium.build_atrium(20000, seed=4, with_textures=True)
    out = [(cornell_flat, k) for k in ss.cornell_cases(cornell_flat) + ss.cornell_subrange_cases(cornell_flat)]
    return out + [(flat, k) for k in ss.atrium_cases(flat)]


def _bind(flat, k):
    sl = slice(k["first"], k["first"] + k["count"])
    return flat.positions[sl], flat.normals[sl], flat.tangents[sl]


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_the_cases_are_the_ones_the_issue_names(cases):
    counts = [k["count"] for _, k in cases]
    assert counts[2:6] == [1, 63, 65, 257] and sorted({k["joint_count"] for _, k in cases}) == [1, 2, 33]
    for flat, k in cases:
        j, w = k["joints"], k["weights"]
        assert j.dtype == np.uint16 and w.dtype == F and j.shape == w.shape == (k["count"], 4)
        assert int(j.max()) == k["joint_count"] - 1                     # the highest index is used
        assert np.all(np.abs(w.sum(1, dtype=np.float64) - 1) < 4 * U)   # rows normalised in float32
        assert k["matrices"].shape == (k["joint_count"], 16) and k["matrices"].dtype == F
    assert any((k["weights"] == 0).any() for _, k in cases)             # some influences exactly 0
    flat, k = cases[-1]
    assert k["first"] + k["count"] == len(flat.positions)
    assert all(k["first"] % 2 == 1 for _, k in cases[2:4])
    # a mirrored joint and a non-uniformly scaled one
    m = cases[1][1]["matrices"].reshape(-1, 4, 4)[:, :3, :3].astype(np.float64)
    assert (np.linalg.det(m) < 0).sum() == 1
    sv = np.linalg.svd(m, compute_uv=False)
    assert (sv[:, 0] / sv[:, 2] > 1.5).sum() == 1


def test_vectorised_equals_the_scalar_loop_in_every_bit(cases):
    for flat, k in cases:
        p, n, t = _bind(flat, k)
        got = np_skin.skin(k["joints"], k["weights"], k["matrices"], p, n, t)
        ref = np_skin.skin_scalar(k["joints"], k["weights"], k["matrices"], p, n, t)
        for a, b, name in zip(got, ref, ("positions", "normals", "tangents")):
            assert a.dtype == F and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (k["first"], name)


def test_float64_evaluation_within_the_rounding_bound(cases):
    """Every term w_i * J_i[r][c] * a_c of p'[r] passes through at most 8 roundings (its product, up to three additions of the blend, the
    product with the coordinate, up to three additions of the row), so |p' - exact| <= gamma_8 * S with S the sum of the terms'
    magnitudes and gamma_8 = 8u / (1 - 8u); the unnormalised N has one addition less and no translation.  The normalisation of a float32
    N (three squares and two additions of positive terms: 3u on d, half of it after the root; then the root, the reciprocal and the
    product, u each) stays within 4.5u relative: 5u is asserted."""
    g8 = 8 * U / (1 - 8 * U)
    for flat, k in cases:
        p, n, t = _bind(flat, k)
        j, w = k["joints"].astype(np.int64), k["weights"].astype(np.float64)
        J = k["matrices"].astype(np.float64).reshape(-1, 4, 4)[:, :, :3]  # [k, c, r]
        M = sum(w[:, i, None, None] * J[j[:, i]] for i in range(4))
        A = sum(np.abs(w[:, i, None, None] * J[j[:, i]]) for i in range(4))
        got_p, got_n, got_t = np_skin.skin(k["joints"], k["weights"], k["matrices"], p, n, t)
        Mf = np_skin.blended(k["joints"], k["weights"], k["matrices"])
        p64 = np.einsum("vcr,vc->vr", M[:, :3], p.astype(np.float64)) + M[:, 3]
        S = np.einsum("vcr,vc->vr", A[:, :3], np.abs(p.astype(np.float64))) + A[:, 3]
        assert np.all(np.abs(got_p.astype(np.float64) - p64) <= g8 * S), k["first"]
        for a, got in ((n, got_n), (t[:, :3], got_t[:, :3])):
            N = np_skin.linear(Mf, a)
            N64 = np.einsum("vcr,vc->vr", M[:, :3], a.astype(np.float64))
            S = np.einsum("vcr,vc->vr", A[:, :3], np.abs(a.astype(np.float64)))
            assert np.all(np.abs(N.astype(np.float64) - N64) <= g8 * S), k["first"]
            d = (N.astype(np.float64) ** 2).sum(1, keepdims=True)
            assert np.all(d > 1e-12)  # (no degenerate blend among the cases: the guard has its own test)
            unit = N.astype(np.float64) / np.sqrt(d)
            assert np.all(np.abs(got.astype(np.float64) - unit) <= 5 * U * np.abs(unit)), k["first"]
        assert np.array_equal(_bits(got_t[:, 3]), _bits(t[:, 3]))


def test_guarded_normalise_zero_normal_zero_weights_and_overflow():
    j = np.array([[0, 1, 0, 1]] * 4, np.uint16)
    w = np.array([[0.5, 0.5, 0, 0], [0, 0, 0, 0], [0.5, 0.5, 0, 0], [1, 0, 0, 0]], F)
    m = ss.joint_matrices(2, 3)
    m[0, 0:3] *= F(1e30)  # joint 0 stretches x beyond what a squared length holds
    p = np.ones((4, 3), F)
    n = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0]], F)           # a zero normal; an all-zero weight row; a plain one; overflow
    t = np.array([[1, 0, 0, -1], [1, 0, 0, 1], [0, 0, 0, 1], [1, 0, 0, -1]], F)  # (a zero tangent in the plain row)
    for fn in (np_skin.skin, np_skin.skin_scalar):
        P, N, T = fn(j, w, m, p, n, t)
        assert not N[0].any() and not N[1].any() and not P[1].any() and not T[1, :3].any() and not T[2, :3].any()
        assert np.array_equal(T[:, 3], t[:, 3])
        assert abs(float(np.linalg.norm(N[2].astype(np.float64))) - 1) < 4 * U
        # d overflows to inf: N stays as the blend gave it (finite, huge), not 0 and not NaN
        assert np.all(np.isfinite(N[3])) and np.linalg.norm(N[3].astype(np.float64)) > 1e29
        assert np.all(np.isfinite(P)) and not np.isnan(N).any() and not np.isnan(T).any()
    a, b = np_skin.skin(j, w, m, p, n, t), np_skin.skin_scalar(j, w, m, p, n, t)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))
