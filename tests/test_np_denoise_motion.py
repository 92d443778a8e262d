"""The restatement of the denoiser's motion entry (np_denoise_motion.NpMotionDenoiser) on the planes of denoise_motion_planes: what it
must equal when nothing moved, what it gains on the movers, how well-conditioned its cases are, which branches they reach and whether a
one-line departure from the rule is seen.  numpy only."""
import numpy as np
import pytest

import denoise_motion_planes as dm
import denoise_planes as dp
import np_denoise as nd
from np_denoise_motion import MOTION_VARIANT, NpMotionDenoiser

F = np.float32
E32_BOUND = 5e-5  # the project's condition on a case for the GPU tests' 4 E32 bar (tests/test_np_denoise.py)
MAIN = (48, 40)

MOTION_CASES = [dict(W=W, H=H, pan=pan, iterations=K) for W, H in dm.SIZES for pan in (False, True) for K in (0, 5)] + \
               [dict(W=MAIN[0], H=MAIN[1], iterations=K) for K in (1, 2)] + \
               [dict(W=W, H=H, iterations=0, max_history=mh) for W, H in dm.SIZES for mh in (1, 2)] + \
               [dict(W=MAIN[0], H=MAIN[1], iterations=K, w0_block=True) for K in (0, 5)] + \
               [dict(W=MAIN[0], H=MAIN[1], iterations=K, nan_pixel=True) for K in (0, 5)]


def _ids(kw):
    return "-".join(f"{k}{v}" for k, v in kw.items())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("K", (0, 5))
def test_equals_the_plain_restatement_when_nothing_moved(K):
    """prevPosition = position (w = 1): every call of denoise_planes' main case comes out of NpMotionDenoiser as out of NpDenoiser,
    in every bit, history lengths included -- the reset, the dolly and the NaN-free twelve-call script."""
    calls = dp.case(*MAIN, iterations=K)
    plain, valid, _, lengths = dp.replay(calls, np.float32)
    moved = []
    for c in calls:
        g = dict(c["planes"])
        g["prevPosition"] = g["position"].copy()
        g["prevPosition"][..., 3] = np.where(nd.geom_valid(g["position"], g["normal"]), F(1), g["position"][..., 3])
        moved.append(dict(c, planes=g))
    outs, valid2, _, lengths2 = dm.replay(moved, np.float32)
    for a, b, la, lb, va, vb in zip(plain, outs, lengths, lengths2, valid, valid2):
        assert np.array_equal(va, vb) and np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(la), _bits(lb))


def test_history_follows_the_movers():
    """Still camera, the spheres in motion, temporal stage with the default max_history: with the previous positions the unit
    sphere's pixels keep their history (median length i + 1 at frame i, at least 90 % of them at full length -- the restatement
    measured 95.6 % and more), without them every frame starts again (median 1).  Static pixels do not change in any bit."""
    calls = dm.case(*MAIN, iterations=0)
    outs_m, _, _, len_m = dm.replay(calls, np.float32)
    outs_p, _, _, len_p = dm.replay(dm.without_motion(calls), np.float32)
    for i, c in enumerate(calls):
        obj = c["planes"]["object"]
        unit, static = obj == 0, obj >= 4
        assert unit.sum() >= 50 and static.sum() > 500
        if i >= 1:
            full = float((len_m[i][unit] == i + 1).mean())
            print(f"frame {i}: median with motion {np.median(len_m[i][unit])}, without {np.median(len_p[i][unit])}, at full length {full:.3f}")
            assert np.median(len_m[i][unit]) == i + 1 and np.median(len_p[i][unit]) == 1
            assert full >= 0.90
        assert np.array_equal(_bits(outs_m[i][static]), _bits(outs_p[i][static]))
        assert np.array_equal(_bits(len_m[i][static]), _bits(len_p[i][static]))


@pytest.mark.parametrize("kw", MOTION_CASES, ids=_ids)
def test_motion_cases_are_well_conditioned(kw):
    """E32 <= 5e-5 on every case the GPU tests use, so that 4 E32 is a bar of the size the plain entry is held to.  Pixels without
    geometry and .w keep the fill's bits."""
    r = dm.reference(**kw)
    print(kw, f"E32 {r['E32']:.2e}")
    assert r["E32"] <= E32_BOUND
    fill = dm.fill(kw["W"], kw["H"])
    for o32, o64, v in zip(r["out32"], r["out64"], r["valid"]):
        assert np.array_equal(_bits(o32[~v]), _bits(fill[~v])) and np.array_equal(o64[~v], fill[~v].astype(np.float64))
        assert np.array_equal(_bits(o32[..., 3]), _bits(fill[..., 3]))


@pytest.mark.parametrize("kw", [dict(pan=False), dict(pan=True), dict(w0_block=True), dict(nan_pixel=True)], ids=_ids)
def test_cases_reach_every_branch_of_the_taps(kw):
    r = dm.reference(*MAIN, **kw)
    total = {k: sum(c[k] for c in r["cover"]) for k in r["cover"][0]}
    print(kw, total)
    assert total["taps_accepted"] > 1000 and total["taps_plane_only"] > 0 and total["taps_normal_only"] > 0
    if kw.get("pan"):
        assert total["q_outside"] > 0
    if kw.get("w0_block"):
        assert total["not_existed"] >= 4 * (dm.FRAMES - 3)
    if kw.get("nan_pixel"):
        assert total["xp_not_finite"] == dm.FRAMES - 2 and total["behind_prev"] >= dm.FRAMES - 2


def test_marked_pixels_take_no_history():
    """prevPosition.w == 0 and a NaN Xp: history length 1 at exactly those pixels, while their neighbours on the sphere keep theirs"""
    for kw, first in ((dict(w0_block=True), 3), (dict(nan_pixel=True), 2)):
        r = dm.reference(*MAIN, iterations=0, **kw)
        base = dm.reference(*MAIN, iterations=0)
        for i in range(first, dm.FRAMES):
            p = r["calls"][i]["planes"]["prevPosition"]
            marked = (r["calls"][i]["planes"]["object"] == 0) & ((p[..., 3] == 0) | ~np.isfinite(p[..., :3]).all(-1))
            assert marked.sum() >= 1
            assert np.all(r["lengths"][i][marked] == 1)
            assert np.all(base["lengths"][i][marked] > 1)
            assert np.all(np.isfinite(r["out32"][i]))


DEPARTURES = dict(plane_test_against_pos=dict(plane_on_pos=True), xp_under_current_viewproj=dict(project_cur_vp=True), w0_ignored=dict(ignore_w0=True))


@pytest.mark.parametrize("name", DEPARTURES)
def test_departure_is_seen(name):
    """Each one-line departure from the rule moves the float32 output of the moving case by at least 20 E32 from the float64 twin,
    the bar of tests/test_np_denoise.py.  The first two on the main moving case (the pan: both view-projections and the plane test
    matter there); the third needs pixels with w == 0 and runs on that case."""
    kw = dict(w0_block=True) if name == "w0_ignored" else dict(pan=True)
    r = dm.reference(*MAIN, **kw)
    outs, valid, _, _ = dm.replay(r["calls"], np.float32, **DEPARTURES[name])
    assert all(np.array_equal(a, b) for a, b in zip(valid, r["valid"]))
    worst = max(dp.case_err(outs, r["out64"], valid))
    print(f"{name}: {worst:.2e} = {worst / r['E32']:.0f} E32")
    assert worst >= 20 * r["E32"]


def test_unchanged_departure_arguments_change_nothing():
    r = dm.reference(*MAIN)
    outs, _, _, _ = dm.replay(r["calls"][:4], np.float32, **MOTION_VARIANT)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(outs, r["out32"]))


def test_plain_and_motion_calls_mix_on_one_instance():
    """a dict without prevPosition takes the parent's stage: alternating the two on one instance equals, while prev = position, the
    plain replay"""
    calls = dm.case(*MAIN, iterations=1, static_prev=True)
    den = NpMotionDenoiser(*MAIN)
    ref = nd.NpDenoiser(*MAIN)
    for i, c in enumerate(calls[:5]):
        g = c["planes"] if i % 2 else dm.without_motion([c])[0]["planes"]
        a = den.denoise(c["view_proj"], g, out=dm.fill(*MAIN), iterations=1)
        b = ref.denoise(c["view_proj"], dm.without_motion([c])[0]["planes"], out=dm.fill(*MAIN), iterations=1)
        assert np.array_equal(_bits(a), _bits(b))
