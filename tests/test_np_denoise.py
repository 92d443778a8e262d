"""Properties of the numpy restatement of the diffuse denoiser (tests/np_denoise.py), on synthetic planes: what the GPU kernels
are compared against has to behave like a denoiser first."""
import hashlib

import numpy as np
import pytest

import denoise_planes as dp
import denoise_scenes as ds
import np_denoise as nd

F = np.float32
W, H = 48, 32


def _const(v):
    return np.broadcast_to(np.asarray(v, F), (H, W, 3)).copy()


def test_oct_normal_round_trip():
    rng = np.random.default_rng(1)
    n = rng.normal(size=(20000, 3)).astype(F)
    n = np.concatenate([n, np.eye(3, dtype=F), -np.eye(3, dtype=F)])
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)
    bits = nd.oct_encode(n[:, 0], n[:, 1], n[:, 2])
    assert not np.any(bits == nd.INVALID)
    back = np.stack(nd.oct_decode(bits), -1)
    assert np.abs(back - n).max() < 1e-4
    assert np.abs(np.linalg.norm(back, axis=1) - 1).max() < 1e-6


def test_constant_field_comes_back_within_one_ulp():
    z = np.zeros((H, W))
    z[:, W // 2:] = -4.0  # two depths: the filter runs its edge logic too
    z[:3, :5] = np.nan    # and some background
    rad = _const((0.25, 0.125, 0.0625))
    alb = _const((0.5, 0.25, 0.5))
    vp, g = ds.planes(W, H, z, rad, alb)
    want = ds.decode(g["nrdRadianceHitDist"])
    valid = np.isfinite(z)
    den = nd.NpDenoiser(W, H)
    for _ in range(3):
        out = den.denoise(vp, g, iterations=5)
        ulps = np.abs(out[..., :3].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps[valid].max() <= 1
        assert np.all(out[~valid] == 0)


def test_planes_at_different_depths_do_not_mix():
    z = np.zeros((H, W))
    z[:, W // 2:] = -10.0  # right half 10 units behind the left half, same normal
    rad = np.zeros((H, W, 3), F)
    rad[:, : W // 2] = 0.5
    vp, g = ds.planes(W, H, z, rad, _const((0.5, 0.5, 0.5)))
    den = nd.NpDenoiser(W, H)
    for _ in range(2):
        out = den.denoise(vp, g, iterations=5)
        assert out[:, W // 2:, :3].max() < 1e-6  # across-edge contribution
        assert np.abs(out[:, : W // 2, :3] - 0.5).max() < 1e-6


def test_identical_cameras_temporal_only_is_the_running_mean():
    rng = np.random.default_rng(3)
    z = np.zeros((H, W))
    alb = rng.uniform(0.2, 0.9, (H, W, 3)).astype(F)
    den = nd.NpDenoiser(W, H)
    frames = []
    for n in range(12):
        rad = rng.uniform(0, 2, (H, W, 3)).astype(F)
        vp, g = ds.planes(W, H, z, rad, alb)
        frames.append(ds.decode(g["nrdRadianceHitDist"]).astype(np.float64))
        out = den.denoise(vp, g, iterations=0, max_history=32)
        mean = np.mean(frames, axis=0)
        assert np.abs(out[..., :3] - mean).max() <= 2e-6 * max(1.0, mean.max())
        assert np.all(den.mom[..., 2] == n + 1)  # len = min(len_prev, max_history - 1) + 1
    # max_history caps the window: alpha never drops below 1 / max_history
    den2 = nd.NpDenoiser(W, H)
    for n in range(6):
        den2.denoise(vp, g, iterations=0, max_history=4)
    assert np.all(den2.mom[..., 2] == 4)


def test_disoccluded_pixel_restarts_history():
    z = np.zeros((H, W))
    vp, g = ds.planes(W, H, z, _const((0.3, 0.3, 0.3)), _const((0.5, 0.5, 0.5)))
    den = nd.NpDenoiser(W, H)
    den.denoise(vp, g)
    den.denoise(vp, g)
    assert np.all(den.mom[..., 2] == 2)
    z2 = z.copy()
    z2[8:16, 10:20] = 3.0  # a box appears in front of the plane: its pixels have no history
    vp, g2 = ds.planes(W, H, z2, _const((0.3, 0.3, 0.3)), _const((0.5, 0.5, 0.5)))
    den.denoise(vp, g2)
    box = np.zeros((H, W), bool)
    box[8:16, 10:20] = True
    assert np.all(den.mom[..., 2][box] == 1) and np.all(den.mom[..., 2][~box] == 3)
    # reset drops every history; background pixels never get one
    den.reset()
    den.denoise(vp, g2)
    assert np.all(den.mom[..., 2] == 1)


def test_camera_pan_reprojects_history():
    """A pan moves the history with the surface: the pixels that stay on screen keep their length, the newly visible strip restarts."""
    z = np.zeros((H, W))
    den = nd.NpDenoiser(W, H)
    vp0, g0 = ds.planes(W, H, z, _const((0.3, 0.3, 0.3)), _const((0.5, 0.5, 0.5)), eye=(0, 0, 15), center=(0, 0, 0))
    den.denoise(vp0, g0)
    vp1, g1 = ds.planes(W, H, z, _const((0.3, 0.3, 0.3)), _const((0.5, 0.5, 0.5)), eye=(3.0, 0, 15), center=(3.0, 0, 0))
    den.denoise(vp1, g1)
    length = den.mom[..., 2]
    assert (length == 2).mean() > 0.8 and (length == 1).any()
    # the pixels that lost their history are on the side the camera moved towards (+x)
    cols = np.where(np.any(length == 1, axis=0))[0]
    assert cols.min() > W // 2


# ---- the float64 twin and the synthetic planes of tests/denoise_planes.py ------------------------------------------------------
# Error measure everywhere: dp.rel_err, |x - ref| / max(|ref|, 1e-3) per channel at the valid pixels, ref = the float64 twin.
MAIN = dp.SIZES[0]
E32_BOUND = 5e-5  # a condition on the inputs (see test_cases_are_well_conditioned), not on any code


def test_float32_default_is_bit_identical_to_the_restatement_before_the_dtype_parameter(monkeypatch):
    """The digest was taken from the module as it stood before it got a dtype (float32 only, module constant F), over the
    settings script at 17x33: out, colour history, moments and geometry of all eight calls.  exp is pinned to the rounded binary64
    one on both sides, so the digest holds whatever the numpy build makes of the last bit of a binary32 exp."""
    monkeypatch.setattr(nd, "_exp", lambda x: np.exp(np.asarray(x, np.float64)).astype(x.dtype))
    W, H = 17, 33
    den = nd.NpDenoiser(W, H)
    h = hashlib.sha256()
    for c in dp.case(W, H, settings=True):
        out = den.denoise(c["view_proj"], c["planes"], out=dp.fill(W, H), iterations=c["iterations"], max_history=c["max_history"])
        for a in (out, den.hist, den.mom, den.geom_pos, den.geom_oct):
            assert a.dtype in (np.float32, np.uint32)
            h.update(np.ascontiguousarray(a).tobytes())
    assert h.hexdigest() == "a0f5b36643a30335b06ce32661deefeca048093c5c0ebb122c59929a6b787042"


def test_generator_is_deterministic_and_float64_twin_is_float64():
    a, b = dp.case(7, 5), dp.case(7, 5)
    for x, y in zip(a, b):
        assert np.array_equal(x["view_proj"], y["view_proj"])
        assert all(np.array_equal(x["planes"][k], y["planes"][k]) and x["planes"][k].dtype == np.float32 for k in x["planes"])
    r = dp.reference(7, 5)
    assert r["out64"][0].dtype == np.float64 and r["out32"][0].dtype == np.float32
    assert not np.array_equal(dp.case(7, 5, seed=21)[0]["planes"]["nrdRadianceHitDist"], a[0]["planes"]["nrdRadianceHitDist"])


CASES = [dict(W=W, H=H, iterations=K) for W, H in dp.SIZES for K in (0, 5)] + \
        [dict(W=MAIN[0], H=MAIN[1], iterations=K) for K in (1, 2)] + \
        [dict(W=MAIN[0], H=MAIN[1], iterations=0, max_history=mh) for mh in (1, 2)] + \
        [dict(W=W, H=H, settings=True) for W, H in dp.SIZES[:2]] + [dict(W=MAIN[0], H=MAIN[1], nan_frame=5)]


@pytest.mark.parametrize("kw", CASES, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_cases_are_well_conditioned(kw):
    """E32(case) <= 5e-5 for every case the GPU tests use (measured: 1.95e-5 for the main case at K = 5, below for the others).  A
    case above the bound gets another seed, noise level or camera, never another bound.  It also shows that no discontinuous
    decision (tap acceptance, len >= 4, floor, the albedo arms) falls differently in binary32 and binary64: one that did would move
    a pixel by far more than this."""
    r = dp.reference(**kw)
    print(kw, f"E32 {r['E32']:.2e}")
    assert r["E32"] <= E32_BOUND
    fill = dp.fill(kw["W"], kw["H"])
    for o32, o64, v in zip(r["out32"], r["out64"], r["valid"]):
        assert np.array_equal(o32[~v].view(np.uint32), fill[~v].view(np.uint32)) and np.array_equal(o64[~v], fill[~v].astype(np.float64))
        assert np.array_equal(o32[..., 3].view(np.uint32), fill[..., 3].view(np.uint32))


def _enclosed_invalid(valid):
    """the pixels without geometry from which a pixel with geometry is met in all four directions before the image border"""
    H, W = valid.shape
    seen = [np.zeros((H, W), bool) for _ in range(4)]
    for x in range(1, W):
        seen[0][:, x] = seen[0][:, x - 1] | valid[:, x - 1]
        seen[1][:, W - 1 - x] = seen[1][:, W - x] | valid[:, W - x]
    for y in range(1, H):
        seen[2][y] = seen[2][y - 1] | valid[y - 1]
        seen[3][H - 1 - y] = seen[3][H - y] | valid[H - y]
    return ~valid & seen[0] & seen[1] & seen[2] & seen[3]


def test_main_case_reaches_every_branch():
    """Counts from the float64 twin (NpDenoiser.cover) over the twelve calls of the main case."""
    r = dp.reference(*MAIN)
    cover, first = r["cover"], r["cover"][0]
    total = {k: sum(c[k] for c in cover) for k in first}
    print(total)
    for c in cover:
        assert c["nz_neg"] >= 0.2 * c["valid"]
        for k in ("arm_specular", "arm_black", "arm_diffuse", "floored"):
            assert c[k] >= 50, (k, c)
    assert total["taps_accepted"] > 1000
    assert total["taps_plane_only"] > 0 and total["taps_normal_only"] > 0  # rejected by the plane distance / the normal test alone
    assert total["behind_prev"] > 0 and total["q_outside"] > 0
    assert cover[6]["behind_prev"] > 100  # the dolly back
    assert sum(c["var_long"] > 0 for c in cover) >= 3 and sum(c["var_short"] > 0 for c in cover) >= 3
    # the two still frames: q = p exactly, one tap of weight 1 per pixel
    assert cover[4]["taps_accepted"] == cover[4]["valid"] and cover[5]["taps_accepted"] == cover[5]["valid"]
    # the call after reset() takes no history
    assert cover[8]["taps_accepted"] == 0 and np.all(r["lengths"][8][r["valid"][8]] == 1)
    # background inside geometry, and every one-sided arm of the viewZ gradient
    v = r["valid"][0]
    hole = _enclosed_invalid(v)
    assert hole.sum() >= 8
    ys, xs = np.nonzero(hole)
    assert v[ys, xs - 1].any() and v[ys, xs + 1].any() and v[ys - 1, xs].any() and v[ys + 1, xs].any()
    # the history length reaches max_history
    for mh in (1, 2):
        r2 = dp.reference(*MAIN, iterations=0, max_history=mh)
        assert all(ln[va].max() <= mh for ln, va in zip(r2["lengths"], r2["valid"]))
        assert (r2["lengths"][3][r2["valid"][3]] == mh).mean() > 0.8
    assert r["lengths"][5].max() == 6 and r["lengths"][11].max() == 4


MUTATIONS = dict(
    b3_corner_weight=dict(b3_end=0.06), g3_centre_edge_swapped=dict(g3=(0.25, 0.5)), six_squarings=dict(squarings=6),
    sigma_l_4p1=dict(sigma_l=4.1), ez_eps_1p1em3=dict(ez_eps=1.1e-3), three_over_len=dict(short_scale=3.0), len_ge_5=dict(long_len=5.0),
    central_difference=dict(central_grad=True), fx_fy_swapped=dict(swap_fxfy=True), plane_tolerance_0p011=dict(plane_tol=0.011),
    normal_test_0p5=dict(normal_cos=0.5), min_of_tap_lengths=dict(len_min=True), oct_fold_sign_dropped=dict(fold_sign=False),
    specular_test_0p9=dict(spec=0.9), amax_ge_0=dict(amin=0.0), channel_floor_dropped=dict(floor=False))


@pytest.mark.parametrize("name", MUTATIONS)
def test_mutation_is_seen(name):
    """Each departure from the kernels' formulas, applied to the float32 restatement, moves its worst frame of the main case by at
    least 20 E32 from the float64 twin: five times the bar the GPU output is held to (4 E32).  Measured: the smallest is the B3
    corner weight at 137 E32."""
    r = dp.reference(*MAIN)
    outs, valid, _, _ = dp.replay(r["calls"], np.float32, **MUTATIONS[name])
    assert all(np.array_equal(a, b) for a, b in zip(valid, r["valid"]))
    worst = max(dp.case_err(outs, r["out64"], valid))
    print(f"{name}: {worst:.2e} = {worst / r['E32']:.0f} E32")
    assert worst >= 20 * r["E32"]


def test_unmutated_variant_arguments_change_nothing():
    r = dp.reference(*MAIN)
    outs, _, _, _ = dp.replay(r["calls"][:5], np.float32, **nd.VARIANT)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(outs, r["out32"]))


def test_one_nan_sample_counts_as_black():
    """One pixel's Y is NaN in call 5 of 12: every output of that and all later calls is finite, in both dtypes, and bit for bit
    what a black sample (Y = Co = Cg = 0) at that pixel gives."""
    r = dp.reference(*MAIN, nan_frame=5)
    rad = r["calls"][5]["planes"]["nrdRadianceHitDist"]
    ys, xs = np.nonzero(np.isnan(rad[..., 0]))
    assert len(ys) == 1 and r["valid"][5][ys[0], xs[0]]
    for o32, o64 in zip(r["out32"], r["out64"]):
        assert np.isfinite(o32).all() and np.isfinite(o64).all()
    calls = [dict(c) for c in r["calls"]]
    black = {k: v.copy() for k, v in calls[5]["planes"].items()}
    black["nrdRadianceHitDist"][ys[0], xs[0], :3] = 0
    calls[5]["planes"] = black
    outs, _, _, _ = dp.replay(calls, np.float32)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(outs, r["out32"]))
    clean = dp.reference(*MAIN)
    assert not np.array_equal(clean["out32"][5], r["out32"][5]) and np.array_equal(clean["out32"][4], r["out32"][4])
