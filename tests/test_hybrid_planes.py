"""CPU checks that make tests/test_gpu_hybrid_planes.py mean something: the synthetic planes of tests/hybrid_planes.py reach the branches
they are built for (counted from the oracle alone: conditions on the inputs, not measurements), the oracle's answer for them does not
depend on its tree, the numpy restatement reads the shader the same way, and oracle_py.post is float64's pow on all six arms.

One branch of the list cannot be reached: hybridStorePixel's clamp of the radiance at 65504.  Every segment adds
min(prd.hitValue * curWeight, 10) (rgen:250), so a finite radiance is at most 10 (depth - 1) <= 70 whatever the albedo, and a
non-finite one is replaced by 0 before the clamp.  The other side of the clamp, a negative radiance (albedo -0.25) stored as 0, is
reached and counted instead."""
import numpy as np
import pytest

import hybrid_planes as hp
import oracle_py

F = np.float32


def _alpha_decode(alpha):
    """alpha = max(visibility, 0.01) * (1 - ao / 4) of a frame-0 pixel -> (shadowed: 1 / 0 / -1 unknown, ao count 0..4 or -1)"""
    table = {}
    for vis in (1.0, 0.01):
        for ao in range(5):
            a = F(F(1.0) * F(vis)) * F(F(1.0) - F(ao) * F(0.25))
            table.setdefault(F(a).tobytes(), []).append((0 if vis == 1.0 else 1, ao))
    out = np.full(alpha.shape + (2,), -1, np.int32)
    for idx in np.ndindex(alpha.shape):
        m = table.get(F(alpha[idx]).tobytes())
        if m:
            out[idx] = m[0] if len(m) == 1 else (-1, m[0][1])  # (alpha 0: four AO hits, either visibility)
    return out[..., 0], out[..., 1]


@pytest.fixture(scope="module")
def coverage():
    """Branch counts over the case list, from the oracle's frame-0 replay of every non-degenerate case and the ray log of every
    shaded pixel (hybrid_pixel_rays).  Also the per-case ray totals of the logs, which must be the counters."""
    cov = {k: 0 for k in ("no_shadow_ray_dot_negative", "shadow_ray_tmax_le_tmin", "shadow_blocked", "shadow_unblocked", "mirror_first_ray",
                          "miss_at_depth_1", "hitdist_halved", "hitdist_not_halved", "radiance_negative_stored_as_zero", "norm_hit_dist_0",
                          "norm_hit_dist_1", "norm_hit_dist_between", "terminator_dot_negative", "terminator_dot_not_negative")}
    cov.update({f"ao_{k}": 0 for k in range(5)})
    cov.update({f"gi_path_length_{k}": 0 for k in range(8)})
    cov.update({f"boundary_side_{k}": 0 for k in range(1, 7)})
    cov["boundary_mirror"] = {k: set() for k in range(1, 7)}
    for name in hp.NON_DEGENERATE:
        c = hp.CASES[name]
        W, H = c["size"]
        sh, ao_on, gi_on = c["toggles"]
        ref = hp.reference(name)
        g, meta = ref["g"], ref["meta"]
        r0 = ref if c["frame"] == 0 else hp.oracle_run(name, frame=0)
        _, orc, _ = hp.scene(c["scene"])
        cam = hp.camera(c["scene"], W, H)
        pc = hp.push_constants(name, frame=0)
        shadowed, ao = _alpha_decode(r0["accum"][..., 3])
        n_closest = n_shadow = 0
        first_o, first_d = [], []
        for y, x in zip(*np.nonzero(ref["shaded"])):
            acc, rays = orc.hybrid_pixel_rays(pc, cam, W, int(x), int(y), g, seed=c["seed"], flags=c["row_major"], use_bvh=True)
            assert np.array_equal(hp.bits(acc), hp.bits(r0["accum"][y, x])), (name, x, y)
            direct = rays[rays[:, 6] == F(0.1)]
            gi = rays[rays[:, 6] == F(0.001)]
            assert len(direct) + len(gi) == len(rays)
            closest = gi[gi[:, 8] == 0]
            n_closest += len(closest)
            n_shadow += len(rays) - len(closest)
            kind = hp.KINDS[meta["kind"][y, x]]
            if sh:
                traced = len(direct) == 4 * ao_on + 1
                cov["no_shadow_ray_dot_negative"] += not traced
                if kind == "terminator":
                    cov["terminator_dot_negative" if not traced else "terminator_dot_not_negative"] += 1
                if traced:
                    cov["shadow_ray_tmax_le_tmin"] += bool(direct[0, 7] <= direct[0, 6])
                    cov["shadow_blocked"] += shadowed[y, x] == 1
                    cov["shadow_unblocked"] += shadowed[y, x] == 0
            if ao_on and ao[y, x] >= 0:
                cov[f"ao_{ao[y, x]}"] += 1
            if gi_on:
                mirror = bool(hp.mirror_like(g["roughMetal"][y, x]))
                cov["mirror_first_ray"] += mirror and len(closest) > 0
                cov[f"gi_path_length_{len(closest)}"] += 1
                side = meta["variant"][y, x] // 100 if kind == "material" else 0
                if side:
                    cov[f"boundary_side_{side}"] += 1
                    cov["boundary_mirror"][side].add(mirror)
                if not mirror and len(closest) == 1 and len(gi) == 1 and c["depth"] > 2:
                    first_o.append(closest[0, :3]); first_d.append(closest[0, 3:6])
                w = r0["rad"][y, x, 3]
                cov["norm_hit_dist_0"] += w == 0
                cov["norm_hit_dist_1"] += w == 1
                cov["norm_hit_dist_between"] += 0 < w < 1
                cov["radiance_negative_stored_as_zero"] += bool((r0["accum"][y, x, :3] < 0).any())
                if not mirror and len(gi) >= 2 and gi[1, 8] == 1:  # diffuse first segment with its shadow ray: lightDist = tmax + 0.1
                    rough, vz = float(g["roughMetal"][y, x, 0]), float(g["nrdViewZ"][y, x])
                    t = min(max(2.0 ** (-25.0 * rough * rough), 0.0), 1.0)
                    f = (3.0 + abs(vz)) * ((1.0 - t) + 20.0 * t)
                    full, half = np.clip((float(gi[1, 7]) + 0.1) / f, 0, 1), np.clip(0.5 * (float(gi[1, 7]) + 0.1) / f, 0, 1)
                    if abs(full - half) > 8e-3 * full:  # (apart by more than the binary16 step and the 0.1 added back in float64)
                        cov["hitdist_not_halved"] += abs(w - full) <= 2e-3 * full
                        cov["hitdist_halved"] += abs(w - half) <= 2e-3 * half
        if first_o:
            _, _, _, gid, _ = orc.trace_rays(np.array(first_o), np.array(first_d), 0.001, 10000.0)
            cov["miss_at_depth_1"] += int((gid < 0).sum())
        assert (n_closest, n_shadow) == (ref["counters"]["rays_closest"], ref["counters"]["rays_shadow"]), name
        assert ref["counters"]["pixels"] == W * H
    return cov


BRANCHES_16 = ["no_shadow_ray_dot_negative", "shadow_ray_tmax_le_tmin", "shadow_blocked", "shadow_unblocked", "mirror_first_ray", "miss_at_depth_1",
               "hitdist_halved", "hitdist_not_halved", "radiance_negative_stored_as_zero", "norm_hit_dist_0", "norm_hit_dist_1", "norm_hit_dist_between"]
BRANCHES_16 += [f"ao_{k}" for k in range(5)] + [f"gi_path_length_{k}" for k in range(8)]


@pytest.mark.parametrize("branch", BRANCHES_16)
def test_every_branch_is_taken_by_16_pixels(coverage, branch):
    """gi_path_length_k: k closest-hit rays, every k from 0 to the largest depth - 1 = 7"""
    assert coverage[branch] >= 16, (branch, coverage[branch])


def test_both_sides_of_the_boundary_and_of_the_terminator(coverage):
    """at least 4 pixels on each of the six sides of ratio = 0.8 (below / at / above around (0, 0.8) by the metalness, above / at / below
    around (0.2f, 1) by the roughness) and of each sign of dot(L, N) on the terminator; `at` and `above` take the mirror arm, `below`
    the diffuse one, in binary32"""
    for side in range(1, 7):
        assert coverage[f"boundary_side_{side}"] >= 4, side
    want = {1: {False}, 2: {True}, 3: {True}, 4: {True}, 5: {True}, 6: {False}}
    assert coverage["boundary_mirror"] == want
    assert coverage["terminator_dot_negative"] >= 4 and coverage["terminator_dot_not_negative"] >= 4


def test_case_list_is_what_the_gpu_test_needs():
    cs = hp.CASES
    assert {c["toggles"] for c in cs.values()} == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    assert {c["depth"] for c in cs.values()} == {0, 1, 2, 5, 8}
    assert {c["frame"] for c in cs.values()} == {0, 1, 7}
    assert {c["row_major"] for c in cs.values()} == {0, 1} and {c["lights"] for c in cs.values()} == {1, "all"}
    assert {c["size"] for c in cs.values()} == set(hp.SIZES) and max(w * h for w, h in hp.SIZES) == 72 * 40
    assert not hp.reference("all-clear")["shaded"].any() and hp.reference("single")["shaded"].sum() == 1
    layouts, kinds = set(), set()
    for name in hp.NON_DEGENERATE:
        r = hp.reference(name)
        layouts |= set(np.unique(r["meta"]["layout"]))
        kinds |= set(np.unique(r["meta"]["kind"]))
        assert not r["meta"]["degenerate"].any()
        old = hp.old_accum(name)
        assert old.min() >= -2 and old.max() <= 50 and (old.size < 400 or ((old < 0).any() and (old > 40).any()))
    assert layouts == set(range(len(hp.LAYOUTS))) and kinds == set(range(len(hp.KINDS))) - {hp.K["degenerate"]}
    d = hp.reference("degenerate")
    assert set(np.unique(d["meta"]["variant"][d["meta"]["degenerate"]])) == set(range(8))
    # the tiles of the plain layouts hold 0, 1, 63 and 64 shaded lanes; the clear lanes use -0.0 and .w values other than 1
    r = hp.reference("cornell-all")
    per_tile = {int(r["shaded"][y:y + 8, x:x + 8].sum()) for y in range(0, 40, 8) for x in range(0, 72, 8)}
    assert {0, 1, 63, 64, 32, 8} <= per_tile
    clear = ~r["shaded"]
    assert np.signbit(r["g"]["position"][clear][:, :3]).any() and (r["g"]["normal"][clear][:, 3] != 1).any()


@pytest.mark.parametrize("name", [n for n, c in hp.CASES.items() if c["scene"] == "cornell"])
def test_oracle_answer_does_not_depend_on_its_tree(name):
    """Cornell: the tree walk and the loop over all triangles give the same words and the same counters"""
    a, b = hp.reference(name), hp.oracle_run(name, use_bvh=False)
    for k in ("accum", "rad"):
        assert np.array_equal(hp.bits(a[k]), hp.bits(b[k])), k
    for k in ("rays_closest", "rays_shadow", "pixels", "hits", "diffuse_hits", "tex_taps"):
        assert a["counters"][k] == b["counters"][k], k


RESTATEMENT_PER_KIND = 40


@pytest.mark.parametrize("bar", ["hybrid_d2", "hybrid"])
def test_second_restatement_agrees_on_the_planes(bar):
    """np_pathtrace.hybrid_pixels (the shader read a second time, brute-force float64 ray queries) against the oracle with the bars of
    tests/test_second_restatement.py: "hybrid_d2" for the cases up to depth 2, "hybrid" for the deeper ones.  Those bars are statistics of
    an image of about a thousand pixels (a share of pixels, a relative difference of the ray totals), so the pixels of all cases under
    one bar are taken together: up to RESTATEMENT_PER_KIND of every kind of every case (the first in row order), clear pixels included."""
    import np_pathtrace as npt
    from test_second_restatement import check

    got, want, rays_np, rays_orc = [], [], np.zeros(2, np.int64), np.zeros(2, np.int64)
    for name in hp.NON_DEGENERATE:
        c = hp.CASES[name]
        if (c["depth"] <= 2) != (bar == "hybrid_d2"):
            continue
        W, H = c["size"]
        ref = hp.reference(name)
        g, meta = ref["g"], ref["meta"]
        pick = np.zeros((H, W), bool)
        for k in np.unique(meta["kind"]):
            ys, xs = np.nonzero(meta["kind"] == k)
            pick[ys[:RESTATEMENT_PER_KIND], xs[:RESTATEMENT_PER_KIND]] = True
        ys, xs = np.nonzero(pick)
        orc = hp.scene(c["scene"])[1]
        sc = _np_scene(c["scene"])
        sc.rays_closest = sc.rays_shadow = 0
        pc = hp.push_constants(name)
        cam = hp.camera(c["scene"], W, H)
        vi = np.array(list(cam.viewInverse.m), F)  # column-major, as GlobalUniforms stores it
        gp = {k: g[k][ys, xs] for k in ("color", "position", "normal", "roughMetal")}
        old = hp.old_accum(name)[ys, xs] if pc.frame > 0 else None
        with np.errstate(all="ignore"):
            got.append(npt.hybrid_pixels(sc, pc, vi, W, H, c["seed"], xs, ys, gp, accum_old=old, row_major_seed=bool(c["row_major"])))
        want.append(ref["accum"][ys, xs])
        rays_np += (sc.rays_closest, sc.rays_shadow)
        for y, x in zip(ys, xs):  # the oracle's ray counts of the same pixels, from their logs
            _, rays = orc.hybrid_pixel_rays(pc, cam, W, int(x), int(y), g, seed=c["seed"], flags=c["row_major"], use_bvh=True)
            rays_orc += (int(((rays[:, 6] == F(0.001)) & (rays[:, 8] == 0)).sum()), int((rays[:, 8] == 1).sum()))
    got, want = np.concatenate(got), np.concatenate(want)
    print(f"{bar}: {len(got)} pixels, rays restatement {rays_np.tolist()} oracle {rays_orc.tolist()}")
    check(bar, got, want, rays_np, rays_orc)


_NP_SCENES = {}


def _np_scene(name):
    import np_pathtrace as npt

    if name not in _NP_SCENES:
        _NP_SCENES[name] = npt.NpScene(hp.scene(name)[0])
    return _NP_SCENES[name]


@pytest.mark.parametrize("arm", hp.POST_ARMS)
def test_oracle_post_is_float64_pow_on_every_arm(arm):
    m, r = hp.post_inputs(257)
    want = hp.post_float64(m, r, *arm)
    assert np.isnan(want).any() and np.isinf(want).any() and (want == 0).any()
    hp.assert_post(oracle_py.post(m, r, *arm), want)
