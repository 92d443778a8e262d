"""The hit shader's BRDF tail on the record strata of tests/shade_records.py, on the CPU: the oracle (orc_eval_shade) against the numpy
restatement in binary32 and against the same text evaluated in binary64 (np_shading.shade(rec, dtype)).

  * the three agree on WHICH outputs are non-finite, word for word, on every record of every stratum (and on which of those are NaN,
    and on the sign of the infinities).  Only the `light` stratum holds such records: a light exactly at the hit point gives
    L = 0 / 0 = NaN, which rchit:166 sends into the NEE branch (`dot(L, N) <= 0` is false), so hitValue and shadowRayDir are NaN there
    (lightDist is 0); at a hit offset by 1e5 the "hair away" light rounds onto the hit point and does the same.  Records whose
    twin is non-finite where a binary32 evaluation is finite, or the other way round: none in any stratum (the cap is 1 %).
  * the discrete outputs -- lobe, PRNG state, ray origin -- are equal on every record.  No stratum produces a lobe disagreement (a draw
    within rounding of `ratio`), so none is excused.
  * oracle against numpy binary32, every record bounded: the bar is four times the maximum measured when
    profiles/shade_records_parity.json was taken (numpy's sin / cos / power may differ between builds by an ulp, which conditioning
    amplifies; an output that uses sqrt and division only, such as lightDist, measures 0 and must stay equal).
  * against the twin, per stratum and output: the oracle's maximum error and 0.999-quantile are at most 1.5 times numpy binary32's, and
    fewer than 0.5 % of the records have an oracle error above twice numpy binary32's + 1e-6.  An error both binary32 evaluations share
    is conditioning (DESIGN.md section 3 says where); one the oracle has alone is a wrong term.

VKRT_SHADE_PARITY_JSON=<file> writes the measured figures there (how profiles/shade_records_parity.json was taken)."""
import json
import os

import numpy as np
import pytest

import np_shading
import shade_records as sr

WHAT = ("tests/test_shade_records.py on the CPU: oracle (orc_eval_shade) vs oracle/np_shading.py in binary32 and in binary64 (the twin), "
        "on the strata of tests/shade_records.py. Relative error of a row and output: max |x - y| / (max |.| of the row over both + 1e-3); "
        "_abs: max |x - y|; share_over_twice: share of rows with oracle error > 2 x numpy32 error + 1e-6. "
        "Rows with a non-finite word of the output are not measured (nonfinite_rows; the three evaluations agree on them). "
        "Taken with VKRT_SHADE_PARITY_JSON set.")


def test_strata_hold_what_they_claim():
    total = sum(sr.records(s).shape[0] for s in sr.STRATA)
    assert total < 100000 and all(sr.records(s).shape[0] >= 2000 for s in sr.STRATA)
    bits = lambda rec, w: np.ascontiguousarray(rec[:, w]).view(np.int32)  # noqa: E731
    m = sr.records("material")
    assert set(m[:, 20].tolist()) == {float(np.float32(x)) for x in sr.ROUGHNESS} and set(m[:, 19].tolist()) == {float(np.float32(x)) for x in sr.METALLIC}
    combos = {(r, me, e > 0, d, s) for r, me, e, d, s in zip(m[:, 20].tolist(), m[:, 19].tolist(), m[:, 21].tolist(), bits(m, 33).tolist(), bits(m, 34).tolist())}
    assert len(combos) == 7 * 6 * 2 * 3 * 2 and set(map(tuple, m[:, 15:18].tolist())) == {(a, b, c) for a in (0.0, 1.0) for b in (0.0, 1.0) for c in (0.0, 1.0)}
    v = sr.records("view")
    D = v[:, 12:15].astype(np.float64)
    length = np.linalg.norm(D, axis=1)
    ndv = -(D * v[:, 3:6]).sum(1) / length
    i = np.arange(len(v))
    assert np.allclose(ndv, np.array(sr.N_DOT_V)[i % 7], rtol=0, atol=3e-7) and np.allclose(length / np.array(sr.RAY_LENGTH)[(i // 7) % 3], 1.0, atol=1e-6)
    assert {(x, y) for x, y in zip((i % 7).tolist(), ((i // 7) % 3).tolist())} == {(x, y) for x in range(7) for y in range(3)}
    l = sr.records("light")
    i = np.arange(len(l))
    place = i % 5
    ldir = l[:, 24:27].astype(np.float64) - l[:, 0:3]
    dist = np.linalg.norm(ldir, axis=1)
    near_origin = np.abs(l[:, 0:3]).max(1) < 10
    ln = (ldir * l[:, 3:6]).sum(1)
    assert np.all(np.abs(ln[(place == 0) & near_origin]) < 1e-5) and np.all(ln[(place == 1)] < 0) and np.all(dist[place == 3] == 0)
    assert np.allclose(dist[(place == 2) & near_origin], 1e-4, rtol=0.05) and np.all(dist[place == 4] > 9e4) and (~near_origin).sum() == len(l) // 2
    assert {(p, t, c, f) for p, t, c, f in zip(place.tolist(), bits(l, 31).tolist(), bits(l, 35).tolist(), near_origin.tolist())} == \
        {(p, t, c, f) for p in range(5) for t in sr.LIGHT_TYPES for c in sr.LIGHTS_COUNT for f in (False, True)}
    d = sr.records("draws")
    dv = sr.draw_values(d)
    i = np.arange(len(d))
    assert np.array_equal(dv[i, i % 4], np.where((i // 4) % 2 == 0, 0, 0x00FFFFFF))
    _, a, _, _ = sr.evaluate("draws")
    first, zero, metal = (i % 4 == 0), ((i // 4) % 2 == 0), d[:, 19]
    # r1 = 0 is below ratio = 0.5 and 1 (diffuse) and not below ratio = 0 (specular); r1 = 1 - 2^-24 is below ratio = 1 only
    assert np.all(a[first & zero & (metal != 1), 12] == 0) and np.all(a[first & zero & (metal == 1), 12] == 1)
    assert np.all(a[first & ~zero & (metal != -1), 12] == 1) and np.all(a[first & ~zero & (metal == -1), 12] == 0)
    # the second draw of a diffuse record is the light index: draw 0x00FFFFFF reaches the top index and not lightsCount itself
    top = (i % 4 == 1) & ~zero & (a[:, 12] == 0)
    lc = bits(d, 35)[top]
    idx = (np.float32(0x00FFFFFF) / np.float32(16777216.0) * lc.astype(np.float32)).astype(np.int32)
    assert top.sum() > 50 and set(lc.tolist()) == {3, 16} and np.array_equal(idx, lc - 1)
    # the cosine sampler's sqrt(r1) = 0 and sqrt(1 - r1) = 2^-12 (third draw, diffuse), the GGX sampler's cosTheta = 1 (third draw = 0, specular)
    third = i % 4 == 2
    assert (third & zero & (a[:, 12] == 0)).sum() > 50 and (third & ~zero & (a[:, 12] == 0)).sum() > 50 and (third & (a[:, 12] == 1)).sum() > 50
    assert set(metal.tolist()) == set(sr.DRAWS_METALLIC) and len(d) == 4 * 2 * 3 * 2 * 64
    f = sr.records("frame")
    nn = np.linalg.norm(f[:, 3:6].astype(np.float64), axis=1)
    k = np.arange(len(f)) % 5
    assert np.array_equal(f[k == 0, 6:9], f[k == 0, 3:6]) and np.all(f[k == 1, 6:9] == 0)
    assert np.allclose(nn[k == 2], 0.5, atol=1e-6) and np.allclose(nn[k == 3], 2.0, atol=1e-6)
    assert np.all((np.cross(f[k == 4, 3:6].astype(np.float64), f[k == 4, 6:9]) * f[k == 4, 9:12]).sum(1) < 0)


def test_seed_inversion_round_trips():
    """seed_for_draw against the forward LCG of the restatement, for all four depths."""
    state = np.array([0, 0x00FFFFFF, 0xAB000000, 0x12FFFFFF, 0xFFFFFFFF], np.uint64)
    for k in range(1, 5):
        s = sr.seed_for_draw(k, state)
        for _ in range(k):
            s, _bits = np_shading._lcg(s)
        assert np.array_equal(s, state.astype(np.uint32))


def test_nan_light_direction_takes_the_nee_branch():
    """Named regression (rchit:166): a light at the hit point makes L NaN; `dot(L, N) <= 0` is false, so NEE runs and the hit value is
    NaN in the oracle, in the restatement and in the twin.  (The restatement used to write `dot > 0`, the opposite choice.)"""
    rec = sr.records("default")[:64].copy()
    rec[:, 24:27] = rec[:, 0:3]
    rec[:, 19] = 0.0                                    # ratio 0.5: about half of the records take the diffuse lobe
    rec[:, 31] = np.zeros(64, np.int32).view(np.float32)  # point light
    import oracle_py

    with np.errstate(all="ignore"):
        rows = [oracle_py.eval_shade(rec), np_shading.shade(rec), np_shading.shade(rec, np.float64)]
    diffuse = rows[0][:, 12] == 0
    assert 10 < diffuse.sum() < 54
    for r in rows:
        assert np.isnan(r[diffuse, 0:3]).all() and np.isnan(r[diffuse, 14:17]).all() and np.all(r[diffuse, 13] == 0)
        assert np.isfinite(r[~diffuse, 0:17]).all()


@pytest.mark.parametrize("name", sr.STRATA)
def test_nonfinite_outputs_are_the_same_set(name):
    _, a, b, t = sr.evaluate(name)
    a, b, t = a[:, :17], b[:, :17], t[:, :17]
    for other, what in ((b, "numpy binary32"), (t, "binary64 twin")):
        assert np.array_equal(np.isnan(a), np.isnan(other)), (name, what, np.argwhere(np.isnan(a) != np.isnan(other))[:4].tolist())
        assert np.array_equal(np.isinf(a), np.isinf(other)), (name, what, np.argwhere(np.isinf(a) != np.isinf(other))[:4].tolist())
        inf = np.isinf(a)
        assert np.array_equal(np.sign(a[inf]), np.sign(other[inf])), (name, what)
    if name != "light":
        assert np.isfinite(a).all(), name


@pytest.mark.parametrize("name", sr.STRATA)
def test_discrete_outputs_are_equal(name):
    rec, a, b, t = sr.evaluate(name)
    state = np.ascontiguousarray(a[:, 17]).view(np.uint32)
    for other, what in ((b, "numpy binary32"), (t, "binary64 twin")):
        assert np.array_equal(a[:, 12], other[:, 12]), (name, what, "lobe", int((a[:, 12] != other[:, 12]).sum()))
        assert np.array_equal(state, np_shading.out_seed(other)), (name, what, "PRNG state")
        assert np.array_equal(a[:, 3:6], other[:, 3:6]), (name, what, "ray origin")
    assert np.array_equal(a[:, 3:6], rec[:, 0:3]) and np.all(a[:, 18:20] == 0)
    # the state is the record's seed advanced by the lobe's draws: four on the diffuse lobe, three on the specular one
    s = np.ascontiguousarray(rec[:, 32]).view(np.uint32)
    steps = []
    for _ in range(4):
        s, _bits = np_shading._lcg(s)
        steps.append(s)
    assert np.array_equal(state, np.where(a[:, 12] == 0, steps[3], steps[2]))


@pytest.mark.parametrize("name", sr.STRATA)
def test_oracle_agrees_with_numpy_binary32_on_every_record(name):
    sr.check_parity(name)


@pytest.mark.parametrize("name", sr.STRATA)
def test_oracle_is_no_further_from_the_twin_than_numpy_binary32(name):
    got = sr.measure(name)
    for _, _, what in sr.OUTPUTS:
        g = got[what]
        print(f"{name} {what}: vs twin max {g['oracle_vs_twin_max']:.3e} / {g['numpy32_vs_twin_max']:.3e}, q999 {g['oracle_vs_twin_q999']:.3e} / "
              f"{g['numpy32_vs_twin_q999']:.3e}, share over twice {g['share_over_twice']:.4%}")
        assert g["oracle_vs_twin_max"] <= 1.5 * g["numpy32_vs_twin_max"], (name, what)
        assert g["oracle_vs_twin_q999"] <= 1.5 * g["numpy32_vs_twin_q999"], (name, what)
        assert g["share_over_twice"] < 0.005, (name, what)


def test_collect_parity_json():
    """VKRT_SHADE_PARITY_JSON=<file>: write the measured figures there; without it, the committed file must cover every stratum and output."""
    path = os.environ.get("VKRT_SHADE_PARITY_JSON")
    if path:
        strata = {}
        for name in sr.STRATA:
            _, a, _, _ = sr.evaluate(name)
            strata[name] = {"records": int(a.shape[0]), "nonfinite_rows": int((~np.isfinite(a[:, :17])).any(1).sum()), "outputs": sr.measure(name)}
        with open(path, "w") as f:
            json.dump({"what": WHAT, "strata": strata}, f, indent=1)
            f.write("\n")
    bars = sr.committed_figures()
    assert set(bars) == set(sr.STRATA)
    for name in sr.STRATA:
        assert bars[name]["records"] == sr.records(name).shape[0] and set(bars[name]["outputs"]) == {w for _, _, w in sr.OUTPUTS}
