"""Record strata for the hit shader's BRDF tail (oracle.cpp orc_eval_shade / vkrt_debug_eval_shade: 40 floats in, 20 out), with no GPU
dependency: tests/test_shade_records.py (oracle against the numpy restatement and its binary64 twin) and
tests/test_gpu_shade_records.py (device against oracle, bit for bit) evaluate the same records.

Every stratum starts from np_shading.random_records with a fixed seed and overwrites the fields that define it; the crossed factors
cycle with the record index, so every combination occurs and the rest of the record stays random.

  default   the generator as it is
  material  roughness and metalness at and beyond the clamps, base-colour components 0 and 1, emissive x depth x isSpecular
  view      N.V from 0.1 down to 0 and below the surface, ray directions of length 1e-3, 1 and 1e3
  light     the light in the tangent plane, behind, at 1e-4, at the hit point, at 1e5; every light type; lightsCount 1..16; far hits
  draws     seeds whose first, second, third or fourth draw is exactly 0 or exactly (2^24 - 1) / 2^24
  frame     degenerate shading frames: tangent parallel to N, zero tangent, non-unit N, left-handed binormal
"""
import json
import os

import numpy as np

import np_shading

F = np.float32
LCG_A, LCG_C = 1664525, 1013904223
LCG_A_INV = pow(LCG_A, -1, 2 ** 32)  # the multiplier is odd

ROUGHNESS = (0.0, 0.005, 0.01, 0.99, 1.0, 1.5, -0.2)
METALLIC = (0.0, 0.01, 0.99, 1.0, 1.2, -0.3)
N_DOT_V = (1e-1, 1e-2, 1e-3, 1e-4, 0.0, -1e-2, -0.5)
RAY_LENGTH = (1e-3, 1.0, 1e3)
LIGHT_PLACES = ("plane", "behind", "near", "at_p", "far")
LIGHT_TYPES = (0, 1, 2, -1)
LIGHTS_COUNT = (1, 2, 3, 8, 16)
DRAWS_METALLIC = (0.0, 1.0, -1.0)
FRAMES = ("tangent_parallel", "tangent_zero", "normal_half", "normal_double", "left_handed")

STRATA = ("default", "material", "view", "light", "draws", "frame")


def _base(n, seed):
    return np_shading.random_records(n, np.random.default_rng(seed))


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _set_bits(rec, word, values):
    rec[:, word] = np.ascontiguousarray(values, np.int64).astype(np.uint32).view(F)


def _tangential(rec, rng):
    """A random unit vector in the tangent plane of each record, in binary64 (the record's N is unit only to binary32 rounding, hence
    the division; the second pass removes what cancellation left of a t that was nearly parallel to N)."""
    N = rec[:, 3:6].astype(np.float64)
    t = rng.standard_normal(N.shape)
    for _ in range(2):
        t = _unit(t - (t * N).sum(1, keepdims=True) / (N * N).sum(1, keepdims=True) * N)
    return t


def default(n=20000, seed=5):
    return _base(n, seed)


def material(n=4032, seed=11):
    """7 roughness x 6 metalness x 12 (emissive on/off x depth {0, 1, 3} x isSpecular {0, 1}) x 8 base colours of {0, 1}^3."""
    rec = _base(n, seed)
    i = np.arange(n)
    rec[:, 20] = np.array(ROUGHNESS, F)[i % 7]
    rec[:, 19] = np.array(METALLIC, F)[(i // 7) % 6]
    e = (i // 42) % 12
    rec[:, 21:24] = np.where((e % 2 == 1)[:, None], np.array([1.5, 0.25, 3.0], F), F(0))
    _set_bits(rec, 33, np.array([0, 1, 3])[(e // 2) % 3])
    _set_bits(rec, 34, e // 6)
    c = (i // 504) % 8
    rec[:, 15:18] = np.stack([c & 1, (c >> 1) & 1, (c >> 2) & 1], 1).astype(F)
    return rec


def view(n=4200, seed=12):
    """V = c N + sqrt(1 - c^2) t for c = N.V of the list and a random tangential t; worldRayDir = -V times the length."""
    rng = np.random.default_rng(seed + 1000)  # (not the generator's own stream: its first draw is N)
    rec = _base(n, seed)
    i = np.arange(n)
    c = np.array(N_DOT_V)[i % 7][:, None]
    length = np.array(RAY_LENGTH)[(i // 7) % 3][:, None]
    V = c * rec[:, 3:6].astype(np.float64) + np.sqrt(1.0 - c * c) * _tangential(rec, rng)
    rec[:, 12:15] = (-V * length).astype(F)
    return rec


def light(n=4000, seed=13):
    """5 placements x 4 types x 5 lightsCount x {near the origin, hit offset by 1e5}."""
    rng = np.random.default_rng(seed + 1000)  # (not the generator's own stream: its first draw is N)
    rec = _base(n, seed)
    i = np.arange(n)
    place = i % 5
    far_hit = (i // 100) % 2 == 1
    rec[:, 0:3] += np.where(far_hit[:, None], F(1e5), F(0))
    P = rec[:, 0:3].astype(np.float64)
    N = rec[:, 3:6].astype(np.float64)
    t = _tangential(rec, rng)
    up = _unit(N + 0.9 * _unit(rng.standard_normal((n, 3))))
    d = rng.uniform(1.0, 9.0, (n, 1))
    pos = np.where((place == 0)[:, None], P + d * t,                       # L.N = 0 as nearly as binary32 allows
          np.where((place == 1)[:, None], P + d * _unit(t - rng.uniform(0.05, 2.0, (n, 1)) * N),  # behind the surface
          np.where((place == 2)[:, None], P + 1e-4 * up,                   # a hair away (at a far hit: within an ulp of P, or P itself)
          np.where((place == 3)[:, None], P, P + 1e5 * up))))              # at the hit point itself; far away
    rec[:, 24:27] = pos.astype(F)
    rec[place == 3, 24:27] = rec[place == 3, 0:3]
    _set_bits(rec, 31, np.array(LIGHT_TYPES)[(i // 5) % 4])
    _set_bits(rec, 35, np.array(LIGHTS_COUNT)[(i // 20) % 5])
    return rec


def seed_for_draw(k, state):
    """The 32-bit seed whose k-th LCG step (k >= 1) arrives at `state`."""
    s = np.asarray(state, np.uint64)
    for _ in range(k):
        s = ((s - LCG_C) * LCG_A_INV) & 0xFFFFFFFF
    return s.astype(np.uint32)


def draws(n=3072, seed=14):
    """Draw k in 1..4 of the record is exactly 0 or exactly 0x00FFFFFF / 2^24 (the state's top byte runs through all 256 values), crossed
    with metallic {0, 1, -1} and lightsCount {3, 16}.  Metallic 0 takes the diffuse lobe at r1 = 0 (draws: lobe, light index, two of
    the cosine sampler); metallic 1 has ratio = 0, so r1 = 0 is NOT below it and the lobe is specular (draws: lobe, two of the GGX
    sampler).  The low 24 bits of the LCG are a generator of their own, so an extreme draw fixes the draws before it: a second draw of
    0 or 0x00FFFFFF follows r1 = 0.836 or 0.960, which ratio = 0.5 never sends to the diffuse lobe.  Metallic -1 (ratio = 1, every
    draw diffuse) is there so that the top light index and sqrt(1 - r1) = 2^-12 are reached at all."""
    rec = _base(n, seed)
    i = np.arange(n)
    k = 1 + i % 4
    target = np.where((i // 4) % 2 == 0, 0, 0x00FFFFFF)
    rec[:, 19] = np.array(DRAWS_METALLIC, F)[(i // 8) % 3]
    _set_bits(rec, 35, np.where((i // 24) % 2 == 0, 3, 16))
    state = (((i // 48) * 4 + i % 4) % 256).astype(np.uint64) << np.uint64(24) | target.astype(np.uint64)
    s = np.zeros(n, np.uint32)
    for kk in range(1, 5):
        s[k == kk] = seed_for_draw(kk, state[k == kk])
    _set_bits(rec, 32, s)
    return rec


def frame(n=2000, seed=15):
    rec = _base(n, seed)
    v = np.arange(n) % 5
    rec[v == 0, 6:9] = rec[v == 0, 3:6]                                   # tangent parallel to N
    rec[v == 1, 6:9] = 0                                                   # zero tangent
    rec[v == 2, 3:6] *= F(0.5)                                             # |N| = 0.5
    rec[v == 3, 3:6] *= F(2.0)                                             # |N| = 2
    lh = np.cross(rec[:, 3:6].astype(np.float64), rec[:, 6:9].astype(np.float64))
    rec[v == 4, 9:12] = -lh[v == 4].astype(F)                              # binormal = -(N x T)
    return rec


_GENERATORS = {"default": default, "material": material, "view": view, "light": light, "draws": draws, "frame": frame}
_cache = {}


def records(name):
    """The stratum's records [n, 40] float32 (generated once per process; callers must not write to them)."""
    if name not in _cache:
        r = np.ascontiguousarray(_GENERATORS[name](), F)
        r.setflags(write=False)
        _cache[name] = r
    return _cache[name]


def draw_values(rec, count=4):
    """The first `count` PRNG draws of each record as 24-bit integers [n, count]."""
    s = np.ascontiguousarray(rec[:, 32]).view(np.uint32).astype(np.uint64)
    out = []
    for _ in range(count):
        s = (s * LCG_A + LCG_C) & 0xFFFFFFFF
        out.append(s & 0x00FFFFFF)
    return np.stack(out, 1)


# ---- evaluation on the CPU: the oracle, the numpy restatement in binary32 and its binary64 twin -----------------------------------
# continuous outputs: (first word, end, name); the discrete ones are the lobe [12], the PRNG state [17] and the ray origin [3:6]
OUTPUTS = ((0, 3, "hitValue"), (6, 9, "rayDirection"), (9, 12, "weight"), (13, 14, "lightDist"), (14, 17, "shadowRayDir"))
_evaluated = {}


def evaluate(name):
    """(records, oracle rows, numpy binary32 rows, binary64 twin rows) of a stratum, computed once per process and shared read-only."""
    if name not in _evaluated:
        import oracle_py

        rec = records(name)
        with np.errstate(all="ignore"):
            rows = (oracle_py.eval_shade(rec), np_shading.shade(rec), np_shading.shade(rec, np.float64))
        for r in rows:
            r.setflags(write=False)
        _evaluated[name] = (rec,) + rows
    return _evaluated[name]


def _row_error(x, y):
    """Per row: max over the output's words of |x - y| / (max |.| of the row over both + 1e-3), and of |x - y| itself."""
    d = np.abs(x - y)
    scale = np.maximum(np.abs(x), np.abs(y)).max(axis=1) + 1e-3
    return d.max(axis=1) / scale, d.max(axis=1)


def measure(name):
    """The measured figures of one stratum, per continuous output, over the rows whose words of that output are finite in all three
    evaluations (the other rows are the business of the non-finite-set check, which demands that the three agree on them):
      oracle_vs_numpy32_max          max relative difference of the two binary32 evaluations
      *_vs_twin_max / _q999 / _abs   relative error against the binary64 twin: maximum, 0.999-quantile, and the maximum absolute error
      share_over_twice               share of rows whose oracle error exceeds twice numpy binary32's + 1e-6"""
    _, a, b, t = evaluate(name)
    out = {}
    for lo, hi, what in OUTPUTS:
        ok = np.isfinite(a[:, lo:hi]).all(1) & np.isfinite(b[:, lo:hi]).all(1) & np.isfinite(t[:, lo:hi]).all(1)
        x, y, z = a[ok, lo:hi].astype(np.float64), b[ok, lo:hi].astype(np.float64), t[ok, lo:hi]
        e_ab, _ = _row_error(x, y)
        e_a, abs_a = _row_error(x, z)
        e_b, abs_b = _row_error(y, z)
        out[what] = {"rows": int(ok.sum()),
                     "oracle_vs_numpy32_max": float(e_ab.max()),
                     "oracle_vs_twin_max": float(e_a.max()), "oracle_vs_twin_q999": float(np.quantile(e_a, 0.999)),
                     "numpy32_vs_twin_max": float(e_b.max()), "numpy32_vs_twin_q999": float(np.quantile(e_b, 0.999)),
                     "oracle_vs_twin_abs": float(abs_a.max()), "numpy32_vs_twin_abs": float(abs_b.max()),
                     "share_over_twice": float(np.mean(e_a > 2.0 * e_b + 1e-6))}
    return out


PARITY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "shade_records_parity.json")


def committed_figures():
    return json.load(open(PARITY_JSON))["strata"]


def check_parity(name):
    """Oracle against numpy binary32 on every record of the stratum, at four times the committed measured maximum."""
    got, bars = measure(name), committed_figures()[name]["outputs"]
    for _, _, what in OUTPUTS:
        m, bar = got[what]["oracle_vs_numpy32_max"], 4.0 * bars[what]["oracle_vs_numpy32_max"]
        print(f"{name} {what}: oracle vs numpy binary32 max {m:.3e} (bar {bar:.3e}) over {got[what]['rows']} rows")
        assert got[what]["rows"] == bars[what]["rows"], (name, what)
        assert m <= bar, (name, what, m, bar)
