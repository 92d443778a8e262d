"""Synthetic planes that reach every branch of the diffuse denoiser, and the replay of a denoiser over them.

numpy only, deterministic in the seed, no renderer and no scene file: analytic ray casting in float64 through the pixel centres
of dnProject's convention (ndc = 2 (x + 0.5) / W - 1), stored as the float32 planes Renderer.gbuffer_raycast + hybrid_trace
leave (color, position, normal, roughMetal, nrdViewZ, nrdRadianceHitDist) with a column-major viewProj.

The world: a unit sphere, three spheres 2-3 pixels in radius (at 48x40), a floor with a rectangular hole (background inside
geometry) and an upright wall that meets the floor in a 90 degree crease, with background above it.  The camera looks along +z,
so the wall and the spheres' near sides have nz < 0 (the fold of the oct encoding).  Six materials, laid out in world-space
cells, put every arm of dnAlbedo on both sides of its threshold.  The radiance is a smooth positive signal times gamma noise
(shape 4: 50 % relative deviation) times the demodulation factor, so the demodulated signal is of order 1 everywhere and its
variance is never near zero (1 / (4 sqrt(var) + 1e-10) is then well-conditioned).

Normals are snapped to the oct grid (decode(encode(n)) in float64) before they are stored: the 16-bit rounding in dnOctEncode is
then decided by a wide margin, the same in binary32 and binary64.  This is a condition on the inputs; every branch of the
encoding, the fold included, still runs."""
import functools

import numpy as np

import np_denoise as nd

F = np.float32
SIZES = ((48, 40), (17, 33), (7, 5), (1, 1))

# (albedo, roughness, metallic).  ratio = metal * (1 - rough) in binary32: 0.79 and 0.81 around the 0.8 of the specular test
MATERIALS = (
    ((0.7, 0.5, 0.3), 1.0, 0.0),           # 0 ordinary diffuse
    ((0.6, 0.6, 0.4), 0.21, 1.0),          # 1 ratio 0.79: demodulated
    ((0.5, 0.7, 0.6), 0.19, 1.0),          # 2 ratio 0.81: specular arm, factor 1
    ((0.9e-3, 0.5e-3, 0.2e-3), 1.0, 0.0),  # 3 albedo maximum 0.9e-3: black arm, factor 1
    ((1.1e-3, 0.4e-3, 0.7e-3), 1.0, 0.0),  # 4 albedo maximum 1.1e-3: demodulated, two channels on the floor
    ((0.6, 0.0, 0.4), 1.0, 0.0),           # 5 one channel 0: that channel on the floor
)
SPHERES = (((0.0, 1.0, 0.0), 1.0), ((-1.6, 0.35, -1.5), 0.35), ((1.3, 0.35, -2.0), 0.35), ((0.3, 0.3, -2.6), 0.3))
FLOOR = (-6.0, 6.0, -16.0, 4.0)  # y = 0 over x0..x1, z0..z1
HOLE = (-3.4, -2.2, -1.5, 0.5)
WALL = (-6.0, 6.0, 0.0, 3.0)     # z = 4 over x0..x1, y0..y1
LOOK = np.array([0.0, -0.12, 1.0])
FOVY = np.deg2rad(60.0)

# eye, reset() before the call.  A slow pan and rise (0.3 to 2 pixels a frame at 48x40), two still frames (q = p exactly), a dolly
# back (floor points now visible lie behind the previous camera), a jump to the other side without reset(), a reset(), more pan.
CAMERA_SCRIPT = (
    ((-1.00, 1.60, -6.0), False), ((-0.95, 1.62, -6.0), False), ((-0.80, 1.70, -6.0), False), ((-0.50, 1.85, -6.0), False),
    ((-0.50, 1.85, -6.0), False), ((-0.50, 1.85, -6.0), False), ((-0.50, 1.85, -10.0), False), ((1.10, 1.60, -6.0), False),
    ((1.05, 1.62, -6.0), True), ((0.95, 1.65, -6.0), False), ((0.80, 1.72, -6.0), False), ((0.50, 1.80, -6.0), False),
)
# (iterations, max_history) per call on one handle, over the first eight cameras: every change of K rotates the colour planes
SETTINGS_SCRIPT = ((5, 32), (0, 1), (1, 2), (5, 32), (2, 1), (0, 2), (0, 32), (3, 1))


def _oct_snap(n):
    """float64 unit normals -> the nearest oct-grid normal (the encoding of np_denoise / dnOctEncode, restated in float64)"""
    v = n / np.abs(n).sum(-1, keepdims=True)
    x, y = v[..., 0], v[..., 1]
    neg = v[..., 2] < 0
    sx, sy = np.where(x >= 0, 1.0, -1.0), np.where(y >= 0, 1.0, -1.0)
    x, y = np.where(neg, (1 - np.abs(y)) * sx, x), np.where(neg, (1 - np.abs(x)) * sy, y)
    x, y = np.rint(x * 32767) / 32767, np.rint(y * 32767) / 32767
    z = 1 - np.abs(x) - np.abs(y)
    t = np.maximum(-z, 0)
    x, y = x + np.where(x >= 0, -t, t), y + np.where(y >= 0, -t, t)
    m = np.stack([x, y, z], -1)
    return m / np.linalg.norm(m, axis=-1, keepdims=True)


def camera(eye, W, H):
    """(column-major viewProj [16] float32, eye, right, up, forward, tan half-fov x, y) of the camera at eye looking along LOOK"""
    eye = np.asarray(eye, np.float64)
    f = LOOK / np.linalg.norm(LOOK)
    r = np.cross(f, (0.0, 1.0, 0.0))
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    V = np.eye(4)
    V[0, :3], V[1, :3], V[2, :3] = r, u, -f
    V[:3, 3] = -V[:3, :3] @ eye
    ty = np.tan(FOVY / 2)
    tx = ty * W / H
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1], P[2, 2], P[2, 3], P[3, 2] = 1 / tx, -1 / ty, -1.0001, -0.1, -1.0  # row 0 of the image is the top
    return (P @ V).T.reshape(-1).astype(F), V, eye, r, u, f, tx, ty


def render(eye, W, H, seed, frame):
    """(viewProj, planes) of one frame"""
    vp, V, o, r, u, f, tx, ty = camera(eye, W, H)
    xs, ys = np.meshgrid((np.arange(W) + 0.5) / W * 2 - 1, (np.arange(H) + 0.5) / H * 2 - 1)
    d = xs[..., None] * tx * r - ys[..., None] * ty * u + f  # view depth 1 per unit of t
    best = np.full((H, W), np.inf)
    nrm = np.zeros((H, W, 3))

    def take(t, n, ok):
        nonlocal best, nrm
        ok = ok & (t > 1e-6) & (t < best)
        best = np.where(ok, t, best)
        nrm = np.where(ok[..., None], n, nrm)

    for c, R in SPHERES:
        oc = o - np.asarray(c)
        a, b, cc = (d * d).sum(-1), (d * oc).sum(-1), oc @ oc - R * R
        disc = b * b - a * cc
        t = (-b - np.sqrt(np.maximum(disc, 0))) / a
        take(t, ((o + t[..., None] * d) - np.asarray(c)) / R, disc > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -o[1] / d[..., 1]
        X = o + t[..., None] * d
        on = (X[..., 0] >= FLOOR[0]) & (X[..., 0] <= FLOOR[1]) & (X[..., 2] >= FLOOR[2]) & (X[..., 2] <= FLOOR[3])
        on &= ~((X[..., 0] > HOLE[0]) & (X[..., 0] < HOLE[1]) & (X[..., 2] > HOLE[2]) & (X[..., 2] < HOLE[3]))
        take(t, np.array([0.0, 1.0, 0.0]), on & np.isfinite(t))
        t = (4.0 - o[2]) / d[..., 2]
        X = o + t[..., None] * d
        on = (X[..., 0] >= WALL[0]) & (X[..., 0] <= WALL[1]) & (X[..., 1] >= WALL[2]) & (X[..., 1] <= WALL[3])
        take(t, np.array([0.0, 0.0, -1.0]), on & np.isfinite(t))
    hit = np.isfinite(best)
    t = np.where(hit, best, 0.0)
    X = o + t[..., None] * d
    n = _oct_snap(np.where(hit[..., None], nrm, (0.0, 0.0, 1.0)))
    cell = np.floor(X / 0.8 + 0.25).astype(np.int64)
    mat = (cell[..., 0] + 3 * cell[..., 1] + 5 * cell[..., 2]) % len(MATERIALS)
    alb = np.array([m[0] for m in MATERIALS])[mat]
    rough = np.array([m[1] for m in MATERIALS])[mat]
    metal = np.array([m[2] for m in MATERIALS])[mat]
    factor = np.where(((mat == 2) | (mat == 3))[..., None], 1.0, np.maximum(alb, 1e-3))
    phase = np.array([0.0, 0.7, 1.9])
    signal = 1.5 + 0.6 * np.sin(1.3 * X[..., 0:1] + 0.5 + phase) * np.cos(0.9 * X[..., 2:3] + phase) + 0.3 * np.sin(2.0 * X[..., 1:2] - phase)
    noise = np.random.default_rng([seed, frame]).gamma(4.0, 0.25, (H, W, 3))
    rgb = signal * noise * factor
    R_, G_, B_ = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    ycocg = np.stack([0.25 * R_ + 0.5 * G_ + 0.25 * B_, 0.5 * R_ - 0.5 * B_, -0.25 * R_ + 0.5 * G_ - 0.25 * B_], -1)
    h3, h1 = hit[..., None], hit
    g = {k: np.zeros((H, W, 4), F) for k in ("color", "position", "normal", "nrdRadianceHitDist")}
    g["position"][..., :3] = np.where(h3, X, 0)
    g["normal"][..., :3] = np.where(h3, n, 0)
    g["color"][..., :3] = np.where(h3, alb, 0)
    for k, name in enumerate(("color", "position", "normal")):
        g[name][..., 3] = np.where(h1, alb[..., k], 0)
    g["roughMetal"] = np.where(h3, np.stack([rough, metal], -1), 0).astype(F)
    g["nrdViewZ"] = np.where(h1, -t, 0).astype(F)
    g["nrdRadianceHitDist"][..., :3] = np.where(h3, ycocg, 0)
    g["nrdRadianceHitDist"][..., 3] = np.where(h1, t * np.linalg.norm(d, axis=-1), 0)
    return vp, g


def case(W, H, iterations=5, max_history=32, settings=False, nan_frame=None, seed=20):
    """The calls of one test case: a list of dicts (view_proj, planes, reset, iterations, max_history).  settings: the
    SETTINGS_SCRIPT's per-call settings over the first eight cameras.  nan_frame: that frame's radiance Y is NaN at one pixel
    with geometry near the image centre."""
    calls = []
    script = CAMERA_SCRIPT[:len(SETTINGS_SCRIPT)] if settings else CAMERA_SCRIPT
    for i, (eye, reset) in enumerate(script):
        vp, g = render(eye, W, H, seed, i)
        K, mh = SETTINGS_SCRIPT[i] if settings else (iterations, max_history)
        if i == nan_frame:
            valid = nd.geom_valid(g["position"], g["normal"])
            ys, xs = np.nonzero(valid)
            k = np.argmin((ys - H // 2) ** 2 + (xs - W // 2) ** 2)
            g["nrdRadianceHitDist"][ys[k], xs[k], 0] = np.nan
        calls.append(dict(view_proj=vp, planes=g, reset=reset, iterations=K, max_history=mh))
    return calls


def fill(W, H):
    """what out holds before each call: .w and the pixels without geometry must keep these bits"""
    return np.random.default_rng(7).uniform(1.0, 8.0, (H, W, 4)).astype(F)


def replay(calls, dtype=np.float32, **variant):
    """One NpDenoiser of dtype over the calls: (outputs [H,W,4] per call, valid masks, branch counts, final history lengths)"""
    H, W = calls[0]["planes"]["nrdViewZ"].shape
    den = nd.NpDenoiser(W, H, dtype=dtype, **variant)
    outs, valids, covers, lengths = [], [], [], []
    for c in calls:
        if c["reset"]:
            den.reset()
        outs.append(den.denoise(c["view_proj"], c["planes"], out=fill(W, H).astype(dtype), iterations=c["iterations"],
                                max_history=c["max_history"]))
        valids.append(den.valid)
        covers.append(dict(den.cover))
        lengths.append(den.mom[..., 2].copy())
    return outs, valids, covers, lengths


def rel_err(x, ref, valid):
    """max over the valid pixels and the channels of |x - ref| / max(|ref|, 1e-3); a non-finite x counts as infinite"""
    if not valid.any():
        return 0.0
    x, ref = np.asarray(x, np.float64)[..., :3][valid], np.asarray(ref, np.float64)[..., :3][valid]
    e = np.abs(x - ref) / np.maximum(np.abs(ref), 1e-3)
    return float(np.where(np.isfinite(e), e, np.inf).max())


def case_err(outs, refs, valids):
    """rel_err per call"""
    return [rel_err(o, r, v) for o, r, v in zip(outs, refs, valids)]


@functools.lru_cache(maxsize=None)
def reference(W, H, iterations=5, max_history=32, settings=False, nan_frame=None):
    """A case and its two CPU replays, computed once and shared (read-only) by the tests: dict with calls, out32, out64, valid,
    cover (branch counts per call, from the float64 twin), lengths (history lengths per call, float64 twin) and E32, the float32
    restatement's largest rel_err against the float64 twin over all calls."""
    calls = case(W, H, iterations, max_history, settings, nan_frame)
    out32, valid, _, _ = replay(calls, np.float32)
    out64, valid64, cover, lengths = replay(calls, np.float64)
    assert all(np.array_equal(a, b) for a, b in zip(valid, valid64))
    return dict(calls=calls, out32=out32, out64=out64, valid=valid, cover=cover, lengths=lengths, E32=max(case_err(out32, out64, valid)))
