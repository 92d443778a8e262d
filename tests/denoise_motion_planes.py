"""Synthetic planes with moving objects for the motion entry of the diffuse denoiser, and the replay of a denoiser over them.

The world of denoise_planes (its camera, oct-grid normals, materials, floor with a hole, wall) with the four spheres in motion: the unit
sphere moves by DELTA = +(0.05, 0.02, 0.08) per frame, the three small ones by -DELTA / 2.  Materials and the radiance signal are
attached to the spheres' own coordinates, so a surface point keeps its albedo and its expected radiance while it moves (as a real
mover's would); floor and wall are the static part.

Besides the planes of denoise_planes a frame has "prevPosition" [H,W,4] float32, what Renderer.gbuffer_raycast(motion=True) would give:
float32(X - delta of the pixel's sphere) on sphere pixels, the position plane's own bits elsewhere, w = 1 on geometry; on the first
frame the whole plane is the position plane's bits (nothing has moved yet).  "object" [H,W] int8 (sphere 0-3, 4 floor, 5 wall, -1
background) is for the tests' pixel sets and is no input of the denoiser."""
import functools

import numpy as np

import denoise_planes as dp
import np_denoise as nd
from denoise_planes import MATERIALS, _oct_snap, camera, fill, rel_err  # noqa: F401  (re-exported for the tests)
from np_denoise_motion import NpMotionDenoiser

F = np.float32
SIZES = dp.SIZES
FRAMES = 8
DELTA = np.array([0.05, 0.02, 0.08])
STEPS = (DELTA, -0.5 * DELTA, -0.5 * DELTA, -0.5 * DELTA)  # per-frame motion of dp.SPHERES[k]
STILL_EYE = (-0.5, 1.85, -6.0)
PAN_EYES = tuple(e for e, _ in dp.CAMERA_SCRIPT[:6])  # the last eye is held for the frames after the sixth


def centres(frame):
    return [np.asarray(c) + frame * STEPS[k] for k, (c, _) in enumerate(dp.SPHERES)]


def render(eye, W, H, seed, frame):
    """(viewProj, planes) of one frame: denoise_planes.render with the spheres at centres(frame), plus prevPosition and object"""
    vp, V, o, r, u, f, tx, ty = camera(eye, W, H)
    xs, ys = np.meshgrid((np.arange(W) + 0.5) / W * 2 - 1, (np.arange(H) + 0.5) / H * 2 - 1)
    d = xs[..., None] * tx * r - ys[..., None] * ty * u + f  # view depth 1 per unit of t
    best = np.full((H, W), np.inf)
    nrm = np.zeros((H, W, 3))
    obj = np.full((H, W), -1, np.int8)

    def take(t, n, ok, k):
        nonlocal best, nrm, obj
        ok = ok & (t > 1e-6) & (t < best)
        best = np.where(ok, t, best)
        nrm = np.where(ok[..., None], n, nrm)
        obj = np.where(ok, np.int8(k), obj)

    cs = centres(frame)
    for k, (_, R) in enumerate(dp.SPHERES):
        oc = o - cs[k]
        a, b, cc = (d * d).sum(-1), (d * oc).sum(-1), oc @ oc - R * R
        disc = b * b - a * cc
        t = (-b - np.sqrt(np.maximum(disc, 0))) / a
        take(t, ((o + t[..., None] * d) - cs[k]) / R, disc > 0, k)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -o[1] / d[..., 1]
        X = o + t[..., None] * d
        on = (X[..., 0] >= dp.FLOOR[0]) & (X[..., 0] <= dp.FLOOR[1]) & (X[..., 2] >= dp.FLOOR[2]) & (X[..., 2] <= dp.FLOOR[3])
        on &= ~((X[..., 0] > dp.HOLE[0]) & (X[..., 0] < dp.HOLE[1]) & (X[..., 2] > dp.HOLE[2]) & (X[..., 2] < dp.HOLE[3]))
        take(t, np.array([0.0, 1.0, 0.0]), on & np.isfinite(t), 4)
        t = (4.0 - o[2]) / d[..., 2]
        X = o + t[..., None] * d
        on = (X[..., 0] >= dp.WALL[0]) & (X[..., 0] <= dp.WALL[1]) & (X[..., 1] >= dp.WALL[2]) & (X[..., 1] <= dp.WALL[3])
        take(t, np.array([0.0, 0.0, -1.0]), on & np.isfinite(t), 5)
    hit = np.isfinite(best)
    t = np.where(hit, best, 0.0)
    X = o + t[..., None] * d
    n = _oct_snap(np.where(hit[..., None], nrm, (0.0, 0.0, 1.0)))
    # the coordinates materials and signal are attached to: the sphere's own (where it stood at frame 0) on sphere pixels
    moved = np.zeros((H, W, 3))   # how far the pixel's object has moved since frame 0
    step = np.zeros((H, W, 3))    # ... and since the previous frame
    for k in range(len(dp.SPHERES)):
        moved = np.where((obj == k)[..., None], frame * STEPS[k], moved)
        step = np.where((obj == k)[..., None], STEPS[k], step)
    Xo = X - moved
    cell = np.floor(Xo / 0.8 + 0.25).astype(np.int64)
    mat = (cell[..., 0] + 3 * cell[..., 1] + 5 * cell[..., 2]) % len(MATERIALS)
    alb = np.array([m[0] for m in MATERIALS])[mat]
    rough = np.array([m[1] for m in MATERIALS])[mat]
    metal = np.array([m[2] for m in MATERIALS])[mat]
    factor = np.where(((mat == 2) | (mat == 3))[..., None], 1.0, np.maximum(alb, 1e-3))
    phase = np.array([0.0, 0.7, 1.9])
    signal = 1.5 + 0.6 * np.sin(1.3 * Xo[..., 0:1] + 0.5 + phase) * np.cos(0.9 * Xo[..., 2:3] + phase) + 0.3 * np.sin(2.0 * Xo[..., 1:2] - phase)
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
    prev = g["position"].copy()
    if frame > 0:
        sphere = (obj >= 0) & (obj < len(dp.SPHERES))
        prev[..., :3] = np.where(sphere[..., None], (X - step).astype(F), prev[..., :3])
        prev[..., 3] = np.where(h1, F(1), prev[..., 3])
    g["prevPosition"] = prev
    g["object"] = obj
    return vp, g


def case(W, H, pan=False, iterations=5, max_history=32, w0_block=False, nan_pixel=False, static_prev=False, seed=20):
    """The calls of one case: FRAMES dicts (view_proj, planes, reset, iterations, max_history), no reset anywhere.
    pan: the eyes of PAN_EYES instead of the still camera.  w0_block: from frame 3 on, prevPosition.w = 0 on a block of up to 4x4
    pixels around the middle of the unit sphere's pixels.  nan_pixel: from frame 2 on, prevPosition.xyz = NaN at the unit sphere's
    pixel nearest the middle of its pixels.  static_prev: prevPosition = position with w = 1 on geometry (what a scene at rest gives)."""
    calls = []
    for i in range(FRAMES):
        eye = PAN_EYES[min(i, len(PAN_EYES) - 1)] if pan else STILL_EYE
        vp, g = render(eye, W, H, seed, i)
        valid = nd.geom_valid(g["position"], g["normal"])
        if static_prev:
            g["prevPosition"] = g["position"].copy()
            g["prevPosition"][..., 3] = np.where(valid, F(1), g["position"][..., 3])
        ys, xs = np.nonzero(g["object"] == 0)
        if ys.size:
            cy, cx = int(np.median(ys)), int(np.median(xs))
            if w0_block and i >= 3:
                blk = np.zeros((H, W), bool)
                blk[max(cy - 2, 0):cy + 2, max(cx - 2, 0):cx + 2] = True
                g["prevPosition"][..., 3][blk & (g["object"] == 0)] = 0
            if nan_pixel and i >= 2:
                k = np.argmin((ys - cy) ** 2 + (xs - cx - 3) ** 2)
                g["prevPosition"][ys[k], xs[k], :3] = np.nan
        calls.append(dict(view_proj=vp, planes=g, reset=False, iterations=iterations, max_history=max_history))
    return calls


def without_motion(calls):
    """the same calls for the plain entry point: no prevPosition plane"""
    return [dict(c, planes={k: p for k, p in c["planes"].items() if k != "prevPosition"}) for c in calls]


def replay(calls, dtype=np.float32, **variant):
    """One NpMotionDenoiser of dtype over the calls: (outputs [H,W,4] per call, valid masks, branch counts, history lengths per call)"""
    H, W = calls[0]["planes"]["nrdViewZ"].shape
    den = NpMotionDenoiser(W, H, dtype=dtype, **variant)
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


@functools.lru_cache(maxsize=None)
def reference(W, H, pan=False, iterations=5, max_history=32, w0_block=False, nan_pixel=False):
    """A case and its two CPU replays, computed once and shared (read-only) by the tests, like denoise_planes.reference: calls, out32,
    out64, valid, cover and lengths (per call; cover from the float64 twin, lengths from the float32 replay) and E32."""
    calls = case(W, H, pan, iterations, max_history, w0_block, nan_pixel)
    out32, valid, _, lengths = replay(calls, np.float32)
    out64, valid64, cover, _ = replay(calls, np.float64)
    assert all(np.array_equal(a, b) for a, b in zip(valid, valid64))
    return dict(calls=calls, out32=out32, out64=out64, valid=valid, cover=cover, lengths=lengths, E32=max(dp.case_err(out32, out64, valid)))
