"""Properties of the numpy restatement of the diffuse denoiser (tests/np_denoise.py), on synthetic planes: what the GPU kernels
are compared against has to behave like a denoiser first."""
import numpy as np

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
