"""Synthetic G-buffer / NRD planes for the denoiser tests: fronto-parallel planes seen by the default camera, laid out as
Renderer.gbuffer_raycast(view_matrix=...) + hybrid_trace leave them (numpy float32)."""
import numpy as np

import camera_np

F = np.float32


def ycocg(rgb):
    """linear -> YCoCg as raytraceHybrid.rgen:273-281 packs it (before the half store)"""
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    return np.stack([(r * F(0.25) + g * F(0.5)) + b * F(0.25), (r * F(0.5) + g * F(0)) + b * F(-0.5),
                     (r * F(-0.25) + g * F(0.5)) + b * F(-0.25)], -1).astype(F)


def decode(rad):
    t = rad[..., 0] - rad[..., 2]
    return np.maximum(np.stack([t + rad[..., 1], rad[..., 0] + rad[..., 2], t - rad[..., 1]], -1), F(0)).astype(F)


def planes(W, H, plane_z, radiance, albedo, eye=(0, 0, 15), center=(0, 0, 0)):
    """plane_z [H,W]: world z of the fronto-parallel plane each pixel sees (NaN = background); radiance, albedo [H,W,3] linear.
    Returns (view_proj[16] column-major float32, planes dict)."""
    vp, view_inv, proj_inv = camera_np.global_uniforms(eye=eye, center=center, width=W, height=H)
    V = camera_np.look_at(eye, center, (0, 1, 0))
    xs, ys = np.meshgrid((np.arange(W) + 0.5) / W * 2 - 1, (np.arange(H) + 0.5) / H * 2 - 1)
    tgt = np.stack([xs, ys, np.ones_like(xs), np.ones_like(xs)], -1) @ proj_inv.astype(np.float64).T
    d = tgt[..., :3] / np.linalg.norm(tgt[..., :3], axis=-1, keepdims=True)
    d = d @ view_inv.astype(np.float64)[:3, :3].T
    o = np.asarray(eye, np.float64)
    hit = np.isfinite(plane_z)
    t = (np.where(hit, plane_z, 0.0) - o[2]) / d[..., 2]
    pos = o + t[..., None] * d
    vz = (np.concatenate([pos, np.ones((H, W, 1))], -1) @ V.T)[..., 2]
    g = {k: np.zeros((H, W, 4), F) for k in ("color", "position", "normal", "nrdRadianceHitDist")}
    g["roughMetal"] = np.zeros((H, W, 2), F)
    g["nrdViewZ"] = np.zeros((H, W), F)
    g["position"][..., :3] = np.where(hit[..., None], pos, 0)
    g["normal"][..., 2] = np.where(hit, 1.0, 0.0)
    g["color"][..., 3], g["position"][..., 3], g["normal"][..., 3] = (np.where(hit, albedo[..., k], g[("color", "position", "normal")[k]][..., 3])
                                                                     for k in range(3))
    g["roughMetal"][..., 0] = np.where(hit, 1.0, 0.0)
    g["nrdViewZ"][...] = np.where(hit, vz, 0.0)
    g["nrdRadianceHitDist"][..., :3] = np.where(hit[..., None], ycocg(np.asarray(radiance, F)), 0)
    g["nrdRadianceHitDist"][..., 3] = np.where(hit, 0.5, 0.0)
    return np.asarray(vp, F).T.reshape(-1).copy(), g
