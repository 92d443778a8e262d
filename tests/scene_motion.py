"""Seeded instance motions shared by the refit tests (test_gpu_refit.py, test_gpu_bvh_bounds.py): rigid motions about an instance's own
centre with a non-uniform scale, optionally mirrored, applied through Renderer.update_nodes."""
import copy

import numpy as np


def _row_major(m16):
    return np.asarray(m16, np.float64).reshape(4, 4).T  # worldMatrix is column-major


def _col_major(M):
    return np.ascontiguousarray(M.T.reshape(16), np.float32)


def _rigid(rng, centre, mirror=False, scale=True):
    """A motion about the instance's own centre: rotation about a random axis, a translation, a non-uniform scale (optionally mirrored)."""
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(-0.6, 0.6)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(4)
    R[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    S = np.diag(list(rng.uniform(0.8, 1.25, 3) if scale else np.ones(3)) + [1.0])
    if mirror:
        S[0, 0] = -S[0, 0]
    T0, T1 = np.eye(4), np.eye(4)
    T0[:3, 3] = -centre
    T1[:3, 3] = centre + rng.uniform(-0.4, 0.4, 3)
    return T1 @ R @ S @ T0


def _centre(flat, i):
    pm = flat.prim_meshes[flat.nodes[i]["primMesh"]]
    v = flat.positions[pm["vertexOffset"]:pm["vertexOffset"] + pm["vertexCount"]].astype(np.float64)
    c = 0.5 * (v.min(0) + v.max(0)) if len(v) else np.zeros(3)
    return (_row_major(flat.nodes[i]["worldMatrix"]) @ np.append(c, 1.0))[:3]


def moved(flat, nodes, seed, mirror_first=True, scale=True):
    """(moved FlatScene, {node: column-major matrix}) for a seeded motion of `nodes`."""
    rng = np.random.default_rng(seed)
    out = copy.copy(flat)
    out.nodes = flat.nodes.copy()
    mats = {}
    for j, i in enumerate(nodes):
        M = _rigid(rng, _centre(flat, i), mirror=mirror_first and j == 0, scale=scale) @ _row_major(flat.nodes[i]["worldMatrix"])
        mats[int(i)] = _col_major(M)
        out.nodes[i]["worldMatrix"] = mats[int(i)]
    return out, mats


def apply(r, mats, stream=None):
    for i, m in sorted(mats.items()):
        r.update_nodes(i, m[None], stream=stream)
