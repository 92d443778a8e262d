"""numpy float32 restatement of k_hit_motion (csrc/motion.hip; include/vkrt.h vkrt_hit_motion): the surface point of hit records from a
FlatScene's nodes, positions, indices and primitive meshes, in the kernel's operation order (built with -ffp-contract=off: every
binary operation rounds once, nothing is fused):

    bw = ((1 - u) - v, u, v)
    Pk = ((m00 x + m01 y) + m02 z) + m03, ... the rows of the node's object -> world matrix on vertex k of the triangle
    xyz = ((0 + P0 bw0) + P1 bw1) + P2 bw2,  w = 1

A record that is not a hit of the scene -- instance or primitive out of range, a non-finite u or v -- gives (0, 0, 0, 0), as
vkrt_hit_surface's validation does.  `current` of the device is this on the scene's arrays as they are, `previous` on the arrays as they
were at the last vkrt_scene_motion_mark."""
import numpy as np

F = np.float32


def valid_records(flat, hits):
    """bool [N]: the records of `hits` ([N, 8] 4-byte words, vkrt_hit) that name a triangle of the scene with finite u, v"""
    h = np.ascontiguousarray(hits).reshape(-1, 8)
    f, i = h.view(np.float32), h.view(np.int32)
    inst, prim = i[:, 3].astype(np.int64), i[:, 4].astype(np.int64)
    ok = (inst >= 0) & (inst < len(flat.nodes)) & np.isfinite(f[:, 1]) & np.isfinite(f[:, 2])
    pm = flat.prim_meshes[flat.nodes["primMesh"][np.where(ok, inst, 0)]]
    return ok & (prim >= 0) & (prim < pm["indexCount"].astype(np.int64) // 3)


def hit_points(flat, hits, world_matrices=None, positions=None):
    """float32 [N, 4].  world_matrices ([nodes, 16], column-major) and positions ([V, 3]) default to the scene's own: pass the arrays of
    another moment for the points of that moment."""
    h = np.ascontiguousarray(hits).reshape(-1, 8)
    f, i = h.view(np.float32), h.view(np.int32)
    ok = valid_records(flat, h)
    M = np.asarray(flat.nodes["worldMatrix"] if world_matrices is None else world_matrices, F).reshape(-1, 16)
    P = np.asarray(flat.positions if positions is None else positions, F).reshape(-1, 3)
    inst = np.where(ok, i[:, 3], 0).astype(np.int64)
    prim = np.where(ok, i[:, 4], 0).astype(np.int64)
    pm = flat.prim_meshes[flat.nodes["primMesh"][inst]]
    first = pm["firstIndex"].astype(np.int64) + 3 * prim
    first = np.where(ok, first, 0)
    off = pm["vertexOffset"].astype(np.int64)
    u, v = f[:, 1].astype(F), f[:, 2].astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        bw = ((F(1) - u) - v, u, v)
        m = M[inst]  # column-major: row r, column c at m[:, 4 c + r]
        out = np.zeros((h.shape[0], 4), F)
        acc = [np.zeros(h.shape[0], F) for _ in range(3)]
        for k in range(3):
            vi = np.where(ok, flat.indices[first + k].astype(np.int64) + off, 0)
            x, y, z = P[vi, 0], P[vi, 1], P[vi, 2]
            for r in range(3):
                pr = ((m[:, r] * x + m[:, 4 + r] * y) + m[:, 8 + r] * z) + m[:, 12 + r]
                acc[r] = acc[r] + pr * bw[k]
        for r in range(3):
            out[:, r] = acc[r]
    out[:, 3] = 1
    out[~ok] = 0
    return out
