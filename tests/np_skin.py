"""Linear-blend skinning as include/vkrt.h states it (vkrt_scene_skin_vertices), restated in numpy float32, vectorised: what k_skin must
give in every bit.  binary32, source order, no contraction; element (r, c) of joint k is m[16 k + 4 c + r], rows 0..2 only:

    M[r][c] = ((w0*J[j0][r][c] + w1*J[j1][r][c]) + w2*J[j2][r][c]) + w3*J[j3][r][c]
    p'[r]   = ((M[r][0]*p.x + M[r][1]*p.y) + M[r][2]*p.z) + M[r][3]
    N[r]    = (M[r][0]*n.x + M[r][1]*n.y) + M[r][2]*n.z ;  d = (N.x*N.x + N.y*N.y) + N.z*N.z
    n'      = (d > 0 && d < inf) ? N * (1.0f / sqrtf(d)) : N
    t'.xyz  = the same from t ;  t'.w = tw
"""
import numpy as np

F = np.float32


def blended(joints, weights, matrices):
    """M[v, c, r] (r = 0..2): the blended matrix of every vertex, float32.  joints (n, 4) integers, weights (n, 4), matrices (J, 16)."""
    J = np.ascontiguousarray(matrices, F).reshape(-1, 4, 4)[:, :, :3]  # [k, c, r]
    j = np.asarray(joints).astype(np.int64)
    w = np.ascontiguousarray(weights, F)
    g = [J[j[:, i]] for i in range(4)]
    x = [w[:, i, None, None] for i in range(4)]
    with np.errstate(all="ignore"):
        return ((x[0] * g[0] + x[1] * g[1]) + x[2] * g[2]) + x[3] * g[3]


def linear(M, a):
    """(M[r][0]*a.x + M[r][1]*a.y) + M[r][2]*a.z per row: (n, 3) float32"""
    a = np.ascontiguousarray(a, F)
    with np.errstate(all="ignore"):
        return (M[:, 0, :] * a[:, 0:1] + M[:, 1, :] * a[:, 1:2]) + M[:, 2, :] * a[:, 2:3]


def normalize_guarded(N):
    with np.errstate(all="ignore"):
        d = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
        ok = (d > 0) & (d < np.inf)
        inv = F(1.0) / np.sqrt(np.where(ok, d, F(1.0)))
        out = np.where(ok[:, None], N * inv[:, None], N)
    assert out.dtype == F
    return out


def skin(joints, weights, matrices, positions, normals, tangents):
    """(positions', normals', tangents') of the bind-pose arrays (n, 3), (n, 3), (n, 4): float32 arrays"""
    M = blended(joints, weights, matrices)
    with np.errstate(all="ignore"):
        p = linear(M, positions) + M[:, 3, :]
    n = normalize_guarded(linear(M, normals))
    tan = np.ascontiguousarray(tangents, F)
    t = np.concatenate([normalize_guarded(linear(M, tan[:, :3])), tan[:, 3:4]], axis=1)
    assert p.dtype == F and n.dtype == F and t.dtype == F
    return p, n, t


def skin_scalar(joints, weights, matrices, positions, normals, tangents):
    """the same, one vertex and one float32 operation at a time (the check of the vectorised form)"""
    m = np.ascontiguousarray(matrices, F).reshape(-1)
    n_v = len(joints)
    P, N, T = np.zeros((n_v, 3), F), np.zeros((n_v, 3), F), np.zeros((n_v, 4), F)
    with np.errstate(all="ignore"):
        for v in range(n_v):
            j = [int(x) for x in joints[v]]
            w = [F(x) for x in weights[v]]
            M = [[((w[0] * m[16 * j[0] + 4 * c + r] + w[1] * m[16 * j[1] + 4 * c + r]) + w[2] * m[16 * j[2] + 4 * c + r]) + w[3] * m[16 * j[3] + 4 * c + r]
                  for c in range(4)] for r in range(3)]
            p = [F(x) for x in positions[v]]
            P[v] = [((M[r][0] * p[0] + M[r][1] * p[1]) + M[r][2] * p[2]) + M[r][3] for r in range(3)]
            for src, dst in ((normals[v], N), (tangents[v], T)):
                a = [F(x) for x in src[:3]]
                q = [(M[r][0] * a[0] + M[r][1] * a[1]) + M[r][2] * a[2] for r in range(3)]
                d = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]
                if d > 0 and d < np.inf:
                    inv = F(1.0) / np.sqrt(d)
                    q = [x * inv for x in q]
                dst[v, :3] = q
            T[v, 3] = tangents[v][3]
    return P, N, T
