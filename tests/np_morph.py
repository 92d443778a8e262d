"""Morph targets as include/vkrt.h states them (vkrt_scene_morph_vertices), restated in numpy float32: what k_morph_live / k_morph_bind
must give in every bit.  binary32, source order, no contraction; per component:

    P = p;  for k = 0..T-1 in index order:  if (w[k] != 0)  P = P + w[k] * dP[k]         (the product rounded, then the sum)
    N, Tn likewise from n, t with dN, dT -- only if the morph has that delta array
    n'      = (the morph has normal deltas and some w[k] != 0) ? normalizeGuarded(N) : n
    t'.xyz  = likewise ;  t'.w = tw

morph() is vectorised over the vertices, morph_scalar() does one vertex and one float32 operation at a time.  The keyword arguments of
morph() switch on the WRONG variants that tests/test_np_morph.py must tell apart from the stated arithmetic; nothing else uses them.
"""
import numpy as np

from np_skin import normalize_guarded

F = np.float32


def _accumulate(base, deltas, w, fused=False, reverse=False, multiply_zero=False):
    out = np.ascontiguousarray(base, F).copy()
    if deltas is None:
        return out
    d = np.ascontiguousarray(deltas, F)
    order = range(len(w) - 1, -1, -1) if reverse else range(len(w))
    with np.errstate(all="ignore"):
        for k in order:
            if w[k] == 0 and not multiply_zero:
                continue
            if fused:  # one rounding: the product is exact in float64
                out = (out.astype(np.float64) + np.float64(w[k]) * d[k].astype(np.float64)).astype(F)
            else:
                out = out + w[k] * d[k]
    assert out.dtype == F
    return out


def morph(weights, positions, normals, tangents, position_deltas=None, normal_deltas=None, tangent_deltas=None, fused=False, reverse=False,
          always_normalize=False, multiply_zero=False):
    """(positions', normals', tangents') of the base arrays (n, 3), (n, 3), (n, 4) and deltas (T, n, 3) or None: float32 arrays"""
    w = np.ascontiguousarray(weights, F)
    kw = dict(fused=fused, reverse=reverse, multiply_zero=multiply_zero)
    tan = np.ascontiguousarray(tangents, F)
    some = bool((w != 0).any()) or always_normalize
    p = _accumulate(positions, position_deltas, w, **kw)
    n = _accumulate(normals, normal_deltas, w, **kw)
    t = _accumulate(tan[:, :3], tangent_deltas, w, **kw)
    if (normal_deltas is not None and some) or always_normalize:
        n = normalize_guarded(n)
    if (tangent_deltas is not None and some) or always_normalize:
        t = normalize_guarded(t)
    t = np.concatenate([t, tan[:, 3:4]], axis=1)
    assert p.dtype == F and n.dtype == F and t.dtype == F
    return p, n, t


def morph_scalar(weights, positions, normals, tangents, position_deltas=None, normal_deltas=None, tangent_deltas=None):
    """the same, one vertex and one float32 operation at a time (the check of the vectorised form)"""
    w = [F(x) for x in weights]
    n_v = len(positions)
    P, N, T = np.zeros((n_v, 3), F), np.zeros((n_v, 3), F), np.zeros((n_v, 4), F)
    some = any(x != 0 for x in w)
    with np.errstate(all="ignore"):
        for v in range(n_v):
            for src, deltas, dst, unit in ((positions, position_deltas, P, False), (normals, normal_deltas, N, True), (tangents, tangent_deltas, T, True)):
                a = [F(x) for x in src[v][:3]]
                if deltas is not None:
                    for k in range(len(w)):
                        if w[k] != 0:
                            for c in range(3):
                                prod = F(w[k] * F(deltas[k][v][c]))
                                a[c] = F(a[c] + prod)
                    if unit and some:
                        d = F(F(F(a[0] * a[0]) + F(a[1] * a[1])) + F(a[2] * a[2]))
                        if d > 0 and d < np.inf:
                            inv = F(F(1.0) / np.sqrt(d))
                            a = [F(x * inv) for x in a]
                dst[v, :3] = a
            T[v, 3] = tangents[v][3]
    return P, N, T
