"""numpy restatement of triangle pre-splitting (lbvh.hip: k_split_priority, k_split_budget, k_split_refs), stage by stage, written from the
kernels' header comment and operation order.  The library is compiled without contraction and the splitter uses + - * /, fminf / fmaxf,
comparisons, float-to-unsigned conversion and a count of leading zeros, so every stage but the one cbrtf is the same bits in numpy binary32:

  priority      splitCell / splitPlane / splitPriority up to x = ldexpf(gain / sceneArea, m - 20); the priority itself is cbrt(x)
  budget_scale  k_split_budget: the float64 sum in the kernel's order, count(D), the doublings and the bisection
  pieces        splitClip / splitTriangle for one triangle: boxes in emission order and the cell (half-spaces) of every piece
  clip_exact    the triangle clipped to a cell in rational arithmetic: what a piece's box has to contain

Each stage takes the stage before it as an argument, so a test can feed it the device's output and a last-bit difference of cbrtf never
reaches the piece lists.  Inputs are the world-space 48-B records in flattened-id order and the watertight flag (records() makes them
from vertices the way k_flatten does, for the tests that run without a device)."""
from fractions import Fraction

import numpy as np

import np_bvh
import np_bvh_build as nb

F32 = np.float32
GRID_BITS = 21
CELLS = F32(2097152.0)
MAX_PER_TRI = 255
STACK = 16
PAD = F32(4.76837158203125e-07)  # 8 * 2^-24
INF = F32(np.inf)
MUTANTS = ("no_pad", "no_snap", "no_clamp", "short_axis", "half_and_half", "face_ends_axis")


# ---- the splitter's view of the scene -----------------------------------------------------------------------------------------------

def records(pos, watertight, world=None):
    """The 9 geometry floats of every record ([n, 12], words 9..11 zero) from vertices pos [3n, 3]: vkrt_xform_point with the node's
    object-to-world rows (world: 4x4 row-major, default identity), then vkrt_tri_record."""
    p = np.asarray(pos, F32).reshape(-1, 3, 3)
    if world is not None:
        m = np.asarray(world, np.float64).astype(F32)
        p = np.stack([((m[r, 0] * p[..., 0] + m[r, 1] * p[..., 1]) + m[r, 2] * p[..., 2]) + m[r, 3] for r in range(3)], -1).astype(F32)
    rec = np.zeros((p.shape[0], 12), F32)
    rec[:, 0:3] = p[:, 0]
    rec[:, 3:6] = p[:, 1] if watertight else p[:, 1] - p[:, 0]
    rec[:, 6:9] = p[:, 2] if watertight else p[:, 2] - p[:, 0]
    return rec


class Scene:
    """loadSplitTri / loadSplitGrid for all records: v [T, 3, 3] the vertices as the selected triangle test sees them, full [T, 6] the
    whole-triangle boxes, slop [T], and the grid (lo, ext) from the ordered-integer scene bounds."""

    def __init__(self, rec, watertight):
        rec = np.asarray(rec, F32).reshape(-1, 12)
        v0, r1, r2 = rec[:, 0:3], rec[:, 3:6], rec[:, 6:9]
        with np.errstate(all="ignore"):
            if watertight:
                v1, v2, e1, e2 = r1, r2, r1 - v0, r2 - v0
            else:
                v1, v2, e1, e2 = v0 + r1, v0 + r2, r1, r2
        self.v = np.stack([v0, v1, v2], 1).astype(F32)
        self.slop = np_bvh.tri_slop(e1, e2)
        lo, hi = np_bvh.record_bounds(rec, watertight)
        self.full = np.concatenate([lo, hi], 1).astype(F32)
        slo, shi = nb.scene_bounds(lo, hi)
        self.glo = slo.astype(F32)
        self.gext = (shi - slo).astype(F32)
        self.T = rec.shape[0]

    @property
    def grid(self):
        return self.glo, self.gext


def _cells(grid, k, x):
    """splitCell for arrays."""
    lo, ext = grid
    with np.errstate(all="ignore"):
        t = (x - lo[k]) / ext[k] if ext[k] > 0 else np.zeros_like(x)
        t = np.minimum(np.maximum(t * CELLS, F32(0)), CELLS - F32(1))
    return t.astype(np.int64)


def _bit_index(x):
    """31 - clz(x) for positive int64 arrays (x < 2^21)."""
    m = np.zeros(x.shape, np.int64)
    for b in range(GRID_BITS):
        m = np.where((x >> b) & 1 == 1, b, m)
    return m


def priority(sc):
    """k_split_priority up to the cube root.  Returns (x [T] binary32 -- the device's priority is cbrtf(x) --, zero [T] bool: the
    triangles whose priority is 0 by rule (slop > 0, no cutting plane, gain <= 0, scene area <= 0), p64 [T] = cbrt(float64(x)))."""
    v = sc.v
    lo = np.minimum(v[:, 0], np.minimum(v[:, 1], v[:, 2]))
    hi = np.maximum(v[:, 0], np.maximum(v[:, 1], v[:, 2]))
    T = sc.T
    m_best = np.full(T, -1, np.int64)
    ext_best = np.zeros(T, F32)
    glo, gext = sc.grid
    with np.errstate(all="ignore"):
        for k in range(3):
            qa, qb = _cells(sc.grid, k, lo[:, k]), _cells(sc.grid, k, hi[:, k])
            ok = np.zeros(T, bool)
            m = np.zeros(T, np.int64)
            while True:  # splitPlane's search: a plane on a face of the box is passed over for the planes on the box's side of it
                live = ~ok & (qa != qb)
                if not live.any():
                    break
                mq = _bit_index(np.where(live, qa ^ qb, 1))
                q = (qb >> mq) << mq
                c = (glo[k] + q.astype(F32) * (gext[k] / CELLS)).astype(F32)
                found = live & (c > lo[:, k]) & (c < hi[:, k])
                ok |= found
                m = np.where(found, mq, m)
                above = live & ~found & (c >= hi[:, k])
                qb = np.where(above, q - 1, qb)
                qa = np.where(live & ~found & ~above, q, qa)
            ext = (hi[:, k] - lo[:, k]).astype(F32)
            take = ok & ((m > m_best) | ((m == m_best) & (ext > ext_best)))
            m_best = np.where(take, m, m_best)
            ext_best = np.where(take, ext, ext_best)
        d = (hi - lo).astype(F32)
        e1, e2 = (v[:, 1] - v[:, 0]).astype(F32), (v[:, 2] - v[:, 0]).astype(F32)
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        gain = F32(2) * ((d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2]) + d[:, 2] * d[:, 0]) - ((np.abs(nx) + np.abs(ny)) + np.abs(nz))
        s = gext
        scene_area = F32(2) * ((s[0] * s[1] + s[1] * s[2]) + s[2] * s[0])
        zero = (sc.slop > 0) | (m_best < 0) | ~(gain > 0) | ~(scene_area > 0)
        x = np.ldexp((gain / scene_area).astype(F32), (m_best - (GRID_BITS - 1)).astype(np.int32)).astype(F32)
    x = np.where(zero, F32(0), x).astype(F32)
    return x, zero, np.cbrt(x.astype(np.float64))


# ---- k_split_budget ----------------------------------------------------------------------------------------------------------------

def _strided_sum64(a):
    """Thread t of 1024 adds a[t], a[t + 1024], ... in sequence in float64; then the tree reduction off = 512 .. 1."""
    a = np.asarray(a, np.float64)
    rows = -(-a.size // 1024)
    pad = np.zeros(rows * 1024, np.float64)
    pad[: a.size] = a
    red = np.zeros(1024, np.float64)
    for row in pad.reshape(rows, 1024):
        red = red + row
    off = 512
    while off > 0:
        red[:off] = red[:off] + red[off:2 * off]
        off >>= 1
    return float(red[0])


def split_counts(prio, D):
    """min((unsigned)(D * prio[g]), 255): the splits of every triangle."""
    with np.errstate(all="ignore"):
        prod = (F32(D) * np.asarray(prio, F32)).astype(F32)
    return np.minimum(prod, F32(MAX_PER_TRI)).astype(np.int64)  # (truncation and the cap commute for products >= 0)


def count(prio, D):
    return int(split_counts(prio, D).sum())


def budget_scale(prio, budget):
    """k_split_budget: D as binary32."""
    prio = np.asarray(prio, F32)
    total = _strided_sum64(prio)
    if not total > 0.0 or budget == 0:
        return F32(0)
    lo = F32(float(budget) / total)
    if count(prio, lo) > budget:
        lo = F32(0)
    hi = F32(max(lo, F32(1e-30)) * F32(2))
    with np.errstate(all="ignore"):
        for _ in range(16):
            if not count(prio, hi) <= budget:
                break
            lo, hi = hi, F32(hi * F32(2))
        for _ in range(24):
            mid = F32(F32(0.5) * F32(lo + hi))
            if count(prio, mid) <= budget:
                lo = mid
            else:
                hi = mid
    return F32(lo)


# ---- splitClip / splitTriangle for one triangle --------------------------------------------------------------------------------------

def _cell1(grid, k, x):
    lo, ext = grid
    t = (x - lo[k]) / ext[k] if ext[k] > 0 else F32(0)
    t = min(max(F32(t * CELLS), F32(0)), CELLS - F32(1))
    return int(t)


def split_plane(grid, b, mutant=None):
    """splitPlane: (axis or -1, position, bit index m) of the most important median plane cutting box b (6 binary32 values)."""
    lo, ext = grid
    axis, m_best, ext_best, pos = -1, -1, F32(0), F32(0)
    for k in range(3):
        qa, qb = _cell1(grid, k, b[k]), _cell1(grid, k, b[3 + k])
        m = -1
        while qa != qb:  # a plane on a face of the box is passed over for the planes on the box's side of it
            mq = (qa ^ qb).bit_length() - 1
            q = (qb >> mq) << mq
            c = F32(lo[k] + F32(F32(q) * F32(ext[k] / CELLS)))
            if c > b[k] and c < b[3 + k]:
                m = mq
                break
            if mutant == "face_ends_axis":
                break
            if c >= b[3 + k]:
                qb = q - 1
            else:
                qa = q
        if m < 0:
            continue
        e = F32(b[3 + k] - b[k])
        tie = e < ext_best if mutant == "short_axis" else e > ext_best
        if m > m_best or (m == m_best and tie):
            axis, m_best, ext_best, pos = k, m, e, c
    return axis, pos, m_best


def split_clip(v, b, axis, pos, mutant=None):
    """splitClip: (ok, L, R), the boxes of the two halves of piece b of the triangle v [3][3] cut at x_axis = pos."""
    L = [INF, INF, INF, -INF, -INF, -INF]
    R = [INF, INF, INF, -INF, -INF, -INF]

    def grow(d, p, pad):
        for k in range(3):
            d[k] = min(d[k], F32(p[k] - pad[k]))
            d[3 + k] = max(d[3 + k], F32(p[k] + pad[k]))

    zero = (F32(0), F32(0), F32(0))
    for e in range(3):
        va, vb = v[e], v[(e + 1) % 3]
        da, db = va[axis], vb[axis]
        if da <= pos:
            grow(L, va, zero)
        if da >= pos:
            grow(R, va, zero)
        if (da < pos and db > pos) or (da > pos and db < pos):
            w = F32(F32(pos - da) / F32(db - da))
            p = [F32(va[k] + F32(w * F32(vb[k] - va[k]))) for k in range(3)]
            pad = [F32(0) if mutant == "no_pad" else F32(PAD * max(abs(va[k]), abs(vb[k]))) for k in range(3)]
            if mutant != "no_snap":
                p[axis] = pos
            pad[axis] = F32(0)
            grow(L, p, pad)
            grow(R, p, pad)
    if mutant != "no_clamp":
        for k in range(3):
            L[k] = max(L[k], b[k]); L[3 + k] = min(L[3 + k], b[3 + k])
            R[k] = max(R[k], b[k]); R[3 + k] = min(R[3 + k], b[3 + k])
    L[3 + axis] = min(L[3 + axis], pos)
    R[axis] = max(R[axis], pos)
    ok = all(L[k] <= L[3 + k] and R[k] <= R[3 + k] for k in range(3))
    return ok, L, R


def pieces(v, full, slop, grid, s, mutant=None, stack_size=STACK):
    """splitTriangle for s splits.  Returns (boxes [n, 6] binary32 in emission order, cells: per piece the list of (axis, position,
    side) half-spaces -- side -1: x_axis <= position, +1: x_axis >= position -- on the path that produced it)."""
    v = [[F32(c) for c in p] for p in np.asarray(v, F32)]
    b0 = [min(v[0][k], min(v[1][k], v[2][k])) for k in range(3)] + [max(v[0][k], max(v[1][k], v[2][k])) for k in range(3)]
    stack = [(b0, int(s), ())]
    boxes, cells = [], []
    slop = F32(slop)
    while stack:
        b, left, cell = stack.pop()
        cut = False
        axis, pos, L, R = -1, F32(0), None, None
        while left > 0 and not cut:
            axis, pos, _ = split_plane(grid, b, mutant)
            if axis < 0:
                break
            ok, L, R = split_clip(v, b, axis, pos, mutant)
            if ok:
                cut = True
            else:  # the triangle lies on one side of the plane inside this box: the box shrinks to that side, one split is spent
                left_ok = L[0] <= L[3] and L[1] <= L[4] and L[2] <= L[5]
                keep = L if left_ok else R
                if not (keep[0] <= keep[3] and keep[1] <= keep[4] and keep[2] <= keep[5]):
                    break
                b = list(keep)
                cell = cell + ((axis, pos, -1 if left_ok else 1),)
                left -= 1
        if not cut or len(stack) + 2 > stack_size:
            boxes.append([max(F32(b[k] - slop), full[k]) for k in range(3)] + [min(F32(b[3 + k] + slop), full[3 + k]) for k in range(3)])
            cells.append(cell)
            continue
        wa = max(F32(L[3] - L[0]), max(F32(L[4] - L[1]), F32(L[5] - L[2])))
        wb = max(F32(R[3] - R[0]), max(F32(R[4] - R[1]), F32(R[5] - R[2])))
        rest = left - 1
        if mutant == "half_and_half":
            sa = rest // 2
        elif F32(wa + wb) > 0:
            sa = int(F32(F32(F32(rest) * F32(wa / F32(wa + wb))) + F32(0.5)))
        else:
            sa = rest // 2
        sa = min(sa, rest)
        sb = rest - sa
        A = (list(L), sa, cell + ((axis, pos, -1),))
        B = (list(R), sb, cell + ((axis, pos, 1),))
        stack += [A, B] if sa >= sb else [B, A]  # the smaller share is taken first
    return np.array(boxes, F32).reshape(-1, 6), cells


def all_pieces(sc, splits, mutant=None):
    """pieces() of every triangle of a Scene for the given splits per triangle.  Returns (counts [T], boxes [sum, 6], cells: list per
    triangle or None where the triangle stays whole -- its only piece is its own box and its cell is all of space)."""
    counts = np.ones(sc.T, np.int64)
    lo = np.minimum(sc.v[:, 0], np.minimum(sc.v[:, 1], sc.v[:, 2]))
    hi = np.maximum(sc.v[:, 0], np.maximum(sc.v[:, 1], sc.v[:, 2]))
    with np.errstate(all="ignore"):
        whole = np.concatenate([np.maximum((lo - sc.slop[:, None]).astype(F32), sc.full[:, 0:3]),
                                np.minimum((hi + sc.slop[:, None]).astype(F32), sc.full[:, 3:6])], 1)
    out, cells = [], [None] * sc.T
    for g in range(sc.T):
        if splits[g] > 0:
            bx, cells[g] = pieces(sc.v[g], sc.full[g], sc.slop[g], sc.grid, int(splits[g]), mutant)
            counts[g] = bx.shape[0]
            out.append(bx)
        else:
            out.append(whole[g:g + 1])
    return counts, np.concatenate(out, 0) if out else np.zeros((0, 6), F32), cells


# ---- exact geometry ------------------------------------------------------------------------------------------------------------------

def clip_exact(v, cell):
    """Sutherland-Hodgman: the triangle v [3][3] (binary32) clipped against the closed half-spaces of `cell`, in rational arithmetic.
    Returns the polygon as a list of 3-tuples of Fraction (empty, a point or a segment given as a degenerate polygon are possible)."""
    poly = [tuple(Fraction(float(c)) for c in p) for p in v]
    for axis, pos, side in cell:
        pos = Fraction(float(pos))
        if not poly:
            break
        out = []
        for i, a in enumerate(poly):
            z = poly[(i + 1) % len(poly)]
            da, dz = (a[axis] - pos) * side, (z[axis] - pos) * side  # >= 0: inside
            if da >= 0:
                out.append(a)
            if (da > 0 and dz < 0) or (da < 0 and dz > 0):
                w = da / (da - dz)
                out.append(tuple(pos if k == axis else a[k] + w * (z[k] - a[k]) for k in range(3)))
        poly = out
    return poly


def vector_area_exact(poly):
    """Twice the polygon's vector area, three Fractions (the fan from its first vertex): zero for a point or a segment.  The pieces of
    a triangle lie in its plane with its orientation, so their areas sum to the triangle's exactly when their vector areas do."""
    n = [Fraction(0)] * 3
    for i in range(1, len(poly) - 1):
        a = [poly[i][k] - poly[0][k] for k in range(3)]
        b = [poly[i + 1][k] - poly[0][k] for k in range(3)]
        n[0] += a[1] * b[2] - a[2] * b[1]
        n[1] += a[2] * b[0] - a[0] * b[2]
        n[2] += a[0] * b[1] - a[1] * b[0]
    return n


def violations(v, cells, boxes):
    """Exact containment of every piece in its box.  Returns (the number of polygon coordinates outside their piece's box, the smallest
    slack as a float: the distance to the nearer face of the box over the coordinates a cut COMPUTED -- those of cut points, without the
    coordinate that lies on a plane of the cell: the margin the pad of the cut points has left; inf when there is none)."""
    bad, slack = 0, None
    vx = [tuple(Fraction(float(c)) for c in p) for p in v]
    for cell, box in zip(cells, boxes):
        lo = [Fraction(float(c)) for c in box[0:3]]
        hi = [Fraction(float(c)) for c in box[3:6]]
        planes = {(axis, Fraction(float(pos))) for axis, pos, _ in cell}
        for p in clip_exact(v, cell):
            for k in range(3):
                if p[k] < lo[k] or p[k] > hi[k]:
                    bad += 1
                if p not in vx and (k, p[k]) not in planes:
                    d = min(p[k] - lo[k], hi[k] - p[k])
                    slack = d if slack is None or d < slack else slack
    return bad, (float(slack) if slack is not None else float("inf"))
