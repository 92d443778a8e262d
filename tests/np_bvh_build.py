"""numpy restatement of the device builders' TOPOLOGY (lbvh.hip, ploc.hip, the host SAH pass over the upper levels) and of the optimum the
wide collapse must reach (wide_collapse.hip), written from the file headers and the papers they cite:

  Morton keys   21 bits per axis of the box centre inside the scene bounds, x lowest; a stable sort of (key, flattened id)
  Karras 2012   "Maximizing Parallelism in the Construction of BVHs, Octrees, and k-d Trees", section 4; equal keys are told apart by position
  Meister & Bittner 2018  "Parallel Locally-Ordered Clustering for Bounding Volume Hierarchy Construction": nearest neighbour in a window
                of the Morton order, mutual pairs merge, the array is compacted, until one cluster is left
  Garanzha et al. 2011    (HLBVH) the levels above subtrees of <= K triangles are rebuilt with a SAH sweep over those subtrees
  the collapse  C(n, i): the cheapest way to show n's subtree as at most i children of one wide node

The library is compiled without contraction and without fast-math, so wherever the builders compute in float32 the same float32
expression in numpy gives the same bits, and the node ids are handed out deterministically: the trees below are the trees the device
must install, node for node.  A hierarchy here is a dict: "children" [T - 1, 2] int64 (>= 0 an internal node, < 0 ~(leaf position)),
"count" [T - 1] triangles below, "lo" / "hi" [T - 1, 3] float32 boxes, "first" [T - 1] lowest leaf position below (Karras only: its
subtrees are runs of the order; -1 elsewhere)."""
import numpy as np

F32 = np.float32
PLOC_RADIUS = 16
TOP_MIN_TRIANGLES = 4096  # the upper-level pass runs above this (PLOC only)
TOP_SWEEP_MAX = 1024      # ranges up to this size get the full sweep, larger ones 32 bins
TOP_BINS = 32


# ---- keys and order -------------------------------------------------------------------------------------------------------------

def scene_bounds(lo, hi):
    """What k_flatten accumulates: min / max of the triangle boxes as the builders see them -- slop included."""
    return np.asarray(lo, F32).min(axis=0), np.asarray(hi, F32).max(axis=0)


def _spread21(v):
    v = np.asarray(v, np.uint64)
    out = np.zeros(v.shape, np.uint64)
    for b in range(21):
        out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def morton_cells(lo, hi, slo, shi):
    """The 21-bit cell of every box centre on each axis, [T, 3] uint64."""
    lo = np.asarray(lo, F32)
    hi = np.asarray(hi, F32)
    c = F32(0.5) * (lo + hi)
    ext = (np.asarray(shi, F32) - np.asarray(slo, F32)).astype(F32)
    with np.errstate(all="ignore"):
        t = np.where(ext > 0, (c - np.asarray(slo, F32)) / ext, F32(0)).astype(F32)
        t = t * F32(2097152.0)
    t = np.minimum(np.maximum(t, F32(0)), F32(2097151.0))
    return t.astype(np.int64).astype(np.uint64)  # truncation of a value in [0, 2^21)


def morton_keys(lo, hi, slo=None, shi=None):
    """63-bit keys of boxes lo / hi [T, 3] float32 (in flattened-id order) inside the scene bounds (default: their own)."""
    if slo is None:
        slo, shi = scene_bounds(lo, hi)
    q = morton_cells(lo, hi, slo, shi)
    return _spread21(q[:, 0]) | (_spread21(q[:, 1]) << np.uint64(1)) | (_spread21(q[:, 2]) << np.uint64(2))


def sorted_order(keys):
    """Flattened ids in leaf order: ascending key, ascending id within equal keys."""
    return np.argsort(np.asarray(keys, np.uint64), kind="stable")


# ---- Karras radix tree ----------------------------------------------------------------------------------------------------------

def _bit_length(x):
    x = np.asarray(x, np.uint64).copy()
    n = np.zeros(x.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        m = (x >> np.uint64(s)) != 0
        n += m * s
        x = np.where(m, x >> np.uint64(s), x)
    return n + (x != 0)


def _delta(keys, i, j):
    """Length of the common prefix of the (key, position) pairs at i and j: equal keys share all 64 key bits and then the leading bits
    of their 32-bit positions; -1 outside the array."""
    n = keys.size
    ok = (j >= 0) & (j < n)
    jj = np.clip(j, 0, n - 1)
    x = keys[i] ^ keys[jj]
    d = np.where(x == 0, 64 + 32 - _bit_length((i ^ jj).astype(np.uint64)), 64 - _bit_length(x))
    return np.where(ok, d, -1)


def karras(keys):
    """The radix tree over sorted keys [T] uint64, T >= 2: internal node i sits at one end of its range of positions."""
    keys = np.asarray(keys, np.uint64)
    n = keys.size
    assert n >= 2
    i = np.arange(n - 1, dtype=np.int64)
    d = np.where(_delta(keys, i, i + 1) - _delta(keys, i, i - 1) >= 0, 1, -1)
    dmin = _delta(keys, i, i - d)
    lmax = np.full(n - 1, 2, np.int64)
    while True:  # an upper bound of the range's length, by doubling
        grow = _delta(keys, i, i + lmax * d) > dmin
        if not grow.any():
            break
        lmax = np.where(grow, lmax * 2, lmax)
    l = np.zeros(n - 1, np.int64)
    t = lmax // 2
    while (t >= 1).any():  # the other end, by bisection
        take = (t >= 1) & (_delta(keys, i, i + (l + t) * d) > dmin)
        l = np.where(take, l + t, l)
        t = t // 2
    j = i + l * d
    dnode = _delta(keys, i, j)
    s = np.zeros(n - 1, np.int64)
    t = l.copy()
    live = np.ones(n - 1, bool)
    while live.any():  # the split: the last position that shares more than the node's prefix with i
        t = np.where(live, (t + 1) >> 1, t)
        take = live & (_delta(keys, i, i + (s + t) * d) > dnode)
        s = np.where(take, s + t, s)
        live &= t > 1
    gamma = i + s * d + np.minimum(d, 0)
    first, last = np.minimum(i, j), np.maximum(i, j)
    left = np.where(first == gamma, ~gamma, gamma)
    right = np.where(last == gamma + 1, ~(gamma + 1), gamma + 1)
    return {"children": np.stack([left, right], 1), "count": last - first + 1, "first": first}


def karras_recursive(keys):
    """The definition, top-down: a range [a, b] splits after g, the last position whose (key, position) pair has a 0 in the highest bit
    that differs inside the range.  The left child, over [a, g], is node g; the right one, over [g + 1, b], is node g + 1; the root is
    node 0; a range of one position is that leaf."""
    n = len(keys)
    aug = [(int(k) << 32) | p for p, k in enumerate(keys)]
    children = np.zeros((n - 1, 2), np.int64)
    count = np.zeros(n - 1, np.int64)
    first = np.zeros(n - 1, np.int64)
    stack = [(0, 0, n - 1)]
    while stack:
        node, a, b = stack.pop()
        bit = (aug[a] ^ aug[b]).bit_length() - 1
        g = max(p for p in range(a, b + 1) if not (aug[p] >> bit) & 1)
        count[node], first[node] = b - a + 1, a
        for c, (x, y, nid) in enumerate(((a, g, g), (g + 1, b, g + 1))):
            if x == y:
                children[node, c] = ~x
            else:
                children[node, c] = nid
                stack.append((nid, x, y))
    return {"children": children, "count": count, "first": first}


def fit_boxes(h, leaf_lo, leaf_hi):
    """Bottom-up boxes of a hierarchy (min / max are exact: no order matters); fills h["lo"], h["hi"]."""
    ch = h["children"]
    n = ch.shape[0]
    lo = np.zeros((n, 3), F32)
    hi = np.zeros((n, 3), F32)
    for lvl in reversed(levels_of(ch)):
        for c in range(2):
            r = ch[lvl, c]
            clo = np.where((r < 0)[:, None], leaf_lo[np.where(r < 0, ~r, 0)], lo[np.maximum(r, 0)])
            chi = np.where((r < 0)[:, None], leaf_hi[np.where(r < 0, ~r, 0)], hi[np.maximum(r, 0)])
            lo[lvl] = clo if c == 0 else np.minimum(lo[lvl], clo)
            hi[lvl] = chi if c == 0 else np.maximum(hi[lvl], chi)
    h["lo"], h["hi"] = lo, hi
    return h


def levels_of(children, root=0):
    """Internal nodes level by level from the root."""
    out = []
    cur = np.array([root], np.int64)
    while cur.size:
        out.append(cur)
        r = children[cur].reshape(-1)
        cur = r[r >= 0]
    return out


# ---- PLOC -----------------------------------------------------------------------------------------------------------------------

def _half_area(lo, hi):
    d = hi - lo
    return (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2]) + d[..., 2] * d[..., 0]


def _merge_cost(metric, lo_i, hi_i, n_i, lo_j, hi_j, n_j, a_j):
    """What cluster i pays for merging with j, float32 (the terms that depend on i alone are left out: they do not change i's choice).
    0: the area of the union (the paper's distance); 1: that minus j's area; otherwise what the merge adds to the SAH sum."""
    with np.errstate(all="ignore"):
        u = _half_area(np.minimum(lo_i, lo_j), np.maximum(hi_i, hi_j))
        if metric == 0:
            return u
        if metric == 1:
            return u - a_j
        return u * (n_i + n_j) - a_j * n_j


def _ploc_apply(nn, lo, hi, ref, cnt, next_id, out):
    """Mutual picks merge into the lower position; ids from next_id downwards in position order; survivors keep their order."""
    nc = nn.size
    i = np.arange(nc)
    mutual = (nn >= 0) & (nn[np.maximum(nn, 0)] == i)
    absorbs = mutual & (i < nn)
    absorbed = mutual & (i > nn)
    a = np.flatnonzero(absorbs)
    b = nn[a]
    ids = next_id - np.arange(a.size)
    out["children"][ids, 0], out["children"][ids, 1] = ref[a], ref[b]
    lo, hi, ref, cnt = lo.copy(), hi.copy(), ref.copy(), cnt.copy()
    lo[a], hi[a] = np.minimum(lo[a], lo[b]), np.maximum(hi[a], hi[b])
    cnt[a] = cnt[a] + cnt[b]
    ref[a] = ids
    out["lo"][ids], out["hi"][ids], out["count"][ids] = lo[a], hi[a], cnt[a]
    keep = ~absorbed
    return lo[keep], hi[keep], ref[keep], cnt[keep], a.size


def _ploc_out(T):
    return {"children": np.zeros((T - 1, 2), np.int64), "count": np.zeros(T - 1, np.int64), "lo": np.zeros((T - 1, 3), F32),
            "hi": np.zeros((T - 1, 3), F32), "first": np.full(T - 1, -1, np.int64)}


def _ploc_loop(leaf_lo, leaf_hi, metric, pick):
    T = leaf_lo.shape[0]
    assert T >= 2
    out = _ploc_out(T)
    lo, hi = np.asarray(leaf_lo, F32).copy(), np.asarray(leaf_hi, F32).copy()
    ref = ~np.arange(T, dtype=np.int64)
    cnt = np.ones(T, np.int64)
    next_id = T - 2
    forced = False
    passes = []
    while ref.size > 1:
        nc = ref.size
        i = np.arange(nc)
        if forced:  # the pass after one that merged nothing: neighbours pair up
            nn = np.where((i ^ 1) < nc, i ^ 1, -1)
        elif metric == 98:  # the hook: picks that are never mutual
            nn = np.where(i + 1 < nc, i + 1, -1)
        else:
            nn = pick(lo, hi, cnt, metric)
        lo, hi, ref, cnt, merged = _ploc_apply(nn, lo, hi, ref, cnt, next_id, out)
        assert merged > 0 or not forced, "a forced pass must merge"
        passes.append((nc, merged, forced))
        forced = merged == 0
        next_id -= merged
    assert next_id == -1
    out["passes"] = passes
    return out


def _pick_vectorised(lo, hi, cnt, metric):
    """nc x 33 candidates: position i ^ 1 first, then the 32 positions within the radius in ascending order; the first strictly
    smallest cost wins."""
    nc = cnt.size
    i = np.arange(nc)
    offs = np.array([o for o in range(-PLOC_RADIUS, PLOC_RADIUS + 1) if o != 0])
    cand = np.concatenate([(i ^ 1)[:, None], i[:, None] + offs[None, :]], axis=1)
    valid = (cand >= 0) & (cand < nc)
    valid[:, 1:] &= cand[:, 1:] != cand[:, :1]
    j = np.clip(cand, 0, nc - 1)
    area = _half_area(lo, hi)
    nf = cnt.astype(F32)
    d = _merge_cost(metric, lo[:, None, :], hi[:, None, :], nf[:, None], lo[j], hi[j], nf[j], area[j])
    assert np.isfinite(d[valid]).all(), "non-finite merge cost"
    d = np.where(valid, d, np.inf)
    col = np.argmin(d, axis=1)
    return np.where(valid[i, col], cand[i, col], -1)


def _pick_scalar(lo, hi, cnt, metric):
    """The rule as a plain loop (the witness of _pick_vectorised)."""
    nc = cnt.size
    area = _half_area(lo, hi)
    nn = np.full(nc, -1, np.int64)
    for i in range(nc):
        def cost(j):
            return _merge_cost(metric, lo[i], hi[i], F32(cnt[i]), lo[j], hi[j], F32(cnt[j]), area[j])
        best, pick = F32(np.inf), -1
        partner = i ^ 1
        if partner < nc:
            best, pick = cost(partner), partner
        for j in range(max(0, i - PLOC_RADIUS), min(nc - 1, i + PLOC_RADIUS) + 1):
            if j == i or j == partner:
                continue
            c = cost(j)
            if c < best or pick < 0:
                best, pick = c, j
        nn[i] = pick
    return nn


def ploc(leaf_lo, leaf_hi, metric=2):
    """The clustering over leaf boxes in Morton order ([T, 3] float32 each)."""
    return _ploc_loop(leaf_lo, leaf_hi, metric, _pick_vectorised)


def ploc_scalar(leaf_lo, leaf_hi, metric=2):
    return _ploc_loop(leaf_lo, leaf_hi, metric, _pick_scalar)


# ---- the SAH pass over the upper levels -------------------------------------------------------------------------------------------

def top_frontier(h, T):
    """K, the sorted ids of the internal nodes with more than K triangles, and the frontier -- the subtrees (or single leaves) of
    <= K triangles hanging under them -- as references sorted ascending (leaves, negative, come first)."""
    K = max(16, T // 2048)
    ch, cnt = h["children"], h["count"]
    above = cnt > K
    ids = np.flatnonzero(above)
    kids = ch[ids].reshape(-1)
    small = np.where(kids < 0, True, ~above[np.maximum(kids, 0)])
    return K, ids, np.sort(kids[small])


class _TopBuilder:
    def __init__(self, ref, cnt, lo, hi, ids):
        self.ref, self.cnt, self.lo, self.hi, self.ids = ref.copy(), cnt.copy(), lo.copy(), hi.copy(), ids
        self.next = 0
        self.nodes = []  # (id, left, right, count, lo, hi) in build order

    def _permute(self, a, b, p):
        for arr in (self.ref, self.cnt, self.lo, self.hi):
            arr[a:b] = arr[a:b][p]

    @staticmethod
    def sweep_costs(cnt, lo, hi):
        """Cost of every split k = 1 .. n - 1 of entries in the given order: area(left) * count(left) + area(right) * count(right)."""
        llo, lhi = np.minimum.accumulate(lo, axis=0), np.maximum.accumulate(hi, axis=0)
        rlo, rhi = np.minimum.accumulate(lo[::-1], axis=0)[::-1], np.maximum.accumulate(hi[::-1], axis=0)[::-1]
        lc, rc = np.cumsum(cnt), np.cumsum(cnt[::-1])[::-1]
        return _half_area(llo[:-1], lhi[:-1]) * lc[:-1].astype(F32) + _half_area(rlo[1:], rhi[1:]) * rc[1:].astype(F32)

    def _sort_keys(self, a, b, axis):
        return np.lexsort((self.ref[a:b], self.lo[a:b, axis] + self.hi[a:b, axis]))  # by centre (lo + hi), then by reference

    def _sweep(self, a, b):
        n = b - a
        best = None
        for axis in range(3):
            p = self._sort_keys(a, b, axis)
            c = self.sweep_costs(self.cnt[a:b][p], self.lo[a:b][p], self.hi[a:b][p])
            k = np.arange(1, n)
            off = np.abs(k - n // 2)  # equal costs: the split nearest the middle, then the first found
            cmin = c.min()
            at = np.flatnonzero(c == cmin)
            w = at[np.argmin(off[at])]
            cand = (float(cmin), int(off[w]), axis, int(k[w]))
            if best is None or cand[:2] < best[:2]:
                best = cand
        assert np.isfinite(best[0]), "non-finite sweep cost"
        axis, split = best[2], best[3]
        self._permute(a, b, self._sort_keys(a, b, axis))
        return a + split

    def _binned(self, a, b):
        c = (self.lo[a:b] + self.hi[a:b]).astype(F32)
        clo, chi = c.min(axis=0), c.max(axis=0)
        best, best_axis, best_bin = F32(np.inf), -1, 0
        bins_of = {}
        for axis in range(3):
            ext = F32(chi[axis] - clo[axis])
            if not ext > 0:
                continue
            scale = F32(TOP_BINS) / ext
            bins = np.clip(((c[:, axis] - clo[axis]) * scale).astype(np.int64), 0, TOP_BINS - 1)
            bins_of[axis] = bins
            blo = np.full((TOP_BINS, 3), np.inf, F32)
            bhi = np.full((TOP_BINS, 3), -np.inf, F32)
            np.minimum.at(blo, bins, self.lo[a:b])
            np.maximum.at(bhi, bins, self.hi[a:b])
            bc = np.bincount(bins, weights=self.cnt[a:b], minlength=TOP_BINS).astype(np.int64)
            llo, lhi = np.minimum.accumulate(blo, axis=0), np.maximum.accumulate(bhi, axis=0)
            rlo, rhi = np.minimum.accumulate(blo[::-1], axis=0)[::-1], np.maximum.accumulate(bhi[::-1], axis=0)[::-1]
            lc, rc = np.cumsum(bc), np.cumsum(bc[::-1])[::-1]
            for k in range(1, TOP_BINS):  # left = bins below k
                if lc[k - 1] == 0 or rc[k] == 0:
                    continue
                cost = _half_area(llo[k - 1], lhi[k - 1]) * F32(lc[k - 1]) + _half_area(rlo[k], rhi[k]) * F32(rc[k])
                # equal costs on one axis: the cut nearest the middle bin
                if cost < best or (cost == best and best_axis == axis and abs(k - TOP_BINS // 2) < abs(best_bin - TOP_BINS // 2)):
                    best, best_axis, best_bin = cost, axis, k
        n = b - a
        if best_axis < 0:
            return a + n // 2  # all centres coincide
        left = bins_of[best_axis] < best_bin
        self._permute(a, b, np.concatenate([np.flatnonzero(left), np.flatnonzero(~left)]))  # a partition that keeps order
        split = int(left.sum())
        return a + (split if 0 < split < n else n // 2)

    def build(self, a, b):
        if b - a == 1:
            return int(self.ref[a])
        nid = int(self.ids[self.next])
        self.next += 1
        split = self._binned(a, b) if b - a > TOP_SWEEP_MAX else self._sweep(a, b)
        slot = len(self.nodes)
        self.nodes.append(None)
        lo, hi, cnt = self.lo[a:b].min(axis=0), self.hi[a:b].max(axis=0), int(self.cnt[a:b].sum())
        left = self.build(a, split)
        right = self.build(split, b)
        self.nodes[slot] = (nid, left, right, cnt, lo, hi)
        return nid


def top_levels_sah(h, leaf_lo, leaf_hi):
    """The hierarchy with its levels above the frontier rebuilt; new nodes take the ids of the nodes they replace in build order
    (node, then its left subtree, then its right one), the root keeps id 0.  Returns (hierarchy, frontier size)."""
    import sys

    T = leaf_lo.shape[0]
    K, ids, fr = top_frontier(h, T)
    F = fr.size
    if not (2 <= F <= 32768 and ids.size + 1 == F):
        return h, F
    leaf = fr < 0
    pos, node = np.where(leaf, ~fr, 0), np.maximum(fr, 0)
    cnt = np.where(leaf, 1, h["count"][node])
    lo = np.where(leaf[:, None], leaf_lo[pos], h["lo"][node]).astype(F32)
    hi = np.where(leaf[:, None], leaf_hi[pos], h["hi"][node]).astype(F32)
    tb = _TopBuilder(fr, cnt, lo, hi, ids)
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * F + 1000))
    try:
        tb.build(0, F)
    finally:
        sys.setrecursionlimit(old)
    out = {k: v.copy() for k, v in h.items() if isinstance(v, np.ndarray)}
    for nid, left, right, c, blo, bhi in tb.nodes:
        out["children"][nid] = (left, right)
        out["count"][nid], out["lo"][nid], out["hi"][nid] = c, blo, bhi
        out["first"][nid] = -1
    return out, F


# ---- emission -------------------------------------------------------------------------------------------------------------------

def emit(h, T, k_leaf):
    """The BVH2 a walk from the root sees: (root reference, {node id: (left reference, right reference)}).  A subtree of <= k_leaf
    triangles is one leaf ~((first position << 3) | (count - 1)); the root node always stands."""
    if T <= k_leaf:
        return ~(T - 1), {}
    ch, cnt, first = h["children"], h["count"], h["first"]
    out = {}
    stack = [0]
    while stack:
        n = stack.pop()
        refs = []
        for c in ch[n]:
            c = int(c)
            if c < 0:
                refs.append(~((~c) << 3))
            elif cnt[c] <= k_leaf:
                assert first[c] >= 0, "a collapsed leaf must be a run of the order"
                refs.append(~((int(first[c]) << 3) | (int(cnt[c]) - 1)))
            else:
                refs.append(c)
                stack.append(c)
        out[n] = tuple(refs)
    return 0, out


# ---- checks of a hierarchy ------------------------------------------------------------------------------------------------------

def check_hierarchy(h, T):
    """Every leaf once, node ids exactly 0 .. T - 2 with node 0 the root, counts consistent."""
    ch = h["children"]
    assert ch.shape == (T - 1, 2)
    lv = levels_of(ch)
    reached = np.concatenate(lv)
    assert np.array_equal(np.sort(reached), np.arange(T - 1)), "node ids are not 0 .. T - 2, each reached once from node 0"
    leaves = ~ch[ch < 0]
    assert np.array_equal(np.sort(leaves), np.arange(T)), "a leaf is missing or repeated"
    cnt = np.zeros(T - 1, np.int64)
    for lvl in reversed(lv):
        r = ch[lvl]
        cnt[lvl] = np.where(r < 0, 1, cnt[np.maximum(r, 0)]).sum(axis=1)
    assert np.array_equal(cnt, h["count"]), "triangle counts"
    return lv


def depth_of(h):
    return len(levels_of(h["children"]))


# ---- the collapse optimum -------------------------------------------------------------------------------------------------------

def collapse_tables(h, leaf_lo, leaf_hi, dtype=np.float64):
    """The tables of the collapse over the binary tree with unit leaves and float32 boxes, evaluated in `dtype`:
       C(n, 1) = min(area x prims if prims <= 3, area + D(n, 8)),  C(n, i) = min(C(n, i - 1), D(n, i)),
       D(n, j) = min over k = 1 .. j - 1 of C(left, min(k, 7)) + C(right, min(j - k, 7));  a leaf costs its area for every i.
    Returns a dict: "C" [T - 1, 8] (column 0 unused), "D8", "area" [T - 1], "leaf_area" [T], and the choices that reach the minima
    under the usual rules of such a table -- the lowest k among equal sums, the leaf form when it costs no more than the node form, no
    extra slot unless it is strictly cheaper: "leaf_form" [T - 1], "k8" [T - 1] (k of D(n, 8)), "k" [T - 1, 8] (k of D(n, i) where
    C(n, i) = D(n, i) < C(n, i - 1), else 0)."""
    ch, cnt = h["children"], h["count"]
    n = ch.shape[0]
    two = dtype(2)
    area = (two * _half_area(h["lo"].astype(dtype), h["hi"].astype(dtype))).astype(dtype)
    leaf_area = (two * _half_area(np.asarray(leaf_lo, F32).astype(dtype), np.asarray(leaf_hi, F32).astype(dtype))).astype(dtype)
    t = {"C": np.zeros((n, 8), dtype), "D8": np.zeros(n, dtype), "area": area, "leaf_area": leaf_area, "leaf_form": np.zeros(n, bool),
         "k8": np.zeros(n, np.int64), "k": np.zeros((n, 8), np.int64)}
    C = t["C"]
    inf = dtype(np.inf)
    for lvl in reversed(levels_of(ch)):
        side = []
        for c in range(2):
            r = ch[lvl, c]
            side.append(np.where((r < 0)[:, None], leaf_area[np.where(r < 0, ~r, 0)][:, None], C[np.maximum(r, 0)]).astype(dtype))
        L, R = side

        def D(j):
            sums = np.stack([L[:, min(k, 7)] + R[:, min(j - k, 7)] for k in range(1, j)], axis=1)
            first = np.argmin(sums, axis=1)
            return sums[np.arange(lvl.size), first], first + 1

        d8, k8 = D(8)
        internal = area[lvl] + d8
        leaf = np.where(cnt[lvl] <= 3, area[lvl] * cnt[lvl].astype(dtype), inf)
        t["leaf_form"][lvl] = leaf <= internal
        C[lvl, 1] = np.where(leaf <= internal, leaf, internal)
        t["D8"][lvl], t["k8"][lvl] = d8, k8
        for i in range(2, 8):
            d, k = D(i)
            better = d < C[lvl, i - 1]
            C[lvl, i] = np.where(better, d, C[lvl, i - 1])
            t["k"][lvl, i] = np.where(better, k, 0)
    return t


def collapse_optimum(h, leaf_lo, leaf_hi):
    """The SAH sum (not divided by the root's area) of the best wide tree, in float64: the root is always a wide node; its children
    are the best 8-slot cut -- or, when the whole scene is cheapest as one leaf (<= 3 triangles), that one leaf child."""
    t = collapse_tables(h, leaf_lo, leaf_hi)
    return float(t["area"][0] + t["C"][0, 1]) if t["leaf_form"][0] else float(t["C"][0, 1])


def collapse_cuts(h, t):
    """The wide tree read off the tables t top-down: {binary node a wide node stands for: (sorted references of its children, sorted
    references of those among them that are leaf children)}.  A child with i slots to spend takes the largest i' <= i at which a slot
    more was strictly cheaper and hands k of them to its left subtree; with one slot it is a child itself -- a leaf child if it is a
    triangle or took the leaf form, else a wide node of its own."""
    ch = h["children"]
    out = {}
    todo = [0]
    while todo:
        root = todo.pop()
        if root == 0 and t["leaf_form"][0]:
            out[0] = ((0,), (0,))
            continue
        kids = []
        k8 = int(t["k8"][root])
        stack = [(int(ch[root, 1]), min(8 - k8, 7)), (int(ch[root, 0]), min(k8, 7))]
        while stack:
            c, i = stack.pop()
            if c >= 0:
                while i > 1 and t["k"][c, i] == 0:
                    i -= 1
            if c < 0 or i == 1:
                kids.append(c)
                continue
            k = int(t["k"][c, i])
            stack.append((int(ch[c, 1]), min(i - k, 7)))
            stack.append((int(ch[c, 0]), min(k, 7)))
        assert 2 <= len(kids) <= 8
        leaves = [c for c in kids if c < 0 or t["leaf_form"][c]]
        todo.extend(c for c in kids if not (c < 0 or t["leaf_form"][c]))
        out[root] = (tuple(sorted(kids)), tuple(sorted(leaves)))
    return out
