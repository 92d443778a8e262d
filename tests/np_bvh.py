"""numpy restatement of the tree layouts, their box rules and the SAH cost (include/vkrt.h sah_cost), written from the headers that define
them -- not from the kernels -- so that the tests can hold every builder and the refit to it:

  tri_prep.h   vkrt_tri_slop / vkrt_tri_bounds: a triangle's box from its 48-B record, in float32 in the header's operation order
  wide_node.h  vkrt_wnode_quantise / vkrt_wnode_store_planes: the grid and the 8-bit planes of a wide8 node
  bvh_host.h   the 80-B wide8 node words; device_scene.h: the 64-B BVH2 node (two float boxes, two refs, leaf = ~(first << 3 | count - 1))

exact_wide8 / exact_bvh2 recompute, bottom-up and level by level, the node words a tree with the given topology must hold when each leaf box
is the union of its records' whole-triangle boxes (the build rule without pre-splitting, and the refit rule always)."""
import numpy as np

F32 = np.float32
QMAX = 255
TRAV_DONE = -0x80000000
_SLOP_K = F32(9.5367431640625e-07)  # 16 * 2^-24


# ---- tri_prep.h -----------------------------------------------------------------------------------------------------------------

def tri_slop(e1, e2):
    """vkrt_tri_slop for [n, 3] float32 edges."""
    e1 = np.asarray(e1, F32)
    e2 = np.asarray(e2, F32)
    with np.errstate(all="ignore"):
        l1 = (e1[:, 0] * e1[:, 0] + e1[:, 1] * e1[:, 1]) + e1[:, 2] * e1[:, 2]
        l2 = (e2[:, 0] * e2[:, 0] + e2[:, 1] * e2[:, 1]) + e2[:, 2] * e2[:, 2]
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        a2 = (cx * cx + cy * cy) + cz * cz
        ln = np.sqrt(np.where(l1 > l2, l1, l2))
        inv_sin = np.sqrt((l1 * l2) / a2)
        s = (_SLOP_K * ln) * inv_sin
        s = np.where(s < ln, s, ln)
        return np.where((a2 > 0) & (inv_sin > F32(8)), s, F32(0)).astype(F32)


def record_bounds(rec, watertight):
    """Box of every 48-B record ([n, 12] float32): (v0, e1, e2) Moeller-Trumbore records or watertight (p0, p1, p2) ones, read as refit.hip
    reads them and boxed by vkrt_tri_bounds.  Returns (lo, hi), [n, 3] float32 each."""
    rec = np.asarray(rec, F32).reshape(-1, 12)
    p0, r1, r2 = rec[:, 0:3], rec[:, 3:6], rec[:, 6:9]
    with np.errstate(all="ignore"):
        if watertight:
            e1, e2, q1, q2 = r1 - p0, r2 - p0, r1, r2
        else:
            e1, e2 = r1, r2
            q1, q2 = p0 + e1, p0 + e2
    slop = tri_slop(e1, e2)[:, None]
    lo, hi = p0.copy(), p0.copy()
    for q in (q1, q2):
        lo = np.where(q < lo, q, lo)
        hi = np.where(q > hi, q, hi)
    with np.errstate(all="ignore"):
        return (lo - slop).astype(F32), (hi + slop).astype(F32)


# ---- wide_node.h ----------------------------------------------------------------------------------------------------------------

def quantise(lo, hi, mask, slo, shi):
    """vkrt_wnode_quantise for n nodes: lo, hi [n, 3] float32; mask [n] slot bits; slo, shi [n, 8, 3] float32.
    Returns eb [n, 3] (biased exponents) and qlo, qhi [n, 3, 8] (int64 planes, 0 in empty slots)."""
    lo = np.asarray(lo, F32).reshape(-1, 3)
    hi = np.asarray(hi, F32).reshape(-1, 3)
    n = lo.shape[0]
    occ = ((np.asarray(mask, np.int64).reshape(-1, 1) >> np.arange(8)) & 1).astype(bool)  # [n, 8]
    slo = np.asarray(slo, F32).reshape(n, 8, 3).transpose(0, 2, 1).astype(np.float64)   # [n, 3, 8]
    shi = np.asarray(shi, F32).reshape(n, 8, 3).transpose(0, 2, 1).astype(np.float64)
    o = lo.astype(np.float64)
    ext = hi.astype(np.float64) - o
    with np.errstate(all="ignore"):
        m, ex = np.frexp(ext / float(QMAX))
    e = np.where(ext > 0, np.where(m == 0.5, ex - 1, ex), -126).astype(np.int64)
    e = np.clip(e, -126, 126)
    occ3 = occ[:, None, :]
    while True:  # every occupied slot's hi must fit QMAX cells (ceil may need one more)
        sc = np.ldexp(1.0, e)[:, :, None]
        with np.errstate(all="ignore"):
            over = np.any(occ3 & (np.ceil((shi - o[:, :, None]) / sc) > QMAX), axis=2)
        bump = over & (e < 126)
        if not bump.any():
            break
        e = e + bump
    eb = (e + 127).astype(np.int64)
    sc = np.ldexp(1.0, eb - 127)[:, :, None]
    o3 = o[:, :, None]
    with np.errstate(all="ignore"):
        ql = np.clip(np.floor((slo - o3) / sc), 0, QMAX)
        qh = np.clip(np.ceil((shi - o3) / sc), 0, QMAX)
        ql = np.where(occ3, ql, 0).astype(np.int64)
        qh = np.where(occ3, qh, 0).astype(np.int64)
        while True:
            dec = (ql > 0) & (o3 + ql * sc > slo)
            if not dec.any():
                break
            ql = ql - dec
        while True:
            inc = occ3 & (qh < QMAX) & (o3 + qh * sc < shi)
            if not inc.any():
                break
            qh = qh + inc
    return eb, ql, qh


def quantise_on_grid(origin, eb, lo, hi):
    """The tightest conservative planes of boxes lo, hi ([n, 3]) on given grids (origin [n, 3] float32, eb [n, 3]): the floor / ceil
    rule of vkrt_wnode_quantise without choosing the grid.  Returns qlo, qhi [n, 3] int64."""
    o = np.asarray(origin, F32).astype(np.float64)
    sc = np.ldexp(1.0, np.asarray(eb, np.int64) - 127)
    lo = np.asarray(lo, np.float64)  # (float32 boxes, or decoded ones: exact in double)
    hi = np.asarray(hi, np.float64)
    with np.errstate(all="ignore"):
        ql = np.clip(np.floor((lo - o) / sc), 0, QMAX).astype(np.int64)
        qh = np.clip(np.ceil((hi - o) / sc), 0, QMAX).astype(np.int64)
        while True:
            dec = (ql > 0) & (o + ql * sc > lo)
            if not dec.any():
                break
            ql = ql - dec
        while True:
            inc = (qh < QMAX) & (o + qh * sc < hi)
            if not inc.any():
                break
            qh = qh + inc
    return ql, qh


def store_planes(qlo, qhi):
    """vkrt_wnode_store_planes: [n, 3, 8] planes -> words 8..19, [n, 12] uint32."""
    q = np.concatenate([qlo, qhi], axis=1).astype(np.uint32)  # [n, 6, 8]
    q = q.reshape(-1, 6, 2, 4)
    w = q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | (q[..., 3] << 24)
    return w.reshape(-1, 12).astype(np.uint32)


# ---- wide8 node words (bvh_host.h) -------------------------------------------------------------------------------------------------

def decode_wide8(nodes):
    """Fields of [N, 20] uint32 wide8 nodes: origin [N, 3] float32, eb [N, 3], imask, childBase, triBase [N], meta [N, 8], qlo, qhi [N, 3, 8]."""
    n = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 20)
    origin = n[:, 0:3].view(F32)
    eb = np.stack([(n[:, 3] >> (8 * k)) & 255 for k in range(3)], 1).astype(np.int64)
    imask = (n[:, 3] >> 24).astype(np.int64)
    meta = np.stack([(n[:, 6 + (s >> 2)] >> (8 * (s & 3))) & 255 for s in range(8)], 1).astype(np.int64)
    planes = np.stack([np.stack([(n[:, 8 + 2 * p + (s >> 2)] >> (8 * (s & 3))) & 255 for s in range(8)], 1) for p in range(6)], 1).astype(np.int64)
    return {"origin": origin, "eb": eb, "imask": imask, "childBase": n[:, 4].astype(np.int64), "triBase": n[:, 5].astype(np.int64), "meta": meta,
            "qlo": planes[:, 0:3], "qhi": planes[:, 3:6]}


def _popcount(x):
    x = np.asarray(x, np.int64)
    c = np.zeros_like(x)
    for b in range(32):
        c += (x >> b) & 1
    return c


def wide8_levels(d):
    """Node indices level by level from the root (node 0); raises on a node reached twice or out of range."""
    N = d["imask"].shape[0]
    levels = []
    cur = np.array([0], np.int64) if N else np.zeros(0, np.int64)
    seen = np.zeros(N, bool)
    while cur.size:
        assert cur.min() >= 0 and cur.max() < N, "child index outside the node array"
        assert not seen[cur].any() and np.unique(cur).size == cur.size, "node reached twice"
        seen[cur] = True
        levels.append(cur)
        im = d["imask"][cur]
        kids = [d["childBase"][cur] + _popcount(im & ((1 << s) - 1)) for s in range(8)]
        has = [((im >> s) & 1).astype(bool) for s in range(8)]
        cur = np.concatenate([k[h] for k, h in zip(kids, has)])
    return levels


def _leaf_slots(d, idx):
    """Leaf children of nodes idx: (is_leaf [n, 8], count [n, 8], first slot [n, 8])."""
    meta = d["meta"][idx]
    internal = ((d["imask"][idx][:, None] >> np.arange(8)) & 1).astype(bool)
    leaf = (meta != 0) & ~internal
    cnt = np.where(leaf, _popcount(meta >> 5), 0)
    first = d["triBase"][idx][:, None] + (meta & 31)
    return leaf, cnt, first


def exact_wide8(nodes, rec_lo, rec_hi):
    """The node words a wide8 tree of this topology holds when every leaf box is the union of its records' boxes (rec_lo / rec_hi [T, 3]
    float32) and every node is quantised by the header's rule.  Returns (expected [N, 20] uint32 -- words 4..7 copied: topology --, per-node
    float box lo / hi [N, 3], per-slot float boxes slo / shi [N, 8, 3], decoded fields)."""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 20)
    d = decode_wide8(nodes)
    N = nodes.shape[0]
    rec_lo = np.asarray(rec_lo, F32)
    rec_hi = np.asarray(rec_hi, F32)
    T = rec_lo.shape[0]
    nlo = np.full((N, 3), np.inf, F32)
    nhi = np.full((N, 3), -np.inf, F32)
    slo = np.full((N, 8, 3), np.inf, F32)
    shi = np.full((N, 8, 3), -np.inf, F32)
    for idx in reversed(wide8_levels(d)):
        im = d["imask"][idx]
        leaf, cnt, first = _leaf_slots(d, idx)
        for s in range(8):
            internal = ((im >> s) & 1).astype(bool)
            child = d["childBase"][idx] + _popcount(im & ((1 << s) - 1))
            lo_s = np.full((idx.size, 3), np.inf, F32)
            hi_s = np.full((idx.size, 3), -np.inf, F32)
            lo_s[internal] = nlo[child[internal]]
            hi_s[internal] = nhi[child[internal]]
            for k in range(3):
                use = leaf[:, s] & (cnt[:, s] > k)
                t = first[use, s] + k
                assert t.size == 0 or t.max() < T, "leaf slot outside the triangle records"
                lo_s[use] = np.minimum(lo_s[use], rec_lo[t])
                hi_s[use] = np.maximum(hi_s[use], rec_hi[t])
            slo[idx, s] = lo_s
            shi[idx, s] = hi_s
        nlo[idx] = slo[idx].min(axis=1)
        nhi[idx] = shi[idx].max(axis=1)
    mask = np.zeros(N, np.int64)
    for s in range(8):
        mask |= (d["meta"][:, s] != 0).astype(np.int64) << s
    eb, qlo, qhi = quantise(nlo, nhi, mask, slo, shi)
    exp = nodes.copy()
    exp[:, 0:3] = nlo.view(np.uint32)
    exp[:, 3] = (eb[:, 0] | (eb[:, 1] << 8) | (eb[:, 2] << 16) | (d["imask"] << 24)).astype(np.uint32)
    exp[:, 8:20] = store_planes(qlo, qhi)
    return exp, nlo, nhi, slo, shi, d


def decoded_wide8_boxes(d):
    """Decoded slot boxes in float64: origin + q * 2^(e - 127), [N, 8, 3] lo / hi (exact in double)."""
    sc = np.ldexp(1.0, d["eb"] - 127)[:, :, None]
    o = d["origin"].astype(np.float64)[:, :, None]
    return (o + d["qlo"] * sc).transpose(0, 2, 1), (o + d["qhi"] * sc).transpose(0, 2, 1)


# ---- BVH2 (device_scene.h) --------------------------------------------------------------------------------------------------------

def decode_bvh2(nodes):
    n = np.ascontiguousarray(nodes, F32).reshape(-1, 16)
    box = np.stack([n[:, 0:6], n[:, 6:12]], 1)  # [N, 2, 6] = (lo, hi) per child
    refs = n[:, 12:14].view(np.int32).astype(np.int64)
    return box, refs


def leaf_code(ref):
    code = (~np.asarray(ref, np.int64)) & 0xFFFFFFFF
    return code >> 3, (code & 7) + 1


def bvh2_levels(refs, root_ref):
    """Internal nodes level by level from root_ref (device arrays hold radix nodes no walk reaches: only the walk counts)."""
    N = refs.shape[0]
    levels = []
    cur = np.array([root_ref], np.int64) if root_ref >= 0 else np.zeros(0, np.int64)
    seen = np.zeros(N, bool)
    while cur.size:
        assert cur.min() >= 0 and cur.max() < N, "child index outside the node array"
        assert not seen[cur].any() and np.unique(cur).size == cur.size, "node reached twice"
        seen[cur] = True
        levels.append(cur)
        r = refs[cur].reshape(-1)
        cur = r[r >= 0]
    return levels


def exact_bvh2(nodes, root_ref, rec_lo, rec_hi):
    """Expected child boxes ([N, 2, 6] float32; NaN for nodes no walk reaches) of a BVH2 of this topology with leaf boxes = unions of their
    records' boxes, and the list of reached levels."""
    box, refs = decode_bvh2(nodes)
    N = box.shape[0]
    rec_lo = np.asarray(rec_lo, F32)
    rec_hi = np.asarray(rec_hi, F32)
    T = rec_lo.shape[0]
    exp = np.full((N, 2, 6), np.nan, F32)
    levels = bvh2_levels(refs, root_ref)
    for idx in reversed(levels):
        for c in range(2):
            r = refs[idx, c]
            lo = np.full((idx.size, 3), np.inf, F32)
            hi = np.full((idx.size, 3), -np.inf, F32)
            internal = r >= 0
            ch = r[internal]
            lo[internal] = np.minimum(exp[ch, 0, 0:3], exp[ch, 1, 0:3])
            hi[internal] = np.maximum(exp[ch, 0, 3:6], exp[ch, 1, 3:6])
            first, cnt = leaf_code(r)
            for k in range(8):
                use = (~internal) & (cnt > k)
                t = first[use] + k
                assert t.size == 0 or t.max() < T, "leaf slot outside the triangle records"
                lo[use] = np.minimum(lo[use], rec_lo[t])
                hi[use] = np.maximum(hi[use], rec_hi[t])
            exp[idx, c, 0:3] = lo
            exp[idx, c, 3:6] = hi
    return exp, levels


# ---- SAH cost (include/vkrt.h sah_cost) --------------------------------------------------------------------------------------------

def area64(lo, hi):
    d = np.asarray(hi, np.float64) - np.asarray(lo, np.float64)
    return 2.0 * (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])


def sah_wide8(nodes, slo, shi, levels=None, root_area=None):
    """[sum over reached nodes of A(node) + sum over leaf children of A(child) x count] / A(root) in float64, from per-slot boxes slo / shi
    [N, 8, 3] (float or decoded); a node's box is the union of its occupied slots."""
    d = decode_wide8(nodes)
    if levels is None:
        levels = wide8_levels(d)
    if not levels:
        return 0.0
    reached = np.concatenate(levels)
    occ = d["meta"][reached] != 0
    lo = np.where(occ[:, :, None], slo[reached], np.inf).min(axis=1)
    hi = np.where(occ[:, :, None], shi[reached], -np.inf).max(axis=1)
    leaf, cnt, _ = _leaf_slots(d, reached)
    with np.errstate(invalid="ignore"):
        leaf_area = np.where(leaf, area64(slo[reached], shi[reached]), 0.0)  # (empty slots may hold infinite boxes)
    total = area64(lo, hi).sum() + (leaf_area * cnt).sum()
    ra = area64(lo[0], hi[0]) if root_area is None else root_area
    return float(total / ra) if ra > 0 else 0.0


def sah_bvh2(nodes, root_ref, box=None, levels=None):
    """The same for a BVH2 from its child boxes (box [N, 2, 6], default: the stored ones).  A root leaf costs its count."""
    b, refs = decode_bvh2(nodes)
    if box is None:
        box = b
    if root_ref < 0:
        return float(leaf_code(root_ref)[1]) if root_ref != TRAV_DONE else 0.0
    if levels is None:
        levels = bvh2_levels(refs, root_ref)
    reached = np.concatenate(levels)
    bx = box[reached].astype(np.float64)
    lo = np.minimum(bx[:, 0, 0:3], bx[:, 1, 0:3])
    hi = np.maximum(bx[:, 0, 3:6], bx[:, 1, 3:6])
    total = area64(lo, hi).sum()
    for c in range(2):
        r = refs[reached, c]
        _, cnt = leaf_code(r)
        total += (area64(bx[:, c, 0:3], bx[:, c, 3:6]) * np.where(r < 0, cnt, 0)).sum()
    ra = area64(lo[0], hi[0])
    return float(total / ra) if ra > 0 else 0.0


# ---- which reference sits in which slot (pre-split trees) -----------------------------------------------------------------------------

def slot_references(a, ids, ref_tri, ref_lo, ref_hi, scene_lo, scene_hi):
    """The reference (row of vkrt_debug_split_references) in every slot of a device-built tree `a` (read_accel) whose slots hold the
    triangles `ids` (read_triangle_ids).  BVH2: the slots are the leaves in order, the stable sort of the references' Morton keys inside
    the scene bounds of the whole triangles -- restated and held to ids.  wide8: the collapse renumbers the slots, and the slots of one
    triangle carry the same record; a piece goes to a slot of its triangle whose leaf child's decoded box contains the piece's box (a
    perfect matching per triangle, tightest leaf boxes first).  The assignment is a witness only: the caller proves the tree's words
    exact under it."""
    import np_bvh_build as nb

    ids = np.asarray(ids, np.int64)
    ref_tri = np.asarray(ref_tri, np.int64)
    R = ref_tri.size
    assert ids.size == R, f"{ids.size} slots for {R} references"
    assert np.array_equal(np.sort(ids), np.sort(ref_tri)), "the slots do not hold the references' triangles (as multisets)"
    if a["layout"] != 1:
        order = nb.sorted_order(nb.morton_keys(ref_lo, ref_hi, scene_lo, scene_hi))
        bad = np.flatnonzero(ref_tri[order] != ids)
        assert bad.size == 0, f"{bad.size} of {R} slots differ from the stable Morton sort of the references, first slot {int(bad[0]) if bad.size else -1}"
        return order
    d = decode_wide8(a["nodes"])
    dlo, dhi = decoded_wide8_boxes(d)
    N = d["imask"].shape[0]
    leaf, cnt, first = _leaf_slots(d, np.arange(N))
    slot_lo = np.full((R, 3), np.inf)
    slot_hi = np.full((R, 3), -np.inf)
    for s in range(8):
        for k in range(3):
            use = leaf[:, s] & (cnt[:, s] > k)
            slot_lo[first[use, s] + k] = dlo[use, s]
            slot_hi[first[use, s] + k] = dhi[use, s]
    out = np.full(R, -1, np.int64)
    refs_of = np.argsort(ref_tri, kind="stable")   # references grouped by triangle
    slots_of = np.argsort(ids, kind="stable")      # slots grouped by triangle: the same group sizes
    count = np.bincount(ref_tri)
    start = np.concatenate([[0], np.cumsum(count)])
    single = np.flatnonzero(count == 1)
    out[slots_of[start[single]]] = refs_of[start[single]]
    rl, rh = np.asarray(ref_lo, np.float64), np.asarray(ref_hi, np.float64)
    for g in np.flatnonzero(count > 1):
        rr, ss = refs_of[start[g]:start[g + 1]], slots_of[start[g]:start[g + 1]]
        fits = np.all(rl[rr][:, None] >= slot_lo[ss][None], axis=2) & np.all(rh[rr][:, None] <= slot_hi[ss][None], axis=2)  # [ref, slot]
        tight = np.argsort(np.prod(slot_hi[ss] - slot_lo[ss] + 1e-300, axis=1), kind="stable")
        owner = {}  # slot -> ref (Kuhn's augmenting paths)

        def place(i, seen):
            for j in tight:
                if fits[i, j] and j not in seen:
                    seen.add(j)
                    if j not in owner or place(owner[j], seen):
                        owner[j] = i
                        return True
            return False

        for i in np.argsort(fits.sum(axis=1), kind="stable"):  # the pieces with the fewest candidates first
            assert place(int(i), set()), f"triangle {int(g)}: no slot's leaf box contains piece {int(i)} of {rr.size}"
        for j, i in owner.items():
            out[ss[j]] = rr[i]
    assert np.array_equal(np.sort(out), np.arange(R))
    return out
