"""Closest-point queries (vkrt_closest_point, Renderer.closest_point): per query the nearest point of the scene's surface within a radius.

The result is defined by include/vkrt.h -- Ericson's point/triangle function in binary64 on the binary32 values of the triangle records,
the smallest key (dist2, flattened triangle id) over the candidates with dist2 < radius^2 -- so every check is exact: the reference below
is a numpy restatement of that rule, run as brute force over the records read_accel() returns, and whole result buffers are compared bit
for bit.  Scenes and builder kinds are those of test_gpu_ray_query.py."""
import ctypes as C
import hashlib
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import test_gpu_ray_query as Q
from scene_motion import apply, moved

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KINDS = Q.KINDS
scenes = Q.scenes  # (the module fixture: Cornell, the small atrium, the triangle soup)
N = 4001           # queries per case: 62 full waves and one lane


# ---- the reference: the rule of include/vkrt.h in numpy binary64 ----------------------------------------------------------------------
def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _point_triangle(q, p0, e1, e2):
    """q: float64 [Q, 1, 3]; p0, e1, e2: float64 [1, T, 3] (binary32 values) -> (u, v, dist2) float64 [Q, T]"""
    with np.errstate(all="ignore"):
        apx, apy, apz = (q[..., k] - p0[..., k] for k in range(3))
        ax, ay, az = (e1[..., k] for k in range(3))
        bx, by, bz = (e2[..., k] for k in range(3))
        d1, d2 = _dot(ax, ay, az, apx, apy, apz), _dot(bx, by, bz, apx, apy, apz)
        bpx, bpy, bpz = apx - ax, apy - ay, apz - az
        d3, d4 = _dot(ax, ay, az, bpx, bpy, bpz), _dot(bx, by, bz, bpx, bpy, bpz)
        cpx, cpy, cpz = apx - bx, apy - by, apz - bz
        d5, d6 = _dot(ax, ay, az, cpx, cpy, cpz), _dot(bx, by, bz, cpx, cpy, cpz)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        den = 1.0 / ((va + vb) + vc)
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        rows = [((d1 <= 0) & (d2 <= 0), 0.0, 0.0),
                ((d3 >= 0) & (d4 <= d3), 1.0, 0.0),
                ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1 / (d1 - d3), 0.0),
                ((d6 >= 0) & (d5 <= d6), 0.0, 1.0),
                ((vb <= 0) & (d2 >= 0) & (d6 <= 0), 0.0, d2 / (d2 - d6)),
                ((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), 1.0 - w, w)]
        u, v = vb * den, vc * den
        for cond, ru, rv in reversed(rows):  # (the first row that holds wins)
            u, v = np.where(cond, ru, u), np.where(cond, rv, v)
        dx, dy, dz = (apx - u * ax) - v * bx, (apy - u * ay) - v * by, (apz - u * az) - v * bz
        return u, v, _dot(dx, dy, dz, dx, dy, dz)


def _records(r, watertight=False):
    """(p0, e1, e2 float32 [T, 3], gid, instance int32 [T]) of the installed tree's records, in slot order"""
    tris = r.read_accel()["tris"]
    ints = tris.view(np.int32)
    p0, e1, e2 = tris[:, 0:3].copy(), tris[:, 3:6].copy(), tris[:, 6:9].copy()
    if watertight:  # the record holds (p0, p1, p2): the edges are formed in binary32
        e1, e2 = e1 - p0, e2 - p0
    return p0, e1, e2, (ints[:, 9] & 0x7FFFFFFF).copy(), ints[:, 10].copy()


def _brute(points, rec, keep=None, pairs=1 << 20):
    """Per point the smallest key (dist2, gid) over the records (those of `keep`, a bool per record): (dist2 float64, gid int32, u, v
    float64); (inf, -1, 0, 0) where no record has a comparable dist2.  Chunked over the points, chunks on a few threads."""
    p0, e1, e2, gid, _ = rec
    if keep is not None:
        p0, e1, e2, gid = p0[keep], e1[keep], e2[keep], gid[keep]
    n, T = len(points), len(gid)
    D, G, U, V = np.full(n, np.inf), np.full(n, -1, np.int32), np.zeros(n), np.zeros(n)
    if T == 0 or n == 0:
        return D, G, U, V
    P0, E1, E2 = (a.astype(np.float64)[None] for a in (p0, e1, e2))
    step = max(1, pairs // T)

    def run(lo):
        hi = min(n, lo + step)
        with np.errstate(all="ignore"):
            u, v, d = _point_triangle(points[lo:hi].astype(np.float64)[:, None, :], P0, E1, E2)
        d = np.where(np.isnan(d), np.inf, d)
        m = d.min(1)
        g = np.where(d == m[:, None], gid[None, :], np.iinfo(np.int32).max).min(1)
        j = np.argmax((d == m[:, None]) & (gid[None, :] == g[:, None]), 1)
        rows = np.arange(hi - lo)
        ok = np.isfinite(m)
        D[lo:hi] = m
        G[lo:hi] = np.where(ok, g, -1)
        U[lo:hi] = np.where(ok, u[rows, j], 0.0)
        V[lo:hi] = np.where(ok, v[rows, j], 0.0)

    with ThreadPoolExecutor(8) as ex:
        list(ex.map(run, range(0, n, step)))
    return D, G, U, V


def _merge(a, b):
    """the smaller key of two brute-force results, per point"""
    take = (b[0] < a[0]) | ((b[0] == a[0]) & (b[1] >= 0) & ((a[1] < 0) | (b[1] < a[1])))
    return tuple(np.where(take, y, x) for x, y in zip(a, b))


def _expected(points, radius, best, table, cull=0xFF):
    """the uint32 [N, 8] buffer the call must write: `best` = the brute-force keys over the triangles the cull mask admits"""
    D, G, U, V = best
    r = np.asarray(radius, np.float32)
    with np.errstate(all="ignore"):
        valid = np.isfinite(points).all(1) & (r > 0) & (cull != 0)
        hit = valid & (G >= 0) & (D < r.astype(np.float64) * r.astype(np.float64))
        t = np.sqrt(D.astype(np.float32))
    out = np.zeros((len(points), 8), np.uint32)
    out[:, 0] = np.where(hit, t, r).astype(np.float32).view(np.uint32)
    out[~hit, 0] = r.view(np.uint32)[~hit]  # (the radius as given: a NaN keeps its bits)
    out[:, 1] = np.where(hit, U.astype(np.float32), np.float32(0)).astype(np.float32).view(np.uint32)
    out[:, 2] = np.where(hit, V.astype(np.float32), np.float32(0)).astype(np.float32).view(np.uint32)
    g = np.where(hit, G, 0)
    ints = np.stack([table[g, 0], table[g, 1], table[g, 2], g, table[g, 3]], 1).astype(np.int32)
    ints[~hit] = -1
    out[:, 3:] = ints.view(np.uint32)
    return out, hit


# ---- hostile queries ------------------------------------------------------------------------------------------------------------------
def _hostile_points(rec, n, seed):
    """float32 [n, 3]: uniform in the padded bounds; exactly on vertices; on edges; at random barycentrics; in the planes of the bounds and
    at their corners and centre (axis-aligned walls: equidistant triangles); at centroids offset along the normal by 1e-6 and by 1e3; far
    outside; a few with a NaN or infinite component."""
    rng = np.random.default_rng(seed)
    p0, e1, e2 = (a.astype(np.float64) for a in rec[:3])
    verts = np.concatenate([p0, p0 + e1, p0 + e2])
    verts = verts[np.isfinite(verts).all(1)]
    lo, hi = verts.min(0), verts.max(0)
    ext = hi - lo
    kind = rng.choice(9, n, p=[0.30, 0.08, 0.08, 0.15, 0.08, 0.10, 0.05, 0.05, 0.11])
    k = rng.integers(0, len(p0), n)
    pts = rng.uniform(lo - 0.1 * ext - 0.1, hi + 0.1 * ext + 0.1, (n, 3))
    m = kind == 1
    which = rng.integers(0, 3, n)
    pts[m] = np.where(which[m, None] == 0, p0[k[m]], np.where(which[m, None] == 1, (rec[0] + rec[1])[k[m]], (rec[0] + rec[2])[k[m]]))
    m = kind == 2
    s = rng.random((n, 1))
    pts[m] = np.where(which[m, None] == 0, p0[k[m]] + s[m] * e1[k[m]],
                      np.where(which[m, None] == 1, p0[k[m]] + s[m] * e2[k[m]], p0[k[m]] + e1[k[m]] + s[m] * (e2[k[m]] - e1[k[m]])))
    m = kind == 3
    w = rng.dirichlet((1, 1, 1), n)
    pts[m] = p0[k[m]] + w[m, 1:2] * e1[k[m]] + w[m, 2:3] * e2[k[m]]
    m = kind == 4  # in a plane of the bounds (half of them on a grid of exact binary fractions), or at a corner / the centre
    ax = rng.integers(0, 3, n)
    side = rng.integers(0, 2, n)
    grid = lo + ext * (rng.integers(0, 9, (n, 3)) / 8.0)
    pts[m] = np.where((rng.random(n) < 0.5)[m, None], grid[m], pts[m])
    for a in range(3):
        mm = m & (ax == a)
        pts[mm, a] = np.where(side[mm] == 0, lo[a], hi[a])
    corner = m & (rng.random(n) < 0.3)
    pts[corner] = np.where(rng.integers(0, 2, (n, 3))[corner] == 0, lo, hi)
    pts[m & (rng.random(n) < 0.05)] = 0.5 * (lo + hi)
    nrm = np.cross(e1, e2)
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), np.array([0.0, 1.0, 0.0]))
    cen = p0 + (e1 + e2) / 3.0
    sign = np.where(rng.random((n, 1)) < 0.5, 1.0, -1.0)
    m = kind == 5
    pts[m] = cen[k[m]] + sign[m] * 1e-6 * nrm[k[m]]
    m = kind == 6
    pts[m] = cen[k[m]] + sign[m] * 1e3 * nrm[k[m]]
    m = kind == 7
    d = rng.normal(size=(n, 3))
    pts[m] = 0.5 * (lo + hi) + d[m] / np.linalg.norm(d[m], axis=1, keepdims=True) * 100.0 * np.linalg.norm(ext)
    pts = pts.astype(np.float32)
    bad = rng.random(n) < 0.01
    pts[bad, rng.integers(0, 3, bad.sum())] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), bad.sum())
    return pts


def _radius_mix(best, n, seed):
    """inf; the 30th percentile of the true distances; 0; negative; NaN; the t of the true answer (a miss: the comparison is strict) and the
    binary32 above it; twice the true distance"""
    rng = np.random.default_rng(seed)
    D = best[0]
    with np.errstate(all="ignore"):
        t = np.sqrt(D.astype(np.float32))
    fin = np.isfinite(t)
    p30 = np.float32(np.percentile(t[fin], 30)) if fin.any() else np.float32(1.0)
    kind = rng.choice(8, n, p=[0.40, 0.20, 0.04, 0.03, 0.03, 0.10, 0.08, 0.12])
    r = np.full(n, np.inf, np.float32)
    r[kind == 1] = p30
    r[kind == 2] = rng.choice(np.array([0.0, -0.0], np.float32), (kind == 2).sum())
    r[kind == 3] = -rng.uniform(0.1, 5.0, (kind == 3).sum()).astype(np.float32)
    r[np.nonzero(kind == 3)[0][::4]] = -np.inf
    r[kind == 4] = np.nan
    m = (kind == 5) & fin
    r[m] = t[m]
    m = (kind == 6) & fin
    r[m] = np.nextafter(t[m], np.float32(np.inf))
    m = (kind == 7) & fin
    r[m] = 2.0 * t[m]
    return r


def _query(r, points, radius, **kw):
    """uint32 [N, 8]: the buffer of one call"""
    import torch

    q = torch.as_tensor(np.concatenate([points, np.asarray(radius, np.float32).reshape(-1, 1)], 1), device="cuda:0")
    h = r.closest_point(q, **kw)
    torch.cuda.current_stream().synchronize()
    assert tuple(h.buffer.shape) == (len(points), 8)
    return h.buffer.cpu().numpy().view(np.uint32).copy()


def _assert_equal(got, want, what):
    bad = np.nonzero((got != want).any(1))[0]
    if len(bad):
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ; first {i}: got t={got[i, 0:1].view(np.float32)[0]!r} "
                             f"{got[i].tolist()} want t={want[i, 0:1].view(np.float32)[0]!r} {want[i].tolist()}")


def _only_faults_may_move(r):
    c = r.counters()
    assert c["traversal_faults"] == 0
    assert all(c[k] == 0 for k in ("rays_closest", "rays_shadow", "hits", "pixels", "nodes_visited", "tris_tested")), c


@pytest.fixture(scope="module")
def cases(scenes):
    """Per scene, computed once and left unchanged: the hostile queries, their radii, the brute-force keys per instance-mask class
    (instance i has class i % 3; Cornell and the soup are used with one class only) and the expected buffer of the default call."""
    out = {}

    def get(name):
        if name not in out:
            flat, _ = scenes[name]
            r = Q._renderer(flat, "sah", 1)
            rec = _records(r)
            r.close()
            pts = _hostile_points(rec, N, seed={"cornell": 101, "soup": 102, "atrium_small": 103}[name])
            classes = 3 if name == "atrium_small" else 1
            per = [_brute(pts, rec, keep=None if classes == 1 else rec[4] % 3 == c) for c in range(classes)]
            best = per[0]
            for b in per[1:]:
                best = _merge(best, b)
            radius = _radius_mix(best, N, seed=7)
            table = Q._flattened(flat)
            want, hit = _expected(pts, radius, best, table)
            out[name] = {"flat": flat, "points": pts, "radius": radius, "per_class": per, "best": best, "table": table, "want": want, "hit": hit}
        return out[name]

    return get


# ---- 1. exact against brute force -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("kind", KINDS)
def test_results_equal_the_brute_force_bit_for_bit(cases, kind, layout):
    from vkrt_amd import abi

    for name in ("cornell", "soup", "atrium_small"):
        c = cases(name)
        assert c["hit"].mean() > 0.5 and (~c["hit"]).mean() > 0.05, c["hit"].mean()  # (neither branch is vacuous)
        variants = [({}, "default"), ({abi.VKRT_OPT_WATERTIGHT: 1}, "watertight")]
        if name != "cornell":
            variants.append(({abi.VKRT_OPT_SPLIT_BUDGET: 30}, "split 30"))
        for options, label in variants:
            r = Q._renderer(c["flat"], kind, layout, {abi.VKRT_OPT_SPLIT_BUDGET: 0, **options})
            r.reset_counters()
            got = _query(r, c["points"], c["radius"])
            _assert_equal(got, c["want"], f"{name} {kind} layout {layout} {label}")
            _only_faults_may_move(r)
            r.close()


def test_watertight_records_give_the_same_reference(cases, scenes):
    """the rule on the records of a watertight build -- (p0, p1, p2), edges formed in binary32 -- is the rule on the default records"""
    from vkrt_amd import abi

    c = cases("soup")
    r = Q._renderer(c["flat"], "sah", 1, {abi.VKRT_OPT_WATERTIGHT: 1})
    rec = _records(r, watertight=True)
    r.close()
    best = _brute(c["points"][:600], rec)
    for a, b in zip(best, c["best"]):
        assert np.array_equal(a, b[:600])


# ---- 2. byte-identical buffers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "atrium_small", "nonuniform"])
def test_buffers_are_identical_across_builders_layouts_and_split_budgets(scenes, name):
    """"nonuniform": the atrium tessellated like an artist-made scene (room-sized triangles, needles): the scene pre-splitting acts on, so
    its trees hold several references to one record -- which must change nothing.  Its answers are also checked against the brute force."""
    from vkrt_amd import abi

    if name == "nonuniform":
        import atrium

        flat, _ = atrium.build_atrium(20000, seed=3, with_textures=False, variant="nonuniform")
        atrium.rotate_scene(flat, dict(atrium.DEFAULT_CAMERA), 35.0, 20.0)
    else:
        flat, _ = scenes[name]
    r = Q._renderer(flat, "sah", 1, {abi.VKRT_OPT_SPLIT_BUDGET: 0})
    rec = _records(r)
    r.close()
    n = 8001
    pts = _hostile_points(rec, n, seed=211)
    radius = np.where(np.random.default_rng(3).random(n) < 0.5, np.float32(np.inf), np.float32(0.05 if name == "soup" else 0.5)).astype(np.float32)
    digests, split, first = {}, {}, None
    for kind in KINDS:
        for layout in (1, 0):
            for budget in (0, 30):
                r = Q._renderer(flat, kind, layout, {abi.VKRT_OPT_SPLIT_BUDGET: budget})
                info = r.accel_info()
                split[(kind, layout, budget)] = info["reference_count"] > info["triangle_count"]
                buf = _query(r, pts, radius)
                digests[(kind, layout, budget)] = hashlib.sha256(buf.tobytes()).hexdigest()
                first = buf if first is None else first
                assert r.counters()["traversal_faults"] == 0
                r.close()
    assert len(set(digests.values())) == 1, digests
    assert not any(v for k, v in split.items() if k[2] == 0), split
    assert 0.3 < (first[:, 6].view(np.int32) >= 0).mean() < 0.99
    if name == "nonuniform":
        assert all(split[(kind, layout, 30)] for kind in ("ploc", "lbvh") for layout in (1, 0)), split
        m = 1001
        want, hit = _expected(pts[:m], radius[:m], _brute(pts[:m], rec), Q._flattened(flat))
        _assert_equal(first[:m], want, "nonuniform")
        assert 0.3 < hit.mean() < 0.99


# ---- 3. masks -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 0])
def test_cull_masks_equal_the_masked_brute_force(cases, layout):
    c = cases("atrium_small")
    flat = c["flat"]
    r = Q._renderer(flat, "ploc", layout)
    r.reset_counters()
    masks = (np.arange(len(flat.nodes)) % 3 + 1).astype(np.uint8)
    r.set_instance_visibility(0, masks, np.zeros(len(masks), np.uint8))
    inf = np.full(N, np.inf, np.float32)
    for cull in (0x1, 0x2, 0x3):
        admitted = [k for k in range(3) if (k + 1) & cull]  # class k = instances with mask k + 1
        best = c["per_class"][admitted[0]]
        for k in admitted[1:]:
            best = _merge(best, c["per_class"][k])
        for radius in (c["radius"], inf):
            want, hit = _expected(c["points"], radius, best, c["table"], cull)
            _assert_equal(_query(r, c["points"], radius, cull_mask=cull), want, f"cull 0x{cull:x} layout {layout}")
        if cull != 0x3:
            assert np.all((masks[want[hit, 3].view(np.int32)] & cull) != 0)
            assert (want[:, 6] != _expected(c["points"], inf, c["best"], c["table"])[0][:, 6]).mean() > 0.1  # (the mask changes answers)
    none = _query(r, c["points"], c["radius"], cull_mask=0)
    miss = np.zeros((N, 8), np.uint32)
    miss[:, 0] = c["radius"].view(np.uint32)
    miss[:, 3:] = 0xFFFFFFFF
    assert np.array_equal(none, miss)
    # 0xFF through an options struct is the call with opts = NULL
    import torch
    from vkrt_amd import abi

    q = torch.as_tensor(np.concatenate([c["points"], c["radius"].reshape(-1, 1)], 1), device="cuda:0")
    out = torch.zeros((N, 8), dtype=torch.float32, device="cuda:0")
    opts = abi.QueryOpts(16, 0, 0xFF, 12345)  # (anyhit_seed is ignored)
    assert r.lib.vkrt_closest_point(r._h, C.c_void_p(q.data_ptr()), N, C.byref(opts), C.c_void_p(out.data_ptr()), None) == abi.VKRT_OK
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), _query(r, c["points"], c["radius"]))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), c["want"])
    _only_faults_may_move(r)
    r.close()


# ---- 4. motion and deformation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 0])
def test_stale_tree_is_refused_and_a_refit_answers_like_a_fresh_build(scenes, layout):
    import torch
    from scene_deform import send, third_of_meshes, twisted
    from vkrt_amd import abi

    flat, _ = scenes["atrium_small"]
    idx = np.sort(np.random.default_rng(23).choice(len(flat.nodes), len(flat.nodes) // 3, replace=False))
    mv, mats = moved(flat, idx, 23)
    r = Q._renderer(flat, "ploc", layout)
    fresh = Q._renderer(mv, "ploc", layout)
    pts = _hostile_points(_records(fresh), N, seed=307)
    radius = np.where(np.random.default_rng(5).random(N) < 0.6, np.float32(np.inf), np.float32(0.3)).astype(np.float32)
    q = torch.as_tensor(np.concatenate([pts, radius.reshape(-1, 1)], 1), device="cuda:0")
    hits = torch.full((N, 8), 7.0, dtype=torch.float32, device="cuda:0")

    def raw():
        return r.lib.vkrt_closest_point(r._h, C.c_void_p(q.data_ptr()), N, None, C.c_void_p(hits.data_ptr()), None)

    apply(r, mats)
    assert raw() == abi.VKRT_ERR_NOT_BUILT and b"vkrt_scene_update_nodes" in r.lib.vkrt_last_error()
    torch.cuda.synchronize()
    assert bool((hits == 7.0).all())  # (nothing was written)
    r.refit()
    a, b = _query(r, pts, radius), _query(fresh, pts, radius)
    assert np.array_equal(a, b)
    assert 0.5 < (a[:, 6].view(np.int32) >= 0).mean() < 0.99
    fresh.close()
    meshes = third_of_meshes(mv)
    df = twisted(mv, meshes)
    send(r, df, meshes)
    assert raw() == abi.VKRT_ERR_NOT_BUILT
    r.refit()
    fresh = Q._renderer(df, "ploc", layout)
    a2, b2 = _query(r, pts, radius), _query(fresh, pts, radius)
    assert np.array_equal(a2, b2)
    assert (a2 != a).any()  # (the deformation changes answers)
    assert r.counters()["traversal_faults"] == 0
    r.close()
    fresh.close()


# ---- 5. chaining with hit_surface ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "soup", "atrium_small"])
def test_hit_surface_takes_the_records(cases, name):
    """Every hit record is a valid surface record with the right material, and the float64 point recomputed from the flat arrays at
    (instance, primitive, u, v) lies at distance t from the query within 32 x 2^-24 x the largest |coordinate| among the scene's bounds
    and the query: the rounding of the transform and of the edge subtractions.  The soup's needles (smallest corner sine < 1e-2; it
    makes 15 % of them, plus 2 % degenerate) are excluded from the distance check only: their (u, v) of the record's edges do not
    carry over to the float64 edges."""
    import torch

    c = cases(name)
    flat = c["flat"]
    r = Q._renderer(flat, "ploc", 1)
    q = torch.as_tensor(np.concatenate([c["points"], c["radius"].reshape(-1, 1)], 1), device="cuda:0")
    h = r.closest_point(q)
    s = r.surface(h)
    torch.cuda.synchronize()
    buf = h.buffer.cpu().numpy().view(np.uint32)
    _assert_equal(buf, c["want"], name)
    hit = c["hit"]
    valid, mat = s.valid.cpu().numpy(), s.material.cpu().numpy()
    assert np.array_equal(valid == 1, hit)
    assert np.array_equal(mat[hit], c["table"][buf[hit, 6].view(np.int32), 3]) and np.all(mat[~hit] == -1)
    tri = Q._world_triangles(flat)[buf[hit, 6].view(np.int32)]
    u, v, t = (buf[hit, k].view(np.float32).astype(np.float64) for k in (1, 2, 0))
    p = tri[:, 0] + u[:, None] * (tri[:, 1] - tri[:, 0]) + v[:, None] * (tri[:, 2] - tri[:, 0])
    qp = c["points"][hit].astype(np.float64)
    err = np.abs(np.linalg.norm(p - qp, axis=1) - t)
    lo, hi = Q._world_bounds(flat)
    scale = np.maximum(np.abs(qp).max(1), max(np.abs(lo).max(), np.abs(hi).max()))
    e = [tri[:, (k + 1) % 3] - tri[:, k] for k in range(3)]
    sines = []
    for k in range(3):
        a, b = e[k], -e[(k + 2) % 3]
        la, lb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
        with np.errstate(all="ignore"):
            sines.append(np.where((la > 0) & (lb > 0), np.linalg.norm(np.cross(a, b), axis=1) / (la * lb), 0.0))
    needle = (np.min(sines, 0) < 1e-2) & (name == "soup")  # (the other scenes are checked whole)
    assert needle.mean() < 0.20, needle.mean()
    ratio = err[~needle] / (2.0 ** -24 * scale[~needle])
    print(f"{name}: {hit.sum()} hits, {needle.sum()} on needles; |distance - t| / (2^-24 scale): max {ratio.max():.3f}")
    assert ratio.max() <= 32.0, ratio.max()
    pos = s.position.cpu().numpy()[hit].astype(np.float64)  # the library's own binary32 position agrees to the same bound (+ its rounding)
    assert (np.abs(np.linalg.norm(pos - qp, axis=1) - t)[~needle] <= 40.0 * 2.0 ** -24 * scale[~needle]).all()
    r.close()


# ---- 6. the walk prunes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("kind", KINDS)
def test_the_walk_prunes(scenes, kind, layout):
    """a guard against a walk that does not prune (100 %), not a speed target"""
    flat, _ = scenes["atrium_small"]
    r = Q._renderer(flat, kind, layout)
    tri = Q._world_triangles(flat)
    rng = np.random.default_rng(409)
    k = rng.integers(0, len(tri), N)
    w = rng.dirichlet((1, 1, 1), N)
    pts = (tri[k] * w[:, :, None]).sum(1).astype(np.float32)
    nodes, tris = r.closest_point_work(pts, radius=np.inf)
    refs = r.accel_info()["reference_count"]
    print(f"{kind} layout {layout}: {nodes / N:.1f} nodes, {tris / N:.1f} of {refs} triangle records per query")
    assert nodes > 0 and tris >= N  # (every query tests at least the triangle it lies on)
    assert tris / N < 0.05 * refs, (tris / N, refs)
    assert r.closest_point_work(pts, radius=np.inf, cull_mask=0) == (0, 0)
    assert r.counters()["traversal_faults"] == 0
    r.close()


# ---- 7. edge sizes and the arrays' checks -------------------------------------------------------------------------------------------------
def test_edge_sizes_and_array_checks(cases):
    import torch
    from vkrt_amd import abi

    c = cases("cornell")
    r = Q._renderer(c["flat"], "ploc", 1)
    for n in (1, 65):
        _assert_equal(_query(r, c["points"][:n], c["radius"][:n]), c["want"][:n], f"n = {n}")
    # [N, 3] points with a scalar and with a tensor radius; an `out` buffer
    p3 = torch.as_tensor(c["points"][:65], device="cuda:0")
    inf_want = _expected(c["points"][:65], np.full(65, np.inf, np.float32), tuple(x[:65] for x in c["best"]), c["table"])[0]
    out = torch.zeros((65, 8), dtype=torch.int32, device="cuda:0")
    h = r.closest_point(p3, out=out)
    torch.cuda.synchronize()
    assert h.buffer.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy().view(np.uint32), inf_want)
    h = r.closest_point(p3, radius=torch.as_tensor(c["radius"][:65], device="cuda:0"))
    torch.cuda.synchronize()
    assert np.array_equal(h.buffer.cpu().numpy().view(np.uint32), c["want"][:65])
    empty = r.closest_point(torch.empty((0, 4), dtype=torch.float32, device="cuda:0"))
    assert tuple(empty.buffer.shape) == (0, 8)
    lib, hd, E = r.lib, r._h, abi.VKRT_ERR_INVALID_ARGUMENT
    assert lib.vkrt_closest_point(hd, None, 0, None, None, None) == abi.VKRT_OK
    q = torch.zeros((9, 4), dtype=torch.float32, device="cuda:0")
    hits = torch.zeros((9, 8), dtype=torch.float32, device="cuda:0")
    qp, hp = q.data_ptr(), hits.data_ptr()
    for a, b, word in ((None, hp, b"NULL array"), (qp, None, b"NULL array"), (qp + 4, hp, b"misaligned"), (qp, hp + 8, b"misaligned")):
        assert lib.vkrt_closest_point(hd, C.c_void_p(a) if a else None, 2, None, C.c_void_p(b) if b else None, None) == E
        assert word in lib.vkrt_last_error(), lib.vkrt_last_error()
    flags = abi.QueryOpts(16, 0x10, 0xFF, 0)
    assert lib.vkrt_closest_point(hd, C.c_void_p(qp), 2, C.byref(flags), C.c_void_p(hp), None) == E
    r.close()


@pytest.mark.parametrize("layout", [0, 1])
def test_a_scene_of_two_triangles(layout):
    """BVH2: the device builders make the root a leaf"""
    flat = Q._triangle_soup(n=2, seed=5)
    leaf_roots = 0
    for kind in KINDS:
        r = Q._renderer(flat, kind, layout)
        root = r.read_accel()["root_ref"]
        leaf_roots += root < 0 and root != -2 ** 31
        rec = _records(r)
        pts = _hostile_points(rec, 257, seed=11)
        best = _brute(pts, rec)
        radius = _radius_mix(best, 257, seed=13)
        want, hit = _expected(pts, radius, best, Q._flattened(flat))
        _assert_equal(_query(r, pts, radius), want, f"two triangles, {kind}, layout {layout}")
        assert 0.3 < hit.mean() < 0.95
        assert r.counters()["traversal_faults"] == 0
        r.close()
    assert layout == 1 or leaf_roots > 0
