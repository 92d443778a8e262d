"""Seeded vertex deformations shared by the vertex-update tests (test_gpu_vertex_update.py) and the probe: a twist about y, a travelling
sine displacement, a collapse to one point -- each returns a deformed copy of the FlatScene (what a fresh scene is created from) whose
changed vertex ranges are then sent through Renderer.update_vertices.  Normals are recomputed from the deformed triangles and tangents
re-orthogonalised against them; both sides of a comparison read the same arrays, so only determinism matters here, not the shading
model."""
import copy
import hashlib

import numpy as np

ATTRS = ("positions", "normals", "tangents", "texcoords0")


def mesh_range(flat, m):
    """(first, count): the absolute vertex range of primitive-mesh m"""
    pm = flat.prim_meshes[m]
    return int(pm["vertexOffset"]), int(pm["vertexCount"])


def with_arrays(flat, **arrays):
    """A copy of `flat` with the given vertex arrays replaced (the others shared)."""
    out = copy.copy(flat)
    for k, a in arrays.items():
        assert k in ATTRS, k
        setattr(out, k, np.ascontiguousarray(a, np.float32))
    return out


def _unit(v):
    n = np.linalg.norm(v, axis=1, keepdims=True)
    return np.where(n > 1e-20, v / np.maximum(n, 1e-20), np.array([0.0, 1.0, 0.0]))


def recompute_shading(flat, pos, meshes):
    """Area-weighted vertex normals of the deformed triangles of `meshes` and tangents made orthogonal to them (w kept): float32 arrays
    for the whole scene, changed only inside the meshes' ranges."""
    nrm = flat.normals.astype(np.float64).copy()
    tan = flat.tangents.astype(np.float64).copy()
    for m in meshes:
        pm = flat.prim_meshes[m]
        first, count = mesh_range(flat, m)
        idx = flat.indices[int(pm["firstIndex"]): int(pm["firstIndex"]) + int(pm["indexCount"]) // 3 * 3].astype(np.int64).reshape(-1, 3)
        p = pos[first:first + count].astype(np.float64)
        fn = np.cross(p[idx[:, 1]] - p[idx[:, 0]], p[idx[:, 2]] - p[idx[:, 0]])
        acc = np.zeros((count, 3))
        for k in range(3):
            np.add.at(acc, idx[:, k], fn)
        n = _unit(acc)
        t = tan[first:first + count, :3]
        t = _unit(t - n * (n * t).sum(1, keepdims=True))
        nrm[first:first + count] = n
        tan[first:first + count, :3] = t
    return nrm.astype(np.float32), tan.astype(np.float32)


def twisted(flat, meshes, turns_per_unit=0.35):
    """`meshes` twisted about the vertical axis through their own centre, the angle growing with height; normals and tangents follow."""
    pos = flat.positions.astype(np.float64).copy()
    for m in meshes:
        first, count = mesh_range(flat, m)
        p = pos[first:first + count]
        c = 0.5 * (p.min(0) + p.max(0))
        a = turns_per_unit * (p[:, 1] - p[:, 1].min())
        x, z = p[:, 0] - c[0], p[:, 2] - c[2]
        p[:, 0] = c[0] + np.cos(a) * x + np.sin(a) * z
        p[:, 2] = c[2] - np.sin(a) * x + np.cos(a) * z
    pos = pos.astype(np.float32)
    nrm, tan = recompute_shading(flat, pos, meshes)
    return with_arrays(flat, positions=pos, normals=nrm, tangents=tan)


def sine(flat, meshes, phase=0.0, amplitude=0.12, wavelength=1.3, base=None):
    """A travelling sine displacement of `meshes` along their rest normals (base = the undeformed scene, default `flat`): object-space
    amplitude x sin(2 pi (x + y + z) / wavelength + phase)."""
    base = base or flat
    pos = flat.positions.astype(np.float64).copy()
    for m in meshes:
        first, count = mesh_range(base, m)
        p0 = base.positions[first:first + count].astype(np.float64)
        n0 = base.normals[first:first + count].astype(np.float64)
        pos[first:first + count] = p0 + n0 * (amplitude * np.sin(2 * np.pi * p0.sum(1) / wavelength + phase))[:, None]
    pos = pos.astype(np.float32)
    nrm, tan = recompute_shading(base, pos, meshes)
    return with_arrays(flat, positions=pos, normals=nrm, tangents=tan)


def collapsed(flat, m):
    """Every vertex of mesh m at the mesh's first vertex: zero-area triangles."""
    pos = flat.positions.copy()
    first, count = mesh_range(flat, m)
    pos[first:first + count] = pos[first]
    return with_arrays(flat, positions=pos)


def third_of_meshes(flat, seed=23):
    """A third of the primitive-meshes, with the most-instanced one (a column or an arch in the atrium) among them."""
    n = len(flat.prim_meshes)
    uses = np.bincount(flat.nodes["primMesh"], minlength=n)
    pick = set(np.random.default_rng(seed).choice(n, max(1, n // 3), replace=False).tolist())
    pick.add(int(np.argmax(uses)))
    return sorted(pick)


def send(r, flat, meshes=None, ranges=None, attrs=ATTRS, device=None, stream=None):
    """The vertex ranges of `meshes` (or explicit (first, count) `ranges`) of `flat` through Renderer.update_vertices: numpy arrays (the
    host path) or, with device = a torch device, tensors there (the device path).  Returns the tensors it made (keep them alive until
    the stream has passed the calls)."""
    ranges = list(ranges) if ranges is not None else [mesh_range(flat, m) for m in meshes]
    keep = []
    for first, count in ranges:
        kw = {}
        for k in attrs:
            a = np.ascontiguousarray(getattr(flat, k)[first:first + count])
            if device is not None:
                import torch

                a = torch.as_tensor(a).to(device, non_blocking=False)
                keep.append(a)
            kw[k] = a
        r.update_vertices(first, stream=stream, **kw)
    return keep


# ---- what the comparisons of test_gpu_refit.py use, for the tests of deformation -------------------------------------------------
def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t).tobytes()).hexdigest()[:16]


def random_rays(flat, n=60000, seed=5):
    rng = np.random.default_rng(seed)
    lo, hi = flat.positions.min(0), flat.positions.max(0)
    o = rng.uniform(lo - 0.5, hi + 0.5, (n, 3)).astype(np.float32)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d


def assert_sound(chk, node_count):
    assert chk["triangles_missing"] == 0 and chk["triangles_repeated"] == 0 and chk["box_violations"] == 0 and chk["bad_references"] == 0, chk
    assert chk["triangles_uncovered"] == 0, chk
    assert chk["nodes_reached"] == node_count, chk


def assert_same_trace(a, b):
    ta, ua, va, ga = a
    tb, ub, vb, gb = b
    assert np.array_equal(ga, gb)
    for x, y in ((ta, tb), (ua, ub), (va, vb)):
        assert np.array_equal(x[ga >= 0].view(np.uint32), y[gb >= 0].view(np.uint32))


def accel_bytes(r):
    """(layout, root, node bytes, record bytes) of the installed tree as read_accel() returns it.  BVH2: the nodes a walk from the root
    reaches, in index order -- a device-built BVH2 array also holds radix nodes inside collapsed leaves that nothing reads and no build
    or refit defines (include/vkrt.h, vkrt_debug_read_accel), which is how test_gpu_bvh_bounds.py compares two builds."""
    import np_bvh

    a = r.read_accel()
    nodes = a["nodes"]
    if a["layout"] == 0:
        _, refs = np_bvh.decode_bvh2(nodes)
        levels = np_bvh.bvh2_levels(refs, a["root_ref"])
        nodes = nodes[np.sort(np.concatenate(levels))] if levels else nodes[:0]
    return a["layout"], a["root_ref"], nodes.tobytes(), a["tris"].tobytes()
