"""Seeded skins shared by the skinning tests (test_np_skin.py, test_gpu_skin.py): for any vertex range of a FlatScene, J joints spread
along the range's y extent, four influences per vertex (the two nearest joints with a linear falloff, two small seeded ones of which
some are exactly 0, rows normalised in float32) and seeded joint matrices (a rotation about z and a translation each; one joint with a
non-uniform scale, one mirrored).  posed() is the scene a fresh Renderer is created from: tests/np_skin.py applied to the ranges."""
import numpy as np

import np_skin
import scene_deform as sd

F = np.float32


def influences(flat, first, count, joint_count, seed):
    """(joints uint16 (count, 4), weights float32 (count, 4)); the highest joint index is used"""
    rng = np.random.default_rng(seed)
    J = int(joint_count)
    y = flat.positions[first:first + count, 1].astype(np.float64)
    ext = y.max() - y.min()
    s = (y - y.min()) / ext * (J - 1) if ext > 0 and J > 1 else np.zeros(count)
    a = np.clip(np.floor(s), 0, max(J - 2, 0)).astype(np.int64)
    b = np.minimum(a + 1, J - 1)
    f = np.clip(s - a, 0.0, 1.0)
    joints = np.stack([a, b, rng.integers(0, J, count), rng.integers(0, J, count)], axis=1)
    small = rng.uniform(0.0, 0.1, (count, 2))
    small[rng.uniform(size=(count, 2)) < 0.4] = 0.0
    joints[0, 2] = J - 1
    w = np.concatenate([np.stack([1.0 - f, f], axis=1), small], axis=1).astype(F)
    w = (w / w.sum(axis=1, keepdims=True, dtype=F)).astype(F)
    assert joints.max() == J - 1 and joints.min() >= 0
    return joints.astype(np.uint16), np.ascontiguousarray(w)


def joint_matrices(joint_count, seed, amount=1.0):
    """(J, 16) float32, column-major like vkrt_node.worldMatrix"""
    rng = np.random.default_rng(seed)
    J = int(joint_count)
    out = np.zeros((J, 4, 4))  # [k, r, c]
    for k in range(J):
        ang = amount * rng.uniform(-0.6, 0.6)
        m = np.eye(4)
        m[0, 0], m[0, 1], m[1, 0], m[1, 1] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)
        m[:3, 3] = amount * rng.uniform(-0.3, 0.3, 3)
        if k == (1 if J >= 3 else 0):
            m[:3, :3] = m[:3, :3] @ np.diag([1.3, 0.7, 1.1])  # non-uniform scale
        if J >= 2 and k == J - 1:
            m[:3, :3] = m[:3, :3] @ np.diag([-1.0, 1.0, 1.0])  # mirrored
        out[k] = m
    return np.ascontiguousarray(out.transpose(0, 2, 1).reshape(J, 16), F)


def make(flat, first, count, joint_count, seed):
    """one skin of a test: dict(first, count, joint_count, joints, weights, matrices)"""
    j, w = influences(flat, first, count, joint_count, seed)
    return dict(first=int(first), count=int(count), joint_count=int(joint_count), joints=j, weights=w, matrices=joint_matrices(joint_count, seed + 1000))


def posed(flat, skins, base=None):
    """A copy of `flat` with every skin's range posed by np_skin from the bind pose in `base` (default `flat`)."""
    base = base or flat
    pos, nrm, tan = flat.positions.copy(), flat.normals.copy(), flat.tangents.copy()
    for k in skins:
        sl = slice(k["first"], k["first"] + k["count"])
        pos[sl], nrm[sl], tan[sl] = np_skin.skin(k["joints"], k["weights"], k["matrices"], base.positions[sl], base.normals[sl], base.tangents[sl])
    return sd.with_arrays(flat, positions=pos, normals=nrm, tangents=tan)


def cornell_cases(flat):
    """Cornell: each of its two boxes (its last two nodes' meshes) as its own skin -- the GPU cases and their CPU restatement share these"""
    meshes = sorted({int(flat.nodes[-2]["primMesh"]), int(flat.nodes[-1]["primMesh"])})
    return [make(flat, *sd.mesh_range(flat, m), jc, 40 + i) for i, (m, jc) in enumerate(zip(meshes, (2, 33)))]


def cornell_subrange_cases(flat):
    """sub-ranges of Cornell that start at an odd vertex, with count 1 and 63 (disjoint; outside them nothing may change)"""
    assert len(flat.positions) >= 1 + 1 + 2 + 63
    return [make(flat, 1, 1, 1, 50), make(flat, 5, 63, 33, 51)]


def atrium_cases(flat):
    """the small atrium: 65 vertices from an odd index inside its most-instanced mesh (a column or an arch: posed in every instance), 257
    from the start of its largest mesh on (they run into the next mesh), and a range that ends at the scene's last vertex"""
    uses = np.bincount(flat.nodes["primMesh"], minlength=len(flat.prim_meshes))
    a, na = sd.mesh_range(flat, int(np.argmax(uses)))
    b, _ = sd.mesh_range(flat, int(np.argmax(flat.prim_meshes["vertexCount"])))
    total, tail = len(flat.positions), 129
    assert na >= 66
    out = [make(flat, a + 1 - a % 2, 65, 1, 60), make(flat, b + 1, 257, 2, 61), make(flat, total - tail, tail, 33, 62)]
    assert disjoint(out) and out[0]["first"] % 2 == 1
    return out


def disjoint(skins):
    r = sorted((k["first"], k["first"] + k["count"]) for k in skins)
    return all(a[1] <= b[0] for a, b in zip(r, r[1:]))
