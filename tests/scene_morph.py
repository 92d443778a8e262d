"""Seeded morphs shared by the morph-target tests (test_np_morph.py, test_gpu_morph.py): for any vertex range of a FlatScene, T targets
of seeded deltas (positions a few percent of the range's extent, normals and tangents of the order of the unit vectors they bend) and
weights of one of four kinds: "zero" (all zero, one of them -0), "negative", "above1", "gaps" (zeros between non-zeros).  morphed() is
the scene a fresh Renderer is created from: tests/np_morph.py applied to the ranges."""
import numpy as np

import np_morph
import scene_deform as sd

F = np.float32
ATTRS = ("position_deltas", "normal_deltas", "tangent_deltas")


def weights(target_count, kind, seed):
    rng = np.random.default_rng(seed)
    T = int(target_count)
    if kind == "zero":
        w = np.zeros(T, F)
        w[T // 2] = F(-0.0)
    elif kind == "negative":
        w = -rng.uniform(0.2, 0.9, T).astype(F)
    elif kind == "above1":
        w = rng.uniform(1.1, 2.0, T).astype(F)
    elif kind == "gaps":
        w = rng.uniform(-0.5, 1.0, T).astype(F)
        w[w == 0] = F(0.25)
        w[1::3] = 0  # (T = 2: w[1]; T = 33: eleven zeros, each between non-zeros)
        w[-1] = F(0.75) if T > 2 else w[-1]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(w, F)


def make(flat, first, count, target_count, seed, attrs=ATTRS, kind="gaps"):
    """one morph of a test: dict(first, count, target_count, position_deltas, normal_deltas, tangent_deltas, weights)"""
    rng = np.random.default_rng(seed)
    T, n = int(target_count), int(count)
    p = flat.positions[first:first + count].astype(np.float64)
    ext = max(float((p.max(0) - p.min(0)).max()), 0.05 * float(np.abs(flat.positions).max()))
    out = dict(first=int(first), count=n, target_count=T, kind=kind)
    for a, scale in zip(ATTRS, (0.08 * ext, 0.5, 0.5)):
        out[a] = np.ascontiguousarray(rng.uniform(-scale, scale, (T, n, 3)), F) if a in attrs else None
    out["weights"] = weights(T, kind, seed + 500)
    return out


def deltas(m):
    return {a: m[a] for a in ATTRS}


def apply(m, positions, normals, tangents, weights=None):
    """np_morph on the base arrays of the morph's range"""
    return np_morph.morph(m["weights"] if weights is None else weights, positions, normals, tangents, **deltas(m))


def morphed(flat, morphs, base=None):
    """A copy of `flat` with every morph's range posed by np_morph from the base shape in `base` (default `flat`)."""
    base = base or flat
    pos, nrm, tan = flat.positions.copy(), flat.normals.copy(), flat.tangents.copy()
    for m in morphs:
        sl = slice(m["first"], m["first"] + m["count"])
        pos[sl], nrm[sl], tan[sl] = apply(m, base.positions[sl], base.normals[sl], base.tangents[sl])
    return sd.with_arrays(flat, positions=pos, normals=nrm, tangents=tan)


def cornell_cases(flat):
    """Cornell: each of its two boxes (its last two nodes' meshes) as its own morph, all three attributes: 2 targets with weights above
    1, 33 targets with gaps -- the GPU cases and their CPU restatement share these"""
    meshes = sorted({int(flat.nodes[-2]["primMesh"]), int(flat.nodes[-1]["primMesh"])})
    spec = ((2, "above1"), (33, "gaps"))
    return [make(flat, *sd.mesh_range(flat, m), T, 40 + i, kind=kind) for i, (m, (T, kind)) in enumerate(zip(meshes, spec))]


def cornell_subrange_cases(flat):
    """sub-ranges of Cornell that start at an odd vertex (disjoint; outside them nothing may change): count 1 with one target of
    positions only, count 2 with all-zero weights, count 63 with normals only"""
    assert len(flat.positions) >= 1 + 1 + 2 + 63
    return [make(flat, 1, 1, 1, 50, attrs=("position_deltas",), kind="negative"), make(flat, 3, 2, 2, 52, kind="zero"),
            make(flat, 5, 63, 2, 51, attrs=("normal_deltas",), kind="gaps")]


def cornell_many_target_cases(flat):
    """more targets than a wave has lanes (the kernel reads the weights 64 at a time): 130 with gaps, weights 63, 64 and 129 in use, and
    the most a morph may have, 256, all in use; small odd ranges clear of the cases above"""
    a = make(flat, 69, 5, 130, 53, kind="gaps")
    a["weights"][[63, 64, 129]] = (F(0.5), F(-0.25), F(0.75))
    a["weights"][[62, 65, 128]] = 0
    return [a, make(flat, 75, 3, 256, 54, attrs=("position_deltas", "normal_deltas"), kind="negative")]


def atrium_cases(flat):
    """the small atrium: 65 vertices from an odd index inside its most-instanced mesh (morphed in every instance), 257 from an odd index
    near the start of its largest mesh on, and a range that ends at the scene's last vertex"""
    uses = np.bincount(flat.nodes["primMesh"], minlength=len(flat.prim_meshes))
    a, na = sd.mesh_range(flat, int(np.argmax(uses)))
    b, _ = sd.mesh_range(flat, int(np.argmax(flat.prim_meshes["vertexCount"])))
    total, tail = len(flat.positions), 129
    assert na >= 66
    out = [make(flat, a + 1 - a % 2, 65, 2, 60, kind="negative"), make(flat, b + 1 - b % 2, 257, 33, 61, kind="gaps"),
           make(flat, total - tail, tail, 1, 62, attrs=("position_deltas", "tangent_deltas"), kind="above1")]
    assert disjoint(out) and out[0]["first"] % 2 == 1 and out[1]["first"] % 2 == 1
    return out


def disjoint(morphs):
    r = sorted((m["first"], m["first"] + m["count"]) for m in morphs)
    return all(a[1] <= b[0] for a, b in zip(r, r[1:]))
