"""A synthetic scene of many instances of two small meshes, for the node-update tests (test_gpu_node_update.py): 300 nodes -- more than
one 256-thread workgroup of the transform kernel, so its tail is exercised -- on a 20 x 15 grid, alternately a two-triangle quad and a
12-triangle box, each with a seeded rotation of its own."""
import numpy as np

from vkrt_amd.flat_scene import LIGHT_DTYPE, MAT_DTYPE, NODE_DTYPE, PRIM_DTYPE, FlatScene

NODES = 300
COLUMNS, SPACING = 20, 3.0


def _meshes():
    quad = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32)
    quad_idx = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    box = np.array([[x, y, z] for z in (-0.6, 0.6) for y in (-0.8, 0.8) for x in (-1.0, 1.0)], np.float32)
    faces = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]  # outward winding
    box_idx = np.array([k for a, b, c, d in faces for k in (a, b, c, a, c, d)], np.uint32)
    pos = np.concatenate([quad, box])
    nrm = np.concatenate([np.tile(np.array([0, 0, 1], np.float32), (4, 1)), box / np.linalg.norm(box, axis=1, keepdims=True)]).astype(np.float32)
    tan = np.tile(np.array([1, 0, 0, 1], np.float32), (len(pos), 1))
    uv = (pos[:, :2] * 0.5 + 0.5).astype(np.float32)
    pm = np.zeros(2, PRIM_DTYPE)
    pm[0] = (0, 6, 0, 4, 0)
    pm[1] = (6, 36, 4, 8, 1)
    return pos, nrm, tan, uv, np.concatenate([quad_idx, box_idx]), pm


def instances_scene(nodes=NODES, seed=31):
    pos, nrm, tan, uv, idx, pm = _meshes()
    mats = np.zeros(2, MAT_DTYPE)
    for k, colour in enumerate(((0.8, 0.7, 0.6, 1.0), (0.4, 0.6, 0.8, 1.0))):
        mats[k]["pbrBaseColorFactor"] = colour
        mats[k]["roughnessFactor"] = 0.9
        for t in ("pbrBaseColorTexture", "metallicRoughnessTexture", "normalTexture", "emissiveTexture"):
            mats[k][t] = -1
    lights = np.zeros(1, LIGHT_DTYPE)
    lights[0] = ((0.5 * COLUMNS * SPACING, 20.0, 30.0), (1, 1, 1), 3000.0, 0)
    rng = np.random.default_rng(seed)
    nd = np.zeros(nodes, NODE_DTYPE)
    for i in range(nodes):
        a = rng.uniform(-0.5, 0.5)
        M = np.eye(4)
        M[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        M[:3, 3] = ((i % COLUMNS) * SPACING, (i // COLUMNS) * SPACING, rng.uniform(-0.3, 0.3))
        nd[i]["worldMatrix"] = np.ascontiguousarray(M.T.reshape(16), np.float32)  # column-major
        nd[i]["primMesh"] = i & 1
    return FlatScene(pos, nrm, tan, uv, idx, pm, mats, lights, nd, [])


def rays_from_above(n=20000, seed=6, nodes=NODES):
    """(origins, directions) float32 [n, 3]: from above and below the grid, nearly along z, so that both facings of the quads are hit"""
    rng = np.random.default_rng(seed)
    rows = (nodes + COLUMNS - 1) // COLUMNS
    o = np.stack([rng.uniform(-2, COLUMNS * SPACING, n), rng.uniform(-2, rows * SPACING, n), np.where(rng.random(n) < 0.5, 8.0, -8.0)], 1)
    d = np.stack([rng.uniform(-0.15, 0.15, n), rng.uniform(-0.15, 0.15, n), -np.sign(o[:, 2])], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)
