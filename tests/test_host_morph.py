"""The C++ glTF loader's morph targets (host/gltf_loader.cpp) through host_py: a small morphed .gltf + .bin written here -- a bar with two
dense targets (POSITION and NORMAL; POSITION alone), a quad whose POSITION targets are sparse accessors (u8 indices over zeros, u16
indices over a bufferView), a triangle with a sparse target with u32 indices; mesh.weights and a node's override -- must come back as
the arrays the test wrote.  Every value is a small dyadic number, so the float32 products of np_morph on them are exact."""
import copy

import numpy as np
import pytest

from test_host_skin import BAR_IDX, BAR_POS, QUAD_IDX, QUAD_POS, TRI_POS, _Bin, _same, _write

F = np.float32

BAR_DP = np.array([[[0, 0, 0.5], [0, 0, 0.5], [0.25, 0, 0], [0.25, 0, 0], [0.5, 0.5, 0], [0.5, 0.5, 0]],
                   [[0, -0.25, 0], [0, -0.25, 0], [0, 0, 0], [0, 0, 0], [-0.5, 0, 0.125], [-0.5, 0, 0.125]]], F)
BAR_DN = np.array([[0.5, 0, 0], [0.5, 0, 0], [0, 0.25, 0], [0, 0.25, 0], [0, 0, -0.5], [0, 0, -0.5]], F)  # target 0 only
QUAD_SPARSE0 = (np.array([1, 3], np.uint8), np.array([[0, 0, 0.5], [0.25, 0.25, 0]], F))                   # over zeros
QUAD_BASE1 = np.array([[0, 0, 0.125], [0, 0, 0.125], [0, 0, 0.125], [0, 0, 0.125]], F)
QUAD_SPARSE1 = (np.array([0, 2], np.uint16), np.array([[0.5, 0, 0], [0, -0.5, 0]], F))                     # over QUAD_BASE1
TRI_SPARSE = (np.array([2], np.uint32), np.array([[0, 0.75, 0.25]], F))
MESH_WEIGHTS, NODE_WEIGHTS, TRI_WEIGHTS = [0.5, 0.25], [0.75, -0.5], [0.5]


def _sparse(b, count, indices, values, base=None):
    """a sparse VEC3 float accessor: `indices` (their dtype is the component type) and `values` in views of their own"""
    ctype = {np.dtype(np.uint8): 5121, np.dtype(np.uint16): 5123, np.dtype(np.uint32): 5125}[indices.dtype]
    acc = {"componentType": 5126, "count": int(count), "type": "VEC3"}
    if base is not None:
        acc = b.accessors[b.add(base, 5126, "VEC3")]
    views = []
    for a in (indices, values):
        b.data += b"\0" * (-len(b.data) % 4)
        b.views.append({"buffer": 0, "byteOffset": len(b.data), "byteLength": a.nbytes})
        b.data += a.tobytes()
        views.append(len(b.views) - 1)
    acc["sparse"] = {"count": len(indices), "indices": {"bufferView": views[0], "componentType": ctype}, "values": {"bufferView": views[1]}}
    if base is None:
        b.accessors.append(acc)
    return b.accessors.index(acc)


def _dense(indices, values, count, base=None):
    out = np.zeros((count, 3), F) if base is None else base.copy()
    out[indices.astype(np.int64)] = values
    return out


QUAD_DP = np.stack([_dense(*QUAD_SPARSE0, 4), _dense(*QUAD_SPARSE1, 4, QUAD_BASE1)])
TRI_DP = _dense(*TRI_SPARSE, 3)[None]


def _document():
    """(glTF JSON as a dict, the .bin bytes)"""
    b = _Bin()
    bar = {"attributes": {"POSITION": b.add(BAR_POS, 5126, "VEC3")}, "indices": b.add(BAR_IDX, 5123, "SCALAR"),
           "targets": [{"POSITION": b.add(BAR_DP[0], 5126, "VEC3"), "NORMAL": b.add(BAR_DN, 5126, "VEC3")}, {"POSITION": b.add(BAR_DP[1], 5126, "VEC3")}]}
    quad = {"attributes": {"POSITION": b.add(QUAD_POS, 5126, "VEC3")}, "indices": b.add(QUAD_IDX, 5123, "SCALAR"),
            "targets": [{"POSITION": _sparse(b, 4, *QUAD_SPARSE0)}, {"POSITION": _sparse(b, 4, *QUAD_SPARSE1, base=QUAD_BASE1)}]}
    tri = {"attributes": {"POSITION": b.add(TRI_POS, 5126, "VEC3")}, "targets": [{"POSITION": _sparse(b, 3, *TRI_SPARSE)}]}
    doc = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0, 1, 2]}],
           "nodes": [{"name": "bar", "mesh": 0, "weights": NODE_WEIGHTS},
                     {"name": "bar again", "mesh": 0, "translation": [0, 0, -2], "weights": [1, 1]},  # a later node: its weights do not count
                     {"name": "triangle", "mesh": 1, "translation": [-2, 0, 0]}],
           "meshes": [{"primitives": [bar, quad], "weights": MESH_WEIGHTS}, {"primitives": [tri], "weights": TRI_WEIGHTS}]}
    doc["buffers"] = [{"uri": "scene.bin", "byteLength": len(b.data)}]
    doc["bufferViews"], doc["accessors"] = b.views, b.accessors
    return doc, b.data


def test_morphed_file_comes_back_as_written(tmp_path):
    from vkrt_amd import host_py

    doc, data = _document()
    path = _write(tmp_path, doc, data)
    flat = host_py.load_gltf(path)
    assert _same(flat.positions, np.concatenate([BAR_POS, QUAD_POS, TRI_POS]))  # the base shape, unmorphed
    got = host_py.load_gltf_morphs(path)
    assert [(m["first"], m["count"], m["target_count"]) for m in got] == [(0, 6, 2), (6, 4, 2), (10, 3, 1)]
    bar, quad, tri = got
    assert _same(bar["position_deltas"], BAR_DP) and bar["tangent_deltas"] is None
    assert _same(bar["normal_deltas"], np.stack([BAR_DN, np.zeros_like(BAR_DN)]))  # a target without NORMAL bends no normal
    assert _same(quad["position_deltas"], QUAD_DP) and quad["normal_deltas"] is None and quad["tangent_deltas"] is None
    assert _same(tri["position_deltas"], TRI_DP)
    assert QUAD_DP[0, 1, 2] == 0.5 and QUAD_DP[1, 1, 2] == 0.125 and QUAD_DP[1, 0, 0] == 0.5  # (substituted, zeros, and the base kept)
    # the first node that instances mesh 0 overrides mesh.weights, for every primitive of the mesh; the triangle's node has none
    assert _same(bar["weights"], np.array(NODE_WEIGHTS, F)) and _same(quad["weights"], np.array(NODE_WEIGHTS, F))
    assert _same(tri["weights"], np.array(TRI_WEIGHTS, F))
    assert flat.nodes["primMesh"].tolist() == [0, 1, 0, 1, 2]


def test_mesh_weights_without_a_node_override_and_zeros_without_either(tmp_path):
    from vkrt_amd import host_py

    doc, data = _document()
    del doc["nodes"][0]["weights"]  # the first node has none: the mesh's stay, the second node's still do not count
    del doc["meshes"][1]["weights"]
    got = host_py.load_gltf_morphs(_write(tmp_path, doc, data))
    assert _same(got[0]["weights"], np.array(MESH_WEIGHTS, F)) and _same(got[1]["weights"], np.array(MESH_WEIGHTS, F))
    assert _same(got[2]["weights"], np.zeros(1, F))


def test_file_without_targets_loads_as_before(tmp_path):
    from vkrt_amd import host_py

    doc, data = _document()
    plain = copy.deepcopy(doc)
    for mesh in plain["meshes"]:
        del mesh["weights"]
        for prim in mesh["primitives"]:
            del prim["targets"]
    for node in plain["nodes"]:
        node.pop("weights", None)
    a, b = host_py.load_gltf(_write(tmp_path, doc, data)), host_py.load_gltf(_write(tmp_path, plain, data, "plain"))
    for k in ("positions", "normals", "tangents", "texcoords0", "indices", "nodes"):
        assert _same(getattr(a, k), getattr(b, k)), k
    assert _same(a.prim_meshes, b.prim_meshes)
    assert host_py.load_gltf_morphs(_write(tmp_path, plain, data, "plain")) == []


def _malformed():
    """(name, change to the document, a pattern of the error: it names the accessor, the mesh or the node)"""
    def target(doc, prim, t, sem="POSITION"):
        return doc["meshes"][0]["primitives"][prim]["targets"][t][sem]

    def acc(doc, prim, t, sem="POSITION"):
        return doc["accessors"][target(doc, prim, t, sem)]

    def vec4(doc):
        acc(doc, 0, 0)["type"] = "VEC4"

    def shorts(doc):
        acc(doc, 0, 0, "NORMAL")["componentType"] = 5122

    def count(doc):
        acc(doc, 0, 1)["count"] = len(BAR_POS) - 1

    def texcoord(doc):
        doc["meshes"][0]["primitives"][0]["targets"][0]["TEXCOORD_0"] = target(doc, 0, 0)

    def target_counts(doc):
        doc["meshes"][0]["primitives"][1]["targets"].pop()

    def mesh_weights(doc):
        doc["meshes"][0]["weights"] = [0.5]

    def node_weights(doc):
        doc["nodes"][1]["weights"] = [1, 1, 1]

    def sparse_index_type(doc):
        acc(doc, 1, 0)["sparse"]["indices"]["componentType"] = 5126

    def sparse_index_range(doc):  # the triangle's target substitutes element 2: one vertex less
        tri = doc["meshes"][1]["primitives"][0]
        doc["accessors"][tri["attributes"]["POSITION"]]["count"] = 2
        doc["accessors"][tri["targets"][0]["POSITION"]]["count"] = 2

    def sparse_count(doc):
        acc(doc, 1, 0)["sparse"]["count"] = 5

    def sparse_overrun(doc):
        acc(doc, 1, 0)["sparse"]["values"]["byteOffset"] = 1 << 20

    return [("vec4", vec4, r"POSITION accessor \d+ is not a VEC3 of floats"), ("shorts", shorts, r"NORMAL accessor \d+ is not a VEC3 of floats"),
            ("count", count, r"POSITION accessor \d+ has 5 elements, the primitive has 6 vertices"),
            ("texcoord", texcoord, r"attribute TEXCOORD_0 \(accessor \d+\)"), ("target_counts", target_counts, r"mesh 0 primitive 1 has 1 morph targets"),
            ("mesh_weights", mesh_weights, r"mesh 0: 1 weights for 2 morph targets"), ("node_weights", node_weights, r"node 1: 3 weights for mesh 0's 2"),
            ("sparse_index_type", sparse_index_type, r"POSITION accessor \d+: sparse.indices.componentType 5126"),
            ("sparse_index_range", sparse_index_range, r"POSITION accessor \d+: sparse index 2 outside its 2 elements"),
            ("sparse_count", sparse_count, r"POSITION accessor \d+: sparse.count 5 above"),
            ("sparse_overrun", sparse_overrun, r"POSITION accessor \d+: sparse data overruns")]


@pytest.mark.parametrize("name,change,word", _malformed(), ids=[m[0] for m in _malformed()])
def test_malformed_morph_data_raises(tmp_path, name, change, word):
    from vkrt_amd import host_py

    doc, data = _document()
    doc = copy.deepcopy(doc)
    change(doc)
    with pytest.raises(RuntimeError, match=word):
        host_py.load_gltf_morphs(_write(tmp_path, doc, data))


def test_the_accessor_named_is_the_faulty_one(tmp_path):
    from vkrt_amd import host_py

    doc, data = _document()
    doc = copy.deepcopy(doc)
    idx = doc["meshes"][0]["primitives"][0]["targets"][1]["POSITION"]
    doc["accessors"][idx]["type"] = "VEC2"
    with pytest.raises(RuntimeError, match=rf"POSITION accessor {idx} "):
        host_py.load_gltf_morphs(_write(tmp_path, doc, data))
