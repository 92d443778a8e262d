"""The C++ glTF loader's skins (host/gltf_loader.cpp) through host_py: a small skinned .gltf + .bin written here -- a two-joint bending bar
with u8 joints and float weights, and a second primitive with u16 joints and normalised-u16 weights -- must come back as the arrays the
test wrote.  Every matrix entry is a small dyadic number, so the float32 products of the loader and of numpy are exact and equal."""
import copy
import json

import numpy as np
import pytest

F = np.float32


def _col(m):
    """4x4 [r, c] -> 16 floats column-major"""
    return np.ascontiguousarray(np.asarray(m, F).T.reshape(16))


def _translation(x, y, z):
    m = np.eye(4, dtype=F)
    m[:3, 3] = (x, y, z)
    return m


# the node hierarchy at rest: armature (translated) > joint 0 (translated) > joint 1 (translated, turned half round z, scaled)
ARMATURE = _translation(1, 0, 0)
JOINT0 = _translation(0, 0.5, 0)
JOINT1 = _translation(0, 1, 0) @ np.diag([-1, -1, 1, 1]).astype(F) @ np.diag([2, 0.5, 1, 1]).astype(F)
INVERSE_BIND = [_translation(-1, -0.5, 0), _translation(-1, -1.5, 0.25)]

BAR_POS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 2, 0], [1, 2, 0]], F)
BAR_IDX = np.array([0, 1, 2, 2, 1, 3, 2, 3, 4, 4, 3, 5], np.uint16)
BAR_JOINTS = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0]], np.uint8)
BAR_WEIGHTS = np.array([[1, 0, 0, 0], [1, 0, 0, 0], [0.5, 0.5, 0, 0], [0.25, 0.75, 0, 0], [1, 0, 0, 0], [0.5, 0.5, 0, 0]], F)
QUAD_POS = np.array([[2, 0, 0], [3, 0, 0], [2, 1, 0], [3, 1, 0]], F)
QUAD_IDX = np.array([0, 1, 2, 2, 1, 3], np.uint16)
QUAD_JOINTS = np.array([[1, 0, 0, 0], [1, 0, 1, 0], [0, 1, 0, 1], [1, 1, 1, 1]], np.uint16)
QUAD_WEIGHTS = np.array([[65535, 0, 0, 0], [13107, 52428, 0, 0], [1, 2, 3, 65529], [16384, 16384, 16384, 16383]], np.uint16)
TRI_POS = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], F)


class _Bin:
    def __init__(self):
        self.data, self.views, self.accessors = b"", [], []

    def add(self, array, ctype, atype, normalized=False, count=None):
        array = np.ascontiguousarray(array)
        self.data += b"\0" * (-len(self.data) % 4)
        self.views.append({"buffer": 0, "byteOffset": len(self.data), "byteLength": array.nbytes})
        self.data += array.tobytes()
        acc = {"bufferView": len(self.views) - 1, "componentType": ctype, "count": int(array.shape[0] if count is None else count), "type": atype}
        if normalized:
            acc["normalized"] = True
        if atype == "VEC3" and ctype == 5126:
            acc["min"], acc["max"] = array.min(0).tolist(), array.max(0).tolist()
        self.accessors.append(acc)
        return len(self.accessors) - 1


def _document(skinned=True):
    """(glTF JSON as a dict, the .bin bytes)"""
    b = _Bin()
    bar = {"attributes": {"POSITION": b.add(BAR_POS, 5126, "VEC3")}, "indices": b.add(BAR_IDX, 5123, "SCALAR")}
    quad = {"attributes": {"POSITION": b.add(QUAD_POS, 5126, "VEC3")}, "indices": b.add(QUAD_IDX, 5123, "SCALAR")}
    tri = {"attributes": {"POSITION": b.add(TRI_POS, 5126, "VEC3")}}
    doc = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0, 3, 4]}],
           "nodes": [{"name": "armature", "translation": [1, 0, 0], "children": [1]},
                     {"name": "joint0", "translation": [0, 0.5, 0], "children": [2]},
                     {"name": "joint1", "translation": [0, 1, 0], "rotation": [0, 0, 1, 0], "scale": [2, 0.5, 1]},
                     {"name": "bar", "mesh": 0, "translation": [5, 5, 5]},
                     {"name": "triangle", "mesh": 1, "translation": [-2, 0, 0]}],
           "meshes": [{"primitives": [bar, quad]}, {"primitives": [tri]}]}
    if skinned:
        bar["attributes"]["JOINTS_0"] = b.add(BAR_JOINTS, 5121, "VEC4")
        bar["attributes"]["WEIGHTS_0"] = b.add(BAR_WEIGHTS, 5126, "VEC4")
        quad["attributes"]["JOINTS_0"] = b.add(QUAD_JOINTS, 5123, "VEC4")
        quad["attributes"]["WEIGHTS_0"] = b.add(QUAD_WEIGHTS, 5123, "VEC4", normalized=True)
        ibm = b.add(np.stack([_col(m) for m in INVERSE_BIND]), 5126, "MAT4")
        doc["skins"] = [{"joints": [1, 2], "inverseBindMatrices": ibm, "skeleton": 0}]
        doc["nodes"][3]["skin"] = 0
    doc["buffers"] = [{"uri": "scene.bin", "byteLength": len(b.data)}]
    doc["bufferViews"], doc["accessors"] = b.views, b.accessors
    return doc, b.data


def _write(tmp_path, doc, data, name="scene"):
    (tmp_path / "scene.bin").write_bytes(data)
    path = tmp_path / f"{name}.gltf"
    path.write_text(json.dumps(doc))
    return str(path)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_skinned_file_comes_back_as_written(tmp_path):
    from vkrt_amd import host_py

    doc, data = _document()
    path = _write(tmp_path, doc, data)
    got = host_py.load_gltf_skins(path)
    flat = host_py.load_gltf(path)
    assert got["warnings"] == ""
    V = len(BAR_POS) + len(QUAD_POS) + len(TRI_POS)
    assert len(flat.positions) == V and _same(flat.positions, np.concatenate([BAR_POS, QUAD_POS, TRI_POS]))
    # four influences per vertex of the whole scene: u8 joints widened, normalised u16 weights as x / 65535 in float32, zeros where a
    # primitive has none
    joints = np.concatenate([BAR_JOINTS.astype(np.uint16), QUAD_JOINTS, np.zeros((3, 4), np.uint16)])
    weights = np.concatenate([BAR_WEIGHTS, QUAD_WEIGHTS.astype(F) / F(65535.0), np.zeros((3, 4), F)])
    assert _same(got["joints0"], joints) and _same(got["weights0"], weights)
    assert len(got["skins"]) == 1
    sk = got["skins"][0]
    assert sk["joint_nodes"].tolist() == [1, 2]
    assert _same(sk["inverse_bind"], np.stack([_col(m) for m in INVERSE_BIND]))
    # jointGlobal x inverseBind from the hierarchy at rest: the numpy product
    globals_ = [ARMATURE @ JOINT0, ARMATURE @ JOINT0 @ JOINT1]
    rest = np.stack([_col(g @ ib) for g, ib in zip(globals_, INVERSE_BIND)])
    assert rest.dtype == F and _same(sk["rest_joint_matrices"], rest)
    assert not np.array_equal(rest[1], _col(np.eye(4)))
    assert sk["vertex_ranges"].tolist() == [[0, len(BAR_POS)], [len(BAR_POS), len(QUAD_POS)]]
    # a skinned mesh node's own transform is ignored (identity instance matrices); the unskinned node keeps its own
    assert flat.nodes["primMesh"].tolist() == [0, 1, 2]
    assert _same(flat.nodes["worldMatrix"][0], _col(np.eye(4))) and _same(flat.nodes["worldMatrix"][1], _col(np.eye(4)))
    assert _same(flat.nodes["worldMatrix"][2], _col(_translation(-2, 0, 0)))


def test_identity_inverse_bind_when_absent_and_more_than_four_influences_warn(tmp_path):
    from vkrt_amd import host_py

    doc, data = _document()
    del doc["skins"][0]["inverseBindMatrices"]
    doc["meshes"][0]["primitives"][0]["attributes"]["JOINTS_1"] = doc["meshes"][0]["primitives"][0]["attributes"]["JOINTS_0"]
    doc["meshes"][0]["primitives"][0]["attributes"]["WEIGHTS_1"] = doc["meshes"][0]["primitives"][0]["attributes"]["WEIGHTS_0"]
    got = host_py.load_gltf_skins(_write(tmp_path, doc, data))
    sk = got["skins"][0]
    assert _same(sk["inverse_bind"], np.stack([_col(np.eye(4))] * 2))
    assert _same(sk["rest_joint_matrices"], np.stack([_col(ARMATURE @ JOINT0), _col(ARMATURE @ JOINT0 @ JOINT1)]))
    assert "JOINTS_1" in got["warnings"] and "first four" in got["warnings"]
    assert _same(got["joints0"][:6], BAR_JOINTS.astype(np.uint16))  # the first four are used


def test_file_without_skins_loads_as_before(tmp_path):
    from vkrt_amd import host_py

    doc, data = _document(skinned=False)
    path = _write(tmp_path, doc, data)
    got = host_py.load_gltf_skins(path)
    assert got["skins"] == [] and got["joints0"].shape == (0, 4) and got["weights0"].shape == (0, 4) and got["warnings"] == ""
    flat = host_py.load_gltf(path)
    assert _same(flat.positions, np.concatenate([BAR_POS, QUAD_POS, TRI_POS]))
    assert _same(flat.nodes["worldMatrix"][0], _col(_translation(5, 5, 5))) and _same(flat.nodes["worldMatrix"][2], _col(_translation(-2, 0, 0)))
    # and against the skinned file: the same geometry, only the bar's instance matrices differ
    sdoc, sdata = _document()
    sflat = host_py.load_gltf(_write(tmp_path, sdoc, sdata, "skinned"))
    for k in ("positions", "normals", "tangents", "texcoords0", "indices"):
        assert _same(getattr(flat, k), getattr(sflat, k)), k
    assert _same(flat.prim_meshes, sflat.prim_meshes)


def _malformed():
    """(name, change to the document, a word of the error)"""
    def accessor(doc, attr, prim=0):
        return doc["accessors"][doc["meshes"][0]["primitives"][prim]["attributes"][attr]]

    def joints_float(doc):
        accessor(doc, "JOINTS_0")["componentType"] = 5126

    def joints_vec3(doc):
        accessor(doc, "JOINTS_0")["type"] = "VEC3"

    def joints_count(doc):
        accessor(doc, "JOINTS_0")["count"] = len(BAR_POS) - 1

    def weights_not_normalised(doc):
        del accessor(doc, "WEIGHTS_0", prim=1)["normalized"]

    def weights_count(doc):
        accessor(doc, "WEIGHTS_0")["count"] = len(BAR_POS) - 2

    def no_weights(doc):
        del doc["meshes"][0]["primitives"][0]["attributes"]["WEIGHTS_0"]

    def ibm_count(doc):
        doc["accessors"][doc["skins"][0]["inverseBindMatrices"]]["count"] = 1

    def ibm_type(doc):
        doc["accessors"][doc["skins"][0]["inverseBindMatrices"]]["type"] = "VEC4"

    def joint_outside(doc):
        doc["skins"][0]["joints"] = [1]  # the file's indices reach joint 1
        del doc["skins"][0]["inverseBindMatrices"]

    def joint_not_a_node(doc):
        doc["skins"][0]["joints"] = [1, 9]

    def no_joints(doc):
        doc["skins"][0]["joints"] = []

    def bad_skin_index(doc):
        doc["nodes"][3]["skin"] = 3

    return [("joints_float", joints_float, "JOINTS_0"), ("joints_vec3", joints_vec3, "JOINTS_0"), ("joints_count", joints_count, "JOINTS_0"),
            ("weights_not_normalised", weights_not_normalised, "WEIGHTS_0"), ("weights_count", weights_count, "WEIGHTS_0"),
            ("no_weights", no_weights, "WEIGHTS_0"), ("ibm_count", ibm_count, "inverseBindMatrices"), ("ibm_type", ibm_type, "inverseBindMatrices"),
            ("joint_outside", joint_outside, "joint index"), ("joint_not_a_node", joint_not_a_node, "joint"), ("no_joints", no_joints, "joints"),
            ("bad_skin_index", bad_skin_index, "skin")]


@pytest.mark.parametrize("name,change,word", _malformed(), ids=[m[0] for m in _malformed()])
def test_malformed_skin_data_raises(tmp_path, name, change, word):
    from vkrt_amd import host_py

    doc, data = _document()
    doc = copy.deepcopy(doc)
    change(doc)
    with pytest.raises(RuntimeError, match=word):
        host_py.load_gltf_skins(_write(tmp_path, doc, data))
