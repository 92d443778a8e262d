"""The one staging buffer behind the host paths of vkrt_scene_update_vertices, vkrt_scene_skin_vertices and vkrt_scene_morph_vertices:
one Cornell scene with a skin, a 33-target morph inside it and a 2-target morph outside every skin, posed through the host path on one
stream in an order that uses the buffer at 8 B, grows it twice and then reuses it for smaller calls of all three clients.  After every
step the live vertices of the whole scene -- texture coordinates included -- equal the numpy restatement in every bit."""
import numpy as np
import pytest

import scene_deform as sd
import scene_morph as sm
import scene_skin as ss

pytestmark = pytest.mark.gpu
F = np.float32


def _assert_vertices(r, flat, what):
    got = r.read_vertices(0, len(flat.positions))
    for k in ("positions", "normals", "tangents", "texcoords0"):
        assert np.array_equal(np.ascontiguousarray(got[k], F).view(np.uint32), np.ascontiguousarray(getattr(flat, k), F).view(np.uint32)), (what, k)


def test_host_calls_of_all_three_clients_share_one_growing_staging_buffer(cornell_flat):
    import torch
    from vkrt_amd.renderer import Renderer

    flat = cornell_flat
    N = len(flat.positions)
    a = ss.cornell_cases(flat)[1]  # 33 joints: 2112 B of matrices
    first = a["first"] + 1 + a["first"] % 2
    m1 = sm.make(flat, first, a["count"] - 3 - a["first"] % 2, 33, 77, kind="gaps")  # inside the skin, clear of both of its edges: 132 B of weights
    m2 = sm.make(flat, 1, 4, 2, 78, kind="above1")  # outside every skin: 8 B of weights
    assert a["first"] < m1["first"] and m1["first"] + m1["count"] < a["first"] + a["count"] and m2["first"] + m2["count"] <= a["first"]
    sent = sd.twisted(flat, range(len(flat.prim_meshes)))  # all four attributes of every vertex: 48 N B, more than the matrices
    sent = sd.with_arrays(sent, texcoords0=np.ascontiguousarray(np.random.default_rng(9).uniform(0, 1, (N, 2)), F))
    assert 48 * N > a["joint_count"] * 64 > m1["target_count"] * 4 > m2["target_count"] * 4
    assert not np.array_equal(sent.positions, flat.positions) and not np.array_equal(sent.normals, flat.normals)

    r = Renderer(flat, device=0, build="ploc")
    stream = torch.cuda.Stream(device="cuda:0")
    sk = r.add_skin(a["first"], a["joints"], a["weights"], joint_count=a["joint_count"], stream=stream)
    i1 = r.add_morph(m1["first"], stream=stream, **sm.deltas(m1))
    i2 = r.add_morph(m2["first"], stream=stream, **sm.deltas(m2))
    _assert_vertices(r, flat, "as created")

    r.morph(i2, m2["weights"], stream=stream)                          # 1. the buffer's first use: 8 B
    want = sm.morphed(flat, [m2])
    _assert_vertices(r, want, "1. the outer morph")
    r.skin(sk, a["matrices"], stream=stream)                           # 2. grows
    want = ss.posed(want, [a], base=flat)
    _assert_vertices(r, want, "2. the skin")
    sd.send(r, sent, ranges=[(0, N)], stream=stream)                   # 3. grows again: four parts back to back
    _assert_vertices(r, sent, "3. the whole scene, all four attributes")
    r.morph(i1, m1["weights"], stream=stream)                          # 4. smaller than the buffer; writes the skin's bind pose only
    _assert_vertices(r, sent, "4. the inner morph leaves the live vertices alone")
    r.skin(sk, a["matrices"], stream=stream)                           # 5.
    want = ss.posed(sent, [a], base=sm.morphed(flat, [m1]))
    assert not np.array_equal(want.positions, ss.posed(sent, [a], base=flat).positions)
    _assert_vertices(r, want, "5. the skin over the morphed bind pose")
    other = dict(m2, weights=sm.weights(2, "negative", 701))
    r.morph(i2, other["weights"], stream=stream)                       # 6.
    _assert_vertices(r, sm.morphed(want, [other], base=flat), "6. the outer morph with other weights")
    r.close()
