"""vkrt_hit_surface (Renderer.surface): shading inputs at the hits of ray queries, against the CPU references, bit for bit.

Expected values: NpScene.hit_attributes (oracle/np_pathtrace.py) for position, normal, vertex tangent frame and texture coordinate; the
normal-mapping, base-colour, metallic-roughness and emission lines exactly as np_pathtrace._closest_hit writes them, with every texture
tap taken from OracleScene.sample_texture (numpy's own sRGB table is rounded from binary64, the library's and the oracle's come from
powf, so numpy's taps cannot judge bits); alpha = float32(factor.a) * tap.a; geometric_normal = normalize(cross(p1 - p0, p2 - p0) *
gl_WorldToObjectEXT) in numpy float32.  The acceptance test is a path tracer whose rays go through Renderer.intersect / occluded and
whose hit shader reads Renderer.surface records: its image must be the oracle's and the library's own in every bit.

gl_WorldToObjectEXT is not the shader's arithmetic but the driver's; the project fixes it (oracle.cpp invert3x3,
csrc invert3x3_rows) as the cofactor inverse in binary64, fixed operation order, rounded to binary32.  NpScene takes np.linalg.inv
instead, which gives the same values but, where an entry is zero, not always the same sign of zero (identity: the cofactor form has
-0 off the diagonal, LAPACK +0), and that sign reaches the normals: on Cornell 1280 of 35184 records had `normal` (-1, 0, -0) against
(-1, 0, 0), at 0 ulp.  So the reference below gives NpScene the profile's inverse, restated in numpy in that operation order, after
checking that it equals NpScene's own in value in every entry; hit_attributes and everything after it run unchanged.

NaN results (the normal of a zero-area triangle) are compared as NaN: IEEE 754 leaves the sign and payload of a NaN a machine produces
open, and x86 and gfx950 choose differently."""
import copy
import os
import sys

import numpy as np
import pytest

from conftest import default_camera
import scene_deform
import scene_motion
from test_gpu_ray_query import _hostile_rays, _pack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

F = np.float32
QUADS = ("position", "geometric_normal", "normal", "shading_normal", "tangent", "binormal", "base_color", "emission")
SCALARS = ("texcoord_u", "texcoord_v", "alpha", "metallic", "roughness", "material", "valid", "reserved")
COLUMNS = {}
for _k, (_q, _s) in enumerate(zip(QUADS, SCALARS)):
    COLUMNS[_q] = slice(4 * _k, 4 * _k + 3)
    COLUMNS[_s] = slice(4 * _k + 3, 4 * _k + 4)
GEOMETRY_FIELDS = ("position", "geometric_normal", "normal", "texcoord_u", "texcoord_v", "material", "valid", "reserved")
MATERIAL_FIELDS = ("alpha", "metallic", "roughness", "base_color", "emission")


def _invalid_record():
    rec = np.zeros(32, np.uint32)
    rec[23] = 0xFFFFFFFF  # material = -1
    return rec


def _canon(a):
    """uint32 bits of float32 / int32 words with every NaN folded to one pattern"""
    a = np.ascontiguousarray(a)
    bits = a.view(np.uint32).copy()
    nan = (bits & 0x7FFFFFFF) > 0x7F800000
    bits[nan] = 0x7FC00000
    return bits


def _ulps(a, b):
    """largest distance in units of the last place between two float32 arrays given as bits (same-sign finite values)"""
    ia, ib = a.astype(np.int64), b.astype(np.int64)
    ia = np.where(ia & 0x80000000, 0x80000000 - ia, ia)
    ib = np.where(ib & 0x80000000, 0x80000000 - ib, ib)
    return int(np.abs(ia - ib).max()) if ia.size else 0


def _assert_records(got, want, what, fields=None):
    """got, want: [N, 32] words.  Bit for bit; on a difference name every field that differs, how many records and by how many ulps."""
    g, w = _canon(got), _canon(want)
    assert g.shape == w.shape, (g.shape, w.shape)
    # the integer words are not floats: compare them raw
    for name in ("material", "valid", "reserved"):
        c = COLUMNS[name]
        g[:, c], w[:, c] = np.ascontiguousarray(got).view(np.uint32)[:, c], np.ascontiguousarray(want).view(np.uint32)[:, c]
    bad = []
    for name in (fields or COLUMNS):
        c = COLUMNS[name]
        d = np.any(g[:, c] != w[:, c], axis=1)
        if d.any():
            first = int(np.nonzero(d)[0][0])
            bad.append(f"{name}: {int(d.sum())} of {len(d)} records differ, max {_ulps(g[:, c][d], w[:, c][d])} ulp, first record {first}: "
                       f"got {np.ascontiguousarray(got).view(F)[first, c]} want {np.ascontiguousarray(want).view(F)[first, c]}")
    assert not bad, what + ": " + "; ".join(bad)


def _profile_w2o(o2w):
    """[N, 3, 3] float32: the inverse of the upper-left 3x3 of o2w [N, 3, 4] as the arithmetic profile defines it (cofactors in
    binary64, the operation order of oracle.cpp invert3x3), signs of zero included"""
    m = np.asarray(o2w, F).astype(np.float64)
    a, b, c, d, e, f, g, h, i = (m[:, r, k] for r in range(3) for k in range(3))
    A = e * i - f * h
    B = -(d * i - f * g)
    C = d * h - e * g
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / (a * A + b * B + c * C)
        rows = [A * inv, -(b * i - c * h) * inv, (b * f - c * e) * inv, B * inv, (a * i - c * g) * inv, -(a * f - c * d) * inv,
                C * inv, -(a * h - b * g) * inv, (a * e - b * d) * inv]
    return np.stack(rows, 1).astype(F).reshape(-1, 3, 3)


class Reference:
    """The CPU statement of a vkrt_surface record for a FlatScene: NpScene's attribute fetch + the oracle's texture taps."""

    def __init__(self, flat):
        import np_pathtrace
        import oracle_py

        class _Scene(np_pathtrace.NpScene):
            def texture(sc, tex_index, uv):  # every tap from the C++ oracle (the library's powf table), not from numpy's
                tex_index = np.broadcast_to(np.asarray(tex_index, np.int64), (uv.shape[0],))
                out = np.ones((uv.shape[0], 4), F)
                for ti in np.unique(tex_index):
                    if ti < 0 or ti >= len(flat.textures):
                        continue  # the 1x1 white dummy
                    m = tex_index == ti
                    out[m] = self.orc.sample_texture(int(ti), np.ascontiguousarray(uv[m], F))
                return out

        self.flat = flat
        self.orc = oracle_py.OracleScene(flat, build_bvh=False)
        self.np = _Scene(flat)
        w2o = _profile_w2o(self.np.o2w)
        assert np.array_equal(w2o, self.np.w2o)  # the same inverse in value, entry by entry; only signs of zero may differ
        self.np.w2o = w2o
        self.tri_count = np.array([int(flat.prim_meshes[int(n["primMesh"])]["indexCount"]) // 3 for n in flat.nodes], np.int64)
        self.first_tri = np.concatenate([[0], np.cumsum(self.tri_count)])[:-1]

    def records(self, inst, prim, u, v, material=True):
        """[N, 32] float32 words of the records of valid (instance, primitive, u, v)"""
        import np_pathtrace as P

        inst, prim = np.asarray(inst, np.int64), np.asarray(prim, np.int64)
        u, v = np.asarray(u, F), np.asarray(v, F)
        n = inst.shape[0]
        out = np.zeros((n, 32), F)
        if n == 0:
            return out
        sc, fl = self.np, self.flat
        A = sc.hit_attributes(self.first_tri[inst] + prim, u, v)
        mat, uv = A["mat"], A["uv"]
        out[:, COLUMNS["position"]] = A["world_pos"]
        out[:, COLUMNS["normal"]] = A["world_nrm"]
        out[:, 3], out[:, 7] = uv[:, 0], uv[:, 1]
        # geometric normal: the object-space front face carried to world space by the inverse transpose, like hit_attributes' normals
        i0, i1, i2 = A["i"]
        pos = np.asarray(fl.positions, F).reshape(-1, 3)
        face = P._cross((pos[i1] - pos[i0]).astype(F), (pos[i2] - pos[i0]).astype(F))
        w2o = sc.w2o[inst]
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, COLUMNS["geometric_normal"]] = P._normalize(((face[:, 0:1] * w2o[:, 0, :] + face[:, 1:2] * w2o[:, 1, :]) + face[:, 2:3] * w2o[:, 2, :]).astype(F))
        tangent, binormal, tex_normal = A["world_tag"].copy(), A["world_bin"].copy(), A["world_nrm"].copy()
        pm = fl.prim_meshes[np.asarray(fl.nodes["primMesh"], np.int64)[inst]]
        out[:, 23] = np.maximum(0, pm["materialIndex"].astype(np.int32)).astype(np.int32).view(F)
        out[:, 27] = np.ones(n, np.int32).view(F)
        if material:
            emission = np.asarray(mat["emissiveFactor"], F).copy()                       # np_pathtrace._closest_hit:353-357, no `emits` mask
            et = mat["emissiveTexture"].astype(np.int64)
            m = et > -1
            if m.any():
                emission[m] = emission[m] * sc.texture(et[m], uv[m])[:, :3]
            nt = mat["normalTexture"].astype(np.int64)
            m = nt > -1
            if m.any():                                                                   # :358-367
                tn = P._normalize(sc.texture(nt[m], uv[m])[:, :3] * F(2.0) - F(1.0))
                tn = P._normalize(tangent[m] * tn[:, 0:1] + binormal[m] * tn[:, 1:2] + tex_normal[m] * tn[:, 2:3])
                tex_normal[m] = tn
                t2, b2 = P._coordinate_system(tn)
                tangent[m], binormal[m] = t2, b2
            base, metal, rough = sc.material_inputs(mat, uv)
            alpha = np.asarray(mat["pbrBaseColorFactor"], F)[:, 3].copy()
            bt = mat["pbrBaseColorTexture"].astype(np.int64)
            m = bt > -1
            if m.any():
                alpha[m] = alpha[m] * sc.texture(bt[m], uv[m])[:, 3]
            out[:, COLUMNS["base_color"]], out[:, COLUMNS["emission"]] = base, emission
            out[:, 11], out[:, 15], out[:, 19] = alpha, metal, rough
        out[:, COLUMNS["shading_normal"]], out[:, COLUMNS["tangent"]], out[:, COLUMNS["binormal"]] = tex_normal, tangent, binormal
        return out

    def for_hits(self, hit_words, material=True):
        """[N, 32] words for [N, 8] vkrt_hit words: valid hits through records(), everything else the all-zero record with material -1"""
        h = np.ascontiguousarray(hit_words).view(np.uint32)
        f, i = h.view(F), h.view(np.int32)
        inst, prim, u, v = i[:, 3].astype(np.int64), i[:, 4].astype(np.int64), f[:, 1], f[:, 2]
        ok = (inst >= 0) & (inst < len(self.flat.nodes)) & np.isfinite(u) & np.isfinite(v)
        cnt = np.zeros(len(h), np.int64)
        cnt[ok] = self.tri_count[inst[ok]]
        ok &= (prim >= 0) & (prim < cnt)
        out = np.tile(_invalid_record(), (len(h), 1))
        out[ok] = self.records(inst[ok], prim[ok], u[ok], v[ok], material).view(np.uint32)
        return out, ok


def _camera(W, H, info=None):
    """(GlobalUniforms, view_inverse, proj_inverse as 16 column-major floats each)"""
    import camera_np

    kw = {}
    if info is not None:
        c = info["camera"]
        kw = dict(eye=tuple(c["eye"]), center=tuple(c["center"]), up=tuple(c["up"]), fov=c["fov"])
    _, vi, pi = camera_np.global_uniforms(width=W, height=H, **kw)
    return default_camera(W, H, **kw), np.asarray(vi, F).T.reshape(-1).copy(), np.asarray(pi, F).T.reshape(-1).copy()


def _camera_rays(W, H, info=None):
    import np_pathtrace as P

    _, vi, pi = _camera(W, H, info)
    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys = xs.ravel(), ys.ravel()
    o = P._mat4_vec4(vi, np.tile(np.array([[0, 0, 0, 1]], F), (xs.size, 1)))[:, :3]
    return np.ascontiguousarray(o, F), np.ascontiguousarray(P._pixel_directions(vi, pi, W, H, xs, ys), F)


def _instanced_scene(cornell):
    """Cornell plus three more instances of its largest mesh: one mirrored, one scaled non-uniformly, one only rotated."""
    from vkrt_amd.flat_scene import NODE_DTYPE

    flat = copy.copy(cornell)
    m = int(np.argmax(cornell.prim_meshes["indexCount"]))
    src = int(np.nonzero(cornell.nodes["primMesh"] == m)[0][0])
    base = scene_motion._row_major(cornell.nodes[src]["worldMatrix"])
    centre = scene_motion._centre(cornell, src)
    rng = np.random.default_rng(31)
    extra = np.zeros(3, NODE_DTYPE)
    for k, (mirror, scale) in enumerate(((True, False), (False, True), (False, False))):
        extra[k]["worldMatrix"] = scene_motion._col_major(scene_motion._rigid(rng, centre, mirror=mirror, scale=scale) @ base)
        extra[k]["primMesh"] = m
    flat.nodes = np.concatenate([cornell.nodes, extra])
    dets = [np.linalg.det(scene_motion._row_major(n["worldMatrix"])[:3, :3]) for n in extra]
    assert dets[0] < 0 < dets[1] and dets[2] > 0
    return flat


@pytest.fixture(scope="module")
def scenes():
    import atrium
    from vkrt_amd.flat_scene import FlatScene

    cornell = FlatScene.load_npz(os.path.join(ROOT, "tests", "golden", "cornell_flat.npz"))
    textured, info = atrium.build_atrium(20000, seed=4, with_textures=True)
    emissive, info_e = atrium.build_atrium(20000, seed=4, with_textures=True, variant="emissive_mixed_lights")
    assert len(textured.nodes) == 175 and len(textured.textures) > 0
    m = emissive.materials
    assert (m["emissiveTexture"] > -1).any() and (m["normalTexture"] > -1).any() and (m["pbrBaseColorTexture"] > -1).any()
    assert (m["metallicRoughnessTexture"] > -1).any()
    out = {"cornell": (cornell, None), "atrium": (textured, info), "atrium_emissive": (emissive, info_e), "instances": (_instanced_scene(cornell), None)}
    return {k: (flat, info, Reference(flat)) for k, (flat, info) in out.items()}


def _renderer(flat, build="ploc"):
    from vkrt_amd.renderer import Renderer

    return Renderer(flat, device=0, build=build)


def _words(t):
    import torch

    torch.cuda.synchronize()
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def _scene_hits(r, flat, info, n_random=30000, seed=3):
    """hit records of camera rays and of hostile random rays, as one device tensor [N, 8]"""
    import torch

    W, H = 96, 54
    o, d = _camera_rays(W, H, info)
    ro, rd = _hostile_rays(flat, n_random, seed)
    rays = _pack(np.concatenate([o, ro]), np.concatenate([d, rd]), 0.001, 10000.0)
    return r.intersect(rays).buffer


# ---- 1. every field against the CPU references ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "atrium", "atrium_emissive", "instances"])
def test_every_field_equals_the_references(scenes, name):
    flat, info, ref = scenes[name]
    r = _renderer(flat)
    hits = _scene_hits(r, flat, info)
    full = _words(r.surface(hits, material=True).buffer)
    geo = _words(r.surface(hits, material=False).buffer)
    hw = _words(hits)
    want, ok = ref.for_hits(hw, material=True)
    assert ok.mean() > 0.15 and (~ok).any(), ok.mean()  # hits and misses in one batch
    if name == "instances":  # the mirrored, the scaled and the rotated instance are all hit
        inst = hw.view(np.int32)[:, 3]
        n = len(flat.nodes)
        assert all((inst == k).sum() > 20 for k in (n - 3, n - 2, n - 1))
    _assert_records(full, want, f"{name}, GEOMETRY | MATERIAL")
    want_geo, _ = ref.for_hits(hw, material=False)
    _assert_records(geo, want_geo, f"{name}, GEOMETRY")
    # the two calls against each other: the geometry everywhere, the frame wherever no normal texture replaces it, zeros for the rest
    for f in GEOMETRY_FIELDS:
        assert np.array_equal(geo[:, COLUMNS[f]], full[:, COLUMNS[f]]), f
    mats = hw.view(np.int32)[:, 7]
    plain = ok & (flat.materials["normalTexture"][np.maximum(mats, 0)] < 0)
    assert plain.any() or name.startswith("atrium")
    for f in ("shading_normal", "tangent", "binormal"):
        assert np.array_equal(geo[plain][:, COLUMNS[f]], full[plain][:, COLUMNS[f]]), f
    assert np.array_equal(geo[:, COLUMNS["shading_normal"]], geo[:, COLUMNS["normal"]])  # without the tap the frame is the vertex frame
    for f in MATERIAL_FIELDS:
        assert not geo[:, COLUMNS[f]].any(), f
    if name.startswith("atrium"):
        mapped = ok & ~plain
        assert mapped.sum() > 100  # normal-mapped hits exist and their frame differs from the vertex frame
        assert (full[mapped][:, COLUMNS["shading_normal"]] != full[mapped][:, COLUMNS["normal"]]).any()
        assert (full[ok][:, COLUMNS["alpha"]].view(F) > 0).all()
    if name == "atrium_emissive":
        assert (full[ok][:, COLUMNS["emission"]].view(F) > 0).any()
    # the geometric normal stays on the front side of the object-space winding: M a x M b = det(M) M^-T (a x b), so it is the
    # world-space triangle's own normal, turned round where the instance mirrors (an independent float64 statement)
    gn = np.ascontiguousarray(full[ok][:, COLUMNS["geometric_normal"]]).view(F).astype(np.float64)
    tri = hw.view(np.int32)[ok, 6]
    face = np.cross(ref.np.e1[tri], ref.np.e2[tri])
    det = np.array([np.linalg.det(scene_motion._row_major(nd["worldMatrix"])[:3, :3]) for nd in flat.nodes])[hw.view(np.int32)[ok, 3]]
    length = np.linalg.norm(face, axis=1)
    solid = np.isfinite(gn).all(1) & (length > 1e-12)
    assert solid.mean() > 0.99
    cosine = (gn[solid] * face[solid]).sum(1) / length[solid] * np.sign(det[solid])
    assert (cosine > 1.0 - 1e-4).all(), cosine.min()
    if name == "instances":
        assert (det < 0).any() and (det > 0).any()
    assert r.counters()["traversal_faults"] == 0
    r.close()


# ---- 2. the acceptance test: a path tracer made of the three queries renders the oracle's image ------------------------------------
def _query_pathtracer(r, flat, monkeypatch):
    """np_pathtrace.pathtrace_pixels over a scene whose rays are Renderer.intersect / occluded and whose hit shader reads
    Renderer.surface records and calls the C++ oracle's shadeSurface (oracle_py.eval_shade)."""
    import np_pathtrace as P
    import oracle_py
    import torch

    class QueryScene:
        def __init__(self):
            self.flat = flat
            self.rays_closest = self.rays_shadow = 0
            self.surf = None

        def closest(self, o, d, tmin=0.001, tmax=10000.0):
            self.rays_closest += o.shape[0]
            hits = r.intersect(_pack(o, d, tmin, tmax))
            surf = r.surface(hits)  # back to back on one stream, misses included; one synchronise for both
            torch.cuda.current_stream().synchronize()
            b = hits.buffer.cpu().numpy()
            self.surf = surf.buffer.cpu().numpy()
            tri = b.view(np.int32)[:, 6].astype(np.int64)
            assert np.array_equal(self.surf.view(np.int32)[:, 27], (tri >= 0).astype(np.int32))
            return b[:, 0].copy(), b[:, 1].copy(), b[:, 2].copy(), tri

        def occluded(self, o, d, tmin, tmax):
            self.rays_shadow += o.shape[0]
            tmax = np.broadcast_to(np.asarray(tmax, F), (o.shape[0],))
            occ = r.occluded(_pack(o, d, tmin, tmax))  # per-ray tmax in the packed rays
            torch.cuda.current_stream().synchronize()
            return occ.cpu().numpy() != 0

    sc = QueryScene()

    def closest_hit(sc, pc, prd, lanes, tri, u, v, ray_dir):
        """np_pathtrace._closest_hit with hit_attributes / texture / material_inputs read from the vkrt_surface records"""
        S = sc.surf[sc.surf.view(np.int32)[:, 27] == 1]
        n = lanes.shape[0]
        assert S.shape[0] == n
        emits = (prd.depth[lanes] == 0) | prd.isSpecular[lanes]                      # rchit:83: the integrator's rule
        emittance = np.where(emits[:, None], S[:, COLUMNS["emission"]], F(0)).astype(F)
        s1, _ = P.rnd(prd.seed[lanes])
        _, rl = P.rnd(s1)
        li = (rl * F(pc.lightsCount)).astype(np.int64)
        L = sc.flat.lights[np.clip(li, 0, len(sc.flat.lights) - 1)]
        rec = np.zeros((n, 40), F)
        rec[:, 0:3], rec[:, 3:6], rec[:, 6:9] = S[:, COLUMNS["position"]], S[:, COLUMNS["shading_normal"]], S[:, COLUMNS["tangent"]]
        rec[:, 9:12], rec[:, 12:15] = S[:, COLUMNS["binormal"]], ray_dir
        rec[:, 15:18], rec[:, 19], rec[:, 20], rec[:, 21:24] = S[:, COLUMNS["base_color"]], S[:, 15], S[:, 19], emittance
        rec[:, 24:27], rec[:, 27:30], rec[:, 30] = np.asarray(L["position"], F), np.asarray(L["color"], F), L["intensity"].astype(F)
        rec[:, 31] = L["type"].astype(np.int32).view(F)
        bits = np.zeros((n, 4), np.uint32)
        bits[:, 0], bits[:, 1], bits[:, 2], bits[:, 3] = prd.seed[lanes], 1, 1, pc.lightsCount
        rec[:, 32:36] = bits.view(F)
        out = oracle_py.eval_shade(rec)
        prd.hitValue[lanes] = out[:, 0:3]
        prd.rayOrigin[lanes] = out[:, 3:6]
        prd.rayDirection[lanes] = out[:, 6:9]
        prd.weight[lanes] = out[:, 9:12]
        spec = out[:, 12] != 0
        prd.isSpecular[lanes] = spec
        dm = ~spec
        ld, sd = prd.lightDist[lanes], prd.shadowRayDir[lanes]
        ld[dm], sd[dm] = out[dm, 13], out[dm, 14:17]
        prd.lightDist[lanes], prd.shadowRayDir[lanes] = ld, sd
        prd.seed[lanes] = out[:, 17].copy().view(np.uint32)

    monkeypatch.setattr(P, "_closest_hit", closest_hit)
    return sc


ACCEPTANCE = [
    ("cornell", None, 48, 27, 0, 1, 3), ("cornell", None, 48, 27, 2, 2, 5),
    ("atrium", None, 64, 36, 0, 1, 4), ("atrium", None, 64, 36, 3, 2, 6),
    ("atrium_emissive", None, 64, 36, 0, 1, 4), ("atrium_emissive", None, 64, 36, 3, 2, 6),
    ("atrium", 9, 64, 36, 3, 2, 6), ("cornell", 5, 48, 27, 2, 2, 5),
]


@pytest.mark.parametrize("name,move_seed,W,H,frame,samples,depth", ACCEPTANCE)
def test_query_pathtracer_renders_the_oracles_image(scenes, monkeypatch, name, move_seed, W, H, frame, samples, depth):
    import np_pathtrace as P
    import oracle_py
    import torch
    from vkrt_amd.flat_scene import make_push_constants

    flat, info, _ = scenes[name]
    if move_seed is not None:  # every second node of the atrium / every node of Cornell moved: rotation, non-uniform scale, the first mirrored
        nodes = list(range(0, len(flat.nodes), 2)) if name == "atrium" else list(range(len(flat.nodes)))
        flat, mats = scene_motion.moved(flat, nodes, seed=move_seed)
        assert np.linalg.det(scene_motion._row_major(mats[nodes[0]])[:3, :3]) < 0
    cam, vi, pi = _camera(W, H, info)
    pc = make_push_constants(samples=samples, depth=depth, frame=frame, lights_count=len(flat.lights))
    old = np.random.default_rng(3).random((H, W, 4)).astype(F)
    want, cnt = oracle_py.OracleScene(flat).render(pc, cam, W, H, seed=11, image=old.copy())
    r = _renderer(flat)
    own = r.pathtrace(pc, cam, W, H, seed=11, image=torch.as_tensor(old.copy(), device="cuda:0")).cpu().numpy()
    sc = _query_pathtracer(r, flat, monkeypatch)
    ys, xs = np.mgrid[0:H, 0:W]
    got = P.pathtrace_pixels(sc, pc, vi, pi, W, H, 11, xs.ravel(), ys.ravel(), old=old.reshape(-1, 4)).reshape(H, W, 4)
    print(f"{name} moved={move_seed} frame {frame} spp {samples} depth {depth}: closest rays {sc.rays_closest} (oracle {cnt['rays_closest']}), "
          f"shadow rays {sc.rays_shadow} (oracle {cnt['rays_shadow']})")
    same = (got.view(np.uint32) == want.view(np.uint32)).all(2)
    print(f"  pixels bit-identical with the oracle: {int(same.sum())} of {same.size}; max abs difference "
          f"{np.abs(got.astype(np.float64) - want.astype(np.float64)).max():.3e}")
    assert same.all(), np.argwhere(~same)[:5]
    assert np.array_equal(got.view(np.uint32), own.view(np.uint32))
    assert r.counters()["traversal_faults"] == 0
    r.close()


# ---- 3. no tree needed -----------------------------------------------------------------------------------------------------------
def _hand_records(flat, n, seed, extrapolate=True):
    """[n, 8] words: valid (instance, primitive, u, v) drawn over the whole scene, a tenth of them outside their triangle; the fields
    the call does not read (t, prim_mesh, triangle, material) hold rubbish"""
    rng = np.random.default_rng(seed)
    inst = rng.integers(0, len(flat.nodes), n)
    cnt = np.array([int(flat.prim_meshes[int(nd["primMesh"])]["indexCount"]) // 3 for nd in flat.nodes], np.int64)[inst]
    keep = cnt > 0
    inst, cnt = inst[keep], cnt[keep]
    prim = (rng.random(len(inst)) * cnt).astype(np.int64)
    w = rng.dirichlet((1, 1, 1), len(inst))
    u, v = w[:, 1].astype(F), w[:, 2].astype(F)
    if extrapolate:
        far = rng.random(len(inst)) < 0.1
        u[far] = rng.uniform(-2, 3, far.sum()).astype(F)
        v[far] = rng.uniform(-2, 3, far.sum()).astype(F)
    rec = rng.integers(0, 2 ** 32, (len(inst), 8), dtype=np.uint64).astype(np.uint32)
    rec[:, 1], rec[:, 2] = u.view(np.uint32), v.view(np.uint32)
    rec[:, 3], rec[:, 4] = inst.astype(np.int32).view(np.uint32), prim.astype(np.int32).view(np.uint32)
    return rec


@pytest.mark.parametrize("name", ["atrium_emissive", "instances"])
def test_no_tree_through_the_c_abi(scenes, name):
    """vkrt_scene_create, then vkrt_hit_surface on hand-made records: no vkrt_accel_build anywhere."""
    import ctypes as C
    import torch
    from vkrt_amd import abi
    from vkrt_amd.renderer import load_library

    flat, _, ref = scenes[name]
    lib = load_library()
    desc, keep = flat.to_desc()
    h = C.c_void_p()
    assert lib.vkrt_scene_create(C.byref(desc), 0, C.byref(h)) == abi.VKRT_OK
    try:
        rec = _hand_records(flat, 20000, seed=41)
        hits = torch.as_tensor(rec.view(np.int32), device="cuda:0")
        out = torch.full((len(rec), 32), -1, dtype=torch.int32, device="cuda:0")
        st = torch.cuda.current_stream().cuda_stream
        for material in (True, False):
            fields = abi.VKRT_SURFACE_GEOMETRY | (abi.VKRT_SURFACE_MATERIAL if material else 0)
            assert lib.vkrt_hit_surface(h, hits.data_ptr(), len(rec), fields, out.data_ptr(), st) == abi.VKRT_OK, lib.vkrt_last_error()
            want, ok = ref.for_hits(rec, material)
            assert ok.all()
            _assert_records(_words(out), want, f"{name} before any build, material={material}")
        # the refusals on a live handle, in the documented order; and an intersect on the same handle has no tree
        bad = abi.VKRT_ERR_INVALID_ARGUMENT
        assert lib.vkrt_hit_surface(h, None, 4, 99, out.data_ptr(), st) == bad and b"NULL" in lib.vkrt_last_error()
        assert lib.vkrt_hit_surface(h, hits.data_ptr() + 4, 4, 99, out.data_ptr(), st) == bad and b"misaligned" in lib.vkrt_last_error()
        assert lib.vkrt_hit_surface(h, hits.data_ptr(), 4, abi.VKRT_SURFACE_MATERIAL, out.data_ptr(), st) == bad and b"fields" in lib.vkrt_last_error()
        assert lib.vkrt_hit_surface(h, None, 0, 0, None, st) == bad
        assert lib.vkrt_hit_surface(h, None, 0, abi.VKRT_SURFACE_GEOMETRY, None, st) == abi.VKRT_OK
        rays = torch.zeros((4, 8), device="cuda:0")
        assert lib.vkrt_intersect(h, rays.data_ptr(), 4, 0, out.data_ptr(), st) == abi.VKRT_ERR_NOT_BUILT
        cnt = abi.Counters()
        assert lib.vkrt_counters_read(h, C.byref(cnt)) == abi.VKRT_OK
        assert all(v == 0 for v in cnt.as_dict().values()), cnt.as_dict()  # no counter moves
    finally:
        torch.cuda.synchronize()
        lib.vkrt_scene_destroy(h)
    del keep


def test_surface_points_follow_motion_and_deformation_without_a_refit(scenes):
    import torch
    from vkrt_amd.renderer import VkrtError

    flat, info, _ = scenes["atrium"]
    r = _renderer(flat)
    hits = _scene_hits(r, flat, info, n_random=20000, seed=7)
    hw = _words(hits).copy()
    moved, mats = scene_motion.moved(flat, list(range(0, len(flat.nodes), 3)), seed=13)
    meshes = scene_deform.third_of_meshes(flat)
    target = scene_deform.twisted(moved, meshes)
    scene_motion.apply(r, mats)
    scene_deform.send(r, target, meshes)
    with pytest.raises(VkrtError, match=r"\(5\)"):  # VKRT_ERR_NOT_BUILT: the tree is stale
        r.intersect(_pack(np.zeros((4, 3), F), np.ones((4, 3), F), 0.001, 10.0))
    ref = Reference(target)
    for material in (True, False):
        got = _words(r.surface(hits, material=material).buffer)
        want, ok = ref.for_hits(hw, material)
        assert ok.mean() > 0.3
        _assert_records(got, want, f"old hits on moved and deformed arrays, stale tree, material={material}")
    before, _ = scenes["atrium"][2].for_hits(hw, True)
    assert (before[:, COLUMNS["position"]] != want[:, COLUMNS["position"]]).any()  # the points did move
    # after the refit: fresh hits and their surfaces are those of a scene created from the moved and deformed arrays
    r.refit()
    o, d = _hostile_rays(target, 30000, seed=19)
    rays = _pack(o, d, 0.001, 10000.0)
    fresh = _renderer(target)
    h_a, h_b = r.intersect(rays), fresh.intersect(rays)
    s_a, s_b = r.surface(h_a), fresh.surface(h_b)
    wa, wb = _words(h_a.buffer), _words(h_b.buffer)
    assert np.array_equal(wa, wb) and (wa.view(np.int32)[:, 3] >= 0).mean() > 0.15
    assert np.array_equal(_words(s_a.buffer), _words(s_b.buffer))
    want, _ = ref.for_hits(wa, True)
    _assert_records(_words(s_a.buffer), want, "fresh hits after the refit")
    assert r.counters()["traversal_faults"] == 0
    r.close()
    fresh.close()


# ---- 4. records that are not hits -------------------------------------------------------------------------------------------------
def test_records_that_are_not_hits(scenes):
    import torch

    flat, info, ref = scenes["atrium_emissive"]
    r = _renderer(flat)
    r.reset_counters()
    hits = _scene_hits(r, flat, info, n_random=5000, seed=23)
    hw = _words(hits).copy()
    n = len(hw)
    miss = hw.view(np.int32)[:, 3] < 0
    assert miss.sum() > 100 and (~miss).sum() > 1000
    # hand-made bad records at every fifth place, in turn: instance = node_count, primitive = -1, primitive = the mesh's triangle count,
    # u = NaN, v = +inf, instance = INT_MIN, primitive = INT_MAX, u = -inf, v = NaN with a set sign
    good = np.nonzero(~miss)[0]
    slots = good[::5]
    kinds = np.arange(len(slots)) % 9
    i32, f32 = hw.view(np.int32), hw.view(F)
    cnt = ref.tri_count[i32[slots, 3]]
    i32[slots[kinds == 0], 3] = len(flat.nodes)
    i32[slots[kinds == 1], 4] = -1
    i32[slots[kinds == 2], 4] = cnt[kinds == 2]
    f32[slots[kinds == 3], 1] = np.nan
    f32[slots[kinds == 4], 2] = np.inf
    i32[slots[kinds == 5], 3] = -(2 ** 31)
    i32[slots[kinds == 6], 4] = 2 ** 31 - 1
    f32[slots[kinds == 7], 1] = -np.inf
    hw[slots[kinds == 8], 2] = 0xFFC00001
    assert all((kinds == k).sum() > 5 for k in range(9))
    want, ok = ref.for_hits(hw, True)
    assert not ok[slots].any() and not ok[miss].any() and ok.sum() == n - miss.sum() - len(slots)
    dev = torch.as_tensor(hw.view(np.int32), device="cuda:0")
    for material in (True, False):
        got = _words(r.surface(dev, material=material).buffer)
        w, _ = ref.for_hits(hw, material)
        _assert_records(got, w, f"bad records among good ones, material={material}")
        assert np.array_equal(got[~ok], np.tile(_invalid_record(), ((~ok).sum(), 1)))  # all zero, material -1, valid 0
        assert (got[ok][:, 27] == 1).all()
    c = r.counters()
    assert c["traversal_faults"] == 0
    r.close()


# ---- 5. shapes and ordering --------------------------------------------------------------------------------------------------------
def test_shapes_streams_and_out_reuse(scenes):
    import torch

    flat, info, ref = scenes["atrium"]
    r = _renderer(flat)
    o, d = _hostile_rays(flat, 1000, seed=29)
    rays = _pack(o, d, 0.001, 10000.0)
    all_hits = r.intersect(rays).buffer
    hw = _words(all_hits)
    want, _ = ref.for_hits(hw, True)
    for n in (0, 1, 63, 65, 257, 777):  # 777: not a multiple of the wave or of the block
        s = r.surface(all_hits[:n].contiguous())
        assert tuple(s.buffer.shape) == (n, 32) and tuple(s.position.shape) == (n, 3) and tuple(s.texcoord.shape) == (n, 2)
        _assert_records(_words(s.buffer), want[:n], f"n = {n}")
    # a RayHits and its buffer are the same input; an int32 buffer too
    a = _words(r.surface(r.intersect(rays)).buffer)
    b = _words(r.surface(all_hits.view(torch.int32)).buffer)
    assert np.array_equal(a, want) and np.array_equal(b, want)
    # intersect and surface back to back on a stream of their own, one synchronise at the end; nothing before the call touches `out`
    st = torch.cuda.Stream(device="cuda:0")
    big_o, big_d = _hostile_rays(flat, 200000, seed=37)
    big = _pack(big_o, big_d, 0.001, 10000.0)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        hb = torch.empty((len(big_o), 8), dtype=torch.float32, device="cuda:0")
        sb = torch.empty((len(big_o), 32), dtype=torch.float32, device="cuda:0")
    h = r.intersect(big, out=hb, stream=st)
    s = r.surface(h, out=sb, stream=st)
    st.synchronize()
    assert s.buffer.data_ptr() == sb.data_ptr()
    want_big, ok = ref.for_hits(hb.cpu().numpy().view(np.uint32), True)
    _assert_records(sb.cpu().numpy().view(np.uint32), want_big, "intersect -> surface on one stream")
    # out= reuse: a second call overwrites every word of every record, `reserved` and the fields of invalid records included
    sb.view(torch.int32).fill_(0x5A5A5A5A)
    torch.cuda.synchronize()
    r.surface(h, material=False, out=sb)
    want_geo, _ = ref.for_hits(hb.cpu().numpy().view(np.uint32), False)
    got = _words(sb)
    _assert_records(got, want_geo, "second call into the same buffer")
    assert not (got == 0x5A5A5A5A).any() and not got[:, 31].any()
    # named views
    s = r.surface(all_hits)
    w = _words(s.buffer)
    assert np.array_equal(_words(s.valid).view(np.int32), w.view(np.int32)[:, 27]) and np.array_equal(_words(s.material), w[:, 23])
    assert np.array_equal(_words(s.texcoord.contiguous()), w[:, [3, 7]]) and np.array_equal(_words(s.emission.contiguous()), w[:, 28:31])
    assert np.array_equal(_words(s.roughness.contiguous()), w[:, 19]) and np.array_equal(_words(s.alpha.contiguous()), w[:, 11])
    # wrong device / dtype / shape of hits or out never reach the library
    from vkrt_amd.renderer import VkrtError

    for bad in (all_hits.cpu(), all_hits.double(), all_hits[:, :7], all_hits.t()):
        with pytest.raises(VkrtError):
            r.surface(bad)
    for bad_out in (torch.empty((1000, 31), device="cuda:0"), torch.empty((999, 32), device="cuda:0"), torch.empty((1000, 32)),
                    torch.empty((1000, 32), dtype=torch.float64, device="cuda:0")):
        with pytest.raises(VkrtError):
            r.surface(all_hits, out=bad_out)
    assert r.counters()["traversal_faults"] == 0
    r.close()
