"""vkrt_hybrid_trace_nrd and vkrt_post on the synthetic G-buffer planes of tests/hybrid_planes.py, pixel by pixel against the oracle.

The whole-frame comparisons of tests/test_hybrid.py feed the pass the planes vkrt_gbuffer_raycast has just made (unit normals that
face the camera, points on a surface, a handful of materials, lights metres away, tiles all shaded or all sky) and excuse a share of
pixels.  Here the planes are a caller's own (kinds, tile layouts and cases: tests/hybrid_planes.py; that they reach every branch of
k_hybrid, k_hy_gi_init / k_wf_shade_hybrid and csrc/hybrid_gi.h is shown on the CPU by tests/test_hybrid_planes.py) and no pixel is
excused.  Every case runs through four instantiations: the defaults (work sharing, GI on the wavefront streams), VKRT_OPT_MODE 0 (GI
inside k_hybrid), VKRT_OPT_WF_SHARE 0 and VKRT_OPT_BVH_LAYOUT 0.

Bars, at every pixel of every non-degenerate case:
  accum               word for word the oracle's (a NaN's sign and payload folded, as tests/test_gpu_shade_records.py does).
  counters            rays_closest, rays_shadow and pixels equal the oracle's; traversal_faults == 0.
  nrdRadianceHitDist  where GI ran (shaded, useGI): .xyz word for word (no transcendental is involved); .w word for word or the
                      adjacent binary16 value -- the two sides differ in exp2f's last bits only, a few 1e-7 relative against a
                      binary16 step of 5e-4, so a pixel can at most straddle one rounding boundary -- and word for word where the
                      roughness is 0 or 1 (the argument of exp2f is an integer, its result exact).
                      Everywhere else: the words the caller left there (hp.prefill).  include/vkrt.h says "0 where GI did not run"; that
                      describes the pair of calls (vkrt_gbuffer_raycast_nrd clears the plane, as does oracle_py.hybrid_nrd, which hands
                      zeros in) -- vkrt_hybrid_trace_nrd itself writes GI pixels only and leaves the caller's words alone.
  instantiations      agree with one another word for word in both planes, .w included.
  sharded case        the selected rows of the unsharded result.
VKRT_HYBRID_PARITY_JSON=<file>: the measured counts go there (how profiles/hybrid_planes_parity.json was taken)."""
import functools
import json
import os

import numpy as np
import pytest

import hybrid_planes as hp

F = np.float32
INSTANTIATIONS = ("default", "mode0", "noshare", "bvh2")


def _options(inst, dissolve=False):
    from vkrt_amd import abi

    o = {"default": {}, "mode0": {abi.VKRT_OPT_MODE: 0}, "noshare": {abi.VKRT_OPT_WF_SHARE: 0}, "bvh2": {abi.VKRT_OPT_BVH_LAYOUT: 0}}[inst]
    return {**o, abi.VKRT_OPT_ANYHIT_DISSOLVE: 1} if dissolve else o


_RENDERERS = {}


def _renderer(scene, inst, dissolve=False):
    from vkrt_amd.renderer import Renderer

    key = (scene, inst, dissolve)
    if key not in _RENDERERS:
        _RENDERERS[key] = Renderer(hp.scene(scene, dissolve)[0], device=0, options=_options(inst, dissolve) or None)
    return _RENDERERS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_renderers():
    yield
    for r in _RENDERERS.values():
        r.close()
    _RENDERERS.clear()


def _gpu(call):
    """A HIP error ends the session: nothing more is started on a card that has faulted."""
    try:
        return call()
    except RuntimeError as e:
        pytest.exit(f"GPU call failed, nothing more is run: {e}", returncode=3)


@functools.lru_cache(maxsize=None)
def _result(name, inst, shard=None, dissolve=False):
    """One vkrt_hybrid_trace_nrd call: dict accum, rad (numpy), counters.  shard: (strip rows, count, index)."""
    import torch

    from vkrt_amd import abi

    c = hp.CASES[name]
    W, H = c["size"]
    g, _ = hp.planes(name)
    rows = np.arange(H) if shard is None else np.array([y for y in range(H) if (y // shard[0]) % shard[1] == shard[2]])
    r = _renderer(c["scene"], inst, dissolve)
    pc = hp.push_constants(name)

    def run():
        dev = {k: torch.from_numpy(np.ascontiguousarray(v[rows])).to("cuda:0") for k, v in g.items()}
        dev["nrdRadianceHitDist"] = torch.from_numpy(np.ascontiguousarray(hp.prefill(W, H)[rows])).to("cuda:0")
        old = hp.old_accum(name) if pc.frame > 0 else np.full((H, W, 4), 7.0, F)  # (frame 0 overwrites whatever is there)
        accum = torch.from_numpy(np.ascontiguousarray(old[rows])).to("cuda:0")
        r.reset_counters()
        r.hybrid_trace(pc, hp.camera(c["scene"], W, H), W, H, dev, seed=c["seed"], flags=c["row_major"], accum=accum,
                       shard=None if shard is None else abi.Shard(W, H, *shard))
        torch.cuda.synchronize()
        return dict(accum=accum.cpu().numpy(), rad=dev["nrdRadianceHitDist"].cpu().numpy(), counters=r.counters())

    return _gpu(run)


def _record(key, entry):
    path = os.environ.get("VKRT_HYBRID_PARITY_JSON")
    if not path:
        return
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = entry
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


def _compare(got, ref, rows=None, mask=None):
    """Differences of one result against the oracle over the pixels of mask (default: all): dict of pixel masks"""
    sel = (lambda a: a) if rows is None else (lambda a: a[rows])
    g, meta = {k: sel(v) for k, v in ref["g"].items()}, {k: sel(v) for k, v in ref["meta"].items()}
    gi, want_acc, want_rad = sel(ref["gi"]), sel(ref["accum"]), sel(ref["rad"])
    H, W = gi.shape
    mask = np.ones((H, W), bool) if mask is None else sel(mask)
    fill = sel(hp.prefill(*ref["accum"].shape[1::-1]))
    d = {}
    d["accum"] = np.any(hp.bits(got["accum"]) != hp.bits(want_acc), -1) & mask
    d["rad_xyz"] = np.any(hp.bits(got["rad"][..., :3]) != hp.bits(want_rad[..., :3]), -1) & gi & mask
    w_got, w_want = got["rad"][..., 3], want_rad[..., 3]
    same = hp.bits(w_got) == hp.bits(w_want)
    with np.errstate(invalid="ignore"):
        near = hp.half_neighbours(np.nan_to_num(w_got), np.nan_to_num(w_want)) & ~np.isnan(w_got) & ~np.isnan(w_want)
    exact_rough = (g["roughMetal"][..., 0] == 0) | (g["roughMetal"][..., 0] == 1)
    d["rad_w_neighbour"] = ~same & near & gi & mask                                # allowed, counted
    d["rad_w"] = ~same & (~near | exact_rough) & gi & mask                          # not allowed
    d["untouched"] = np.any(got["rad"].view(np.uint32) != fill.view(np.uint32), -1) & ~gi & mask
    return d, meta


def _check(key, got, ref, rows=None, mask=None, counters=True):
    d, meta = _compare(got, ref, rows, mask)
    entry = {k: hp.by_kind(v, meta) for k, v in d.items()}
    entry["pixels"] = int(d["accum"].size)
    c = got["counters"]
    if counters:
        entry["counters"] = {k: [int(c[k]), int(ref["counters"][k])] for k in ("rays_closest", "rays_shadow", "pixels")}
    entry["traversal_faults"] = int(c["traversal_faults"])
    print(key, entry)
    _record(key, entry)
    for k in ("accum", "rad_xyz", "rad_w", "untouched"):
        assert not d[k].any(), (key, k, entry[k], list(zip(*np.nonzero(d[k])))[:5])
    assert c["traversal_faults"] == 0
    if counters:
        for k in ("rays_closest", "rays_shadow", "pixels"):
            assert c[k] == ref["counters"][k], (key, k, c[k], ref["counters"][k])


@pytest.mark.gpu
@pytest.mark.parametrize("inst", INSTANTIATIONS)
@pytest.mark.parametrize("name", hp.NON_DEGENERATE)
def test_every_pixel_is_the_oracles(name, inst):
    _check(f"{name}/{inst}", _result(name, inst), hp.reference(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", hp.CASES)
def test_instantiations_agree_word_for_word(name):
    """the degenerate case included: whatever a NaN does, it does the same in the four kernels"""
    base = _result(name, INSTANTIATIONS[0])
    for inst in INSTANTIATIONS[1:]:
        other = _result(name, inst)
        for k in ("accum", "rad"):
            assert np.array_equal(hp.bits(base[k]), hp.bits(other[k])), (name, inst, k)


@pytest.mark.gpu
@pytest.mark.parametrize("inst", INSTANTIATIONS)
def test_sharded_case_is_the_rows_of_the_whole_frame(inst):
    name, shard = hp.SHARDED
    H = hp.CASES[name]["size"][1]
    rows = np.array([y for y in range(H) if (y // shard[0]) % shard[1] == shard[2]])
    part, whole = _result(name, inst, shard=shard), _result(name, inst)
    assert part["accum"].shape[0] == len(rows) and 0 < len(rows) < H
    for k in ("accum", "rad"):
        assert np.array_equal(hp.bits(part[k]), hp.bits(whole[k][rows])), k
    _check(f"{name}/{inst}/shard", part, hp.reference(name), rows=rows, counters=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", hp.DISSOLVE)
def test_dissolve_stage_sees_the_pixels_seed(name):
    """VKRT_OPT_ANYHIT_DISSOLVE against the oracle's set_dissolve: the stage draws from the pixel's seed inside the walk, so it is
    sensitive to which lane traced which ray (work sharing, triangle lending)."""
    ref, opaque = hp.reference(name, dissolve=True), hp.reference(name)
    assert np.mean(np.any(hp.bits(ref["accum"]) != hp.bits(opaque["accum"]), -1)) > 0.02  # the stage is on
    _check(f"{name}/dissolve", _result(name, "default", dissolve=True), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("inst", INSTANTIATIONS)
def test_degenerate_pixels_do_no_harm(inst):
    """A NaN or infinity in a position, normal, roughness or viewZ, the position exactly at the light, a zero normal with a non-zero
    position: the call succeeds, traversal_faults == 0, every other pixel of the frame holds the oracle's bits and a degenerate pixel has
    its NaNs where the oracle has them.

    Why the walks end for such rays (read in hyTrace, traverse_share.h, traverse_wide.h, traverse.h before this case first ran).  A
    degenerate pixel gives a ray with NaN in its origin or direction (normalize of a zero or NaN vector; createCoordinateSystem of a
    zero normal) or with tmax < tmin or tmax = NaN (lightDistance - 0.1 at the light).  (1) No address comes from a ray: child and
    triangle indices are read from the node (G.x + popc(...), T.x + bit index), a ray only decides, by comparisons, which bits of a
    node's hit mask are set; the light index comes from rnd() * lightsCount, not from the planes.  (2) Every comparison with a NaN is
    false: `tn <= tf` rejects a child whose slab bounds are NaN (fmaxf / fminf drop a NaN operand, so an axis with a NaN is ignored and
    the other axes decide; with every axis NaN the root is rejected), tr.hit(...) && t > tmin and t < tmax accept no triangle, so such a
    ray is a miss, as in the oracle.  With tmax <= tmin no t passes t > tmin && t < tmax; the children of the root are rejected at once
    where tmin > tmax (1 + 8e-5), otherwise the walk is an ordinary one that accepts nothing.  (3) A walk
    visits a node at most once per ray -- a child's bit is cleared when it is taken, a group leaves the stack when it is popped or given
    away -- so even a ray that is let into every box ends after nodes + triangles steps; the loops also count down sc.stepLimit
    = 4 (nodes + triangles) + 64 and a full stack drops the push, both as a counted traversal fault, never as a write past the stack.
    (4) The sharing wave ends when no lane is busy; adopting needs a donor with pending work, of which there is a finite amount.
    tests/test_gpu_ray_query.py::test_degenerate_rays_are_misses_without_faults relies on the same properties for k_query."""
    name = "degenerate"
    ref = hp.reference(name)
    got = _result(name, inst)
    bad = ref["meta"]["degenerate"]
    assert bad.sum() >= 100
    _check(f"{name}/{inst}", got, ref, mask=~bad, counters=False)
    assert np.array_equal(np.isnan(got["accum"][bad]), np.isnan(ref["accum"][bad]))
    assert np.array_equal(np.isnan(got["rad"][bad & ref["gi"]]), np.isnan(ref["rad"][bad & ref["gi"]]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("arm", hp.POST_ARMS)
def test_post_arms_against_float64(arm, n):
    """k_post's six (rtMode, viewAccumulated, useGI) arms on zeros, negatives, infinities and values up to 1e4, below and past one
    256-thread block: 2e-5 relative + 1e-6 absolute against float64 pow, NaN at exactly the reference's texels"""
    import torch

    m, r = hp.post_inputs(n)
    rnd = _renderer("cornell", "default")
    out = _gpu(lambda: rnd.post(torch.from_numpy(m).to("cuda:0"), torch.from_numpy(r).to("cuda:0"), *arm).cpu().numpy())
    hp.assert_post(out, hp.post_float64(m, r, *arm))


@pytest.mark.gpu
def test_post_without_a_ray_traced_image():
    """rt_img = NULL with rtMode 1 (the path tracer's pass-through): the gamma alone"""
    import torch

    m, r = hp.post_inputs(257)
    rnd = _renderer("cornell", "default")
    out = _gpu(lambda: rnd.post(torch.from_numpy(m).to("cuda:0"), None, rt_mode=1).cpu().numpy())
    hp.assert_post(out, hp.post_float64(m, r, 1, 0, 0))
