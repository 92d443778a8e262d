"""The hit shader's BRDF tail (csrc/shade.h closestHitLobe + closestHitTail) against the oracle, bit for bit.

Record by record: vkrt_debug_eval_shade runs the two functions of the frame kernels on the strata of tests/shade_records.py -- materials
at and beyond the clamps, grazing and below-surface views, lights in the plane / behind / a hair away / at the hit point, every light
type, extreme PRNG draws, degenerate shading frames -- and words 0 to 17 of every record must be the oracle's (orc_eval_shade).  The
arithmetic profile (-ffp-contract=off, the shared sin / cos / pow5) makes the two the same sequence of binary32 operations, so there is
no tolerance; only a NaN's sign and payload, which IEEE leaves open, are folded to one pattern.

Frame by frame: a material chart -- a floor, a 5 x 5 grid of quads with metallic x roughness from {0, 0.01, 0.5, 0.99, 1} x
{0, 0.01, 0.3, 0.99, 1}, one emissive quad, a point light and lights of type 1 and 2, seen from a low camera so that the far rows are
near grazing -- rendered by every frame pipeline that calls the tail, must equal the oracle's render in image bits and ray counters;
the hybrid frame with GI equals the oracle's hybrid frame as tests/test_hybrid.py compares the two."""
import os

import numpy as np
import pytest

import shade_records as sr
from conftest import default_camera

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
RAYS = ("rays_closest", "rays_shadow", "pixels")
CHART_METALLIC = (0.0, 0.01, 0.5, 0.99, 1.0)
CHART_ROUGHNESS = (0.0, 0.01, 0.3, 0.99, 1.0)
W, H = 96, 64
EYE = (0.2, 1.0, 3.5)  # low over the chart: the far row is seen at N.V < 0.2


def _bits(x):
    """float words as uint32 with every NaN folded to one pattern (the sign and payload of a produced NaN are not pinned by IEEE)"""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32).copy()
    nan = (bits & 0x7FFFFFFF) > 0x7F800000
    bits[nan] = 0x7FC00000
    return bits


def _assert_same_rows(got, want, what):
    g, w = _bits(got[:, :18]), _bits(want[:, :18])
    bad = g != w
    assert not bad.any(), (f"{what}: {int(bad.sum())} words differ in {int(bad.any(1).sum())} of {len(g)} records, first (record, word) "
                           f"{np.argwhere(bad)[:4].tolist()}: {got[:, :18][bad][:4]} vs {want[:, :18][bad][:4]}")
    assert np.all(got[:, 18:20] == 0), what


@pytest.mark.parametrize("name", sr.STRATA)
def test_every_record_equals_the_oracle_bit_for_bit(name):
    from vkrt_amd.renderer import eval_shade

    rec, want, _, _ = sr.evaluate(name)
    got = eval_shade(rec)
    assert got.shape == want.shape == (rec.shape[0], 20)
    _assert_same_rows(got, want, name)
    if name == "light":  # the stratum does reach the non-finite outputs, on the device too
        assert np.isnan(got[:, 0:3]).any() and not np.isfinite(want[:, :17]).all()


def test_small_batches_give_the_rows_of_the_big_batch():
    """n = 1, 63, 64, 65, 255, 257: one thread short of, at and past the wave and the 256-thread block (the grid's tail guard)."""
    from vkrt_amd.renderer import eval_shade

    rec, want, _, _ = sr.evaluate("default")
    for n in (1, 63, 64, 65, 255, 257):
        _assert_same_rows(eval_shade(rec[:n]), want[:n], f"first {n}")
        _assert_same_rows(eval_shade(rec[1000:1000 + n]), want[1000:1000 + n], f"{n} from 1000")


def test_lights_count_outside_1_to_16_is_refused():
    from vkrt_amd.renderer import VkrtError, eval_shade

    rec = sr.records("default")[:8].copy()
    for bad in (0, 17, -1):
        rec[5, 35] = np.array([bad], np.int32).view(np.float32)[0]
        with pytest.raises(VkrtError, match="lightsCount"):
            eval_shade(rec)
    assert eval_shade(rec[:0]).shape == (0, 20)


# ---- the material chart ---------------------------------------------------------------------------------------------------------------
def _quad(p0, ex, ey):
    """two triangles of the parallelogram p0, p0 + ex, p0 + ex + ey, p0 + ey"""
    p0, ex, ey = (np.asarray(v, np.float64) for v in (p0, ex, ey))
    return np.array([p0, p0 + ex, p0 + ex + ey, p0, p0 + ex + ey, p0 + ey], np.float32)


def _chart_scene():
    """One instance and one material per quad, in the style of _triangle_scene of tests/test_gpu_bvh_bounds.py: the floor (material 0),
    the 25 chart quads (1 + 5 row + column: metallic by row, far rows last; roughness by column) and the emissive panel (26)."""
    from vkrt_amd.flat_scene import LIGHT_DTYPE, MAT_DTYPE, NODE_DTYPE, PRIM_DTYPE, FlatScene

    quads = [(_quad((-8, 0, 8), (16, 0, 0), (0, 0, -20)), (0, 1, 0))]
    for row in range(5):
        for col in range(5):
            quads.append((_quad((-2.5 + col + 0.1, 0.05, 2.5 - row - 0.1), (0.8, 0, 0), (0, 0, -0.8)), (0, 1, 0)))
    quads.append((_quad((-1.5, 0.0, -3.2), (3, 0, 0), (0, 1.2, 0)), (0, 0, 1)))
    n = len(quads)
    pos = np.concatenate([q for q, _ in quads])
    nrm = np.concatenate([np.tile(np.array(nv, np.float32), (6, 1)) for _, nv in quads])
    pm = np.zeros(n, PRIM_DTYPE)
    nodes = np.zeros(n, NODE_DTYPE)
    mats = np.zeros(n, MAT_DTYPE)
    for k in range(n):
        pm[k] = (6 * k, 6, 0, 6 * n, k)
        nodes[k]["worldMatrix"] = np.eye(4, dtype=np.float32).ravel()
        nodes[k]["primMesh"] = k
        mats[k]["pbrBaseColorTexture"] = mats[k]["metallicRoughnessTexture"] = mats[k]["normalTexture"] = mats[k]["emissiveTexture"] = -1
    mats[0]["pbrBaseColorFactor"] = [0.6, 0.6, 0.6, 1.0]
    mats[0]["roughnessFactor"] = 1.0
    for row, metal in enumerate(CHART_METALLIC):
        for col, rough in enumerate(CHART_ROUGHNESS):
            m = mats[1 + 5 * row + col]
            m["pbrBaseColorFactor"] = [0.9, 0.55 + 0.08 * col, 0.2 + 0.15 * row, 1.0]
            m["metallicFactor"], m["roughnessFactor"] = metal, rough
    mats[n - 1]["pbrBaseColorFactor"] = [0.3, 0.3, 0.3, 1.0]
    mats[n - 1]["roughnessFactor"] = 0.5
    mats[n - 1]["emissiveFactor"] = [2.0, 1.5, 1.0]
    lights = np.zeros(3, LIGHT_DTYPE)
    lights[0] = ((0.3, 3.0, 1.0), (1.0, 0.95, 0.9), 30.0, 0)
    lights[1] = ((2.0, 2.0, 0.0), (1.0, 1.0, 1.0), 20.0, 1)
    lights[2] = ((-2.0, 2.5, -1.0), (0.5, 0.7, 1.0), 20.0, 2)
    m = pos.shape[0]
    return FlatScene(pos, nrm, np.tile(np.array([1, 0, 0, 1], np.float32), (m, 1)), np.zeros((m, 2), np.float32), np.arange(m, dtype=np.uint32),
                     pm, mats, lights, nodes, [])


@pytest.fixture(scope="module")
def chart():
    """(scene, camera, push constants, the oracle's image and counters): 96 x 64, 4 spp, depth 5, rendered once"""
    import oracle_py
    from vkrt_amd.flat_scene import make_push_constants

    flat = _chart_scene()
    cam = default_camera(W, H, eye=EYE, center=(0.0, 0.0, 0.0))
    pc = make_push_constants(samples=4, depth=5, frame=0, lights_count=len(flat.lights))
    orc = oracle_py.OracleScene(flat)
    ref, cref = orc.render(pc, cam, W, H, seed=9, threads=THREADS)
    return flat, cam, pc, orc, ref, cref


def test_chart_shows_every_material_and_a_grazing_far_row(chart):
    """What the frame tests rely on: the camera sees all 27 materials, the far row at N.V below 0.2, and the oracle's paths take both
    lobes and reach the lights (shadow rays are traced for diffuse hits only)."""
    flat, cam, pc, orc, ref, cref = chart
    g = orc.gbuffer(cam, W, H, lights_count=3, threads=THREADS)
    p = g["position"][..., :3]
    on_chart = (np.abs(p[..., 1] - 0.05) < 1e-4)
    cells = set(zip(np.floor(p[on_chart][:, 0] + 2.5).astype(int).tolist(), np.floor(2.5 - p[on_chart][:, 2]).astype(int).tolist()))
    assert cells >= {(c, r) for c in range(5) for r in range(5)}
    assert np.any(np.abs(p[..., 2] + 3.2) < 1e-4) and np.any(np.abs(p[..., 1]) < 1e-6)  # the emissive panel and the floor
    far = on_chart & (p[..., 2] < -1.5)
    v = np.array(EYE) - p[far]
    assert far.sum() > 50 and np.all(v[:, 1] / np.linalg.norm(v, axis=1) < 0.2)
    assert np.isfinite(ref).all() and cref["pixels"] == W * H and 0 < cref["rays_shadow"] < cref["rays_closest"]


def _options():
    from vkrt_amd import abi

    return {"wavefront": {}, "record_camera_rounds": {abi.VKRT_OPT_WF_CAMERA_ROUNDS: 0}, "no_sample_sync": {abi.VKRT_OPT_WF_SAMPLE_SYNC: 0},
            "megakernel": {abi.VKRT_OPT_MODE: 0}, "bvh2": {abi.VKRT_OPT_BVH_LAYOUT: 0}}


@pytest.mark.parametrize("pipeline", ["wavefront", "record_camera_rounds", "no_sample_sync", "megakernel", "bvh2"])
def test_chart_frame_equals_the_oracle_bit_for_bit(chart, pipeline):
    from vkrt_amd.renderer import Renderer

    flat, cam, pc, _, ref, cref = chart
    r = Renderer(flat, device=0, build="sah", options=_options()[pipeline])
    try:
        r.reset_counters()
        img = r.pathtrace(pc, cam, W, H, seed=9).cpu().numpy()
        c = r.counters()
    finally:
        r.close()
    differ = np.any(_bits(img) != _bits(ref), axis=-1)
    assert not differ.any(), (pipeline, int(differ.sum()), np.argwhere(differ)[:4].tolist())
    assert c["traversal_faults"] == 0
    for k in RAYS:
        assert c[k] == cref[k], (pipeline, k, c[k], cref[k])


def test_chart_hybrid_frame_with_gi_equals_the_oracle(chart):
    """G-buffer and hybrid frame (shadows, AO and GI: hybrid.hip shades the GI hits with closestHitShader) against the oracle's, compared as
    tests/test_hybrid.py compares them."""
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Renderer

    flat, cam, _, orc, _, _ = chart

    def mismatch(a, b):
        return float(np.mean(np.any(_bits(a) != _bits(b), axis=-1)))

    r = Renderer(flat, device=0, build="sah")
    try:
        g = r.gbuffer_raycast(cam, W, H, lights_count=3)
        gref = orc.gbuffer(cam, W, H, lights_count=3, threads=THREADS)
        gnp = {k: v.cpu().numpy() for k, v in g.items()}
        for k in gref:
            assert mismatch(gnp[k], gref[k]) < 1e-4, k
        pc = make_push_constants(samples=1, depth=5, frame=0, lights_count=3)
        pc.useShadows, pc.useAO, pc.useGI = 1, 1, 1
        r.reset_counters()
        out = r.hybrid_trace(pc, cam, W, H, g, seed=21).cpu().numpy()
        c = r.counters()
    finally:
        r.close()
    ref, cref = orc.hybrid(pc, cam, W, H, gnp, seed=21, threads=THREADS)
    assert cref["rays_closest"] > 0
    assert abs(c["rays_shadow"] - cref["rays_shadow"]) <= 8 and abs(c["rays_closest"] - cref["rays_closest"]) <= 8
    assert mismatch(out, ref) < 1e-4
    assert float(np.sqrt(np.mean((out - ref) ** 2))) < 1e-3
