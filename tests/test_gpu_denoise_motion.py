"""vkrt_denoise_diffuse_motion on the GPU, on the planes of tests/denoise_motion_planes.py (moving spheres, a still camera and a pan)
and end to end on Cornell with a moving box.

The bars are those of tests/test_gpu_denoise_planes.py, for its reasons: the temporal stage has no expf and equals the float32
restatement (np_denoise_motion.NpMotionDenoiser) bit for bit; the full filter is held to 4 E32(case) against the restatement's float64
twin at every valid pixel of every call, E32 from the two CPU replays and never from GPU output.  tests/test_np_denoise_motion.py shows
E32 <= 5e-5 for every case and that three one-line departures from the motion rule move the result by at least 20 E32.

Measured on an MI355X: the temporal stage is bit-exact in all 24 cases; the full filter's largest error is between 0.87 and 1.06 E32 in
every case (E32 from 1.0e-7 at 1x1 to 3.5e-5 for the still camera at K = 5) and at most 1.1e-6 from the float32 restatement."""
import os
import sys

import numpy as np
import pytest

import denoise_motion_planes as dm
import denoise_planes as dp
from conftest import ROOT, default_camera

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu
F = np.float32
MAIN = dm.SIZES[0]
PLANES = ("color", "position", "normal", "roughMetal", "nrdViewZ", "nrdRadianceHitDist", "prevPosition")


def _cam(view_proj):
    from vkrt_amd import abi

    cam = abi.GlobalUniforms()
    cam.viewProj.m[:] = [float(v) for v in view_proj]
    return cam


def _upload(planes):
    import torch

    return {k: torch.from_numpy(np.ascontiguousarray(planes[k])).to("cuda:0") for k in PLANES if k in planes}


def _run(calls, W, H):
    """one Denoiser over the calls (the motion entry where a call's planes hold prevPosition): outputs as numpy [H,W,4] float32"""
    import torch

    from vkrt_amd.renderer import Denoiser

    dn = Denoiser(0, W, H)
    fill = torch.from_numpy(dm.fill(W, H)).to("cuda:0")
    outs = []
    for c in calls:
        out = dn.denoise(_cam(c["view_proj"]), _upload(c["planes"]), out=fill.clone(), iterations=c["iterations"], max_history=c["max_history"])
        outs.append(out.cpu().numpy())
    dn.close()
    return outs


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_untouched(outs, valids, W, H):
    fill = _bits(dm.fill(W, H))
    for i, (o, v) in enumerate(zip(outs, valids)):
        assert np.array_equal(_bits(o)[~v], fill[~v]), i          # pixels without geometry
        assert np.array_equal(_bits(o)[..., 3], fill[..., 3]), i  # .w


def _differing(outs, want, valids):
    bad = []
    for i, (o, w, v) in enumerate(zip(outs, want, valids)):
        a, b = _bits(o[..., :3][v]), _bits(w[..., :3][v])
        if not np.array_equal(a, b):
            ulp = np.abs(a.astype(np.int64) - b.astype(np.int64))
            bad.append((i, int((ulp > 0).sum()), int(ulp.max())))
    return bad


@pytest.mark.parametrize("max_history", [1, 2, 32])
@pytest.mark.parametrize("pan", [False, True], ids=["still", "pan"])
@pytest.mark.parametrize("W,H", dm.SIZES)
def test_temporal_stage_bit_for_bit(W, H, pan, max_history):
    r = dm.reference(W, H, pan=pan, iterations=0, max_history=max_history)
    outs = _run(r["calls"], W, H)
    _assert_untouched(outs, r["valid"], W, H)
    bad = _differing(outs, r["out32"], r["valid"])
    print(f"temporal {W}x{H} pan {pan} max_history {max_history}: calls that differ (call, values, max ulp): {bad}")
    assert not bad


FULL = {f"still-K{K}": dict(W=MAIN[0], H=MAIN[1], iterations=K) for K in (1, 2, 5)}
FULL["pan-K5"] = dict(W=MAIN[0], H=MAIN[1], pan=True, iterations=5)
FULL.update({f"{W}x{H}-{'pan' if pan else 'still'}-K5": dict(W=W, H=H, pan=pan, iterations=5) for W, H in dm.SIZES[1:] for pan in (False, True)})
FULL["w0-block-K5"] = dict(W=MAIN[0], H=MAIN[1], iterations=5, w0_block=True)
FULL["nan-xp-K5"] = dict(W=MAIN[0], H=MAIN[1], iterations=5, nan_pixel=True)


@pytest.mark.parametrize("name", FULL)
def test_full_filter_within_4_E32_of_the_float64_twin(name):
    kw = FULL[name]
    W, H = kw["W"], kw["H"]
    r = dm.reference(**kw)
    outs = _run(r["calls"], W, H)
    _assert_untouched(outs, r["valid"], W, H)
    err = dp.case_err(outs, r["out64"], r["valid"])
    vs32 = dp.case_err(outs, r["out32"], r["valid"])
    print(f"full {name}: E32 {r['E32']:.3e}  GPU vs float64 twin max {max(err):.3e} = {max(err) / r['E32']:.2f} E32; GPU vs float32 restatement "
          f"max {max(vs32):.3e}")
    assert all(np.isfinite(o[..., :3][v]).all() for o, v in zip(outs, r["valid"]))
    assert max(err) <= 4 * r["E32"]


@pytest.mark.parametrize("iterations", [0, 5])
def test_motion_call_with_prev_equal_position_is_the_plain_call(iterations):
    """Two handles over denoise_planes' twelve-call main case (pan, still frames, a dolly back, a jump, a reset): the motion call with
    prevPosition = position (w = 1 on geometry) against the plain call, bit for bit in every call."""
    import np_denoise as nd
    import torch

    from vkrt_amd.renderer import Denoiser

    W, H = MAIN
    r = dp.reference(W, H, iterations=iterations)
    a, b = Denoiser(0, W, H), Denoiser(0, W, H)
    fill = torch.from_numpy(dp.fill(W, H)).to("cuda:0")
    for i, c in enumerate(r["calls"]):
        if c["reset"]:
            a.reset()
            b.reset()
        g = _upload(c["planes"])
        plain = a.denoise(_cam(c["view_proj"]), g, out=fill.clone(), iterations=iterations).cpu().numpy()
        prev = c["planes"]["position"].copy()
        prev[..., 3] = np.where(nd.geom_valid(c["planes"]["position"], c["planes"]["normal"]), F(1), prev[..., 3])
        g["prevPosition"] = torch.from_numpy(prev).to("cuda:0")
        moved = b.denoise(_cam(c["view_proj"]), g, out=fill.clone(), iterations=iterations).cpu().numpy()
        assert np.array_equal(_bits(plain), _bits(moved)), i
    a.close()
    b.close()


def test_the_two_calls_mix_on_one_handle():
    """calls alternate between the entries on one handle (prev = position): the outputs are those of a handle that takes the plain
    entry throughout"""
    W, H = MAIN
    calls = dm.case(W, H, iterations=2, static_prev=True)[:6]
    mixed = [c if i % 2 else dm.without_motion([c])[0] for i, c in enumerate(calls)]
    a = _run(mixed, W, H)
    b = _run(dm.without_motion(calls), W, H)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(_bits(x), _bits(y)), i


@pytest.mark.parametrize("kw,first", [(dict(w0_block=True), 3), (dict(nan_pixel=True), 2)], ids=["w0", "nan"])
def test_marked_pixels_behave_as_in_the_restatement(kw, first):
    """prevPosition.w == 0 on a block of the unit sphere, a NaN Xp at one of its pixels: temporal stage bit for bit, so those pixels
    hold their own sample alone (history length 1 in the restatement) while the same pixels of the unmarked case hold a blend"""
    W, H = MAIN
    r = dm.reference(W, H, iterations=0, **kw)
    base = dm.reference(W, H, iterations=0)
    outs = _run(r["calls"], W, H)
    assert not _differing(outs, r["out32"], r["valid"])
    for i in range(first, dm.FRAMES):
        p = r["calls"][i]["planes"]["prevPosition"]
        marked = (r["calls"][i]["planes"]["object"] == 0) & ((p[..., 3] == 0) | ~np.isfinite(p[..., :3]).all(-1))
        assert marked.any() and np.all(r["lengths"][i][marked] == 1)
        assert np.isfinite(outs[i]).all()
        assert not np.array_equal(_bits(outs[i][marked]), _bits(base["out32"][i][marked]))


# ---- end to end: Cornell, one box translated between frames -------------------------------------------------------------------------------
def _view_matrix(eye, center):
    import camera_np

    return np.asarray(camera_np.look_at(eye, center, (0, 1, 0)), F).T.reshape(-1).copy()


@pytest.mark.parametrize("iterations", [0, 5])
def test_cornell_with_a_moving_box_end_to_end(cornell_flat, iterations):
    """Six frames of motion_mark -> update_nodes -> refit -> gbuffer_raycast(motion=True) -> hybrid_trace (GI, depth 2) -> Denoiser.
    The box's translation (0.03, 0.02, 0.05) per frame has a component along the normals of each of its visible faces (top +y, front
    +z, a side +-x), so without the previous positions the plane test would reject the box's history.  K = 0: the output equals
    NpMotionDenoiser on the downloaded planes bit for bit, and the box's pixels reach a history longer than 1.  K = 5: finite."""
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Denoiser, Renderer

    from np_denoise_motion import NpMotionDenoiser

    W, H = 64, 36
    L = len(cornell_flat.lights)
    eye, center = (0.0, 0.0, 15.0), (0.0, 0.0, 0.0)
    cam = default_camera(W, H, eye=eye, center=center)
    vm = _view_matrix(eye, center)
    node = len(cornell_flat.nodes) - 1
    base = np.array(cornell_flat.nodes[node]["worldMatrix"], F)
    r = Renderer(cornell_flat, device=0, build="ploc")
    dn = Denoiser(0, W, H)
    ref = NpMotionDenoiser(W, H)
    for f in range(6):
        r.motion_mark()
        m = base.copy()
        m[12:15] += F(f) * np.array([0.03, 0.02, 0.05], F)  # column-major: the translation
        r.update_nodes(node, m[None])
        r.refit()
        g = r.gbuffer_raycast(cam, W, H, lights_count=L, view_matrix=vm, motion=True)
        pc = make_push_constants(samples=1, depth=2, frame=0, lights_count=L)
        pc.useShadows, pc.useAO, pc.useGI = 1, 1, 1
        acc = r.hybrid_trace(pc, cam, W, H, g, seed=40 + f)
        out = dn.denoise(cam, g, out=acc.clone(), iterations=iterations).cpu().numpy()
        planes = {k: v.cpu().numpy() for k, v in g.items()}
        box = planes["hits"].view(np.int32)[..., 3] == node
        assert box.sum() > 20
        if f >= 1:  # (frame 0 sets the node's own matrix again: nothing has moved yet)
            moved = np.abs(planes["prevPosition"][..., :3] - planes["position"][..., :3]).max(-1)
            assert np.all(moved[box] > 0.01) and np.all(moved[~box] == 0)
        if iterations == 0:
            want = ref.denoise(np.asarray(cam.viewProj.m[:], F), planes, out=acc.cpu().numpy().copy(), iterations=0)
            assert np.array_equal(_bits(out), _bits(want)), f
            if f >= 1:
                assert np.median(ref.mom[..., 2][box]) >= 2, f
        else:
            assert np.isfinite(out[..., :3][box]).all() and np.isfinite(out[..., :3]).all()
    dn.close()
    r.close()
