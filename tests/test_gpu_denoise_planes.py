"""vkrt_denoise_diffuse on the synthetic planes of tests/denoise_planes.py, which reach the branches the Cornell pan of
tests/test_gpu_denoise.py does not (the nz < 0 fold of the oct encoding, every arm of dnAlbedo, points behind the previous camera,
a moving 90 degree crease, K and max_history changing per call on one handle, images smaller than a tile).

Two bars.  The temporal stage (iterations = 0) has no expf: its output equals the float32 restatement's bit for bit.  The full
filter is held to 4 E32(case) against the float64 twin of the restatement, at every valid pixel of every call, where E32(case) is
the float32 restatement's own largest error against the twin (dp.rel_err; computed here from the two CPU replays, never from GPU
output).  Why 4: the kernels and the float32 restatement are two binary32 evaluations of one expression tree that differ only in
expf's last bit, so each lies about E32 from the exact value (a factor 2 between them); the other factor 2 is for the maximum over
a few thousand pixels being a noisy statistic.  tests/test_np_denoise.py shows that E32 <= 5e-5 for every case and that each of
sixteen small departures from the formulas moves the result by at least 20 E32.

Measured on an MI355X (profiles/denoise_planes_parity.json): the temporal stage is bit-exact in all twelve cases; the full filter's
largest error is between 0.97 and 1.02 E32 in every case (E32 from 1.3e-7 at 1x1 to 1.9e-5 for the main case at K = 5), and at
most 1.2e-6 from the float32 restatement.  Three device builds with one departure each (B3 corner weight 0.06, six squarings, the
oct fold without its signs) fail the tests listed there, the mildest at 137 E32."""
import json
import os

import numpy as np
import pytest

import denoise_planes as dp

MAIN = dp.SIZES[0]


def _cam(view_proj):
    from vkrt_amd import abi

    cam = abi.GlobalUniforms()
    cam.viewProj.m[:] = [float(v) for v in view_proj]
    return cam


def _upload(planes):
    import torch

    return {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for k, v in planes.items()}


def _run(calls, W, H):
    """one Denoiser over the calls: the outputs as numpy [H,W,4] float32"""
    import torch

    from vkrt_amd.renderer import Denoiser

    dn = Denoiser(0, W, H)
    fill = torch.from_numpy(dp.fill(W, H)).to("cuda:0")
    outs = []
    for c in calls:
        if c["reset"]:
            dn.reset()
        out = dn.denoise(_cam(c["view_proj"]), _upload(c["planes"]), out=fill.clone(), iterations=c["iterations"], max_history=c["max_history"])
        outs.append(out.cpu().numpy())
    dn.close()
    return outs


def _assert_untouched(outs, valids, W, H):
    fill = dp.fill(W, H).view(np.uint32)
    for i, (o, v) in enumerate(zip(outs, valids)):
        assert np.array_equal(o.view(np.uint32)[~v], fill[~v]), i   # pixels without geometry
        assert np.array_equal(o.view(np.uint32)[..., 3], fill[..., 3]), i  # .w


def _record(name, entry):
    """VKRT_DENOISE_PARITY_JSON=<file>: collect the measured figures there (how profiles/denoise_planes_parity.json was taken)"""
    path = os.environ.get("VKRT_DENOISE_PARITY_JSON")
    if not path:
        return
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[name] = entry
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


@pytest.mark.gpu
@pytest.mark.parametrize("max_history", [1, 2, 32])
@pytest.mark.parametrize("W,H", dp.SIZES)
def test_temporal_stage_bit_for_bit(W, H, max_history):
    """k_dn_temporal uses + - * /, sqrtf, floorf, rintf, fminf / fmaxf and conversions only, without contraction: twelve calls of a
    moving camera (still frames, a dolly back, a jump, a reset) give the float32 restatement's bits."""
    r = dp.reference(W, H, iterations=0, max_history=max_history)
    outs = _run(r["calls"], W, H)
    _assert_untouched(outs, r["valid"], W, H)
    differing = []
    for i, (o, want, v) in enumerate(zip(outs, r["out32"], r["valid"])):
        a, b = o[..., :3][v].view(np.uint32), want[..., :3][v].view(np.uint32)
        if not np.array_equal(a, b):
            ulp = np.abs(a.astype(np.int64) - b.astype(np.int64))
            differing.append((i, int((ulp > 0).sum()), int(ulp.max())))
    print(f"temporal {W}x{H} max_history {max_history}: calls that differ (call, values, max ulp): {differing}")
    _record(f"temporal-{W}x{H}-mh{max_history}", dict(differing_calls=differing))
    assert not differing


FULL = {f"main-K{K}": dict(W=MAIN[0], H=MAIN[1], iterations=K) for K in (1, 2, 5)}
FULL["settings"] = dict(W=MAIN[0], H=MAIN[1], settings=True)
FULL.update({f"{W}x{H}-K5": dict(W=W, H=H, iterations=5) for W, H in dp.SIZES[1:]})
FULL["nan-sample"] = dict(W=MAIN[0], H=MAIN[1], nan_frame=5)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FULL)
def test_full_filter_within_4_E32_of_the_float64_twin(name):
    """Every valid pixel of every call, no exemptions.  "settings": K = 5, 0, 1, 5, 2, 0, 0, 3 and max_history = 32, 1, 2, ... on one
    handle (the rotation of the three colour planes).  "nan-sample": one pixel's Y is NaN in call 5; all outputs stay finite and
    within the same bar (it counts as black, as in the restatement).  Figures: profiles/denoise_planes_parity.json."""
    kw = FULL[name]
    W, H = kw["W"], kw["H"]
    r = dp.reference(**kw)
    outs = _run(r["calls"], W, H)
    _assert_untouched(outs, r["valid"], W, H)
    err = dp.case_err(outs, r["out64"], r["valid"])
    vs32 = dp.case_err(outs, r["out32"], r["valid"])
    print(f"full {name}: E32 {r['E32']:.3e}  GPU vs float64 twin max {max(err):.3e} = {max(err) / r['E32']:.2f} E32 (per call "
          f"{[f'{e:.1e}' for e in err]}); GPU vs float32 restatement max {max(vs32):.3e}")
    _record(f"full-{name}", dict(E32=r["E32"], gpu_vs_float64=max(err), gpu_vs_float64_per_call=err, gpu_vs_float32=max(vs32)))
    assert all(np.isfinite(o[..., :3][v]).all() for o, v in zip(outs, r["valid"]))
    assert max(err) <= 4 * r["E32"]


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [0, 5])
def test_reset_equals_a_fresh_handle(iterations):
    """After reset() the next output is, bit for bit, that of a new Denoiser given the same planes: the useHistory = 0 path over
    buffers that hold an earlier sequence."""
    W, H = MAIN
    r = dp.reference(W, H, iterations=iterations)
    assert r["calls"][8]["reset"]
    used = _run(r["calls"][:9], W, H)[8]
    fresh = _run(r["calls"][8:9], W, H)[0]
    assert np.array_equal(used.view(np.uint32), fresh.view(np.uint32))
    kept = _run([r["calls"][7], dict(r["calls"][8], reset=False)], W, H)[1]  # without the reset the history changes the output
    assert not np.array_equal(used, kept)
