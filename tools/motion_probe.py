"""Times the motion entry points on the bench atrium at 1920x1080 and, optionally, measures what they buy: writes
profiles/motion_probe.json.  Medians of --calls calls after --warmup, device events around every call, the variants of a comparison
alternating call by call in one process.

  python tools/motion_probe.py --out profiles/motion_probe.json [--parent-lib /path/to/the/parent/commit's/libvkrt.so] [--quality]

  1  vkrt_gbuffer_raycast_nrd, parent build against this build (--parent-lib: a library built from the parent commit, loaded beside this
     one).  Order per round: parent, branch, parent -- two interleaved series of the parent itself, whose spread is the bar for the branch
  2  vkrt_gbuffer_raycast_hits against 1
  3  vkrt_scene_motion_mark (after the first, allocating call)
  4  vkrt_hit_motion over the frame's records, both outputs; bytes moved over time as a share of the HBM peak
  5  vkrt_denoise_diffuse_motion against vkrt_denoise_diffuse (two handles, the same planes)
  6  --quality: 16 frames, a third of the instances translating, still camera, K = 5: per frame the RMSE of the denoised GI term against
     the mean of --ref-frames clamped 1-path frames of that frame, over mover pixels and over static pixels, with and without motion
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md
W, H = 1920, 1080
# vkrt_hit_motion per record: the record (32 B), two outputs (16 B each), three indices (12 B), three vertexPN quads (48 B), three snapshot
# positions (36 B), three rows of the live and of the snapshot instance record (96 B), primMesh word + table entry (20 B)
HIT_MOTION_STREAM_BYTES = 32 + 32
HIT_MOTION_GATHER_BYTES = 12 + 48 + 36 + 96 + 20


def _timed(fns, calls, warmup):
    """fns: {name: callable}; one call of each per round, in order; returns {name: [ms per call]}"""
    import torch

    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)] for k in fns}
    for i in range(calls):
        for k, f in fns.items():
            ev[k][i][0].record()
            f()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}


def _summary(series):
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "calls": len(v)} for k, v in series.items()}


def _parent_renderer(path, flat):
    """a Renderer whose calls go to the library at `path` (the parent commit's build: it lacks the new symbols)"""
    import vkrt_amd.renderer as R
    from vkrt_amd import abi

    branch = R.load_library()
    plib = C.CDLL(path)
    for s in abi.VKRT_SYMBOLS:
        if hasattr(plib, s):
            f, g = getattr(plib, s), getattr(branch, s)
            f.restype = g.restype
            if g.argtypes is not None:
                f.argtypes = g.argtypes
    R._lib = plib
    try:
        return R.Renderer(flat, device=0, build="ploc")
    finally:
        R._lib = branch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--ref-frames", type=int, default=1024)
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.calls >= 20, "medians of at least 20 calls"

    import numpy as np
    import torch

    import atrium
    import camera_np
    import vkrt_amd
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants, uniforms_from_matrices
    from vkrt_amd.renderer import Denoiser, Renderer

    flat, _ = atrium.build_atrium(a.triangles, seed=1)
    camkw = atrium.DEFAULT_CAMERA
    cam = uniforms_from_matrices(*camera_np.global_uniforms(width=W, height=H, **camkw))
    vm = camera_np.look_at(camkw["eye"], camkw["center"], camkw["up"]).astype("float32").T.reshape(-1)
    L = min(8, len(flat.lights))
    r = Renderer(flat, device=0, build="ploc")
    res = {"workload": f"atrium{a.triangles}_{W}x{H}", "source_hash": vkrt_amd.source_hash(), "hbm_peak_GB_s": HBM_PEAK_GBS,
           "method": f"medians of {a.calls} calls after {a.warmup}, device events around every call, variants alternating call by call"}

    # 1 + 2: the G-buffer pass
    fns = {}
    rp = _parent_renderer(a.parent_lib, flat) if a.parent_lib else None
    if rp is not None:
        fns["parent_nrd_series_a"] = lambda: rp.gbuffer_raycast(cam, W, H, lights_count=L, view_matrix=vm)
    fns["branch_nrd"] = lambda: r.gbuffer_raycast(cam, W, H, lights_count=L, view_matrix=vm)
    if rp is not None:
        fns["parent_nrd_series_b"] = lambda: rp.gbuffer_raycast(cam, W, H, lights_count=L, view_matrix=vm)
    fns["branch_hits"] = lambda: r.gbuffer_raycast(cam, W, H, lights_count=L, view_matrix=vm, hits=True)
    s = _timed(fns, a.calls, a.warmup)
    res["gbuffer"] = _summary(s)
    res["gbuffer"]["note"] = "each call also allocates and zeroes its output planes (Renderer.gbuffer_raycast), the same in every variant"
    if rp is not None:
        m = {k: statistics.median(v) for k, v in s.items()}
        spread = abs(m["parent_nrd_series_a"] - m["parent_nrd_series_b"])
        over = m["branch_nrd"] - 0.5 * (m["parent_nrd_series_a"] + m["parent_nrd_series_b"])
        res["gbuffer"]["parent_series_spread_ms"] = spread
        res["gbuffer"]["branch_minus_parent_ms"] = over
        res["gbuffer"]["branch_within_parent_spread"] = bool(over <= spread)
        res["gbuffer"]["series_ms"] = {k: v for k, v in s.items() if k != "branch_hits"}
        rp.close()
    res["gbuffer"]["hits_over_nrd"] = statistics.median(s["branch_hits"]) / statistics.median(s["branch_nrd"])

    # 3 + 4: the mark and the previous positions
    g = r.gbuffer_raycast(cam, W, H, lights_count=L, view_matrix=vm, hits=True)
    hits = g["hits"].view(-1, 8)
    n = int(hits.shape[0])
    r.motion_mark()
    s = _timed({"motion_mark": lambda: r.motion_mark(), "hit_motion": lambda: r.hit_motion(hits)}, a.calls, a.warmup)
    res["motion_mark"] = _summary({"motion_mark": s["motion_mark"]})["motion_mark"]
    res["motion_mark"]["bytes_copied"] = 2 * (96 * len(flat.nodes) + 12 * len(flat.positions))
    hm = _summary({"hit_motion": s["hit_motion"]})["hit_motion"]
    geom = float((hits.view(torch.int32)[:, 3] >= 0).float().mean())
    stream_b, gather_b = n * HIT_MOTION_STREAM_BYTES, n * geom * HIT_MOTION_GATHER_BYTES
    hm.update(records=n, hit_fraction=geom, stream_bytes=stream_b, gather_bytes_if_nothing_were_shared=gather_b,
              stream_GB_s=stream_b / (hm["median_ms"] * 1e6))
    hm["stream_frac_of_hbm_peak"] = hm["stream_GB_s"] / HBM_PEAK_GBS
    hm["note"] = ("the call also allocates its two outputs.  stream_bytes = records read + both outputs written; the gathers (indices, vertices, "
                  "instance rows) are shared by neighbouring pixels and served by the caches, so they are listed, not added.  Records and "
                  "outputs of one frame fit the 256 MB last-level cache: the rate is not an HBM rate")
    res["hit_motion"] = hm

    # 5: the denoiser
    pc = make_push_constants(samples=1, depth=8, frame=0, lights_count=L)
    pc.useShadows, pc.useAO, pc.useGI = 1, 1, 1
    g = r.gbuffer_raycast(cam, W, H, lights_count=L, view_matrix=vm, motion=True)
    acc = r.hybrid_trace(pc, cam, W, H, g, seed=1)
    plain = {k: v for k, v in g.items() if k != "prevPosition"}
    d0, d1 = Denoiser(0, W, H), Denoiser(0, W, H)
    o0, o1 = acc.clone(), acc.clone()
    s = _timed({"denoise_plain": lambda: d0.denoise(cam, plain, out=o0), "denoise_motion": lambda: d1.denoise(cam, g, out=o1)}, a.calls, a.warmup)
    res["denoise"] = _summary(s)
    res["denoise"]["motion_over_plain"] = statistics.median(s["denoise_motion"]) / statistics.median(s["denoise_plain"])
    res["denoise"]["outputs_equal_on_a_still_scene"] = bool(torch.equal(o0, o1))
    d0.close(); d1.close()

    # 6: quality on movers
    if a.quality:
        rng = np.random.default_rng(5)
        nodes = np.sort(rng.choice(len(flat.nodes), len(flat.nodes) // 3, replace=False))
        steps = rng.standard_normal((len(nodes), 3)).astype(np.float32)
        steps *= 0.04 / np.linalg.norm(steps, axis=1, keepdims=True)
        base = np.array(flat.nodes["worldMatrix"], np.float32)
        is_mover = torch.zeros(len(flat.nodes) + 1, dtype=torch.bool, device="cuda:0")
        is_mover[torch.from_numpy(nodes).to("cuda:0")] = True
        pc = make_push_constants(samples=1, depth=2, frame=0, lights_count=L)
        pc.useShadows, pc.useAO, pc.useGI = 1, 1, 1
        dm, dp = Denoiser(0, W, H), Denoiser(0, W, H)
        frames = []
        for f in range(16):
            r.motion_mark()
            for j, i in enumerate(nodes):
                m = base[i].copy()
                m[12:15] += f * steps[j]
                r.update_nodes(int(i), m[None])
            r.refit()
            g = r.gbuffer_raycast(cam, W, H, lights_count=L, view_matrix=vm, motion=True)
            acc = r.hybrid_trace(pc, cam, W, H, g, seed=1000 * f)
            with_m = dm.denoise(cam, g, out=acc.clone())[..., :3].double()
            without = dp.denoise(cam, {k: v for k, v in g.items() if k != "prevPosition"}, out=acc.clone())[..., :3].double()
            ref = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
            for k in range(a.ref_frames):
                ref += r.hybrid_trace(pc, cam, W, H, g, seed=1000 * f + 1 + k)[..., :3].clamp(min=0).double()
            ref /= a.ref_frames
            inst = g["hits"].view(torch.int32)[..., 3]
            geom = inst >= 0
            mover = geom & is_mover[inst.clamp(min=0).long()]
            static = geom & ~mover
            rmse = lambda x, mask: float(((x - ref)[mask] ** 2).mean().sqrt()) if bool(mask.any()) else None  # noqa: E731
            frames.append({"frame": f, "mover_pixels": int(mover.sum()), "static_pixels": int(static.sum()),
                           "rmse_movers_with_motion": rmse(with_m, mover), "rmse_movers_without": rmse(without, mover),
                           "rmse_static_with_motion": rmse(with_m, static), "rmse_static_without": rmse(without, static),
                           "static_pixels_equal_bits": bool(torch.equal(with_m[static], without[static]))})
            print(json.dumps(frames[-1]), flush=True)
        res["quality"] = {"frames": frames, "ref_frames": a.ref_frames, "depth": 2, "iterations": 5, "moving_nodes": int(len(nodes)),
                          "step_length": 0.04}
        dm.close(); dp.close()
    else:
        res["quality"] = "not measured"
    r.close()
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
