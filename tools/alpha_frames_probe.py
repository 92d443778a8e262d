#!/usr/bin/env python3
"""Cost of the alpha-test stage in rendered frames (VKRT_OPT_ALPHA_TEST): the textured bench atrium (262 k triangles) at 1920x1080,
16 spp, depth 8, with the drapery materials (10..13) made VKRT_ALPHA_MASK, cutoff 0.5, over the procedural alpha pattern of
`tools/query_probe.py --alpha` (a blocky hash in the alpha channel of the base-colour textures).

For the path tracer (vkrt_pathtrace) and for the hybrid frame (vkrt_gbuffer_raycast + vkrt_hybrid_trace with shadows, AO and GI) it
renders frames with the option 0 and 1, alternating call by call after warm-up frames, and records the median frame time from device
events, the library's own trace time and the ray counters of one frame of each.  No ratio is demanded anywhere: rays pass through the
holes, so the two settings trace different rays, and the figures say what a scene with cut-outs costs, not what the test per
candidate costs.

  python tools/alpha_frames_probe.py [--frames 5] [--out profiles/alpha_frames_probe.json]
"""
import argparse
import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

COUNTERS = ("rays_closest", "rays_shadow", "pixels")  # what a plain launch of the wavefront pipeline counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5, help="timed frames per setting and mode")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--build", default="ploc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alpha_frames_probe.json"))
    a = ap.parse_args()

    import torch
    import atrium
    import camera_np
    import vkrt_amd
    from query_probe import ALPHA_MATERIALS, _alpha_pattern
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants, uniforms_from_matrices
    from vkrt_amd.renderer import ALPHA_MASK, Renderer

    flat, _ = atrium.build_atrium(262144, seed=1, with_textures=True)
    flat = copy.copy(flat)
    flat.materials = flat.materials.copy()
    flat.textures = [dict(rgba8=np.ascontiguousarray(t["rgba8"]).copy(), is_srgb=t["is_srgb"]) for t in flat.textures]
    for i in range(4):  # the base-colour textures
        t = flat.textures[i]["rgba8"]
        t[:, :, 3] = _alpha_pattern(t.shape[0], t.shape[1], 32, i + 1)
    for m in ALPHA_MATERIALS:
        if flat.materials["pbrBaseColorTexture"][m] < 0:
            flat.materials["pbrBaseColorTexture"][m] = m % 4
    W, H, SPP, DEPTH = 1920, 1080, 16, 8
    cam = uniforms_from_matrices(*camera_np.global_uniforms(width=W, height=H, **atrium.DEFAULT_CAMERA))
    L = len(flat.lights)
    r = Renderer(flat, device=0, build=a.build)
    modes = np.zeros(len(flat.materials), np.uint32)
    modes[list(ALPHA_MATERIALS)] = ALPHA_MASK
    r.set_material_alpha(0, modes, 0.5)
    pc = make_push_constants(samples=SPP, depth=DEPTH, frame=0, lights_count=L)
    hpc = make_push_constants(samples=1, depth=DEPTH, frame=0, lights_count=L)
    hpc.useShadows, hpc.useAO, hpc.useGI = 1, 1, 1
    image = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    accum = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")

    def pathtrace():
        r.pathtrace(pc, cam, W, H, seed=1, image=image)

    def hybrid():
        g = r.gbuffer_raycast(cam, W, H, lights_count=L)
        r.hybrid_trace(hpc, cam, W, H, g, seed=1, accum=accum)

    result = {"source_hash": vkrt_amd.source_hash(), "device": torch.cuda.get_device_name(0), "build": a.build,
              "scene": "atrium 262144 seed 1, textured; materials 10..13 (drapery) MASK, cutoff 0.5, alpha = 32-texel hash blocks",
              "triangles": int(r.accel_info()["triangle_count"]), "width": W, "height": H, "samples": SPP, "depth": DEPTH,
              "hybrid": "gbuffer_raycast + hybrid_trace, shadows + AO + GI, one frame each",
              "method": f"device events around every frame; option 0 and 1 alternate frame by frame after {a.warmup} warm-up frames of each; medians of "
                        f"{a.frames}", "modes": {}}
    for name, fn in (("pathtrace", pathtrace), ("hybrid", hybrid)):
        ms = {0: [], 1: []}
        entry = {}
        for k in range(a.warmup + a.frames):
            for on in (0, 1):
                r.set_option(abi.VKRT_OPT_ALPHA_TEST, on)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if k >= a.warmup:
                    ms[on].append(e0.elapsed_time(e1))
        for on in (0, 1):
            r.set_option(abi.VKRT_OPT_ALPHA_TEST, on)
            r.reset_counters()
            fn()
            c = r.counters()
            t = sorted(ms[on])
            entry[f"option_{on}"] = {"frame_ms_median": round(t[len(t) // 2], 3), "frame_ms_min_max": [round(t[0], 3), round(t[-1], 3)],
                                     "last_trace_ms": round(r.last_trace_ms(), 3), "counters": {k: int(c[k]) for k in COUNTERS}}
        entry["frame_ms_on_over_off"] = round(entry["option_1"]["frame_ms_median"] / entry["option_0"]["frame_ms_median"], 4)  # reported, not gated
        result["modes"][name] = entry
        print(name, json.dumps(entry), flush=True)
    result["traversal_faults"] = int(r.counters()["traversal_faults"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)
    r.close()


if __name__ == "__main__":
    main()
