"""Refit against rebuild on the bench atrium (262 k triangles, 175 instances): build time per builder and split setting, refit time,
and what a refitted tree costs in ray rate and SAH cost after k steps of rigid motion of a third of the instances.

    python tools/refit_probe.py [--out profiles/r06_refit_probe.json] [--triangles 262144] [--spp 16] [--depth 8]

Device times are HIP events on the caller's stream after a warm-up.  The motion is seeded: every step moves the same third of the
instances by a small rotation (up to 0.08 rad about a random axis through the instance's centre) and a translation (up to 0.1 m).
Pixels are compared too: the refitted and the rebuilt tree must render the same image."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def _row_major(m16):
    return np.asarray(m16, np.float64).reshape(4, 4).T


def _step_matrices(flat, cur, idx, rng):
    """One motion step: {node: new column-major matrix} from the current matrices `cur` (node -> row-major 4x4)."""
    out = {}
    for i in idx:
        pm = flat.prim_meshes[flat.nodes[i]["primMesh"]]
        v = flat.positions[pm["vertexOffset"]:pm["vertexOffset"] + pm["vertexCount"]].astype(np.float64)
        c = (cur[i] @ np.append(0.5 * (v.min(0) + v.max(0)), 1.0))[:3] if len(v) else cur[i][:3, 3]
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        a = rng.uniform(-0.08, 0.08)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        M = np.eye(4)
        M[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
        M[:3, 3] = c - M[:3, :3] @ c + rng.uniform(-0.1, 0.1, 3)
        cur[i] = M @ cur[i]
        out[int(i)] = np.ascontiguousarray(cur[i].T.reshape(16), np.float32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_refit_probe.json"))
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--refits", type=int, default=20, help="timed refits per configuration")
    args = ap.parse_args()

    import torch

    import atrium
    import camera_np
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants, uniforms_from_matrices
    from vkrt_amd.renderer import Renderer

    flat, _ = atrium.build_atrium(args.triangles, seed=1, with_textures=True)
    W, H = args.width, args.height
    cam = uniforms_from_matrices(*camera_np.global_uniforms(width=W, height=H, **atrium.DEFAULT_CAMERA))
    pc = make_push_constants(samples=args.spp, depth=args.depth, frame=0, lights_count=len(flat.lights))
    n = len(flat.nodes)
    idx = np.sort(np.random.default_rng(7).choice(n, n // 3, replace=False))
    res = {"scene": {"triangles": flat.instanced_triangle_count, "instances": n, "moved_instances": int(len(idx))},
           "frame": {"width": W, "height": H, "spp": args.spp, "depth": args.depth}, "device": torch.cuda.get_device_name(0)}

    def dev_ms(fn, reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps

    def frame(r, seed=3):
        r.reset_counters()
        img = r.pathtrace(pc, cam, W, H, seed=seed)
        torch.cuda.synchronize()
        c = r.counters()
        ms = r.last_trace_ms()
        rays = c["rays_closest"] + c["rays_shadow"]
        return {"ms": ms, "grays_per_s": rays / ms / 1e6, "rays": rays,
                "hash": hashlib.sha256(img.cpu().numpy().tobytes()).hexdigest()[:16], "faults": c["traversal_faults"]}

    # build and refit times per builder and split setting
    res["builds"] = []
    for kind in ("ploc", "lbvh"):
        for split in (0, -1):
            r = Renderer(flat, device=0, build=None, options={abi.VKRT_OPT_SPLIT_BUDGET: split})
            r.build(kind)  # warm-up (code objects, rocprim temporaries)
            build_ms = dev_ms(lambda: r.build(kind), 3)
            info = r.accel_info()
            cur = {int(i): _row_major(flat.nodes[i]["worldMatrix"]) for i in idx}
            rng = np.random.default_rng(11)
            r.refit()  # first refit of the build: scratch + level lists
            mats = _step_matrices(flat, cur, idx, rng)
            for i, m in mats.items():
                r.update_nodes(i, m[None])
            refit_ms = dev_ms(r.refit, args.refits)
            t0 = time.perf_counter()
            for _ in range(args.refits):
                r.refit()
            enqueue_ms = (time.perf_counter() - t0) * 1e3 / args.refits
            torch.cuda.synchronize()
            row = {"builder": kind, "split_budget": split, "split_resolved": r.get_option(abi.VKRT_INFO_SPLIT_BUDGET), "build_ms": build_ms,
                   "build_ms_wall": info["build_ms"], "refit_ms": refit_ms, "refit_enqueue_ms_host": enqueue_ms, "node_count": info["node_count"],
                   "reference_count": info["reference_count"]}
            row["build_over_refit"] = build_ms / refit_ms
            res["builds"].append(row)
            print(json.dumps(row), flush=True)
            r.close()

    # ray rate and SAH cost after k motion steps, refitted against rebuilt (PLOC, automatic split budget: the defaults)
    r = Renderer(flat, device=0, build="ploc")
    b = Renderer(flat, device=0, build="ploc")
    base = frame(r)
    res["static"] = {"sah_cost": r.accel_info()["sah_cost"], **base}
    cur = {int(i): _row_major(flat.nodes[i]["worldMatrix"]) for i in idx}
    rng = np.random.default_rng(11)
    res["motion"] = []
    step = 0
    for k in (1, 10, 50):
        while step < k:
            mats = _step_matrices(flat, cur, idx, rng)
            for i, m in mats.items():
                r.update_nodes(i, m[None])
                b.update_nodes(i, m[None])
            r.refit()
            step += 1
        b.build("ploc")
        fr, fb = frame(r), frame(b)
        row = {"steps": k, "refit": fr, "rebuilt": fb, "sah_refit": r.accel_info()["sah_cost"], "sah_rebuilt": b.accel_info()["sah_cost"],
               "ray_rate_refit_over_rebuilt": fr["grays_per_s"] / fb["grays_per_s"], "same_image": fr["hash"] == fb["hash"]}
        res["motion"].append(row)
        print(json.dumps(row), flush=True)
    r.close()
    b.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
