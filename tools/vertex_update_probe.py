"""Deforming meshes against rebuilding on the bench atrium (262 k triangles): what vkrt_scene_update_vertices costs, what update + refit
saves over vkrt_accel_build and over destroy + create + build, and what a refitted tree costs in ray rate and SAH cost after k steps of a
travelling sine displacement of the eight hanging-cloth meshes.

    python tools/vertex_update_probe.py [--out profiles/r06_vertex_update_probe.json] [--triangles 262144] [--spp 16] [--depth 8]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/vertex_update_probe.py --trace-only
    python tools/vertex_update_probe.py --merge-trace DIR [--out ...]     # k_vertex_update's durations from that run, into the file

Call times are HIP events on the caller's stream around back-to-back calls after a warm-up (device source), or a host clock around calls
that end in a synchronise (host source, builds, scene creation).  The kernel's own duration comes from a kernel trace taken in a run
of its own (--trace-only), grouped by launch size.  Pixels are compared too: the refitted and the rebuilt tree must render the same
image at every step."""
import argparse
import csv
import glob
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0  # MI355X spec
BYTES_READ = {"positions": 12, "normals": 12, "tangents": 16, "texcoords0": 8}
BYTES_WRITTEN = 12 + 48  # positions[3 v ..] + the three float4 of vertexPN[v]


def cloth_meshes(flat):
    """The eight hanging cloths of tools/atrium.py: unique meshes placed once, at y = 9.6."""
    uses = np.bincount(flat.nodes["primMesh"], minlength=len(flat.prim_meshes))
    out = [int(n["primMesh"]) for n in flat.nodes if abs(float(n["worldMatrix"][13]) - 9.6) < 1e-4 and uses[n["primMesh"]] == 1]
    assert len(out) == 8, out
    return out


def merge_trace(trace_dir, out):
    """k_vertex_update rows of a rocprofv3 kernel trace, grouped by grid size, into res["kernel"]["trace"]."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel_trace.csv under {trace_dir}"
    groups = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            if "k_vertex_update" not in row.get("Kernel_Name", ""):
                continue
            grid = int(row.get("Grid_Size_X") or row.get("Grid_Size"))
            groups.setdefault(grid, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    res = json.load(open(out))
    k = res["kernel"]
    k["trace"] = []
    for grid, us in sorted(groups.items()):
        us = np.sort(np.array(us))
        row = {"grid_threads": grid, "launches": int(us.size), "median_us": float(np.median(us)), "min_us": float(us[0]), "max_us": float(us[-1])}
        for name in ("whole", "one_mesh"):
            n = k[name]["vertices"]
            if (n + 255) // 256 * 256 == grid:
                row["which"] = name
                row["GB_per_s_median"] = k[name]["bytes_moved"] / (row["median_us"] * 1e-6) / 1e9
                row["frac_of_hbm_peak"] = row["GB_per_s_median"] / HBM_PEAK_GBS
        k["trace"].append(row)
    whole = [r for r in k["trace"] if r.get("which") == "whole"]
    k["note"] = ("frac_of_hbm_peak = bytes_moved / kernel duration / 8 TB/s.  The whole vertex array of this scene is %.1f MB moved per call: "
                 "a launch this small is bound by launch latency and the ramp of one short wave of workgroups, not by HBM, and between "
                 "back-to-back calls the arrays stay resident in the 256 MiB Infinity Cache.  The figure is therefore no statement about "
                 "streaming a mesh that is large against the caches from HBM: not measured." % (k["whole"]["bytes_moved"] / 1e6))
    if whole:
        k["whole"]["kernel_us_median"] = whole[0]["median_us"]
        k["whole"]["frac_of_hbm_peak"] = whole[0]["frac_of_hbm_peak"]
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(k["trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_vertex_update_probe.json"))
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50, help="timed calls per configuration")
    ap.add_argument("--trace-only", action="store_true", help="only the update calls, for a kernel trace")
    ap.add_argument("--merge-trace", default=None, help="directory of a rocprofv3 --kernel-trace run of --trace-only")
    args = ap.parse_args()
    if args.merge_trace:
        return merge_trace(args.merge_trace, args.out)

    import torch

    import atrium
    import camera_np
    import scene_deform as sd
    import vkrt_amd
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants, uniforms_from_matrices
    from vkrt_amd.renderer import Renderer

    flat, _ = atrium.build_atrium(args.triangles, seed=1, with_textures=True)
    V = int(flat.positions.shape[0])
    cloths = cloth_meshes(flat)
    one_first, one_count = sd.mesh_range(flat, cloths[0])
    dev = "cuda:0"
    per_vertex = sum(BYTES_READ.values()) + BYTES_WRITTEN

    def tensors(f, first, count):
        return {k: torch.as_tensor(np.ascontiguousarray(getattr(f, k)[first:first + count]), device=dev) for k in sd.ATTRS}

    def arrays(f, first, count):
        return {k: np.ascontiguousarray(getattr(f, k)[first:first + count]) for k in sd.ATTRS}

    def dev_ms(fn, reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps

    def wall_ms(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    r = Renderer(flat, device=0, build="ploc")
    whole_t, one_t = tensors(flat, 0, V), tensors(flat, one_first, one_count)
    whole_a, one_a = arrays(flat, 0, V), arrays(flat, one_first, one_count)
    st = torch.cuda.current_stream()
    for _ in range(3):  # warm-up: code object, staging buffer of the host path
        r.update_vertices(0, stream=st, **whole_t)
        r.update_vertices(one_first, stream=st, **one_t)
        r.update_vertices(0, **whole_a)
    if args.trace_only:
        for _ in range(args.reps):
            r.update_vertices(0, stream=st, **whole_t)
        for _ in range(args.reps):
            r.update_vertices(one_first, stream=st, **one_t)
        torch.cuda.synchronize()
        r.close()
        return
    res = {"source_hash": vkrt_amd.source_hash(), "device": torch.cuda.get_device_name(0),
           "scene": {"name": f"atrium {args.triangles} seed 1", "triangles": flat.instanced_triangle_count, "instances": len(flat.nodes),
                     "vertices": V, "cloth_meshes": len(cloths), "cloth_vertices": int(sum(sd.mesh_range(flat, m)[1] for m in cloths))},
           "frame": {"width": args.width, "height": args.height, "spp": args.spp, "depth": args.depth}, "hbm_peak_GB_s": HBM_PEAK_GBS}

    # ---- the update alone: all four attributes, the whole vertex array and one cloth mesh, from device and from host memory ----
    kern = {"bytes_per_vertex": {"read": BYTES_READ, "written": BYTES_WRITTEN, "total": per_vertex}}
    for name, first, count, t, a in (("whole", 0, V, whole_t, whole_a), ("one_mesh", one_first, one_count, one_t, one_a)):
        row = {"vertices": count, "bytes_moved": count * per_vertex}
        row["device_source_ms_per_call_events"] = dev_ms(lambda: r.update_vertices(first, stream=st, **t), args.reps)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            r.update_vertices(first, stream=st, **t)
        row["device_source_enqueue_ms_host"] = (time.perf_counter() - t0) * 1e3 / args.reps
        row["host_source_ms_per_call_wall"] = wall_ms(lambda: r.update_vertices(first, **a), max(5, args.reps // 5))
        row["GB_per_s_events"] = row["bytes_moved"] / (row["device_source_ms_per_call_events"] * 1e-3) / 1e9
        kern[name] = row
        print(json.dumps({name: row}), flush=True)
    kern["how"] = ("device_source_ms_per_call_events: HIP events around back-to-back calls (launch gaps included); host_source: host clock, "
                   "the call copies, launches and waits for the stream; trace: kernel durations of a separate kernel-trace run")
    res["kernel"] = kern
    r.close()

    # ---- update + refit against vkrt_accel_build and against destroy + create + build (what a caller had to do before) ----
    dflat = sd.sine(flat, cloths, phase=0.5)
    dall = tensors(dflat, 0, V)
    res["rebuild"] = []
    for kind, split in (("ploc", -1), ("ploc", 0), ("lbvh", -1)):
        opts = {abi.VKRT_OPT_SPLIT_BUDGET: split}
        r = Renderer(flat, device=0, build=kind, options=opts)
        r.build(kind)
        r.refit()  # first refit of the build: scratch + level lists
        torch.cuda.synchronize()

        def update_refit():
            r.update_vertices(0, stream=st, **dall)
            r.refit(stream=st)

        update_refit()
        row = {"builder": kind, "split_budget": split, "split_resolved": r.get_option(abi.VKRT_INFO_SPLIT_BUDGET)}
        row["update_refit_ms_events"] = dev_ms(update_refit, 20)
        row["update_refit_ms_wall"] = wall_ms(update_refit, 20)
        row["build_ms_wall"] = wall_ms(lambda: r.build(kind), 3)
        row["build_ms_reported"] = r.accel_info()["build_ms"]
        r.close()
        holder = [Renderer(flat, device=0, build=kind, options=opts)]

        def recreate():
            holder[0].close()
            holder[0] = Renderer(dflat, device=0, build=kind, options=opts)

        row["destroy_create_build_ms_wall"] = wall_ms(recreate, 2)
        holder[0].close()
        row["build_over_update_refit"] = row["build_ms_wall"] / row["update_refit_ms_wall"]
        row["recreate_over_update_refit"] = row["destroy_create_build_ms_wall"] / row["update_refit_ms_wall"]
        res["rebuild"].append(row)
        print(json.dumps(row), flush=True)

    # ---- ray rate and SAH cost after k steps of the travelling sine, refitted against rebuilt (PLOC, automatic split: the defaults) ----
    W, H = args.width, args.height
    cam = uniforms_from_matrices(*camera_np.global_uniforms(width=W, height=H, **atrium.DEFAULT_CAMERA))
    pc = make_push_constants(samples=args.spp, depth=args.depth, frame=0, lights_count=len(flat.lights))

    def frame(rr, seed=3):
        rr.reset_counters()
        img = rr.pathtrace(pc, cam, W, H, seed=seed)
        torch.cuda.synchronize()
        c = rr.counters()
        ms = rr.last_trace_ms()
        rays = c["rays_closest"] + c["rays_shadow"]
        return {"ms": ms, "grays_per_s": rays / ms / 1e6, "rays": rays, "hash": hashlib.sha256(img.cpu().numpy().tobytes()).hexdigest()[:16],
                "faults": c["traversal_faults"]}

    r = Renderer(flat, device=0, build="ploc")
    b = Renderer(flat, device=0, build="ploc")
    res["static"] = {"sah_cost": r.accel_info()["sah_cost"], **frame(r)}
    res["deformation"] = {"what": "travelling sine along the rest normals of the eight cloth meshes, amplitude 0.12 m, wavelength 1.3 m, "
                                  "phase advancing 0.35 rad per step; positions, normals and tangents updated from device memory",
                          "steps": []}
    step = 0
    for k in (1, 10, 50):
        while step < k:
            step += 1
            cur = sd.sine(flat, cloths, phase=0.35 * step)
            keep = []
            for m in cloths:
                first, count = sd.mesh_range(flat, m)
                t = {a: v for a, v in tensors(cur, first, count).items() if a != "texcoords0"}
                keep.append(t)
                r.update_vertices(first, stream=st, **t)
                b.update_vertices(first, stream=st, **t)
            r.refit(stream=st)
            torch.cuda.synchronize()
        b.build("ploc")
        fr, fb = frame(r), frame(b)
        row = {"steps": k, "refit": fr, "rebuilt": fb, "sah_refit": r.accel_info()["sah_cost"], "sah_rebuilt": b.accel_info()["sah_cost"],
               "ray_rate_refit_over_rebuilt": fr["grays_per_s"] / fb["grays_per_s"], "same_image": fr["hash"] == fb["hash"]}
        assert row["same_image"] and fr["faults"] == 0 and fb["faults"] == 0, row
        res["deformation"]["steps"].append(row)
        print(json.dumps(row), flush=True)
    r.close()
    b.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
