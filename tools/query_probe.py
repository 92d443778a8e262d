"""Ray-query rate probe: vkrt_intersect / vkrt_occluded (k_query) against the per-thread test hook vkrt_debug_trace_rays (k_trace_rays)
on the bench atrium (262 k triangles) with three seeded ray sets:

  camera   1920x1080 pinhole rays through the pixel centres (bench camera);
  diffuse  one cosine-distributed ray from every primary hit point, about the geometric normal on the side the camera sees;
  shadow   one ray from every primary hit point to a light of the scene (tmax = distance - 0.1, like raytrace.rgen:94).

Rates of the product path come from device events around back-to-back launches on one stream (at least ~1 s per set after a
warm-up).  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of a child process that launches both kernels on
the same rays: the hook copies its rays in and out and synchronises on every call, so only its kernel time is comparable.  The hook
takes one scalar (tmin, tmax) per call, so in the child run both kernels get each shadow ray as the unnormalised segment to its light
with bounds (1e-4, 0.999) -- the same segment up to those bounds.

  python tools/query_probe.py --out profiles/r06_query_probe.json
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _world_triangles(flat):
    """float64 [T, 3, 3]: the vertices of every flattened triangle (nodes in order, each node's primMesh triangles in order), in world space."""
    out = []
    for node in flat.nodes:
        pm = flat.prim_meshes[node["primMesh"]]
        idx = flat.indices[int(pm["firstIndex"]): int(pm["firstIndex"]) + int(pm["indexCount"])].astype(np.int64) + int(pm["vertexOffset"])
        M = np.asarray(node["worldMatrix"], np.float64).reshape(4, 4).T  # column-major -> row-major
        out.append((np.c_[flat.positions[idx].astype(np.float64), np.ones(len(idx))] @ M.T)[:, :3].reshape(-1, 3, 3))
    return np.concatenate(out)


def _camera_rays(cam, W, H):
    eye, center, up = (np.asarray(cam[k], np.float64) for k in ("eye", "center", "up"))
    f = center - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    th = np.tan(np.radians(cam["fov"]) * 0.5)
    x = ((np.arange(W) + 0.5) / W * 2 - 1) * th * W / H
    y = (1 - (np.arange(H) + 0.5) / H * 2) * th
    X, Y = np.meshgrid(x, y)
    d = f[None] + X.reshape(-1, 1) * s[None] + Y.reshape(-1, 1) * u[None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.broadcast_to(eye, d.shape).astype(np.float32).copy(), d.astype(np.float32)


def ray_sets(flat, cam, W, H, r, seed):
    """{name: (origins, directions, tmin [N], tmax [N])} -- the diffuse and shadow sets start at the camera rays' hit points."""
    import torch
    from vkrt_amd.renderer import pack_rays

    o, d = _camera_rays(cam, W, H)
    n = o.shape[0]
    sets = {"camera": (o, d, np.full(n, 0.001, np.float32), np.full(n, 1e4, np.float32))}
    h = r.intersect(pack_rays(torch.from_numpy(o).cuda(r.device), torch.from_numpy(d).cuda(r.device)))
    torch.cuda.synchronize()
    tri, t = h.triangle.cpu().numpy(), h.t.cpu().numpy()
    hit = tri >= 0
    W3 = _world_triangles(flat)[tri[hit]]
    p = o[hit].astype(np.float64) + t[hit, None].astype(np.float64) * d[hit].astype(np.float64)
    nrm = np.cross(W3[:, 1] - W3[:, 0], W3[:, 2] - W3[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True) + 1e-30
    nrm *= -np.sign((nrm * d[hit]).sum(1, keepdims=True) + 1e-30)  # the side the camera sees
    rng = np.random.default_rng(seed)
    m = p.shape[0]
    # cosine-distributed about the normal
    r1, r2 = rng.random(m), rng.random(m)
    phi, sq = 2 * np.pi * r1, np.sqrt(r2)
    a = np.where(np.abs(nrm[:, :1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    tx = np.cross(a, nrm)
    tx /= np.linalg.norm(tx, axis=1, keepdims=True)
    ty = np.cross(nrm, tx)
    dd = tx * (np.cos(phi) * sq)[:, None] + ty * (np.sin(phi) * sq)[:, None] + nrm * np.sqrt(1 - r2)[:, None]
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    po = p.astype(np.float32)
    sets["diffuse"] = (po, dd.astype(np.float32), np.full(m, 0.001, np.float32), np.full(m, 1e4, np.float32))
    L = flat.lights["position"].astype(np.float64)[rng.integers(0, len(flat.lights), m)]
    seg = L - p
    dist = np.linalg.norm(seg, axis=1)
    sets["shadow"] = (po, (seg / dist[:, None]).astype(np.float32), np.full(m, 0.001, np.float32), np.maximum(dist - 0.1, 0.002).astype(np.float32))
    sets["shadow_segment"] = (po, seg.astype(np.float32), np.full(m, 1e-4, np.float32), np.full(m, 0.999, np.float32))
    return sets


def time_queries(r, rays, occluded, min_seconds):
    """(Mrays/s, ms per launch, launches) from device events around back-to-back launches on one stream."""
    import torch

    n = rays.shape[0]
    out = torch.empty((n,), dtype=torch.int32, device=rays.device) if occluded else torch.empty((n, 8), dtype=torch.float32, device=rays.device)
    fn = r.occluded if occluded else r.intersect
    for _ in range(3):
        fn(rays, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(rays, out=out)
    e1.record()
    e1.synchronize()
    one = max(e0.elapsed_time(e1), 1e-3)
    k = int(min(5000, max(10, np.ceil(min_seconds * 1e3 / one))))
    e0.record()
    for _ in range(k):
        fn(rays, out=out)
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / k
    return n / ms * 1e-3, ms, k


def _child(npz, reps):
    """Launched under rocprofv3: k_trace_rays (through the test hook) and k_query on the same rays with scalar bounds."""
    import torch
    from vkrt_amd.flat_scene import FlatScene
    from vkrt_amd.renderer import Renderer, pack_rays

    z = np.load(npz, allow_pickle=False)
    flat = FlatScene.load_npz(str(z["scene"]))
    r = Renderer(flat, device=0, build=str(z["build"]))
    for name in ("camera", "diffuse", "shadow_segment"):
        o, d = z[name + "_o"], z[name + "_d"]
        lo, hi = float(z[name + "_tmin"]), float(z[name + "_tmax"])
        anyhit = name == "shadow_segment"
        rays = pack_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), tmin=lo, tmax=hi)
        for _ in range(reps):
            r.trace_rays(o, d, lo, hi, any_hit=anyhit)
            (r.occluded if anyhit else r.intersect)(rays)
        torch.cuda.synchronize()
    r.close()


def _kernel_stats(outdir):
    """{kernel name: (calls, total ns)} from the rocprofv3 --stats CSV(s) under outdir."""
    res = {}
    for f in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name") or row.get("KernelName") or ""
                calls = int(float(row.get("Calls", 0)))
                tot = float(row.get("TotalDurationNs", 0))
                c0, t0 = res.get(name, (0, 0.0))
                res[name] = (c0 + calls, t0 + tot)
    return res


def _kernel_trace(outdir):
    """[(kernel name, duration ns)] in dispatch order from the rocprofv3 kernel-trace CSV(s) under outdir."""
    rows = []
    for f in glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name") or row.get("KernelName") or row.get("Name") or ""
                rows.append((int(row.get("Start_Timestamp", 0)), name, int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    return [(n, d) for _, n, d in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_query_probe.json"))
    ap.add_argument("--build", default="ploc")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5, help="launches of each kernel per set in the rocprofv3 run")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        _child(a.child, a.reps)
        return

    import torch
    import atrium
    import vkrt_amd
    from vkrt_amd.renderer import Renderer, pack_rays

    flat, _ = atrium.build_atrium(262144, seed=1, with_textures=False)
    W, H = 1920, 1080
    r = Renderer(flat, device=0, build=a.build)
    sets = ray_sets(flat, dict(atrium.DEFAULT_CAMERA), W, H, r, a.seed)
    result = {"source_hash": vkrt_amd.source_hash(), "scene": "atrium 262144 seed 1", "triangles": int(r.accel_info()["triangle_count"]),
              "build": a.build, "device": torch.cuda.get_device_name(0), "sets": {}}
    r.reset_counters()
    for name in ("camera", "diffuse", "shadow"):
        o, d, lo, hi = sets[name]
        rays = pack_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), tmin=torch.from_numpy(lo).cuda(), tmax=torch.from_numpy(hi).cuda())
        entry = {"rays": int(o.shape[0])}
        for kind, occ in (("intersect", False), ("occluded", True)):
            mrays, ms, k = time_queries(r, rays, occ, a.seconds)
            entry[kind] = {"mrays_per_s": round(mrays, 1), "ms_per_launch": round(ms, 4), "launches": k}
        h = r.intersect(rays)
        torch.cuda.synchronize()
        entry["hit_fraction"] = round(float((h.triangle >= 0).float().mean()), 4)
        result["sets"][name] = entry
        print(name, json.dumps(entry), flush=True)
    result["traversal_faults"] = int(r.counters()["traversal_faults"])

    # kernel times: k_trace_rays vs k_query under rocprofv3 in a child process, on the same rays with scalar bounds
    tmp = tempfile.mkdtemp(prefix="query_probe_")
    try:
        scene_npz = os.path.join(tmp, "scene.npz")
        flat.save_npz(scene_npz)
        z = {"scene": scene_npz, "build": a.build}
        for name, (lo, hi) in (("camera", (0.001, 1e4)), ("diffuse", (0.001, 1e4)), ("shadow_segment", (1e-4, 0.999))):
            o, d = sets[name][0], sets[name][1]
            z[name + "_o"], z[name + "_d"], z[name + "_tmin"], z[name + "_tmax"] = o, d, np.float32(lo), np.float32(hi)
        np.savez(os.path.join(tmp, "rays.npz"), **z)
        prof = os.path.join(tmp, "prof")
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "qp", "--output-format", "csv",
               "--", sys.executable, os.path.abspath(__file__), "--child", os.path.join(tmp, "rays.npz"), "--reps", str(a.reps)]
        t0 = time.time()
        rc = subprocess.run(cmd, timeout=900).returncode
        result["rocprof"] = {"rc": rc, "seconds": round(time.time() - t0, 1), "reps": a.reps}
        if rc == 0:
            trace = [(n, d) for n, d in _kernel_trace(prof) if "k_trace_rays" in n or "k_query" in n]
            # dispatch order of the child: per set, reps x (k_trace_rays, k_query)
            per = {}
            for i, name in enumerate(("camera", "diffuse", "shadow_segment")):
                part = trace[i * 2 * a.reps:(i + 1) * 2 * a.reps]
                for kern in ("k_trace_rays", "k_query"):
                    ds = sorted(d for n, d in part if kern in n)
                    if ds:
                        med = ds[len(ds) // 2] * 1e-6
                        nr = int(sets[name][0].shape[0])
                        per.setdefault(name, {})[kern] = {"median_ms": round(med, 4), "mrays_per_s": round(nr / med * 1e-3, 1), "launches": len(ds)}
                if "k_query" in per.get(name, {}) and "k_trace_rays" in per.get(name, {}):
                    per[name]["k_query_speedup"] = round(per[name]["k_trace_rays"]["median_ms"] / per[name]["k_query"]["median_ms"], 3)
            result["kernel_times"] = per
            result["kernel_stats"] = {n: {"calls": c, "total_ms": round(t * 1e-6, 3)} for n, (c, t) in _kernel_stats(prof).items()
                                      if "k_trace_rays" in n or "k_query" in n}
            print("kernel_times", json.dumps(per), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)
    r.close()


if __name__ == "__main__":
    main()
