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

The surface leg (--surface) times vkrt_hit_surface (k_hit_surface) on the textured bench atrium: the hit records of the camera rays
(coherent) and of their cosine bounces (incoherent), misses removed, each with VKRT_SURFACE_GEOMETRY and with GEOMETRY | MATERIAL;
device events around 20 calls after 5 warm-up calls, kernel times from a separate `rocprofv3 --kernel-trace --stats` child run that
also renders one bench frame, whose k_wf_shade time per record is the yardstick.  --variant-lib PATH measures a second build of the
library (csrc/Makefile VARIANT=...) in the same run, the two alternating call by call.

  python tools/query_probe.py --surface --out profiles/r06_surface_probe.json

The multi-hit leg (--multi) times vkrt_intersect_multi (k_query_multi) for K = 1, 2, 4, 8, 16 on the camera rays (coherent) and their
cosine bounces (incoherent) of the bench atrium against what a caller had to do without it: K passes of vkrt_intersect, pass j with
tmin = the t of pass j - 1 (a ray that missed gets tmin = tmax and is not walked again).  The rays of every pass are prepared
beforehand, so the peeling time is that of its K launches alone.  The two alternate call by call, an event pair around each, after
warm-up calls of every shape; the medians are compared.  --multi-resources (no GPU) compiles multihit.hip with the flags of
csrc/Makefile and records registers, scratch and static LDS of every k_query_multi instantiation next to the output.

  python tools/query_probe.py --multi-resources && python tools/query_probe.py --multi --out profiles/r06_multihit_probe.json

The alpha leg (--alpha) measures the alpha-test stage of the ray queries (vkrt_scene_set_material_alpha) on the textured bench atrium
with the drapery materials (10..13) made VKRT_ALPHA_MASK, cutoff 0.5, over a procedural alpha pattern (a blocky hash in the alpha channel
of the base-colour textures): vkrt_intersect and vkrt_occluded on the camera, diffuse and shadow sets with the stage, against the same
calls with every material OPAQUE and -- closest hit only, an occlusion query has no such stand-in -- against the emulation the stage
replaces: vkrt_intersect_multi with K = 8, vkrt_hit_surface on the 8 records per ray, and a select of the first admitted one.  The
three alternate call by call (the modes are switched between the calls, outside the timed region); medians.  --alpha-resources (no GPU)
compiles query.hip and multihit.hip with the flags of csrc/Makefile and records registers, scratch and spills of every instantiation
with the stage next to its counterpart without it.

  python tools/query_probe.py --alpha-resources && python tools/query_probe.py --alpha --out profiles/alpha_cutout_probe.json
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


# ---- the surface leg ------------------------------------------------------------------------------------------------------------
HBM_PEAK_GBS = 8000.0
SURFACE_CASES = (("camera", "geometry", False), ("camera", "material", True), ("diffuse", "geometry", False), ("diffuse", "material", True))


def _renderer_of(lib_path, flat, build):
    """A Renderer on its own copy of the library (None: the product build the package names)."""
    import ctypes as C
    from vkrt_amd import abi, renderer

    if lib_path is None:
        return renderer.Renderer(flat, device=0, build=build)
    renderer.load_library()
    saved, renderer._lib = renderer._lib, abi.declare_vkrt(C.CDLL(os.path.abspath(lib_path)))
    try:
        return renderer.Renderer(flat, device=0, build=build)  # (keeps the handle it was made with)
    finally:
        renderer._lib = saved


def _surface_hits(r, sets):
    """{set: [N, 8] device tensor of the hit records of the set's rays, misses removed}"""
    import torch
    from vkrt_amd.renderer import pack_rays

    out = {}
    for name in ("camera", "diffuse"):
        o, d, lo, hi = sets[name]
        rays = pack_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), tmin=torch.from_numpy(lo).cuda(), tmax=torch.from_numpy(hi).cuda())
        h = r.intersect(rays)
        out[name] = h.buffer[h.instance >= 0].contiguous()
    torch.cuda.synchronize()
    return out


def _surface_bytes(flat, hits, material):
    """Algorithmic bytes per hit: 32 in, 128 out, 3 x 4 index, 3 x 48 vertex, 96 instance; with the material 64 + 16 per issued tap."""
    b = 32 + 128 + 12 + 144 + 96
    if not material:
        return float(b)
    m = flat.materials[hits[:, 7].contiguous().cpu().numpy().view(np.int32)]
    taps = sum((m[k] > -1).astype(np.float64) for k in ("pbrBaseColorTexture", "metallicRoughnessTexture", "normalTexture", "emissiveTexture"))
    return float(b + 64 + 16 * taps.mean())


def _surface_child(npz, reps):
    """Launched under rocprofv3: reps calls per case on the saved hit records, then one bench frame (k_wf_shade)."""
    import torch
    from vkrt_amd.flat_scene import FlatScene, make_push_constants
    from vkrt_amd.renderer import Renderer

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import default_camera

    z = np.load(npz, allow_pickle=False)
    flat = FlatScene.load_npz(str(z["scene"]))
    libs = [None] + ([str(z["variant_lib"])] if str(z["variant_lib"]) else [])
    rs = [_renderer_of(p, flat, str(z["build"])) for p in libs]
    for set_name, _, material in SURFACE_CASES:
        hits = torch.from_numpy(z[set_name]).cuda()
        for _ in range(reps):
            for r in rs:  # alternating
                r.surface(hits, material=material)
        torch.cuda.synchronize()
    c = {k: float(z["cam_" + k]) if k == "fov" else tuple(float(x) for x in z["cam_" + k]) for k in ("eye", "center", "up", "fov")}
    W, H = 1920, 1080
    pc = make_push_constants(samples=1, depth=8, frame=0, lights_count=len(flat.lights))
    rs[0].reset_counters()
    rs[0].pathtrace(pc, default_camera(W, H, **c), W, H, seed=7)
    torch.cuda.synchronize()
    with open(str(z["counters_out"]), "w") as f:
        json.dump(rs[0].counters(), f)
    for r in rs:
        r.close()


def surface_leg(a):
    import torch
    import atrium
    import vkrt_amd

    flat, info = atrium.build_atrium(262144, seed=1, with_textures=True)
    cam = dict(info["camera"]) if "camera" in info else dict(atrium.DEFAULT_CAMERA)
    W, H = 1920, 1080
    libs = [("plain", None)] + ([(a.variant_name, a.variant_lib)] if a.variant_lib else [])
    rs = [(name, _renderer_of(p, flat, a.build)) for name, p in libs]
    r = rs[0][1]
    sets = ray_sets(flat, cam, W, H, r, a.seed)
    hits = _surface_hits(r, sets)
    result = {"source_hash": vkrt_amd.source_hash(), "scene": "atrium 262144 seed 1, textured", "build": a.build, "device": torch.cuda.get_device_name(0),
              "hbm_peak_GB_s": HBM_PEAK_GBS, "warmup_calls": 5, "timed_calls": 20, "variants": [n for n, _ in libs], "cases": {}}
    outs = {n: torch.empty((max(h.shape[0] for h in hits.values()), 32), dtype=torch.float32, device="cuda:0") for n, _ in rs}
    for set_name, what, material in SURFACE_CASES:
        h = hits[set_name]
        n = int(h.shape[0])
        entry = {"hits": n, "algorithmic_bytes_per_hit": round(_surface_bytes(flat, h, material), 1), "events": {}}
        for _ in range(5):
            for name, rr in rs:
                rr.surface(h, material=material, out=outs[name][:n])
        torch.cuda.synchronize()
        ms = {name: 0.0 for name, _ in rs}
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20 * len(rs))]
        k = 0
        for _ in range(20):  # the variants alternate call by call, an event pair around every call
            for name, rr in rs:
                ev[k][0].record()
                rr.surface(h, material=material, out=outs[name][:n])
                ev[k][1].record()
                k += 1
        torch.cuda.synchronize()
        k = 0
        for _ in range(20):
            for name, _ in rs:
                ms[name] += ev[k][0].elapsed_time(ev[k][1])
                k += 1
        for name, _ in rs:
            per = ms[name] / 20
            entry["events"][name] = {"ms_per_call": round(per, 4), "ns_per_hit": round(per * 1e6 / n, 3), "mhits_per_s": round(n / per * 1e-3, 1)}
        if len(rs) > 1:  # the variant computes the same records
            torch.cuda.synchronize()
            entry["variant_bit_identical"] = bool(torch.equal(outs[rs[0][0]][:n].view(torch.int32), outs[rs[1][0]][:n].view(torch.int32)))
        result["cases"][set_name + "_" + what] = entry
        print(set_name, what, json.dumps(entry), flush=True)

    tmp = tempfile.mkdtemp(prefix="surface_probe_")
    try:
        scene_npz = os.path.join(tmp, "scene.npz")
        flat.save_npz(scene_npz)
        z = {"scene": scene_npz, "build": a.build, "variant_lib": os.path.abspath(a.variant_lib) if a.variant_lib else "",
             "counters_out": os.path.join(tmp, "counters.json")}
        for k in ("eye", "center", "up", "fov"):
            z["cam_" + k] = np.asarray(cam[k], np.float64)
        for name, h in hits.items():
            z[name] = h.cpu().numpy()
        np.savez(os.path.join(tmp, "hits.npz"), **z)
        prof = os.path.join(tmp, "prof")
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "sp", "--output-format", "csv",
               "--", sys.executable, os.path.abspath(__file__), "--surface-child", os.path.join(tmp, "hits.npz"), "--reps", str(a.reps)]
        t0 = time.time()
        rc = subprocess.run(cmd, timeout=900).returncode
        result["rocprof"] = {"rc": rc, "seconds": round(time.time() - t0, 1), "reps": a.reps}
        if rc == 0:
            trace = _kernel_trace(prof)
            surf = [(n, d) for n, d in trace if "k_hit_surface" in n]
            per_case = a.reps * len(rs)
            for ci, (set_name, what, material) in enumerate(SURFACE_CASES):
                part = surf[ci * per_case:(ci + 1) * per_case]
                entry = result["cases"][set_name + "_" + what]
                entry["kernel"] = {}
                for vi, (name, _) in enumerate(rs):
                    ds = sorted(d for _, d in part[vi::len(rs)])
                    if not ds:
                        continue
                    med_ns = ds[len(ds) // 2]
                    nh = entry["hits"]
                    gbs = entry["algorithmic_bytes_per_hit"] * nh / med_ns
                    entry["kernel"][name] = {"median_ms": round(med_ns * 1e-6, 4), "ns_per_hit": round(med_ns / nh, 3), "mhits_per_s": round(nh / med_ns * 1e3, 1),
                                             "algorithmic_GB_s": round(gbs, 1), "share_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4), "launches": len(ds)}
            shade = [d for n, d in trace if "k_wf_shade" in n]
            cnt = json.load(open(z["counters_out"]))
            records = int(cnt["rays_closest"])  # every closest-hit ray of the frame leaves one record for k_wf_shade (hit or miss)
            if shade and records:
                result["k_wf_shade"] = {"frame": "1920x1080, 1 spp, depth 8", "launches": len(shade), "total_ms": round(sum(shade) * 1e-6, 4), "records": records,
                                        "hits": int(cnt["hits"]), "ns_per_record": round(sum(shade) / records, 3),
                                        "note": "records = closest-hit rays of the frame, hits and misses; the kernel also evaluates the BRDF and streams the path records"}
            result["kernel_stats"] = {n: {"calls": c, "total_ms": round(t * 1e-6, 3)} for n, (c, t) in _kernel_stats(prof).items()
                                      if "k_hit_surface" in n or "k_wf_shade" in n}
            print("kernel", json.dumps({k: v.get("kernel") for k, v in result["cases"].items()}), flush=True)
            print("k_wf_shade", json.dumps(result.get("k_wf_shade")), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)
    for _, rr in rs:
        rr.close()


# ---- the multi-hit leg -----------------------------------------------------------------------------------------------------------
MULTI_KS = (1, 2, 4, 8, 16)
MULTI_RESOURCES = os.path.join(ROOT, "profiles", "r06_multihit_kernel_resources.json")


def multi_resources():
    """Registers, scratch and static LDS of every k_query_multi instantiation from the compiler's metadata (cross-compiles: no GPU)."""
    import re

    csrc = os.path.join(ROOT, "vk-raytracing-engine_amd", "csrc")
    tmp = tempfile.mkdtemp(prefix="multihit_isa_")
    try:
        asm = os.path.join(tmp, "multihit.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-mllvm",
                        "-amdgpu-sched-strategy=max-memory-clause", "-fno-slp-vectorize", "--cuda-device-only", "-S", "-o", asm, "multihit.hip"],
                       cwd=csrc, check=True, stderr=subprocess.DEVNULL)
        text = open(asm).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    kernels = {}
    for block in text.split("  - .agpr_count:")[1:]:
        f = {k: v for k, v in re.findall(r"\.(name|vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count):\s+(\S+)", block)}
        m = re.match(r"_Z13k_query_multiILb([01])ELi(\d+)EE", f.get("name", ""))
        if m:
            kernels[f"{'wide8' if m.group(1) == '1' else 'bvh2'}_tm{m.group(2)}"] = {
                "vgprs": int(f["vgpr_count"]), "sgprs": int(f["sgpr_count"]), "scratch_bytes": int(f["private_segment_fixed_size"]),
                "vgpr_spills": int(f["vgpr_spill_count"]), "static_lds_bytes": int(f["group_segment_fixed_size"])}
    out = {"kernels": kernels, "max_vgprs": max(k["vgprs"] for k in kernels.values()), "max_scratch_bytes": max(k["scratch_bytes"] for k in kernels.values()),
           "dynamic_lds_bytes_per_wave": "256 x stack words of the tree (2 x (depth + 1) on the wide8 layout) + 1280 x max_hits"}
    with open(MULTI_RESOURCES, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", MULTI_RESOURCES, json.dumps({k: out[k] for k in ("max_vgprs", "max_scratch_bytes")}))


def multi_leg(a):
    import torch
    import atrium
    import vkrt_amd
    from vkrt_amd.renderer import Renderer, pack_rays

    flat, _ = atrium.build_atrium(262144, seed=1, with_textures=False)
    W, H = 1920, 1080
    r = Renderer(flat, device=0, build=a.build)
    info = r.accel_info()
    sets = ray_sets(flat, dict(atrium.DEFAULT_CAMERA), W, H, r, a.seed)
    result = {"source_hash": vkrt_amd.source_hash(), "scene": "atrium 262144 seed 1", "triangles": int(info["triangle_count"]), "build": a.build,
              "device": torch.cuda.get_device_name(0), "warmup_calls": 3, "timed_calls_each": a.multi_calls,
              "method": "device events around every call, multi-hit and peeling alternating; medians", "sets": {}}
    if os.path.exists(MULTI_RESOURCES):
        result["kernel_resources"] = json.load(open(MULTI_RESOURCES))
    stack_words = 2 * (int(info["max_depth"]) + 1)
    result["lds_bytes_per_wave"] = {str(k): 256 * stack_words + 1280 * k for k in MULTI_KS}
    r.reset_counters()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    for name in ("camera", "diffuse"):
        o, d, lo, hi = sets[name]
        n = int(o.shape[0])
        od, dd = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        rays = pack_rays(od, dd, tmin=torch.from_numpy(lo).cuda(), tmax=torch.from_numpy(hi).cuda())
        # the rays of every peeling pass, prepared beforehand
        passes, cur = [], rays
        alive = []
        for _ in range(max(MULTI_KS)):
            passes.append(cur)
            h = r.intersect(cur)
            hit = h.triangle >= 0
            alive.append(int(hit.sum()))
            nxt = cur.clone()
            nxt[:, 3] = torch.where(hit, h.t, cur[:, 7])
            cur = nxt
        torch.cuda.synchronize()
        single = torch.empty((n, 8), dtype=torch.float32, device="cuda:0")
        entry = {"rays": n, "hits_per_peeling_pass": alive, "k": {}}
        for k in MULTI_KS:
            out = torch.empty((n, k, 8), dtype=torch.float32, device="cuda:0")
            cnt = torch.empty((n,), dtype=torch.int32, device="cuda:0")
            multi = lambda: r.intersect_multi(rays, k, out=out, counts=cnt)  # noqa: E731
            peel = lambda: [r.intersect(passes[j], out=single) for j in range(k)]  # noqa: E731
            for _ in range(3):
                multi()
                peel()
            torch.cuda.synchronize()
            ev = {"multi": [], "peel": []}
            for _ in range(a.multi_calls):
                ev["multi"].append(timed(multi))
                ev["peel"].append(timed(peel))
            torch.cuda.synchronize()
            ms = {w: sorted(e0.elapsed_time(e1) for e0, e1 in ev[w]) for w in ev}
            med = {w: ms[w][len(ms[w]) // 2] for w in ms}
            returned = int(cnt.sum())
            entry["k"][str(k)] = {"multi_ms": round(med["multi"], 4), "peel_ms": round(med["peel"], 4), "ratio_multi_over_peel": round(med["multi"] / med["peel"], 4),
                                  "multi_ms_min_max": [round(ms["multi"][0], 4), round(ms["multi"][-1], 4)],
                                  "peel_ms_min_max": [round(ms["peel"][0], 4), round(ms["peel"][-1], 4)],
                                  "multi_mrays_per_s": round(n / med["multi"] * 1e-3, 1), "hits_returned": returned,
                                  "multi_mhits_per_s": round(returned / med["multi"] * 1e-3, 1), "full_lists": int((cnt == k).sum())}
            print(name, k, json.dumps(entry["k"][str(k)]), flush=True)
        e = [timed(lambda: r.intersect(rays, out=single)) for _ in range(a.multi_calls)]
        torch.cuda.synchronize()
        one = sorted(e0.elapsed_time(e1) for e0, e1 in e)
        entry["intersect_ms"] = round(one[len(one) // 2], 4)
        entry["k1_over_intersect"] = round(entry["k"]["1"]["multi_ms"] / entry["intersect_ms"], 4)  # (reported, not gated: no shared walk)
        result["sets"][name] = entry
    result["traversal_faults"] = int(r.counters()["traversal_faults"])
    result["required_ratio_le_1"] = {f"{name}_k{k}": result["sets"][name]["k"][str(k)]["ratio_multi_over_peel"] <= 1.0 for name in ("camera", "diffuse")
                                     for k in (4, 8)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out, json.dumps(result["required_ratio_le_1"]))
    r.close()


ALPHA_RESOURCES = os.path.join(ROOT, "profiles", "alpha_cutout_kernel_resources.json")
ALPHA_MATERIALS = (10, 11, 12, 13)  # the drapery of tools/atrium.py


def alpha_resources():
    """Registers, scratch and spills of every k_query / k_query_multi instantiation with the alpha-test stage (VKRT_TM_ALPHA = 16) from the
    compiler's metadata, each next to the instantiation without the bit (cross-compiles: no GPU), and the units' compile times."""
    import re

    csrc = os.path.join(ROOT, "vk-raytracing-engine_amd", "csrc")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-mllvm", "-amdgpu-sched-strategy=max-memory-clause",
             "-fno-slp-vectorize", "--cuda-device-only", "-S"]
    names = {"vgpr_count": "vgprs", "sgpr_count": "sgprs", "private_segment_fixed_size": "scratch_bytes", "vgpr_spill_count": "vgpr_spills",
             "sgpr_spill_count": "sgpr_spills_to_vgpr_lanes", "group_segment_fixed_size": "static_lds_bytes"}
    out = {"hipcc": subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()[0], "flags": " ".join(flags[:-2]),
           "note": "tm = the triangle mode (traverse.h): 1 watertight, 2 dissolve, 8 filter, 16 alpha test; the stage is instantiated with the filter only "
                   "(24..27).  without_stage = the same kernel with tm - 16.  SGPR spills go to VGPR lanes (v_writelane / v_readlane): scratch stays 0.",
           "kernels": {}, "compile_seconds": {}}
    tmp = tempfile.mkdtemp(prefix="alpha_isa_")
    try:
        for unit, pat in (("query", r"_Z7k_queryILb([01])ELb([01])ELi(\d+)EE"), ("multihit", r"_Z13k_query_multiILb([01])ELi(\d+)EE")):
            asm = os.path.join(tmp, unit + ".s")
            t0 = time.time()
            subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-o", asm, unit + ".hip"], cwd=csrc, check=True, stderr=subprocess.DEVNULL)
            out["compile_seconds"][unit + ".hip"] = round(time.time() - t0, 1)
            found = {}
            for block in open(asm).read().split("  - .agpr_count:")[1:]:
                f = {k: v for k, v in re.findall(r"\.(name|" + "|".join(names) + r"):\s+(\S+)", block)}
                m = re.match(pat, f.get("name", ""))
                if m:
                    g = m.groups()
                    kind = ("occluded" if g[0] == "1" else "intersect") + ("_wide8" if g[1] == "1" else "_bvh2") if unit == "query" else \
                        "multi" + ("_wide8" if g[0] == "1" else "_bvh2")
                    found[(kind, int(g[-1]))] = {names[k]: int(f[k]) for k in names}
            for (kind, tm), res in sorted(found.items()):
                if tm & 16:
                    out["kernels"][f"{kind}_tm{tm}"] = dict(res, without_stage=found[(kind, tm - 16)])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    ks = out["kernels"].values()
    out["max_vgprs"] = max(k["vgprs"] for k in ks)
    out["max_scratch_bytes"] = max(k["scratch_bytes"] for k in ks)
    out["max_vgpr_spills"] = max(k["vgpr_spills"] for k in ks)
    with open(ALPHA_RESOURCES, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", ALPHA_RESOURCES, json.dumps({k: out[k] for k in ("max_vgprs", "max_scratch_bytes", "max_vgpr_spills", "compile_seconds")}))


def _alpha_pattern(h, w, block, salt):
    """uint8 [h, w]: a hash that is constant over block x block texels -- cut-outs with interiors and edges"""
    y, x = np.mgrid[0:h, 0:w]
    v = ((x // block).astype(np.uint64) * np.uint64(73856093)) ^ ((y // block).astype(np.uint64) * np.uint64(19349663)) ^ np.uint64(salt * 83492791)
    return (((v * np.uint64(2654435761)) >> np.uint64(7)) & np.uint64(255)).astype(np.uint8)


def alpha_leg(a):
    import copy

    import torch
    import atrium
    import vkrt_amd
    from vkrt_amd.renderer import ALPHA_MASK, Renderer, pack_rays

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
    W, H = 1920, 1080
    r = Renderer(flat, device=0, build=a.build)
    sets = ray_sets(flat, dict(atrium.DEFAULT_CAMERA), W, H, r, a.seed)
    nmat = len(flat.materials)
    modes = np.zeros(nmat, np.uint32)
    modes[list(ALPHA_MATERIALS)] = ALPHA_MASK
    cutoff = 0.5
    modes_t = torch.from_numpy(modes.astype(np.int64)).cuda()
    K = 8
    result = {"source_hash": vkrt_amd.source_hash(), "scene": "atrium 262144 seed 1, textured; materials 10..13 (drapery) MASK, cutoff 0.5, alpha = 32-texel hash blocks",
              "triangles": int(r.accel_info()["triangle_count"]), "build": a.build, "device": torch.cuda.get_device_name(0), "warmup_calls": 3,
              "timed_calls_each": a.multi_calls, "emulation": f"intersect_multi K = {K} + surface on {K} records per ray + select",
              "method": "device events around every call; stage, opaque and emulation alternate call by call, the modes are switched between the calls; medians",
              "sets": {}}
    if os.path.exists(ALPHA_RESOURCES):
        result["kernel_resources"] = {k: v for k, v in json.load(open(ALPHA_RESOURCES)).items() if k.startswith("max_") or k == "compile_seconds"}
    r.reset_counters()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    def stage(on):
        r.set_material_alpha(0, modes if on else np.zeros(nmat, np.uint32), cutoff)

    for name in ("camera", "diffuse", "shadow"):
        o, d, lo, hi = sets[name]
        n = int(o.shape[0])
        rays = pack_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), tmin=torch.from_numpy(lo).cuda(), tmax=torch.from_numpy(hi).cuda())
        hits = torch.empty((n, 8), dtype=torch.float32, device="cuda:0")
        occ = torch.empty((n,), dtype=torch.int32, device="cuda:0")
        mh = torch.empty((n, K, 8), dtype=torch.float32, device="cuda:0")
        cnt = torch.empty((n,), dtype=torch.int32, device="cuda:0")
        sb = torch.empty((n * K, 32), dtype=torch.float32, device="cuda:0")
        col = torch.arange(K, device="cuda:0")[None, :]
        chosen = {}

        def emulate():
            m = r.intersect_multi(rays, K, out=mh, counts=cnt)
            s = r.surface(m.flat(), out=sb)
            masked = modes_t[m.material.clamp(min=0).long()] == ALPHA_MASK
            adm = (col < cnt[:, None]) & (~masked | (s.alpha.view(n, K) >= cutoff))
            first = torch.argmax(adm.to(torch.int8), 1)
            chosen["hit"] = torch.where(adm.any(1)[:, None], mh[torch.arange(n, device="cuda:0"), first].view(torch.int32),
                                        torch.tensor([0, 0, 0, -1, -1, -1, -1, -1], dtype=torch.int32, device="cuda:0")[None, :])
            chosen["judged"] = adm.any(1) | (cnt < K)

        calls = {"intersect_stage": (True, lambda: r.intersect(rays, out=hits)), "intersect_opaque": (False, lambda: r.intersect(rays, out=hits)),
                 "occluded_stage": (True, lambda: r.occluded(rays, out=occ)), "occluded_opaque": (False, lambda: r.occluded(rays, out=occ)),
                 "emulation": (False, emulate)}
        for _ in range(3):
            for on, fn in calls.values():
                stage(on)
                fn()
        torch.cuda.synchronize()
        ev = {k: [] for k in calls}
        for _ in range(a.multi_calls):
            for k, (on, fn) in calls.items():
                stage(on)
                ev[k].append(timed(fn))
        torch.cuda.synchronize()
        ms = {k: sorted(e0.elapsed_time(e1) for e0, e1 in ev[k]) for k in ev}
        med = {k: ms[k][len(ms[k]) // 2] for k in ms}
        # what the stage decided, and that it is what the emulation selects (t, u, v bits and ids; misses: the ids) where the emulation can judge
        stage(False)
        plain = r.intersect(rays).buffer.view(torch.int32).clone()
        stage(True)
        got = r.intersect(rays).buffer.view(torch.int32).clone()
        got_occ = r.occluded(rays).clone()
        torch.cuda.synchronize()
        judged = chosen["judged"]
        hit = chosen["hit"][:, 3] >= 0
        same = torch.where(hit[:, None], got == chosen["hit"], got[:, 3:] .eq(-1).all(1)[:, None].expand(-1, 8)).all(1)
        entry = {"rays": n, "ms": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": {k: [round(ms[k][0], 4), round(ms[k][-1], 4)] for k in ms},
                 "mrays_per_s": {k: round(n / v * 1e-3, 1) for k, v in med.items()},
                 "ratio_intersect_stage_over_opaque": round(med["intersect_stage"] / med["intersect_opaque"], 4),
                 "ratio_occluded_stage_over_opaque": round(med["occluded_stage"] / med["occluded_opaque"], 4),
                 "ratio_intersect_stage_over_emulation": round(med["intersect_stage"] / med["emulation"], 4),
                 "opaque_hits_on_mask_materials": round(float((modes_t[plain[:, 7].clamp(min=0).long()].eq(ALPHA_MASK) & (plain[:, 3] >= 0)).float().mean()), 4),
                 "rays_the_stage_changes": round(float((got != plain).any(1).float().mean()), 4),
                 "occluded_fraction_stage": round(float(got_occ.float().mean()), 4),
                 "emulation_cannot_judge": int((~judged).sum()), "stage_differs_from_emulation_where_judged": int((judged & ~same).sum())}
        result["sets"][name] = entry
        print(name, json.dumps(entry), flush=True)
    result["traversal_faults"] = int(r.counters()["traversal_faults"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_query_probe.json"))
    ap.add_argument("--build", default="ploc")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5, help="launches of each kernel per set in the rocprofv3 run")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--surface", action="store_true", help="the vkrt_hit_surface leg instead of the ray-query legs")
    ap.add_argument("--variant-lib", default=None, help="surface leg: a second build of the library to measure beside the product build")
    ap.add_argument("--variant-name", default="variant")
    ap.add_argument("--surface-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--multi", action="store_true", help="the vkrt_intersect_multi leg: multi-hit calls against peeling with vkrt_intersect")
    ap.add_argument("--multi-calls", type=int, default=15, help="multi leg: timed calls of each kind per K and ray set")
    ap.add_argument("--multi-resources", action="store_true", help="registers / scratch / LDS of k_query_multi from the compiler (no GPU)")
    ap.add_argument("--alpha", action="store_true", help="the alpha-test leg: queries with MASK materials against opaque ones and against the emulation")
    ap.add_argument("--alpha-resources", action="store_true", help="registers / scratch / spills of the kernels with the alpha-test stage (no GPU)")
    a = ap.parse_args()
    if a.alpha_resources:
        alpha_resources()
        return
    if a.alpha:
        if a.out.endswith("r06_query_probe.json"):
            a.out = os.path.join(ROOT, "profiles", "alpha_cutout_probe.json")
        alpha_leg(a)
        return
    if a.multi_resources:
        multi_resources()
        return
    if a.multi:
        if a.out.endswith("r06_query_probe.json"):
            a.out = os.path.join(ROOT, "profiles", "r06_multihit_probe.json")
        multi_leg(a)
        return
    if a.child:
        _child(a.child, a.reps)
        return
    if a.surface_child:
        _surface_child(a.surface_child, a.reps)
        return
    if a.surface:
        if a.out.endswith("r06_query_probe.json"):
            a.out = os.path.join(ROOT, "profiles", "r06_surface_probe.json")
        surface_leg(a)
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
