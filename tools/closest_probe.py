#!/usr/bin/env python3
"""What vkrt_closest_point costs (Renderer.closest_point, csrc/closest.hip).

On the bench atrium (262144 triangles) and on atrium_small (20000, the scene of the tests), on both layouts, for three query sets with
radius = inf --
  surface   points at random barycentrics of random triangles (distance ~ 0: the collision / snapping case),
  near      those points moved by up to 1 % of the scene's extent in a random direction (signed-distance sampling near the surface),
  uniform   points uniform in the bounds padded by 10 % (the worst case: far from everything, many boxes at similar distances)
-- it reports queries/s (event-timed, whole calls) and the averages of the work hook (vkrt_debug_closest_point_work): nodes visited
and triangle records tested per query.  It records the hipcc version and, from the compiler's metadata, the registers and scratch of
every k_closest_point instantiation.  --variant-lib names a second build of the library to time beside the product build: the
experiment "the triangle function in binary32" is such a build, made from a working-tree edit that is not part of the sources.

None of the numbers is a gate: there is no earlier implementation to compare with.

    python tools/closest_probe.py [--out profiles/closest_point_probe.json] [--variant-lib PATH --variant-name NAME]
"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


def _world_triangles(flat):
    out = []
    for node in flat.nodes:
        pm = flat.prim_meshes[node["primMesh"]]
        idx = flat.indices[int(pm["firstIndex"]): int(pm["firstIndex"]) + int(pm["indexCount"])].astype(np.int64) + int(pm["vertexOffset"])
        M = np.asarray(node["worldMatrix"], np.float64).reshape(4, 4).T
        out.append((np.c_[flat.positions[idx].astype(np.float64), np.ones(len(idx))] @ M.T)[:, :3].reshape(-1, 3, 3))
    return np.concatenate(out)


def query_sets(flat, n, seed):
    rng = np.random.default_rng(seed)
    tri = _world_triangles(flat)
    lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
    ext = float(np.linalg.norm(hi - lo))
    k = rng.integers(0, len(tri), n)
    w = rng.dirichlet((1, 1, 1), n)
    surface = (tri[k] * w[:, :, None]).sum(1)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    near = surface + d * (rng.random((n, 1)) * 0.01 * ext)
    uniform = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (n, 3))
    return {name: np.ascontiguousarray(p, np.float32) for name, p in (("surface", surface), ("near", near), ("uniform", uniform))}, ext


def hipcc_version():
    if not HIPCC:
        return None
    out = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout
    m = re.search(r"HIP version:\s*(\S+)", out)
    return m.group(1) if m else "unknown"


def kernel_resources():
    """Registers and scratch of every k_closest_point instantiation from the compiler's metadata, with the flags of csrc/Makefile."""
    if not HIPCC:
        return None
    csrc = os.path.join(ROOT, "vk-raytracing-engine_amd", "csrc")

    def var(name):
        for line in open(os.path.join(csrc, "Makefile")):
            m = re.match(rf"^{name}\s*[:?]?=\s*(.*)$", line)
            if m:
                return m.group(1).strip()
        return ""

    flags = var("FLAGS").replace("$(ARCH)", var("ARCH")).replace("-fPIC", "").split() + var("FLAGS_closest").split()
    tmp = tempfile.mkdtemp(prefix="closest_isa_")
    try:
        asm = os.path.join(tmp, "closest.s")
        subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", "-o", asm, "closest.hip"], cwd=csrc, check=True, stderr=subprocess.DEVNULL)
        text = open(asm).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    kernels = {}
    for block in text.split("  - .agpr_count:")[1:]:
        f = dict(re.findall(r"\.(name|vgpr_count|sgpr_count|private_segment_fixed_size|vgpr_spill_count):\s+(\S+)", block))
        m = re.match(r"_Z15k_closest_pointILb([01])ELb([01])ELb([01])EE", f.get("name", ""))
        if m:
            name = ("wide8" if m.group(1) == "1" else "bvh2") + ("_filter" if m.group(2) == "1" else "") + ("_count" if m.group(3) == "1" else "")
            kernels[name] = {"vgprs": int(f["vgpr_count"]), "sgprs": int(f["sgpr_count"]), "scratch_bytes": int(f["private_segment_fixed_size"]),
                             "vgpr_spills": int(f["vgpr_spill_count"])}
    return kernels


def renderer_of(lib_path, flat, layout):
    """A Renderer on its own copy of the library (None: the product build the package names)."""
    from vkrt_amd import abi, renderer

    opts = {abi.VKRT_OPT_BVH_LAYOUT: layout}
    if lib_path is None:
        return renderer.Renderer(flat, device=0, build="ploc", options=opts)
    renderer.load_library()
    saved, renderer._lib = renderer._lib, abi.declare_vkrt(C.CDLL(os.path.abspath(lib_path)))
    try:
        return renderer.Renderer(flat, device=0, build="ploc", options=opts)
    finally:
        renderer._lib = saved


def time_call(r, q, min_seconds):
    """ms per call of closest_point on the device tensor q ([N, 4]), event-timed over enough calls to fill min_seconds"""
    import torch

    out = torch.empty((q.shape[0], 8), dtype=torch.float32, device=q.device)
    for _ in range(2):
        r.closest_point(q, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r.closest_point(q, out=out)
    e1.record()
    torch.cuda.synchronize()
    k = int(min(200, max(3, min_seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(k):
        r.closest_point(q, out=out)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closest_point_probe.json"))
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--work-queries", type=int, default=1 << 16, help="queries of each set handed to the work hook")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--variant-lib", default=None, help="a second build of the library to time beside the product build")
    ap.add_argument("--variant-name", default="variant")
    a = ap.parse_args()

    import torch
    import atrium

    result = {"hipcc": hipcc_version(), "device": torch.cuda.get_device_name(0), "queries": a.queries, "work_queries": a.work_queries, "radius": "inf",
              "build": "ploc", "kernels": kernel_resources(), "scenes": {}}
    for scene_name, tris, seed in (("atrium", 262144, 1), ("atrium_small", 20000, 4)):
        flat, _ = atrium.build_atrium(tris, seed=seed, with_textures=False)
        sets, ext = query_sets(flat, a.queries, a.seed)
        entry = result["scenes"][scene_name] = {"extent": ext, "layouts": {}}
        for layout, layout_name in ((1, "wide8"), (0, "bvh2")):
            libs = [("product", None)] + ([(a.variant_name, a.variant_lib)] if a.variant_lib else [])
            rs = {name: renderer_of(path, flat, layout) for name, path in libs}
            info = rs["product"].accel_info()
            le = entry["layouts"][layout_name] = {"triangle_count": int(info["triangle_count"]), "reference_count": int(info["reference_count"]), "sets": {}}
            for set_name, pts in sets.items():
                q = torch.as_tensor(np.concatenate([pts, np.full((len(pts), 1), np.inf, np.float32)], 1), device="cuda:0")
                se = le["sets"][set_name] = {}
                ref = None
                for name, r in rs.items():
                    ms, out = time_call(r, q, a.seconds)
                    se[name] = {"ms_per_call": ms, "mqueries_per_s": len(pts) / ms * 1e-3}
                    h = out.cpu().numpy()
                    if ref is None:
                        ref = h
                        se["mean_distance"] = float(h[:, 0].mean())
                    else:  # how far the variant's answers are from the product's
                        se[name]["records_that_differ"] = int((h.view(np.uint32) != ref.view(np.uint32)).any(1).sum())
                        se[name]["max_distance_difference"] = float(np.abs(h[:, 0] - ref[:, 0]).max())
                nodes, tested = rs["product"].closest_point_work(pts[:a.work_queries], radius=np.inf)
                m = min(a.work_queries, len(pts))
                se["nodes_per_query"], se["triangle_records_per_query"] = nodes / m, tested / m
                se["fraction_of_records_tested"] = tested / m / max(1, int(info["reference_count"]))
                print(scene_name, layout_name, set_name, json.dumps(se), flush=True)
            for r in rs.values():
                assert r.counters()["traversal_faults"] == 0
                r.close()
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
