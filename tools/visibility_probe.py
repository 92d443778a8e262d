"""Cost of instance masks and ray flags in the ray queries (vkrt_intersect_ex / vkrt_occluded_ex) on the bench atrium (262 k triangles,
175 instances), with the ray sets of tools/query_probe.py (1080p camera rays, cosine-diffuse rays from their hits, shadow rays):

  defaults     vkrt_intersect_ex with {flags 0, cull mask 0xFF} against vkrt_intersect: the same kernel, the same rate expected;
  half         masks 1 / 2 on alternate instances, cull mask 1, against the same rays on a scene of the admitted instances (its own tree);
  masked_out   rays aimed at the instances of one half of the building, those instances masked out: the filtered walk against the
               unfiltered one on wide8 (the node-mask table prunes the masked subtrees) and on BVH2 (no table: filtered at the triangles);
  cull_back    VKRT_RAY_CULL_BACK_FACING on every instance (FACING_CULL_DISABLE cleared) against no culling.

Rates from device events around back-to-back launches on one stream (at least --seconds per measurement after a warm-up).

  python tools/visibility_probe.py --out profiles/r06_visibility_probe.json
"""
import argparse
import copy
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def rate(call, n, seconds):
    """Mrays/s and ms per launch of call() from device events"""
    import torch

    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    k = int(min(5000, max(10, np.ceil(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)))))
    e0.record()
    for _ in range(k):
        call()
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / k
    return {"mrays_per_s": round(n / ms * 1e-3, 1), "ms_per_launch": round(ms, 4), "launches": k}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_visibility_probe.json"))
    ap.add_argument("--build", default="ploc")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.5)
    a = ap.parse_args()

    import torch
    import atrium
    import vkrt_amd
    from query_probe import ray_sets
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer, pack_rays

    flat, _ = atrium.build_atrium(262144, seed=1, with_textures=False)
    W, H = 1920, 1080
    r = Renderer(flat, device=0, build=a.build)
    sets = ray_sets(flat, dict(atrium.DEFAULT_CAMERA), W, H, r, a.seed)
    packed = {}
    for name in ("camera", "diffuse", "shadow"):
        o, d, lo, hi = sets[name]
        packed[name] = pack_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), tmin=torch.from_numpy(lo).cuda(), tmax=torch.from_numpy(hi).cuda())
    nodes = len(flat.nodes)
    result = {"source_hash": vkrt_amd.source_hash(), "scene": "atrium 262144 seed 1", "instances": nodes, "build": a.build,
              "device": torch.cuda.get_device_name(0), "seconds_per_measurement": a.seconds}

    def run(rr, rays, occ, **kw):
        n = rays.shape[0]
        out = torch.empty((n,), dtype=torch.int32, device="cuda") if occ else torch.empty((n, 8), dtype=torch.float32, device="cuda")
        fn = rr.occluded if occ else rr.intersect
        return rate(lambda: fn(rays, out=out, **kw), n, a.seconds)

    def run_ex_defaults(rr, rays, occ):
        n = rays.shape[0]
        out = torch.empty((n,), dtype=torch.int32, device="cuda") if occ else torch.empty((n, 8), dtype=torch.float32, device="cuda")
        o = abi.QueryOpts(16, 0, 0xFF, 0)
        fn = rr.lib.vkrt_occluded_ex if occ else rr.lib.vkrt_intersect_ex
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        return rate(lambda: fn(rr._h, C.c_void_p(rays.data_ptr()), n, C.byref(o), C.c_void_p(out.data_ptr()), st), n, a.seconds)

    # defaults
    result["defaults"] = {}
    for name, rays in packed.items():
        occ = name == "shadow"
        result["defaults"][name] = {"vkrt_intersect" if not occ else "vkrt_occluded": run(r, rays, occ), "_ex": run_ex_defaults(r, rays, occ)}
        print("defaults", name, json.dumps(result["defaults"][name]), flush=True)

    # half the instances, against the sub-scene's own tree
    masks = (np.arange(nodes) % 2 + 1).astype(np.uint8)
    r.set_instance_visibility(0, masks, None)
    sub = copy.copy(flat)
    sub.nodes = flat.nodes[masks == 1].copy()
    rs = Renderer(sub, device=0, build=a.build)
    result["half"] = {}
    for name, rays in packed.items():
        occ = name == "shadow"
        result["half"][name] = {"masked_cull_1": run(r, rays, occ, cull_mask=1), "sub_scene": run(rs, rays, occ)}
        print("half", name, json.dumps(result["half"][name]), flush=True)
    rs.close()

    # rays into a masked-out region: camera rays whose primary hit is on an instance of the x > centre half; those instances masked out
    o, d, lo, hi = sets["camera"]
    h = r.intersect(packed["camera"])
    torch.cuda.synchronize()
    inst = h.instance.cpu().numpy()
    tx = np.array([np.asarray(n["worldMatrix"], np.float64).reshape(4, 4).T[0, 3] for n in flat.nodes])
    far = tx > np.median(tx)
    aim = (inst >= 0) & far[np.maximum(inst, 0)]
    rays_aim = pack_rays(torch.from_numpy(o[aim]).cuda(), torch.from_numpy(d[aim]).cuda(), tmin=0.001, tmax=1e4)
    vm = np.where(far, 2, 1).astype(np.uint8)
    result["masked_out"] = {"rays": int(aim.sum()), "instances_masked": int(far.sum())}
    for layout in (1, 0):
        rl = r if layout == 1 else Renderer(flat, device=0, build=a.build, options={abi.VKRT_OPT_BVH_LAYOUT: 0})
        rl.set_instance_visibility(0, vm, None)
        key = "wide8_node_table" if layout == 1 else "bvh2_triangles_only"
        result["masked_out"][key] = {"unfiltered": run(rl, rays_aim, False), "cull_mask_1": run(rl, rays_aim, False, cull_mask=1)}
        print("masked_out", key, json.dumps(result["masked_out"][key]), flush=True)
        if rl is not r:
            rl.close()

    # back-face culling
    r.set_instance_visibility(0, np.full(nodes, 0xFF, np.uint8), np.zeros(nodes, np.uint8))
    result["cull_back"] = {}
    for name in ("camera", "diffuse"):
        rays = packed[name]
        result["cull_back"][name] = {"no_culling": run(r, rays, False), "cull_back_facing": run(r, rays, False, ray_flags=abi.VKRT_RAY_CULL_BACK_FACING)}
        print("cull_back", name, json.dumps(result["cull_back"][name]), flush=True)
    result["traversal_faults"] = int(r.counters()["traversal_faults"])
    r.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
