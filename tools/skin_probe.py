"""Times skinning inside the library against what a caller did before, on the bench atrium (262 k triangles): writes
profiles/skin_probe.json.  Two configurations, 32 joints each: the eight hanging-cloth meshes as eight skins, and every vertex of the
scene as one skin.  Medians of --calls calls after --warmup, device events around every call, the variants alternating call by call in
one process (as tools/motion_probe.py does):

  a         vkrt_scene_skin_vertices from device matrices (one launch per skin)
  b         the same blend in torch on the device (gather the four joint matrices, weighted sum, transform, normalise) and
            Renderer.update_vertices on the device path (k_vertex_update), per skin
  a_refit   a followed by vkrt_accel_refit
  b_refit   b followed by vkrt_accel_refit

    python tools/skin_probe.py --out profiles/skin_probe.json [--triangles 262144]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "oracle", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md
JOINTS = 32
# k_skin per vertex: bind pose 40 B + joints 8 B + weights 16 B read; positions 12 B + the position, normal and tangent words of the
# record 40 B written (the four gathered joint matrices come from a 2 KiB palette in cache: not counted)
BYTES_READ, BYTES_WRITTEN = 40 + 8 + 16, 12 + 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.calls >= 20, "medians of at least 20 calls"

    import numpy as np
    import torch

    import atrium
    import scene_deform as sd
    import scene_skin as ss
    import vkrt_amd
    from motion_probe import _summary, _timed
    from vertex_update_probe import cloth_meshes
    from vkrt_amd.renderer import Renderer

    flat, _ = atrium.build_atrium(a.triangles, seed=1)
    V = len(flat.positions)
    dev = "cuda:0"
    res = {"workload": f"atrium{a.triangles}", "vertices": V, "joints": JOINTS, "source_hash": vkrt_amd.source_hash(), "hbm_peak_GB_s": HBM_PEAK_GBS,
           "bytes_per_vertex": {"read": BYTES_READ, "written": BYTES_WRITTEN},
           "method": f"medians of {a.calls} calls after {a.warmup}, device events around every call, variants alternating call by call"}

    def torch_blend(k, J):
        """what a caller wrote before: the blend of include/vkrt.h in torch (its own rounding: the sums are torch's), three SoA arrays"""
        Jm = J.view(-1, 4, 4)[:, :, :3]                                  # [joint, c, r]
        M = (k["w"][:, :, None, None] * Jm[k["j"]]).sum(1)               # [v, c, r]
        p = (M[:, :3] * k["p"][:, :, None]).sum(1) + M[:, 3]
        n = torch.nn.functional.normalize((M[:, :3] * k["n"][:, :, None]).sum(1), dim=1)
        t = torch.nn.functional.normalize((M[:, :3] * k["t"][:, :3, None]).sum(1), dim=1)
        return p.contiguous(), n.contiguous(), torch.cat([t, k["t"][:, 3:]], dim=1).contiguous()

    for name, ranges in (("cloths", [sd.mesh_range(flat, m) for m in cloth_meshes(flat)]), ("all_vertices", [(0, V)])):
        r = Renderer(flat, device=0, build="ploc")
        skins = []
        for i, (first, count) in enumerate(ranges):
            j, w = ss.influences(flat, first, count, JOINTS, 70 + i)
            sl = slice(first, first + count)
            skins.append({"first": first, "count": count, "id": r.add_skin(first, j, w, joint_count=JOINTS),
                          "j": torch.as_tensor(j.astype(np.int64), device=dev), "w": torch.as_tensor(w, device=dev),
                          "p": torch.as_tensor(flat.positions[sl], device=dev), "n": torch.as_tensor(flat.normals[sl], device=dev),
                          "t": torch.as_tensor(flat.tangents[sl], device=dev)})
        poses = [torch.as_tensor(ss.joint_matrices(JOINTS, 80 + i, amount=0.05), device=dev) for i in range(2)]
        r.refit()  # (the first refit of a build allocates and synchronises: done before the timing)
        turn = [0]

        def lib_skin():
            turn[0] += 1
            for k in skins:
                r.skin(k["id"], poses[turn[0] & 1])

        def caller_skin():
            turn[0] += 1
            for k in skins:
                p, n, t = torch_blend(k, poses[turn[0] & 1])
                r.update_vertices(k["first"], positions=p, normals=n, tangents=t)

        def then_refit(f):
            def g():
                f()
                r.refit()
            return g

        s = _timed({"a_skin_vertices": lib_skin, "b_torch_blend_update_vertices": caller_skin, "a_refit": then_refit(lib_skin),
                    "b_refit": then_refit(caller_skin)}, a.calls, a.warmup)
        out = _summary(s)
        n = sum(k["count"] for k in skins)
        moved = n * (BYTES_READ + BYTES_WRITTEN)
        rate = moved / (out["a_skin_vertices"]["median_ms"] * 1e6)
        out.update(skins=len(skins), vertices=n, bytes_moved_per_call=moved, a_GB_s=rate, a_frac_of_hbm_peak=rate / HBM_PEAK_GBS,
                   b_over_a=out["b_torch_blend_update_vertices"]["median_ms"] / out["a_skin_vertices"]["median_ms"],
                   b_refit_over_a_refit=out["b_refit"]["median_ms"] / out["a_refit"]["median_ms"])
        res[name] = out
        r.close()
    res["note"] = ("launches this small are latency-bound and the arrays stay in the last-level cache between calls: a_frac_of_hbm_peak is bytes "
                   "over call time, no HBM streaming rate.  b's torch blend rounds its sums in torch's order, so its vertices are close to, not "
                   "bit for bit, what a writes.")
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
