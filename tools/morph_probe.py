"""Times morph targets inside the library against what a caller did before, on the bench atrium (262 k triangles): writes
profiles/morph_probe.json.  One configuration: every vertex of the scene as one morph with 32 targets of position, normal and tangent
deltas, 4 of them with a non-zero weight.  Medians of --calls calls after --warmup, device events around every call, the variants
alternating call by call in one process (as tools/skin_probe.py does):

  a         vkrt_scene_morph_vertices from device weights (one launch)
  b         the same blend in torch on the device over the 4 active targets (base + sum w * delta, normalise) and
            Renderer.update_vertices on the device path (k_vertex_update)
  a_refit   a followed by vkrt_accel_refit
  b_refit   b followed by vkrt_accel_refit

The measurement runs in a child process under a time limit of its own (--limit seconds); the parent never opens the device and stops
at the child's first failure.

    python tools/morph_probe.py --out profiles/morph_probe.json [--triangles 262144]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "oracle", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md
TARGETS, ACTIVE = 32, (3, 11, 12, 30)
# k_morph_live per vertex: the captured base 40 B read; positions 12 B + the position, normal and tangent words of the record 40 B
# written; per target with a non-zero weight three vec3 deltas, 36 B, read
BYTES_BASE, BYTES_WRITTEN, BYTES_PER_ACTIVE_TARGET = 40, 12 + 40, 36


def measure(a):
    import numpy as np
    import torch

    import atrium
    import vkrt_amd
    from motion_probe import _summary, _timed
    from vkrt_amd.renderer import Renderer

    flat, _ = atrium.build_atrium(a.triangles, seed=1)
    V = len(flat.positions)
    dev = "cuda:0"
    res = {"workload": f"atrium{a.triangles}", "vertices": V, "targets": TARGETS, "active_targets": len(ACTIVE), "source_hash": vkrt_amd.source_hash(),
           "hbm_peak_GB_s": HBM_PEAK_GBS,
           "bytes_per_vertex": {"base_read": BYTES_BASE, "written": BYTES_WRITTEN, "read_per_active_target": BYTES_PER_ACTIVE_TARGET},
           "method": f"medians of {a.calls} calls after {a.warmup}, device events around every call, variants alternating call by call"}
    rng = np.random.default_rng(7)
    ext = float(np.abs(flat.positions).max())
    d = [np.ascontiguousarray(rng.uniform(-s, s, (TARGETS, V, 3)), np.float32) for s in (0.002 * ext, 0.05, 0.05)]
    r = Renderer(flat, device=0, build="ploc")
    morph = r.add_morph(0, position_deltas=d[0], normal_deltas=d[1], tangent_deltas=d[2])
    poses = []
    for i in range(2):
        w = np.zeros(TARGETS, np.float32)
        w[list(ACTIVE)] = rng.uniform(0.2, 1.0, len(ACTIVE)).astype(np.float32) * (1 if i else -1)
        poses.append(torch.as_tensor(w, device=dev))
    act = torch.as_tensor(list(ACTIVE), device=dev)
    dP, dN, dT = (torch.as_tensor(np.ascontiguousarray(x[list(ACTIVE)]), device=dev) for x in d)  # the caller keeps the active targets
    bp, bn, bt = (torch.as_tensor(x, device=dev) for x in (flat.positions, flat.normals, flat.tangents))
    r.refit()  # (the first refit of a build allocates and synchronises: done before the timing)
    turn = [0]

    def lib_morph():
        turn[0] += 1
        r.morph(morph, poses[turn[0] & 1])

    def caller_morph():
        """what a caller wrote before: the blend of include/vkrt.h in torch (its own rounding: the sums are torch's), three SoA arrays"""
        turn[0] += 1
        w = poses[turn[0] & 1][act][:, None, None]
        p = bp + (w * dP).sum(0)
        n = torch.nn.functional.normalize(bn + (w * dN).sum(0), dim=1)
        t = torch.nn.functional.normalize(bt[:, :3] + (w * dT).sum(0), dim=1)
        r.update_vertices(0, positions=p.contiguous(), normals=n.contiguous(), tangents=torch.cat([t, bt[:, 3:]], dim=1).contiguous())

    def then_refit(f):
        def g():
            f()
            r.refit()
        return g

    s = _timed({"a_morph_vertices": lib_morph, "b_torch_blend_update_vertices": caller_morph, "a_refit": then_refit(lib_morph),
                "b_refit": then_refit(caller_morph)}, a.calls, a.warmup)
    out = _summary(s)
    moved = V * (BYTES_BASE + BYTES_WRITTEN + BYTES_PER_ACTIVE_TARGET * len(ACTIVE))
    rate = moved / (out["a_morph_vertices"]["median_ms"] * 1e6)
    out.update(bytes_moved_per_call=moved, a_GB_s=rate, a_frac_of_hbm_peak=rate / HBM_PEAK_GBS,
               b_over_a=out["b_torch_blend_update_vertices"]["median_ms"] / out["a_morph_vertices"]["median_ms"],
               b_refit_over_a_refit=out["b_refit"]["median_ms"] / out["a_refit"]["median_ms"])
    out["a_not_slower_than_b"] = bool(out["a_morph_vertices"]["median_ms"] <= out["b_torch_blend_update_vertices"]["median_ms"]
                                      and out["a_refit"]["median_ms"] <= out["b_refit"]["median_ms"])
    res["all_vertices"] = out
    assert r.counters()["traversal_faults"] == 0
    r.close()
    res["note"] = ("a launch this small is latency-bound and the arrays stay in the last-level cache between calls: a_frac_of_hbm_peak is bytes "
                   "over call time, no HBM streaming rate.  b's torch blend rounds its sums in torch's order, so its vertices are close to, not "
                   "bit for bit, what a writes.")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--limit", type=int, default=240, help="seconds the measuring child process may take")
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert a.calls >= 20, "medians of at least 20 calls"
    if a.child:
        print("MORPH_PROBE " + json.dumps(measure(a)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--warmup", str(a.warmup), "--triangles", str(a.triangles)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    except subprocess.TimeoutExpired:
        print(f"morph_probe: the measurement did not finish within {a.limit} s", file=sys.stderr)
        return 124
    lines = [x for x in p.stdout.splitlines() if x.startswith("MORPH_PROBE ")]
    if p.returncode != 0 or not lines:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        return p.returncode or 1
    line = json.dumps(json.loads(lines[-1][len("MORPH_PROBE "):]), indent=1)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
