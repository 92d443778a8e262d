"""Times vkrt_denoise_diffuse on the BASELINE config-5 stand-in (atrium, 1920x1080, hybrid with shadows + AO + GI depth 8; planes made
once), and writes the result with the compulsory HBM bytes of every kernel, computed from the plane shapes.

  python tools/denoise_probe.py --out timing.json                      # on the GPU: events around 50 calls after 5 warm-up calls
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/denoise_probe.py --calls 10   # per-kernel durations (a run of its own)
  rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAVES GRBM_GUI_ACTIVE \
      -d DIR2 -- python tools/denoise_probe.py --calls 10                                 # counters (a run of its own)
  python tools/denoise_probe.py --merge timing.json --stats DIR/.../kernel_stats.csv --pmc DIR2/.../counter_collection.csv \
      --out profiles/r06_denoise_probe.json
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK_GBS = 8000.0
W, H, ITER = 1920, 1080, 5
# compulsory bytes per pixel (each plane read / written once; taps of neighbours are served by L1 / L2)
BYTES = {
    # reads: position, normal, color 16 each, roughMetal 8, viewZ 4, radiance 16, history geometry / moments / colour 16 each;
    # writes: guide record, geometry, moments, colour 16 each
    "k_dn_temporal": (16 * 3 + 8 + 4 + 16 + 16 * 3) + 16 * 4,
    "k_dn_variance": (16 * 3) + 16,             # record, moments, colour; (rgb, variance)
    "k_dn_atrous": (16 * 2) + 16,               # record, (rgb, variance); (rgb, variance)
    "k_dn_atrous_last_extra": (16 * 3 + 8) + 12,  # the last pass also reads the albedo planes and writes out.xyz
}


def measure(calls, warmup):
    import torch

    import atrium
    import camera_np
    from vkrt_amd.flat_scene import make_push_constants, uniforms_from_matrices
    from vkrt_amd.renderer import Denoiser, Renderer

    flat, _ = atrium.build_atrium(262144, seed=1)
    camkw = atrium.DEFAULT_CAMERA
    cam = uniforms_from_matrices(*camera_np.global_uniforms(width=W, height=H, **camkw))
    vm = camera_np.look_at(camkw["eye"], camkw["center"], camkw["up"]).astype("float32").T.reshape(-1)
    r = Renderer(flat, device=0, build="ploc")
    g = r.gbuffer_raycast(cam, W, H, lights_count=8, view_matrix=vm)
    pc = make_push_constants(samples=1, depth=8, frame=0, lights_count=8)
    pc.useShadows, pc.useAO, pc.useGI = 1, 1, 1
    acc = r.hybrid_trace(pc, cam, W, H, g, seed=1)
    out = acc.clone()
    dn = Denoiser(0, W, H)
    torch.cuda.synchronize()
    for _ in range(warmup):
        dn.denoise(cam, g, out=out, iterations=ITER)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        dn.denoise(cam, g, out=out, iterations=ITER)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / calls
    valid = float(((g["position"][..., :3] != 0).any(-1) | (g["normal"][..., :3] != 0).any(-1)).float().mean())
    dn.close()
    r.close()
    return {"ms_per_call": ms, "calls": calls, "warmup": warmup, "valid_pixel_fraction": valid}


def kernel_stats(path):
    rows = {}
    for row in csv.DictReader(open(path)):
        name = row["Name"].split("(")[0].replace("void ", "").strip()
        if name.startswith("k_dn_"):
            rows[name] = {"calls": int(row["Calls"]), "avg_ms": float(row["AverageNs"]) / 1e6}
    return rows


VALU_PEAK = 1228.8e9  # wave-instructions / s (MI355X_MICROARCH.md), the project's VALU-issue ceiling


def kernel_counters(path):
    """rocprofv3 --pmc counter_collection.csv: per k_dn_* kernel the mean of every counter per launch and the mean launch duration"""
    tot, n, dur = {}, {}, {}
    for row in csv.DictReader(open(path)):
        name = row["Kernel_Name"].split("(")[0].replace("void ", "").strip()
        if not name.startswith("k_dn_"):
            continue
        key = (name, row["Counter_Name"])
        tot[key] = tot.get(key, 0.0) + float(row["Counter_Value"])
        n[key] = n.get(key, 0) + 1
        if row["Counter_Name"] == "SQ_WAVES":
            dur[name] = dur.get(name, 0.0) + float(row["End_Timestamp"]) - float(row["Start_Timestamp"])
    out = {}
    for (name, c), v in tot.items():
        out.setdefault(name, {})[c] = v / n[(name, c)]
    for name, d in dur.items():
        e = out[name]
        e["launch_ns"] = d / n[(name, "SQ_WAVES")]
        e["valu_issue_frac_of_peak"] = e["SQ_INSTS_VALU"] / (e["launch_ns"] * 1e-9) / VALU_PEAK
        e["wait_frac_of_wave_cycles"] = e["SQ_WAIT_INST_ANY"] / e["SQ_WAVE_CYCLES"]
        e["valu_instr_per_wave"] = e["SQ_INSTS_VALU"] / e["SQ_WAVES"]
    return out


def merge(timing, stats_path, pmc_path=None):
    import vkrt_amd

    px = W * H
    k = kernel_stats(stats_path) if stats_path else {}
    pmc = kernel_counters(pmc_path) if pmc_path else {}
    kernels = {}
    for name in ("k_dn_temporal", "k_dn_variance", "k_dn_atrous"):
        b = BYTES[name] * px
        if name == "k_dn_atrous":  # ITER launches per call, the last one with the extra planes
            b = (BYTES[name] * ITER + BYTES["k_dn_atrous_last_extra"]) * px / ITER
        e = {"bytes_per_launch": b}
        if name in k:
            e.update(k[name])
            e["GB_s"] = b / (k[name]["avg_ms"] * 1e6)
            e["frac_of_hbm_peak"] = e["GB_s"] / HBM_PEAK_GBS
        if name in pmc:
            e["counters"] = pmc[name]
        kernels[name] = e
    total_b = sum(kernels[n]["bytes_per_launch"] * (ITER if n == "k_dn_atrous" else 1) for n in kernels)
    res = {"workload": f"atrium262144_{W}x{H}_hybrid_shadows_ao_gi_d8_ploc", "atrous_iterations": ITER, "max_history": 32,
           "source_hash": vkrt_amd.source_hash(), "hbm_peak_GB_s": HBM_PEAK_GBS, "ms_per_call": timing["ms_per_call"],
           "timing": timing, "bytes_per_call": total_b, "GB_s_per_call": total_b / (timing["ms_per_call"] * 1e6), "kernels": kernels,
           "bar_ms": 0.6, "hybrid_frame_ms": 5.0}
    res["frac_of_hbm_peak_per_call"] = res["GB_s_per_call"] / HBM_PEAK_GBS
    at = kernels["k_dn_atrous"].get("counters")
    if at:
        res["binding"] = {
            "kernel": "k_dn_atrous", "resource": "VALU issue, with latency: no single resource at its peak",
            "valu_issue_frac_of_peak": at["valu_issue_frac_of_peak"], "wait_frac_of_wave_cycles": at["wait_frac_of_wave_cycles"],
            "hbm_frac_of_peak": kernels["k_dn_atrous"].get("frac_of_hbm_peak"),
            "note": "SQ_INSTS_VALU per launch / launch time against 1228.8 G wave-instr/s, SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES, in a counter "
                    "pass of their own.  The taps' correctly rounded divisions, square root and expf go through the quarter-rate "
                    "transcendental unit (v_rcp / v_sqrt / v_exp), so the 1228.8 peak is above what this mix can issue."}
    res["frac_of_hybrid_frame"] = timing["ms_per_call"] / 5.0
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--merge", help="timing JSON of an earlier run: combine it with --stats instead of measuring")
    ap.add_argument("--stats", help="rocprofv3 --stats kernel_stats.csv")
    ap.add_argument("--pmc", help="rocprofv3 --pmc counter_collection.csv (SQ_INSTS_VALU SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY ...)")
    a = ap.parse_args()
    res = merge(json.load(open(a.merge)), a.stats, a.pmc) if a.merge else measure(a.calls, a.warmup)
    line = json.dumps(res, indent=1 if a.merge else None)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
