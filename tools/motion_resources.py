#!/usr/bin/env python3
"""Register, scratch and LDS use of the kernels the motion entry points add or touch, from the compiler's own report
(-Rpass-analysis=kernel-resource-usage): no GPU needed.  Writes profiles/motion_kernel_resources.json with

  k_hit_motion, k_dn_temporal, k_dn_motion_temporal          of the working tree
  every k_gbuffer<wide, tm> instantiation                    of the working tree and of a parent revision (git archive into a temp dir)

and checks the two conditions of the feature: no new kernel reserves scratch or spills, and no k_gbuffer instantiation has fewer waves
per SIMD than on the parent (the optional per-pixel hit record is a launch-uniform pointer, not a template parameter).

    python tools/motion_resources.py [--parent REV]        (REV defaults to HEAD^; use HEAD from an uncommitted working tree)"""
import argparse
import json
import os
import re
import subprocess
import sys
import tarfile
import tempfile
import io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("vk-raytracing-engine_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -Wno-unused-result".split()
FIELDS = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes", "Occupancy [waves/SIMD]": "waves_per_simd",
          "SGPRs Spill": "sgpr_spills", "VGPRs Spill": "vgpr_spills", "LDS Size [bytes/block]": "static_lds_bytes"}


def demangle(names):
    out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    return [re.sub(r"^void ", "", o).split("(")[0] for o in out[:len(names)]]


def resources(tree, unit):
    """{kernel name: fields} of one translation unit of the source tree at `tree`"""
    cmd = [HIPCC] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", unit, "-o", os.devnull]
    p = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit(p.stderr)
    kernels, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None and m.group(1).strip() in FIELDS:
            cur[FIELDS[m.group(1).strip()]] = int(m.group(2))
    names = list(kernels)
    return dict(zip(demangle(names), (kernels[n] for n in names))) if names else {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD^")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_kernel_resources.json"))
    a = ap.parse_args()
    rev = subprocess.run(["git", "rev-parse", "--short", a.parent], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    from concurrent.futures import ThreadPoolExecutor

    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(4) as pool:  # (the compiles are child processes; hybrid.hip takes a minute)
        tar = subprocess.run(["git", "archive", a.parent, CSRC, "include"], cwd=ROOT, capture_output=True, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
        jobs = [pool.submit(resources, ROOT, unit) for unit in ("motion.hip", "denoise.hip", "hybrid.hip")] + [pool.submit(resources, tmp, "hybrid.hip")]
        branch = {}
        for j in jobs[:3]:
            branch.update(j.result())
        parent = jobs[3].result()
    new = {k: v for k, v in branch.items() if k in ("k_hit_motion", "k_dn_temporal", "k_dn_motion_temporal")}
    gb = {k: {"branch": v, "parent": parent.get(k)} for k, v in sorted(branch.items()) if k.startswith("k_gbuffer<")}
    problems = []
    if set(new) != {"k_hit_motion", "k_dn_temporal", "k_dn_motion_temporal"}:
        problems.append(f"kernels found: {sorted(new)}")
    for k, v in new.items():
        if v["scratch_bytes"] or v["vgpr_spills"] or v["sgpr_spills"]:
            problems.append(f"{k} reserves scratch or spills: {v}")
    for k, v in gb.items():
        if v["parent"] is None:
            problems.append(f"{k} does not exist on the parent")
        elif v["branch"]["waves_per_simd"] < v["parent"]["waves_per_simd"]:
            problems.append(f"{k}: {v['branch']['waves_per_simd']} waves per SIMD, {v['parent']['waves_per_simd']} on the parent")
    if set(k for k in parent if k.startswith("k_gbuffer<")) != set(gb):
        problems.append("the k_gbuffer instantiations differ from the parent's")
    doc = {"hipcc": subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout.splitlines()[0], "flags": " ".join(FLAGS),
           "parent": rev, "note": "from -Rpass-analysis=kernel-resource-usage, no GPU run.  waves_per_simd = the compiler's occupancy figure.  "
           "k_gbuffer<wide, tm>: the instantiations are those of the parent; the per-pixel hit record is a launch-uniform pointer in HybridParams.",
           "new_kernels": new, "k_gbuffer": gb, "conditions_met": not problems, "problems": problems}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for k, v in new.items():
        print(k, v)
    for k, v in gb.items():
        print(k, "branch", v["branch"], "parent", v["parent"])
    print("conditions met" if not problems else "\n".join(problems))
    return 1 if problems else 0


if __name__ == "__main__":
    sys.exit(main())
