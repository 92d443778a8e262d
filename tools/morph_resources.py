#!/usr/bin/env python3
"""Register, scratch and LDS use of the morph-target kernels (csrc/morph.hip: k_morph_live, k_morph_bind), from the compiler's own
report (-Rpass-analysis=kernel-resource-usage): no GPU needed.  Writes profiles/morph_kernel_resources.json and checks the condition
of the feature: neither kernel reserves scratch or spills a register.

    python tools/morph_resources.py [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from motion_resources import FLAGS, HIPCC, ROOT  # noqa: E402
from skin_resources import resources  # noqa: E402

KERNELS = ("k_morph_live", "k_morph_bind")


def measure():
    """({kernel: fields}, [problems]) of the working tree's morph.hip"""
    found = resources("morph.hip")
    new = {k: found[k] for k in KERNELS if k in found}
    problems = []
    if set(new) != set(KERNELS):
        problems.append(f"kernels found: {sorted(found)}")
    for k, v in new.items():
        if v["scratch_bytes"] or v["vgpr_spills"] or v["sgpr_spills"]:
            problems.append(f"{k} reserves scratch or spills: {v}")
    return new, problems


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morph_kernel_resources.json"))
    a = ap.parse_args()
    new, problems = measure()
    doc = {"hipcc": subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout.splitlines()[0], "flags": " ".join(FLAGS),
           "note": "from -Rpass-analysis=kernel-resource-usage, no GPU run.  waves_per_simd = the compiler's occupancy figure.",
           "kernels": new, "conditions_met": not problems, "problems": problems}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for k, v in new.items():
        print(k, v)
    print("conditions met" if not problems else "\n".join(problems))
    return 1 if problems else 0


if __name__ == "__main__":
    sys.exit(main())
