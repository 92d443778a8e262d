#!/usr/bin/env python3
"""Register, scratch and LDS use of named kernels of one translation unit of csrc/, from the compiler's own report
(-Rpass-analysis=kernel-resource-usage): no GPU needed.  Writes profiles/<unit>_kernel_resources.json and checks the condition the
vertex-animation units were merged under: none of the kernels reserves scratch or spills a register.

    python tools/kernel_resources.py skin.hip k_skin k_skin_capture [--out FILE]
    python tools/kernel_resources.py morph.hip k_morph_live k_morph_bind [--out FILE]"""
import argparse
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from motion_resources import CSRC, FIELDS, FLAGS, HIPCC, ROOT  # noqa: E402


def resources(unit):
    """{kernel name: fields} of one translation unit of the working tree; the name is the one in front of the argument list, without
    its namespaces (the kernels live in vkrt::(anonymous namespace))"""
    cmd = [HIPCC] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", unit, "-o", os.devnull]
    p = subprocess.run(cmd, cwd=os.path.join(ROOT, CSRC), capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit(p.stderr)
    kernels, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            full = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True, check=True).stdout.strip()
            cur = kernels.setdefault(re.search(r"(\w+)\([^()]*\)$", full).group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None and m.group(1).strip() in FIELDS:
            cur[FIELDS[m.group(1).strip()]] = int(m.group(2))
    return kernels


def measure(unit, names):
    """({kernel: fields}, [problems]) of the kernels `names` of the working tree's csrc/<unit>"""
    found = resources(unit)
    new = {k: found[k] for k in names if k in found}
    problems = []
    if set(new) != set(names):
        problems.append(f"kernels found: {sorted(found)}")
    for k, v in new.items():
        if v["scratch_bytes"] or v["vgpr_spills"] or v["sgpr_spills"]:
            problems.append(f"{k} reserves scratch or spills: {v}")
    return new, problems


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("unit", help="a translation unit of csrc/, e.g. skin.hip")
    ap.add_argument("kernels", nargs="+")
    ap.add_argument("--out")
    a = ap.parse_args()
    out = a.out or os.path.join(ROOT, "profiles", os.path.splitext(a.unit)[0] + "_kernel_resources.json")
    new, problems = measure(a.unit, a.kernels)
    doc = {"hipcc": subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout.splitlines()[0], "flags": " ".join(FLAGS),
           "note": "from -Rpass-analysis=kernel-resource-usage, no GPU run.  waves_per_simd = the compiler's occupancy figure.",
           "kernels": new, "conditions_met": not problems, "problems": problems}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for k, v in new.items():
        print(k, v)
    print("conditions met" if not problems else "\n".join(problems))
    return 1 if problems else 0


if __name__ == "__main__":
    sys.exit(main())
