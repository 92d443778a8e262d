#!/usr/bin/env python3
"""Registers, scratch, spills and LDS of every frame-kernel instantiation that carries the alpha-test stage (VKRT_TM_ALPHA = 16,
VKRT_OPT_ALPHA_TEST), each beside its sibling without the bit, from the compiler's metadata; and the proof that the product
instantiation k_wf_traverse<false, true, 64, 0> is the code it was: the SHA-256 of its disassembly text in this tree and in the parent
commit.  Cross-compiles with the flags of csrc/Makefile: no GPU.

  python tools/alpha_frames_resources.py [--parent REV]      writes profiles/alpha_frames_kernel_resources.json

REV (default HEAD^; use HEAD on an uncommitted working tree) is exported with `git archive` into a temporary directory and its
wf_traverse.hip compiled there.  Labels (.LBB<function>_<block>) carry the function's ordinal in the unit, which the new instantiations
shift: they are hashed as .LBB_<block>, and comments are left out."""
import argparse
import hashlib
import io
import json
import os
import re
import shutil
import subprocess
import tarfile
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC_REL = os.path.join("vk-raytracing-engine_amd", "csrc")
OUT = os.path.join(ROOT, "profiles", "alpha_frames_kernel_resources.json")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
TM0 = "_Z13k_wf_traverseILb0ELb1ELi64ELi0EEv11TraceParams9WfBuffersi"
NAMES = {"vgpr_count": "vgprs", "sgpr_count": "sgprs", "private_segment_fixed_size": "scratch_bytes", "vgpr_spill_count": "vgpr_spills",
         "sgpr_spill_count": "sgpr_spills_to_vgpr_lanes", "group_segment_fixed_size": "static_lds_bytes"}
B = {"0": "false", "1": "true"}
# unit -> [(mangled-name pattern, readable name from its groups; the last group is the triangle mode)]
KERNELS = {
    "wf_traverse": [(r"_Z13k_wf_traverseILb([01])ELb([01])ELi(\d+)ELi(\d+)EE", lambda g: f"k_wf_traverse<{B[g[0]]}, {B[g[1]]}, {g[2]}, %d>"),
                    (r"_Z20k_wf_traverse_cameraILb([01])ELi(\d+)EE", lambda g: f"k_wf_traverse_camera<{B[g[0]]}, %d>")],
    "hybrid": [(r"_Z8k_hybridILb([01])ELb([01])ELi(\d+)EE", lambda g: f"k_hybrid<{B[g[0]]}, {B[g[1]]}, %d>"),
               (r"_Z9k_gbufferILb([01])ELi(\d+)EE", lambda g: f"k_gbuffer<{B[g[0]]}, %d>")],
    # (the second argument, the waves per SIMD its launch bounds ask for, is 2 instead of 3 with the stage: reported as min_waves)
    "pathtrace": [(r"_Z11k_pathtraceILb([01])ELi(\d+)ELi(\d+)EE", lambda g: f"k_pathtrace<{B[g[0]]}, %d>")],
}


def makefile_var(csrc, name):
    for line in open(os.path.join(csrc, "Makefile")):
        m = re.match(rf"^{name}\s*[:?]?=\s*(.*)$", line)
        if m:
            return m.group(1).strip()
    return ""


def unit_flags(csrc, unit):
    flags = makefile_var(csrc, "FLAGS").replace("$(ARCH)", makefile_var(csrc, "ARCH")).replace("-fPIC", "").split()
    return flags + makefile_var(csrc, "FLAGS_" + unit).split()


def compile_unit(csrc, unit, out):
    t0 = time.time()
    subprocess.run([HIPCC] + unit_flags(csrc, unit) + ["--cuda-device-only", "-S", "-o", out, unit + ".hip"], cwd=csrc, check=True, stderr=subprocess.DEVNULL)
    return round(time.time() - t0, 1)


def symbol_hash(asm_text, symbol):
    start = asm_text.index(f"\n{symbol}:")
    body = asm_text[start:asm_text.index("\n.Lfunc_end", start)]
    body = re.sub(r"\.LBB\d+_", ".LBB_", body)
    lines = [ln.split(";")[0].rstrip() for ln in body.splitlines()]  # the compiler's comments name blocks by the same ordinal
    lines = [ln for ln in lines if ln.strip()]
    return hashlib.sha256("\n".join(lines).encode()).hexdigest(), len([ln for ln in lines if ln.startswith("\t") and not ln.lstrip().startswith(".")])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD^")
    a = ap.parse_args()
    csrc = os.path.join(ROOT, CSRC_REL)
    out = {"hipcc": subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout.splitlines()[0],
           "flags": {u: " ".join(unit_flags(csrc, u)) for u in KERNELS},
           "note": "tm = the triangle mode (traverse.h): 1 watertight, 2 dissolve, 4 mask-id (k_gbuffer's form of 2), 16 alpha test.  without_stage = the "
                   "same kernel with tm - 16.  An instantiation keeps the amdgpu_waves_per_eu / launch bounds of its sibling, except: the instrumented "
                   "k_wf_traverse<true, true, 64, tm> asks for 4 waves per SIMD instead of 5, and k_pathtrace<false, tm> for 2 instead of 3 "
                   "(min_waves): at the siblings' bounds they would spill VGPRs, as those siblings do.  SGPR spills go to VGPR lanes (v_writelane / "
                   "v_readlane), not to memory.  scratch_touching_instructions counts the scratch_* / buffer_*-through-the-private-segment "
                   "instructions of the kernel body.",
           "kernels": {}, "compile_seconds": {}}
    tmp = tempfile.mkdtemp(prefix="alpha_frames_isa_")
    try:
        for unit, pats in KERNELS.items():
            asm = os.path.join(tmp, unit + ".s")
            out["compile_seconds"][unit + ".hip"] = compile_unit(csrc, unit, asm)
            text = open(asm).read()
            found = {}
            touching = {m.group(1): len(re.findall(r"^\s+scratch_", m.group(2), flags=re.M))
                        for m in re.finditer(r"\n(_Z\w+):[^\n]*\n(.*?)\n\.Lfunc_end", text, flags=re.S)}
            for block in text.split("  - .agpr_count:")[1:]:
                f = dict(re.findall(r"\.(name|" + "|".join(NAMES) + r"):\s+(\S+)", block))
                for pat, label in pats:
                    m = re.match(pat, f.get("name", ""))
                    if m:
                        g = m.groups()
                        found[(label(g), int(g[-1]))] = {NAMES[k]: int(f[k]) for k in NAMES}
                        found[(label(g), int(g[-1]))]["scratch_touching_instructions"] = touching[f["name"]]
                        if unit == "pathtrace":
                            found[(label(g), int(g[-1]))]["min_waves"] = int(g[1])
            for (label, tm), res in sorted(found.items()):
                if tm & 16:
                    out["kernels"][label % tm] = dict(res, without_stage=dict(found[(label, tm - 16)], kernel=label % (tm - 16)))
            if unit == "wf_traverse":
                h, n = symbol_hash(text, TM0)
                out["tm0_symbol"] = {"symbol": TM0, "kernel": "k_wf_traverse<false, true, 64, 0>", "branch_sha256": h, "branch_instruction_lines": n}
        # the parent's wf_traverse.hip, from git
        ptree = os.path.join(tmp, "parent")
        os.makedirs(ptree)
        tar = subprocess.run(["git", "archive", a.parent, CSRC_REL, "include"], cwd=ROOT, check=True, capture_output=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(ptree)
        pasm = os.path.join(tmp, "parent_wf_traverse.s")
        compile_unit(os.path.join(ptree, CSRC_REL), "wf_traverse", pasm)
        h, n = symbol_hash(open(pasm).read(), TM0)
        out["tm0_symbol"].update(parent_rev=subprocess.run(["git", "rev-parse", a.parent], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip(),
                                 parent_sha256=h, parent_instruction_lines=n)
        out["tm0_symbol"]["identical"] = out["tm0_symbol"]["parent_sha256"] == out["tm0_symbol"]["branch_sha256"]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    ks = out["kernels"].values()
    out["max_vgprs"] = max(k["vgprs"] for k in ks)
    out["max_scratch_bytes"] = max(k["scratch_bytes"] for k in ks)
    out["max_vgpr_spills"] = max(k["vgpr_spills"] for k in ks)
    out["max_scratch_touching_instructions"] = max(k["scratch_touching_instructions"] for k in ks)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", OUT, json.dumps({k: out[k] for k in ("max_vgprs", "max_scratch_bytes", "max_vgpr_spills", "compile_seconds")}), json.dumps(out["tm0_symbol"]))


if __name__ == "__main__":
    main()
