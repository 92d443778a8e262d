"""Issue-slot view of the shade kernels' assembly (the sibling of tools/isa_blocks.py, which does this for the traversal kernel):
k_wf_shade, k_wf_shade_camera and k_wf_shade_hybrid of csrc/wavefront.hip, cross-compiled for gfx950 with the flags csrc/Makefile gives
that unit.  Per kernel: VGPRs, scratch, VALU instructions by opcode class and their sum weighted by issue cost ("slots").

    python tools/shade_isa.py                      # compile the working tree, print the table
    python tools/shade_isa.py --blocks             # ... and every basic block of k_wf_shade_camera with its slots and memory ops
    python tools/shade_isa.py --asm FILE.s         # read a listing instead of compiling
    python tools/shade_isa.py --json               # write profiles/shade_isa.json: this tree's counts ("this"); "parent" is kept
    python tools/shade_isa.py --json --as-parent   # ... write them as "parent" (run on a checkout of the parent commit's csrc/, --csrc DIR)

A slot is one full-rate VALU issue.  The weight of an opcode is its cycles per instruction at 8 waves per SIMD in
profiles/r05_issue_microbench.json over those of v_mul_f32, rounded (packed FP32 and the VOP3 integer / min / max / convert classes: 2,
compares and transcendentals: 3).  v_cndmask_b32 counts 1: its own row there is a chain through VCC, the cmp + cndmask pair row prices
it.  Opcodes the microbenchmark does not have take the weight of their class (WEIGHT_BY_PATTERN): 32-bit integer multiplies as
v_mul_lo_u32, 64-bit integer adds 2, the 64-bit multiply-add 4.
"""
import collections
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vk-raytracing-engine_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = {"k_wf_shade": "_Z10k_wf_shade11TraceParams", "k_wf_shade_camera": "_Z17k_wf_shade_camera11TraceParams",
           "k_wf_shade_hybrid": "_Z17k_wf_shade_hybrid11TraceParams"}
SHADE_SOURCES = ("wavefront.hip", "shade.h", "texel.h", "rgen.h", "device_math.h", "wf_streams.h", "hybrid_gi.h", "Makefile")
# opcodes without a row of their own in the microbenchmark, first match wins
WEIGHT_BY_PATTERN = (("v_mad_u64_u32", 4), ("v_mad_i64_i32", 4), ("v_mul_hi_", 2), ("v_mul_lo_", 2), ("_u64", 2), ("_i64", 2), ("_b64", 2), ("_f64", 2),
                     ("v_pk_", 2), ("v_cmp", 3), ("v_rcp", 3), ("v_rsq", 3), ("v_sqrt", 3), ("v_exp", 3), ("v_log", 3), ("v_sin", 3), ("v_cos", 3),
                     ("_sdwa", 2), ("v_cvt", 2), ("v_min", 2), ("v_max", 2), ("v_med3", 2), ("v_bfe", 2), ("v_bfi", 2), ("v_perm", 2), ("v_bcnt", 2),
                     ("v_mbcnt", 2), ("v_lshl_add", 2), ("v_lshl_or", 2), ("v_and_or", 2), ("v_or3", 2), ("v_add3", 2), ("v_xad", 2), ("v_mad_", 2),
                     ("v_lshlrev_b32", 2), ("v_ldexp", 2), ("v_fma_mix", 2), ("v_readlane", 2), ("v_readfirstlane", 2), ("v_writelane", 2))
CLASSES = (("mov", ("v_mov_", "v_accvgpr")), ("packed_f32", ("v_pk_",)), ("addr64", ("v_lshl_add_u64", "v_add_co", "v_addc_co", "v_mad_u64", "v_mad_i64")),
           ("int_mul", ("v_mul_lo_", "v_mul_hi_", "v_mul_u32", "v_mul_i32", "v_mad_u32", "v_mad_i32")), ("select", ("v_cndmask",)), ("compare", ("v_cmp",)),
           ("transcendental", ("v_rcp", "v_rsq", "v_sqrt", "v_exp", "v_log", "v_sin", "v_cos")), ("div_fixup", ("v_div_",)),
           ("convert", ("v_cvt", "v_floor", "v_ceil", "v_trunc", "v_rndne", "v_fract", "v_frexp", "v_ldexp")),
           ("fp32", ("v_fma", "v_mul_f32", "v_add_f32", "v_sub", "v_mac", "v_mul_legacy", "v_min_f32", "v_max_f32", "v_med3_f32")), ("int_other", ("v_",)))


def measured_weights():
    mb = json.load(open(os.path.join(ROOT, "profiles", "r05_issue_microbench.json")))
    unit = mb["v_mul_f32"]["8"]["cyc_per_instr_per_simd"]
    w = {k: max(1, int(round(v["8"]["cyc_per_instr_per_simd"] / unit))) for k, v in mb.items() if isinstance(v, dict) and "8" in v and re.fullmatch(r"v_[a-z0-9_]+", k)}
    w["v_cndmask_b32"] = 1
    return w


def weight(op, measured):
    op = re.sub(r"_(e32|e64|dpp|sdwa)$", lambda m: "_sdwa" if m.group(1) == "sdwa" else "", op)
    if op in measured:
        return measured[op]
    for pat, w in WEIGHT_BY_PATTERN:
        if pat in op:
            return w
    return 1


def klass(op):
    for name, pats in CLASSES:
        if op.startswith(pats):
            return name
    return "int_other"


def makefile_var(name, csrc):
    for line in open(os.path.join(csrc, "Makefile")):
        m = re.match(rf"^{name}\s*[:?]?=\s*(.*)$", line)
        if m:
            return m.group(1).strip()
    raise KeyError(name)


def hipcc_version():
    out = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout
    m = re.search(r"HIP version:\s*(\S+)", out)
    return m.group(1) if m else "unknown"


def compile_asm(csrc=CSRC, unit="wavefront", out=None):
    flags = makefile_var("FLAGS", csrc).replace("$(ARCH)", makefile_var("ARCH", csrc)).replace("-fPIC", "").split()
    flags += makefile_var(f"FLAGS_{unit}", csrc).split()
    out = out or os.path.join(tempfile.mkdtemp(prefix="vkrt_isa_"), f"{unit}.s")
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", "-o", out, f"{unit}.hip"], cwd=csrc, check=True, stderr=subprocess.DEVNULL)
    return out


def kernel_text(text, prefix):
    m = re.search(rf"^({re.escape(prefix)}\w*):", text, flags=re.M)
    sym = m.group(1)
    body = text[m.start():text.index("\n.Lfunc_end", m.start())]
    meta = text[text.index(f".amdhsa_kernel {sym}"):]
    return sym, body, meta[:meta.index(".end_amdhsa_kernel")]


def instructions(body):
    """(block name, opcode) of every instruction line, blocks in layout order"""
    block = "entry"
    for line in body.split("\n"):
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        s = line.strip()
        if m:
            block = m.group(1)
        elif s.startswith("; %bb."):
            block = s.split(":")[0][2:]
        elif s and not s.startswith((";", ".")) and not s.endswith(":"):
            yield block, s.split()[0]


def kernel_stats(text, prefix, measured):
    sym, body, meta = kernel_text(text, prefix)
    by_class, ops, blocks = collections.Counter(), collections.Counter(), collections.OrderedDict()
    valu = slots = 0
    for block, op in instructions(body):
        b = blocks.setdefault(block, {"valu": 0, "slots": 0, "salu": 0, "lds": 0, "vmem": 0})
        if op.startswith("v_"):
            w = weight(op, measured)
            valu += 1
            slots += w
            by_class[klass(op)] += 1
            ops[re.sub(r"_(e32|e64)$", "", op)] += 1
            b["valu"] += 1
            b["slots"] += w
        elif op.startswith("s_"):
            b["salu"] += 1
        elif op.startswith("ds_"):
            b["lds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            b["vmem"] += 1
    return {"symbol": sym, "vgprs": int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1)),
            "scratch_bytes": int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1)),
            "scratch_ops": len(re.findall(r"^\s+scratch_", body, flags=re.M)), "flat_ops": len(re.findall(r"^\s+flat_", body, flags=re.M)),
            "valu": valu, "slots": slots, "by_class": dict(sorted(by_class.items())),
            "top_opcodes": dict(ops.most_common(24)), "body_sha256": hashlib.sha256(re.sub(r";.*", "", body).encode()).hexdigest()[:16]}, blocks


def source_hashes(csrc):
    return {f: hashlib.sha256(open(os.path.join(csrc, f), "rb").read()).hexdigest()[:16] for f in SHADE_SOURCES}


def take(csrc=CSRC, asm=None):
    """{kernel: stats} of a csrc directory (or of a listing), and the per-block tables"""
    measured = measured_weights()
    text = open(asm or compile_asm(csrc)).read()
    stats, blocks = {}, {}
    for name, prefix in KERNELS.items():
        stats[name], blocks[name] = kernel_stats(text, prefix, measured)
    return stats, blocks


def main():
    opt = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None
    csrc = os.path.abspath(opt("--csrc") or CSRC)
    stats, blocks = take(csrc, opt("--asm"))
    for name, s in stats.items():
        print(f"{name}: {s['valu']} VALU = {s['slots']} slots, {s['vgprs']} VGPRs, scratch {s['scratch_bytes']} B, flat ops {s['flat_ops']}")
        print("   " + ", ".join(f"{k} {v}" for k, v in s["by_class"].items()))
    if "--blocks" in sys.argv:
        for b, c in blocks["k_wf_shade_camera"].items():
            print(f"   {b:>12} valu {c['valu']:4d} slots {c['slots']:4d} salu {c['salu']:3d} lds {c['lds']:3d} mem {c['vmem']:3d}")
    if "--json" in sys.argv:
        path = os.path.join(ROOT, "profiles", "shade_isa.json")
        doc = json.load(open(path)) if os.path.exists(path) else {}
        side = "parent" if "--as-parent" in sys.argv else "this"
        doc["hipcc"] = hipcc_version()
        doc["unit"] = "csrc/wavefront.hip with FLAGS + FLAGS_wavefront of csrc/Makefile, --offload-arch=gfx950"
        doc["weights"] = "profiles/r05_issue_microbench.json at 8 waves per SIMD over v_mul_f32, rounded; unmeasured opcodes by class (tools/shade_isa.py)"
        doc[side] = {"sources": source_hashes(csrc), "kernels": stats}
        if "parent" in doc and "this" in doc:
            doc["slots_cut"] = {k: round(1.0 - doc["this"]["kernels"][k]["slots"] / doc["parent"]["kernels"][k]["slots"], 4) for k in KERNELS}
        json.dump(doc, open(path, "w"), indent=1)
        print("wrote", path, "as", side)


if __name__ == "__main__":
    main()
