"""Basic-block view of the traversal kernel's assembly (the method behind profiles/r04_experiments.md #126-#128 and the budget in
DESIGN.md section 5): for every loop of k_wf_traverse<false, true, 64, 0> the blocks in layout order with their VALU / v_mov / SALU /
LDS / global-memory instruction counts and branch targets, and per loop the totals.  The sharing loops are the ones with ds_bpermute.

    tools/isa_stats.sh            # writes /tmp/vkrt_isa/wf_traverse.s
    python tools/isa_blocks.py [/tmp/vkrt_isa/wf_traverse.s] [--blocks]
    python tools/isa_blocks.py --json      # writes profiles/isa_mix.json: the static opcode mix of the sharing closest-hit loop (node
                                           # test block / rest of the loop), tied to the sources by vkrt_amd.source_hash: bench.py's
                                           # roofline.issue_mix prices the kernel against the ceiling that mix allows
    python tools/isa_blocks.py --loops-json [--as-parent] [--csrc DIR] [--bench-json FILE]
                                           # writes profiles/traverse_loop_isa.json: the two sharing loops of k_wf_traverse<false, true, 64, 0>
                                           # and the loop of k_wf_traverse_camera<false, 0> by region (node test, triangle test, lending,
                                           # sharing step, bookkeeping, prologue / epilogue) in VALU instructions and issue slots (weights
                                           # imported from tools/shade_isa.py), the registers and scratch of every instantiation of the
                                           # traversal and query kernels, and -- with the result line of a bench run -- a dynamic estimate
                                           # per wave.  --as-parent --csrc DIR: the same of a checkout of the parent commit's csrc/
"""
import re
import sys

KERNEL = "_Z13k_wf_traverseILb0ELb1ELi64ELi0EEv11TraceParams9WfBuffersi"
HALF_RATE = ("cvt", "min", "max", "cmp", "bfe", "_sdwa", "or3", "mul_lo", "perm", "mad_u", "bcnt", "lshl_add", "lshl_or", "and_or", "add3", "v_pk_", "fma_mix")


def kernel_body(path):
    text = open(path).read()
    a = text.index(f"\n{KERNEL}:")
    return text[a:text.index("\n.Lfunc_end", a)].split("\n")


def blocks(lines):
    """blocks in layout order; `loop` = name of the depth-1 loop a block belongs to (fall-through blocks inherit it)"""
    out, cur = [], None
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+):(.*)", l)
        s = l.strip()
        if m or s.startswith("; %bb."):
            if m:
                name, cmt = m.group(1), m.group(2)
                hdr = re.search(r"(?:Header=|Parent Loop )(BB\d+_\d+)", cmt)
                loop = name[2:] if "Loop Header: Depth=1" in cmt else (hdr.group(1) if hdr else None)
                header = "Loop Header: Depth=1" in cmt
            else:
                name, loop, header = s.split(":")[0][2:], (cur["loop"] if cur else None), False
            cur = {"name": name, "loop": loop, "header": header, "valu": 0, "half": 0, "mov": 0, "salu": 0, "lds": 0, "vmem": 0, "bperm": 0, "br": []}
            out.append(cur)
            continue
        if cur is None or not s or s.startswith(";"):
            continue
        op = s.split()[0]
        if op.startswith("v_"):
            cur["valu"] += 1
            cur["half"] += any(h in op for h in HALF_RATE)
            cur["mov"] += op.startswith("v_mov")
        elif op.startswith("s_cbranch") or op == "s_branch":
            cur["br"].append(op[2:] + "->" + s.split()[1].replace(".LBB", "B"))
            cur["salu"] += 1
        elif op.startswith("s_"):
            cur["salu"] += 1
        elif op.startswith("ds_"):
            cur["lds"] += 1
            cur["bperm"] += "bpermute" in op
        elif op.startswith(("global_", "buffer_", "scratch_")):
            cur["vmem"] += 1
    return out


# ---- --loops-json: the sharing loops by region (profiles/traverse_loop_isa.json, profiles/r11_experiments.md) ---------------------------
CAMERA_KERNEL = "_Z20k_wf_traverse_cameraILb0ELi0EEv11TraceParams9WfBuffersii"
LOOPS = (("k_wf_traverse<false, true, 64, 0> closest-hit", KERNEL, 0), ("k_wf_traverse<false, true, 64, 0> any-hit", KERNEL, 1),
         ("k_wf_traverse_camera<false, 0>", CAMERA_KERNEL, 0))
LOOP_SOURCES = ("traverse_share.h", "traverse_wide.h", "traverse.h", "wf_traverse.hip", "query.hip")
REGIONS = ("node_test", "triangle_test", "lending", "sharing_step", "bookkeeping", "rare_flush")


def share_regions(csrc):
    """line -> region of csrc/traverse_share.h from its `[isa: name]` comments: a marker holds from its line to the next one"""
    import os

    out, cur = {}, None
    for n, l in enumerate(open(os.path.join(csrc, "traverse_share.h")), 1):
        m = re.search(r"\[isa: (\w+)\]", l)
        cur = m.group(1) if m else cur
        out[n] = cur
    if cur is None:
        raise SystemExit(f"{csrc}/traverse_share.h carries no [isa: ...] region comments (a parent checkout gets them added: comments only)")
    return out


def function_lines(path, name):
    """(first, last) line of the definition of function `name` in a C++ source, by brace matching"""
    lines = open(path).read().split("\n")
    for i, l in enumerate(lines):
        if re.search(rf"\b{name}\s*\(", l) and not l.rstrip().endswith(";") and not l.lstrip().startswith("//"):
            depth, seen = 0, False
            for j in range(i, len(lines)):
                depth += lines[j].count("{") - lines[j].count("}")
                seen = seen or "{" in lines[j]
                if seen and depth == 0:
                    return i + 1, j + 1
    return 0, 0


def located(text, symbol):
    """VALU instructions of a kernel of a listing compiled with line tables: dicts (op, file, line, block, loop = the depth-1 loop the
    block lies in or None, inner = inside a depth-2 loop)"""
    files = {int(m.group(1)): (m.group(3) or m.group(2)) for m in re.finditer(r'^\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', text, flags=re.M)}
    a = text.index(f"\n{symbol}:")
    lines = text[a:text.index("\n.Lfunc_end", a)].split("\n")
    parent = {}  # header of an inner loop -> header of its depth-1 loop
    for i, l in enumerate(lines):
        m = re.match(r"^\.L(BB\d+_\d+):.*Parent Loop (BB\d+_\d+) Depth=1", l)
        if m and "Inner Loop Header" in (l + lines[i + 1] if i + 1 < len(lines) else l):
            parent[m.group(1)] = m.group(2)
    out, block, loop, inner, loc = [], "entry", None, False, (None, 0)
    for l in lines:
        s = l.strip()
        m = re.match(r"^(\.LBB\d+_\d+):(.*)", l)
        if m:
            block, cmt = m.group(1), m.group(2)
            if "Loop Header: Depth=1" in cmt:
                loop, inner = block[2:], False
            else:
                h = re.search(r"(?:Header=|Parent Loop )(BB\d+_\d+) Depth=(\d)", cmt)
                loop = (parent.get(h.group(1), h.group(1)) if h else None)
                inner = bool(h) and (h.group(2) == "2" or h.group(1) in parent)
            continue
        if s.startswith("; %bb."):
            block = s.split(":")[0][2:]
            h = re.search(r"Header=(BB\d+_\d+) Depth=(\d)", s)
            if h:
                loop, inner = parent.get(h.group(1), h.group(1)), h.group(2) == "2"
            continue
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            loc = (files.get(int(m.group(1)), "?").split("/")[-1], int(m.group(2)))
            continue
        if s.startswith("v_"):
            out.append({"op": s.split()[0], "file": loc[0], "line": loc[1], "block": block, "loop": loop, "inner": inner,
                        "bperm": False})
        elif s.startswith("ds_bpermute") and out:
            out[-1]["bperm"] = True
    return out


def loop_source_hashes(csrc):
    """sha256 (16 digits) of the five sources of the sharing walk, taken without the [isa: region] comments"""
    import hashlib
    import os

    return {f: hashlib.sha256(re.sub(r"\s*(//|/\*) \[isa: \w+\]( \*/)?", "", open(os.path.join(csrc, f)).read()).encode()).hexdigest()[:16] for f in LOOP_SOURCES}


def loops_by_region(csrc, verify=True, resources=True):
    """the three sharing loops of csrc/wf_traverse.hip by region: VALU instructions and issue slots (weights of tools/shade_isa.py).
    verify: compile the unit without line tables too and demand the same instructions; resources: registers and scratch of every
    traversal and query kernel (compiles csrc/query.hip as well)"""
    import os
    import subprocess
    import tempfile

    import shade_isa

    measured = shade_isa.measured_weights()
    unit_flags = shade_isa.makefile_var("FLAGS_wf_traverse", csrc)
    plain = open(shade_isa.compile_asm(csrc, "wf_traverse")).read() if verify or resources else None
    # the same unit with line tables: every instruction then carries the source line it was made from (inlined callees: their own)
    flags = shade_isa.makefile_var("FLAGS", csrc).replace("$(ARCH)", shade_isa.makefile_var("ARCH", csrc)).replace("-fPIC", "").split()
    dbg = os.path.join(tempfile.mkdtemp(prefix="vkrt_isa_"), "wf_traverse_g.s")
    subprocess.run([shade_isa.HIPCC] + flags + unit_flags.split() + ["-gline-tables-only", "--cuda-device-only", "-S", "-o", dbg, "wf_traverse.hip"],
                   cwd=csrc, check=True, stderr=subprocess.DEVNULL)
    text = open(dbg).read()
    regions = share_regions(csrc)
    far = function_lines(os.path.join(csrc, "traverse.h"), "anyhit_far_first")
    res = {"loops": {}, "outside_loops": {}, "resources": {}}
    for sym in (KERNEL, CAMERA_KERNEL):
        ins = located(text, sym)
        if verify and [i["op"] for i in ins] != [l.split()[0] for l in kernel_body_of(plain, sym) if l.strip().startswith("v_")]:
            raise SystemExit(f"{sym}: the listing with line tables is not the product's instruction for instruction")
        # the sharing loops: depth-1 loops that shuffle
        order = []
        for i in ins:
            if i["loop"] and i["loop"] not in order:
                order.append(i["loop"])
        sharing = [h for h in order if any(i["bperm"] for i in ins if i["loop"] == h)]
        for name, ksym, k in LOOPS:
            if ksym != sym:
                continue
            mine = [i for i in ins if i["loop"] == sharing[k]]
            for i in mine:
                if i["inner"]:
                    i["region"] = "rare_flush"
                elif i["file"] == "traverse_wide.h":
                    i["region"] = "node_test"
                elif i["file"] == "traverse.h" and not far[0] <= i["line"] <= far[1]:
                    i["region"] = "triangle_test"
                elif i["file"] == "traverse_share.h":
                    i["region"] = regions.get(i["line"]) if regions.get(i["line"]) != "prologue_epilogue" else "bookkeeping"
                else:
                    i["region"] = None
            # an instruction made from another header (shuffles, votes, device_math.h) belongs to the code around it: the nearest
            # classified instruction before it in its block, else behind it
            for idx, i in enumerate(mine):
                if i["region"] is None:
                    near = [j for j in mine[:idx][::-1] if j["block"] == i["block"] and j.get("region")][:1] or \
                           [j for j in mine[idx + 1:] if j["block"] == i["block"] and j.get("region")][:1]
                    i["region"] = near[0]["region"] if near else "bookkeeping"
            by = {r: {"valu": 0, "slots": 0} for r in REGIONS}
            for i in mine:
                by[i["region"]]["valu"] += 1
                by[i["region"]]["slots"] += shade_isa.weight(i["op"], measured)
            tot = {"valu": len(mine), "slots": sum(v["slots"] for v in by.values())}
            rest = {k2: tot[k2] - by["node_test"][k2] for k2 in ("valu", "slots")}
            res["loops"][name] = {"header": sharing[k], "regions": by, "total": tot, "outside_node_test": rest}
        out_ins = [i for i in ins if i["loop"] is None]
        res["outside_loops"][sym] = {"valu": len(out_ins), "slots": sum(shade_isa.weight(i["op"], measured) for i in out_ins),
                                     "note": "prologue / epilogue of the whole kernel: every instruction outside its loops"}
    for unit, listing in ((("wf_traverse", plain), ("query", open(shade_isa.compile_asm(csrc, "query")).read())) if resources else ()):
        for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", listing, flags=re.S):
            if re.match(r"_Z\d+k_(wf_traverse|query)", m.group(1)):
                res["resources"][m.group(1)] = {"vgprs": int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", m.group(2)).group(1)),
                                                "scratch_bytes": int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", m.group(2)).group(1))}
    return res


def kernel_body_of(text, symbol):
    a = text.index(f"\n{symbol}:")
    return text[a:text.index("\n.Lfunc_end", a)].split("\n")


def dynamic_estimate(loop, outside, steps):
    """VALU instructions of one wave from the static regions and the step counts of an instrumented frame.  An estimate: a region's
    static count holds every path through it (both sides of a branch, the rare blocks), so the per-iteration terms are upper figures;
    the iteration count lies between max(node, triangle) steps and their sum and is taken in the middle."""
    n, t = steps["wave_node_steps_per_wave"], steps["wave_tri_steps_per_wave"]
    iters = 0.5 * (max(n, t) + n + t)
    r = loop["regions"]
    parts = {"node_test": n * r["node_test"]["valu"],
             "triangle_test": t * r["triangle_test"]["valu"] / 2.0,  # two copies in the loop (own triangle / lent step), one runs per step
             "lending": t * r["lending"]["valu"],
             "sharing_step": iters / steps.get("share_period", 4) * r["sharing_step"]["valu"],
             "bookkeeping": iters * r["bookkeeping"]["valu"],
             "prologue_epilogue": outside["valu"]}
    return {"iterations": iters, "valu_by_region": {k: round(v, 1) for k, v in parts.items()}, "valu_per_wave": round(sum(parts.values()), 1)}


def loops_json():
    import json
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import shade_isa

    opt = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None
    csrc = os.path.abspath(opt("--csrc") or shade_isa.CSRC)
    side = "parent" if "--as-parent" in sys.argv else "this"
    path = os.path.join(root, "profiles", "traverse_loop_isa.json")
    doc = json.load(open(path)) if os.path.exists(path) else {}
    got = loops_by_region(csrc)
    got["sources"] = loop_source_hashes(csrc)
    doc["hipcc"] = shade_isa.hipcc_version()
    doc["unit"] = "csrc/wf_traverse.hip (resources: and csrc/query.hip) with FLAGS + FLAGS_<unit> of csrc/Makefile, --offload-arch=gfx950"
    doc["method"] = ("VALU instructions of the depth-1 loops that shuffle, attributed by the source line each instruction was made from (the same unit "
                     "compiled with line tables, checked to be the product's instruction for instruction): csrc/traverse_wide.h = node test, "
                     "csrc/traverse.h = triangle test, csrc/traverse_share.h by its [isa: region] comments, other headers as the code around them; "
                     "blocks of the depth-2 loops (a group tested out on the spot) are rare_flush.  slots: weights of tools/shade_isa.py.  "
                     "source hashes are taken without the region comments")
    bench = opt("--bench-json")
    if bench:  # step counters of one instrumented bench frame (bench.py's roofline.per_ray) -> per wave of 64 rays
        pr = json.load(open(bench))["roofline"]["per_ray"]
        got["steps"] = {"wave_node_steps_per_wave": pr["nodes_visited"] / pr["node_step_lane_efficiency"],
                        "wave_tri_steps_per_wave": pr["tris_tested"] / pr["tri_step_lane_efficiency"], "share_period": 4,
                        "nodes_per_ray": pr["nodes_visited"], "tris_per_ray": pr["tris_tested"]}
    elif "steps" in doc.get(side, {}):
        got["steps"] = doc[side]["steps"]
    if "steps" in got:
        got["dynamic_estimate"] = {name: dynamic_estimate(l, got["outside_loops"][sym], got["steps"]) for (name, sym, _), l in
                                   ((x, got["loops"][x[0]]) for x in LOOPS)}
    doc[side] = got
    if "parent" in doc and "this" in doc:
        doc["cut_outside_node_test"] = {n: {k: round(1.0 - doc["this"]["loops"][n]["outside_node_test"][k] / doc["parent"]["loops"][n]["outside_node_test"][k], 4)
                                            for k in ("valu", "slots")} for n, _, _ in LOOPS}
    json.dump(doc, open(path, "w"), indent=1)
    for n, _, _ in LOOPS:
        l = got["loops"][n]
        print(f"{n}: {l['total']['valu']} VALU = {l['total']['slots']} slots; outside the node test {l['outside_node_test']['valu']} = {l['outside_node_test']['slots']}")
        print("   " + ", ".join(f"{r} {v['valu']}/{v['slots']}" for r, v in l["regions"].items()))
    print("wrote", path, "as", side)


def main():
    if "--loops-json" in sys.argv:
        return loops_json()
    args = [a for a in sys.argv[1:] if not a.startswith("-")]
    path = args[0] if args else "/tmp/vkrt_isa/wf_traverse.s"
    bb = blocks(kernel_body(path))
    headers = [b for b in bb if b["header"]]
    for h in headers:
        members = [b for b in bb if b["loop"] == h["name"][2:]]
        tot = {k: sum(b[k] for b in members) for k in ("valu", "half", "mov", "salu", "lds", "vmem", "bperm")}
        node = max(members, key=lambda b: b["valu"])
        print(f"loop {h['name']}: {len(members)} blocks, VALU {tot['valu']} (half-rate {tot['half']}, v_mov {tot['mov']}), SALU {tot['salu']}, "
              f"LDS {tot['lds']} (bpermute {tot['bperm']}), memory {tot['vmem']}; node test {node['name']}: {node['valu']} VALU, "
              f"{node['valu'] - node['half']} full-rate + {node['half']} half-rate = {2 * (node['valu'] - node['half']) + 4 * node['half']} cycles")
        if "--json" in sys.argv and tot["bperm"] and "mix" not in locals():  # the first sharing loop = closest-hit walks
            import json
            import os

            root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
            sys.path.insert(0, root)
            import vkrt_amd

            import subprocess
            hv = re.search(r"HIP version:\s*(\S+)", subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout)
            mix = {"source_hash": vkrt_amd.source_hash(), "hipcc": hv.group(1) if hv else "unknown",
                   "kernel": "k_wf_traverse<false, true, 64, 0>", "loop": "sharing closest-hit walk",
                   "node_test": {"valu": node["valu"], "half_rate": node["half"]},
                   "loop_rest": {"valu": tot["valu"] - node["valu"], "half_rate": tot["half"] - node["half"]},
                   "half_rate_classes": list(HALF_RATE),
                   "note": "static counts from the assembly (tools/isa_stats.sh + tools/isa_blocks.py --json); a half-rate opcode takes two issue slots "
                           "of a full-rate one (profiles/r02_issue_microbench.json)"}
            json.dump(mix, open(os.path.join(root, "profiles", "isa_mix.json"), "w"), indent=1)
        if "--blocks" in sys.argv:
            for b in members:
                print(f"   {b['name']:>12} valu {b['valu']:3d} mov {b['mov']:2d} salu {b['salu']:2d} lds {b['lds']:2d} mem {b['vmem']} {' '.join(b['br'])}")


if __name__ == "__main__":
    main()
