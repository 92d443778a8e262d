"""Six traversal waves per SIMD (profiles/r12_experiments.md): what the two product traversal kernels need for them, checked without a
GPU.  csrc/wf_traverse.hip is cross-compiled for gfx950 with the flags csrc/Makefile gives it: k_wf_traverse<false, true, 64, 0> and
k_wf_traverse_camera<false, 0> must fit the 80 registers of six waves with nothing spilled, and their static LDS block plus the stack
that csrc/trav_lds.h sizes for a wide8 tree must be charged at most 1/24 of a CU's LDS up to wide depth 9 -- by the allocation granule
measured on the device (profiles/r12_six_waves.json) -- and more than that from depth 10 on, where the header says five waves.  The
header is compiled alone with the host compiler.  Skipped like tests/test_kernel_isa.py when hipcc is absent or another compiler."""
import json
import os
import re
import shutil
import subprocess

import pytest

import vkrt_amd

CSRC = os.path.join(vkrt_amd.PKG_DIR, "csrc")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
KERNELS = {"k_wf_traverse<false, true, 64, 0>": "_Z13k_wf_traverseILb0ELb1ELi64ELi0EEv11TraceParams9WfBuffersi",
           "k_wf_traverse_camera<false, 0>": "_Z20k_wf_traverse_cameraILb0ELi0EEv11TraceParams9WfBuffersii"}
LDS_PER_CU = 163840
SIX_WAVE_DEPTHS = (6, 7, 8, 9)

PROGRAM = r"""
#include "trav_lds.h"
#include <cstdio>
int main()
{
  printf("granule %u lds %u words %d\n", VKRT_LDS_GRANULE_BYTES, VKRT_LDS_BYTES_PER_CU, VKRT_SHARE_LDS_WORDS_SIX);
  for(unsigned depth = 1; depth <= 16; depth++)
  {
    const unsigned cap = travStackCap(1u, depth, true, POSTPONE_ROOM);  // (-D: VKRT_W8_POSTPONE_ROOM of csrc/device_scene.h, what the host passes)
    const TravLds p = travLdsPlan(cap);
    printf("depth %u cap %u dynamic %zu static %zu charged %zu cu %u simd %u\n", depth, cap, p.dynamicBytes, p.staticBytes, p.chargedBytes, p.wavesPerCu,
           p.wavesPerSimd);
  }
  printf("bvh2 %u %u room %u\n", travStackCap(0u, 30u, false, 0u), travStackCap(0u, 30u, true, 4u), travStackCap(1u, 9u, true, 4u));
  return 0;
}
"""


def postpone_room():
    """VKRT_W8_POSTPONE_ROOM of csrc/device_scene.h: the entries api_accel.cpp adds to a wide8 stack for parked triangle groups"""
    m = re.search(r"^#define VKRT_W8_POSTPONE_ROOM (\d+)\b", open(os.path.join(CSRC, "device_scene.h")).read(), flags=re.M)
    return int(m.group(1))


def lds_plan(depth, granule, static_bytes=1280):
    """csrc/trav_lds.h restated: (stackCap, charged bytes, waves per CU, waves per SIMD) of a wide8 tree of `depth` with triangle postponing"""
    cap = 2 * (depth + 1) + 2 * postpone_room()
    charged = -(-(cap * 256 + static_bytes) // granule) * granule
    return cap, charged, LDS_PER_CU // charged, min(6, LDS_PER_CU // charged // 4)


def makefile_var(name):
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(rf"^{name}\s*[:?]?=\s*(.*)$", line)
        if m:
            return m.group(1).strip()
    raise KeyError(name)


def hipcc_version():
    out = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout
    m = re.search(r"HIP version:\s*(\S+)", out)
    return m.group(1) if m else "unknown"


@pytest.fixture(scope="module")
def record():
    return json.load(open(os.path.join(vkrt_amd.REPO_ROOT, "profiles", "r12_six_waves.json")))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """name -> (body, metadata) of the two product kernels"""
    if not HIPCC:
        pytest.skip("hipcc not found")
    want = json.load(open(os.path.join(vkrt_amd.REPO_ROOT, "profiles", "isa_mix.json"))).get("hipcc")
    if want and want != hipcc_version():
        pytest.skip(f"hipcc {hipcc_version()} is not the compiler of profiles/isa_mix.json ({want})")
    flags = makefile_var("FLAGS").replace("$(ARCH)", makefile_var("ARCH")).replace("-fPIC", "").split()
    flags += makefile_var("FLAGS_wf_traverse").split()
    out = tmp_path_factory.mktemp("six") / "wf_traverse.s"
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", "-o", str(out), "wf_traverse.hip"], cwd=CSRC, check=True, stderr=subprocess.DEVNULL)
    text = open(out).read()
    got = {}
    for name, sym in KERNELS.items():
        start = text.index(f"\n{sym}:")
        meta = text[text.index(f".amdhsa_kernel {sym}"):]
        got[name] = (text[start:text.index("\n.Lfunc_end", start)], meta[:meta.index(".end_amdhsa_kernel")])
    return got


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """what csrc/trav_lds.h computes, compiled alone by the host compiler: depth -> the fields of TravLds"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("trav_lds")
    src = d / "plan.cpp"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-DPOSTPONE_ROOM={postpone_room()}u", "-I", CSRC, "-o", str(d / "plan"), str(src)], check=True)
    out = subprocess.run([str(d / "plan")], capture_output=True, text=True, check=True).stdout.splitlines()
    head = dict(zip(out[0].split()[::2], map(int, out[0].split()[1::2])))
    rows = {}
    for line in out[1:]:
        w = line.split()
        if w[0] == "depth":
            rows[int(w[1])] = dict(zip(w[2::2], map(int, w[3::2])))
    tail = [int(w) for w in out[-1].split() if w.isdigit()]
    return head, rows, tail


def meta_int(meta, key):
    return int(re.search(rf"\.amdhsa_{key}\s+(\d+)", meta).group(1))


@pytest.mark.parametrize("name", list(KERNELS))
def test_product_kernel_fits_the_registers_of_six_waves(kernels, name):
    body, meta = kernels[name]
    vgprs = meta_int(meta, "next_free_vgpr")
    print(name, "vgprs", vgprs, "accum_offset", meta_int(meta, "accum_offset"))
    assert vgprs <= 80, vgprs  # 512 / 6 rounded down to the allocation granule of 8
    assert meta_int(meta, "private_segment_fixed_size") == 0
    assert "scratch_" not in body


def test_header_constants_are_the_measured_ones(plan, record):
    head, _, tail = plan
    assert head["granule"] == record["lds_granule_bytes"]
    assert head["lds"] == LDS_PER_CU == record["lds_bytes_per_cu"]
    assert tail == [32, 32, 28]  # BVH2: depth + 2 whatever the rest; wide8 with four reserved entries: 2 * 10 + 2 * 4


@pytest.mark.parametrize("name", list(KERNELS))
def test_lds_charge_allows_24_waves_per_cu_up_to_wide_depth_9(kernels, plan, record, name):
    _, meta = kernels[name]
    head, rows, _ = plan
    static = meta_int(meta, "group_segment_fixed_size")
    granule = record["lds_granule_bytes"]
    assert static == 4 * head["words"]  # the kernel's static block is the one the header counts
    for depth in SIX_WAVE_DEPTHS:
        r = rows[depth]
        assert r["cap"] == 2 * (depth + 1) + 2 * postpone_room() and r["dynamic"] == r["cap"] * 64 * 4 and r["static"] == static
        assert (r["cap"], r["charged"], r["cu"], r["simd"]) == lds_plan(depth, granule, static)
        charged = -(-(static + r["dynamic"]) // granule) * granule
        print(name, "depth", depth, "dynamic", r["dynamic"], "static", static, "charged", charged)
        assert charged <= LDS_PER_CU // 24, (depth, charged)
        assert r["charged"] == charged and r["cu"] >= 24 and r["simd"] == 6, r


def test_first_deeper_tree_gets_five_waves(plan, record):
    _, rows, _ = plan
    granule = record["lds_granule_bytes"]
    deeper = max(SIX_WAVE_DEPTHS) + 1
    r = rows[deeper]
    charged = -(-(r["static"] + r["dynamic"]) // granule) * granule
    assert charged > LDS_PER_CU // 24
    assert r["charged"] == charged and r["cu"] == LDS_PER_CU // charged and r["simd"] == 5, r
    assert (r["cap"], r["charged"], r["cu"], r["simd"]) == lds_plan(deeper, granule, r["static"])
    # ... and the count only falls from there
    for depth in range(deeper, 16):
        assert rows[depth + 1]["cu"] <= rows[depth]["cu"] < 24
