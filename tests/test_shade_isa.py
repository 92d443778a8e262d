"""What the shade kernels' assembly must keep (profiles/r10_experiments.md): csrc/wavefront.hip cross-compiled for gfx950 on the CPU with the
flags csrc/Makefile gives it; k_wf_shade, k_wf_shade_camera and k_wf_shade_hybrid are checked for the properties the overlapped frame
rests on -- three waves per SIMD, nothing spilled, and no more VALU issue slots than profiles/shade_isa.json records for this commit
(tools/shade_isa.py writes that file and defines a slot).  No GPU needed; skipped when hipcc is absent or is not the compiler of the profile."""
import json
import os
import shutil
import sys

import pytest

import vkrt_amd

sys.path.insert(0, os.path.join(vkrt_amd.REPO_ROOT, "tools"))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
KERNELS = ("k_wf_shade", "k_wf_shade_camera", "k_wf_shade_hybrid")


@pytest.fixture(scope="module")
def profile():
    return json.load(open(os.path.join(vkrt_amd.REPO_ROOT, "profiles", "shade_isa.json")))


@pytest.fixture(scope="module")
def shade_stats(profile, tmp_path_factory):
    if not HIPCC:
        pytest.skip("hipcc not found")
    import shade_isa

    shade_isa.HIPCC = HIPCC
    if profile["hipcc"] != shade_isa.hipcc_version():
        pytest.skip(f"hipcc {shade_isa.hipcc_version()} is not the compiler of profiles/shade_isa.json ({profile['hipcc']}): re-take tools/shade_isa.py --json")
    asm = shade_isa.compile_asm(out=str(tmp_path_factory.mktemp("isa") / "wavefront.s"))
    stats, _ = shade_isa.take(asm=asm)
    return stats


def test_profile_is_of_these_sources_and_records_a_cut(profile):
    import shade_isa

    assert profile["this"]["sources"] == shade_isa.source_hashes(shade_isa.CSRC)  # re-take tools/shade_isa.py --json after a change
    for k in KERNELS:
        this, parent = profile["this"]["kernels"][k], profile["parent"]["kernels"][k]
        assert this["slots"] < parent["slots"], (k, this["slots"], parent["slots"])
        assert sum(this["by_class"].values()) == this["valu"] and sum(parent["by_class"].values()) == parent["valu"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_shade_kernel_keeps_three_waves_and_no_scratch(shade_stats, kernel):
    s = shade_stats[kernel]
    print(kernel, s["vgprs"], "VGPRs", s["scratch_bytes"], "B scratch")
    assert s["vgprs"] <= 168, s["vgprs"]  # three waves per SIMD: 512 / 3, in allocation granules of 8
    assert s["scratch_bytes"] == 0 and s["scratch_ops"] == 0, (s["scratch_bytes"], s["scratch_ops"])


@pytest.mark.parametrize("kernel", KERNELS)
def test_shade_kernel_issues_no_more_slots_than_recorded(shade_stats, profile, kernel):
    got, want = shade_stats[kernel]["slots"], profile["this"]["kernels"][kernel]["slots"]
    print(kernel, got, "slots; recorded", want, "; parent", profile["parent"]["kernels"][kernel]["slots"])
    assert got <= want, (kernel, got, want)


def test_shade_kernels_form_no_packed_fp32(shade_stats):
    # a packed FP32 instruction takes two issue slots and needs its operands moved into register pairs (wavefront.hip WF_SCALAR_FP32)
    for k in KERNELS:
        assert "packed_f32" not in shade_stats[k]["by_class"], (k, shade_stats[k]["by_class"])
