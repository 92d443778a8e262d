"""What the sharing traversal loops must keep outside their node test (profiles/r11_experiments.md): csrc/wf_traverse.hip cross-compiled
for gfx950 on the CPU with the flags csrc/Makefile gives it; the two sharing loops of k_wf_traverse<false, true, 64, 0> and the loop of
k_wf_traverse_camera<false, 0> are taken apart by region as tools/isa_blocks.py --loops-json does, and outside the node test none of
them may hold more VALU instructions or issue slots than profiles/traverse_loop_isa.json records for this commit, which in turn must be
below the parent's.  (tests/test_kernel_isa.py pins the node test and the kernel's registers.)  No GPU needed; skipped when hipcc is
absent or is not the compiler of the profile."""
import json
import os
import shutil
import sys

import pytest

import vkrt_amd

sys.path.insert(0, os.path.join(vkrt_amd.REPO_ROOT, "tools"))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
CSRC = os.path.join(vkrt_amd.PKG_DIR, "csrc")


@pytest.fixture(scope="module")
def profile():
    return json.load(open(os.path.join(vkrt_amd.REPO_ROOT, "profiles", "traverse_loop_isa.json")))


@pytest.fixture(scope="module")
def loops(profile):
    if not HIPCC:
        pytest.skip("hipcc not found")
    import isa_blocks
    import shade_isa

    shade_isa.HIPCC = HIPCC
    if profile["hipcc"] != shade_isa.hipcc_version():
        pytest.skip(f"hipcc {shade_isa.hipcc_version()} is not the compiler of profiles/traverse_loop_isa.json ({profile['hipcc']}): "
                    "re-take tools/isa_blocks.py --loops-json")
    # one compilation, with line tables; that this listing is the product's instruction for instruction was checked when the profile
    # was written (tools/isa_blocks.py --loops-json compiles both)
    return isa_blocks.loops_by_region(CSRC, verify=False, resources=False)["loops"]


def loop_names():
    import isa_blocks

    return [n for n, _, _ in isa_blocks.LOOPS]


def test_profile_is_of_these_sources_and_records_a_cut(profile):
    import isa_blocks

    assert profile["this"]["sources"] == isa_blocks.loop_source_hashes(CSRC)  # re-take tools/isa_blocks.py --loops-json after a change
    assert profile["this"]["sources"] != profile["parent"]["sources"]
    for n in loop_names():
        this, parent = profile["this"]["loops"][n], profile["parent"]["loops"][n]
        for k in ("valu", "slots"):
            assert this["outside_node_test"][k] < parent["outside_node_test"][k], (n, k, this["outside_node_test"], parent["outside_node_test"])
            assert sum(r[k] for r in this["regions"].values()) == this["total"][k]
            assert this["total"][k] - this["regions"]["node_test"][k] == this["outside_node_test"][k]


def test_profile_lists_the_resources_of_every_instantiation(profile):
    """no traversal or query kernel uses more registers' worth of waves or more scratch than its parent did"""
    this, parent = profile["this"]["resources"], profile["parent"]["resources"]
    assert set(this) == set(parent) and len(this) >= 40
    waves = lambda v: min(8, 512 // (8 * -(-v // 8)))  # waves per SIMD the registers allow (allocation granules of 8)
    for k in this:
        assert waves(this[k]["vgprs"]) >= waves(parent[k]["vgprs"]), (k, this[k], parent[k])
        assert this[k]["scratch_bytes"] <= parent[k]["scratch_bytes"], (k, this[k], parent[k])


@pytest.mark.parametrize("index", range(3))
def test_loop_holds_no_more_outside_its_node_test_than_recorded(loops, profile, index):
    name = loop_names()[index]
    got, want, parent = loops[name]["outside_node_test"], profile["this"]["loops"][name]["outside_node_test"], profile["parent"]["loops"][name]["outside_node_test"]
    print(name, got, "recorded", want, "parent", parent, loops[name]["regions"])
    assert got["valu"] <= want["valu"], (name, got, want)
    assert got["slots"] <= want["slots"], (name, got, want)
