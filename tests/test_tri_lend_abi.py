"""CPU-side checks of VKRT_OPT_WF_TRI_LEND (triangle steps of the sharing traversal wave lend pending triangles to free lanes,
csrc/traverse_share.h): the option's number and default in the header, the Python constants, the library's option table and the README
agree, and the option costs no LDS of its own."""
import os
import re

import vkrt_amd
from vkrt_amd import abi

from test_scene_options import option_env, option_table


def _read(*parts):
    return open(os.path.join(vkrt_amd.REPO_ROOT, *parts)).read()


def test_option_constant_follows_the_header():
    hdr = _read("include", "vkrt.h")
    assert abi.VKRT_OPT_WF_TRI_LEND == 17
    assert re.search(r"\bVKRT_OPT_WF_TRI_LEND\s*=\s*17\b", hdr)
    # appended within ABI 4 like options 15 and 16: VKRT_OPT_LAST keeps naming the last option every ABI-4 library has
    assert re.search(r"\bVKRT_OPT_LAST\s*=\s*14\b", hdr)
    assert re.search(r"\bVKRT_OPT_WF_SAMPLE_SYNC\s*=\s*15\b", hdr) and re.search(r"\bVKRT_OPT_WF_CAMERA_ROUNDS\s*=\s*16\b", hdr)
    assert abi.VKRT_OPT_WF_SAMPLE_SYNC == 15 and abi.VKRT_OPT_WF_CAMERA_ROUNDS == 16


def test_default_is_the_headers_and_the_env_hook_is_documented():
    hdr = _read("include", "vkrt.h")
    start = hdr.index("VKRT_OPT_WF_TRI_LEND = 17")
    doc = hdr[start:hdr.index("*/", start)]
    m = re.search(r"(\d) \(default\)", doc)
    assert m and "env VKRT_WF_TRI_LEND" in doc
    table = option_table()
    assert table.shim_option_default(abi.VKRT_OPT_WF_TRI_LEND) == int(m.group(1))
    assert option_env(abi.VKRT_OPT_WF_TRI_LEND) == "VKRT_WF_TRI_LEND"
    assert "`VKRT_OPT_WF_TRI_LEND` / `VKRT_WF_TRI_LEND` | %s |" % m.group(1) in _read("README.md")


def test_option_eight_keeps_its_default_and_mask():
    """the switch travels in a bit of DevScene::shareFlags above the five that VKRT_OPT_WF_SHARE_FLAGS owns"""
    table = option_table()
    assert table.shim_option_default(abi.VKRT_OPT_WF_SHARE_FLAGS) == 25
    assert [table.shim_clamp_option(abi.VKRT_OPT_WF_SHARE_FLAGS, v) for v in (-1, 31, 32, 57, 255)] == [31, 31, 0, 25, 31]  # v & 31
    dev = _read("vk-raytracing-engine_amd", "csrc", "device_scene.h")
    m = re.search(r"#define VKRT_SHARE_TRI_LEND (0x[0-9a-fA-F]+)u", dev)
    assert m and int(m.group(1), 16) & 31 == 0 and bin(int(m.group(1), 16)).count("1") == 1


def test_the_wave_block_in_lds_is_not_grown():
    share = _read("vk-raytracing-engine_amd", "csrc", "traverse_share.h")
    assert re.search(r"#define VKRT_SHARE_LDS_WORDS 384\b", share)  # 64 x (u64 key, slot, u, v, donor): the match rides in donor[]
