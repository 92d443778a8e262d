"""CPU-side checks of VKRT_OPT_WF_CAMERA_ROUNDS (camera rays traced from the pixel grid, csrc/wavefront.hip): the option's number and
default in the header, the Python constants and the library agree, and the option adds nothing to the working set."""
import ctypes as C
import os
import re

import vkrt_amd
from vkrt_amd import abi

from test_scene_options import option_env, option_table


def _read(*parts):
    return open(os.path.join(vkrt_amd.REPO_ROOT, *parts)).read()


def test_option_constant_follows_the_header():
    hdr = _read("include", "vkrt.h")
    assert abi.VKRT_OPT_WF_CAMERA_ROUNDS == 16
    assert re.search(r"\bVKRT_OPT_WF_CAMERA_ROUNDS\s*=\s*16\b", hdr)
    # appended within ABI 4 like option 15: VKRT_OPT_LAST keeps naming the last option every ABI-4 library has
    assert re.search(r"\bVKRT_OPT_LAST\s*=\s*14\b", hdr) and re.search(r"\bVKRT_OPT_WF_SAMPLE_SYNC\s*=\s*15\b", hdr)
    assert abi.VKRT_OPT_WF_SAMPLE_SYNC == 15


def test_default_is_the_headers_and_the_env_hook_is_documented():
    hdr = _read("include", "vkrt.h")
    start = hdr.index("VKRT_OPT_WF_CAMERA_ROUNDS = 16")
    doc = hdr[start:hdr.index("*/", start)]
    m = re.search(r"(\d) \(default\)", doc)
    assert m and "env VKRT_WF_CAMERA_ROUNDS" in doc
    assert option_table().shim_option_default(abi.VKRT_OPT_WF_CAMERA_ROUNDS) == int(m.group(1))
    assert option_env(abi.VKRT_OPT_WF_CAMERA_ROUNDS) == "VKRT_WF_CAMERA_ROUNDS"
    assert "`VKRT_OPT_WF_CAMERA_ROUNDS` / `VKRT_WF_CAMERA_ROUNDS` | %s |" % m.group(1) in _read("README.md")


def test_working_set_bytes_are_unchanged():
    """vkrt_wf_state_bytes, the one sizing function behind vkrt_reserve / vkrt_reserve_frames and the trace calls: count words + per
    path and frame group 544 B of record streams and 16 B of sample state + a 16-B staging plane per group when there are several --
    what it was before the option existed (tests/test_sample_sync_abi.py)."""
    lib = C.CDLL(vkrt_amd.LIB_PATH)
    f = getattr(lib, "_Z19vkrt_wf_state_bytesji", None)
    assert f is not None, "libvkrt.so has no vkrt_wf_state_bytes(unsigned, int): did the signature in csrc/kernels.h change?"
    f.argtypes, f.restype = [C.c_uint32, C.c_int], C.c_size_t
    assert f(0, 1) == f(0, 8) == 256 * 8
    for paths in (64, 3200, 2073600):
        for groups in (1, 2, 3, 8):
            assert f(paths, groups) == 256 * 8 + groups * paths * (544 + 16) + (groups * paths * 16 if groups > 1 else 0), (paths, groups)
