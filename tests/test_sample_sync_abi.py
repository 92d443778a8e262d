"""CPU-side check of the working set the sample-synchronous schedule adds (VKRT_OPT_WF_SAMPLE_SYNC, csrc/wavefront.hip)."""
import ctypes as C

from vkrt_amd import abi


def test_state_bytes_grow_by_16_per_pixel_and_group():
    """vkrt_wf_state_bytes (the one sizing function behind vkrt_reserve_frames and the trace calls): the working set is the count
    words + per path and frame group the 544 B of record streams and 16 B of sample state + the 16 B staging plane of every
    group when there are several."""
    import vkrt_amd

    lib = C.CDLL(vkrt_amd.LIB_PATH)
    # size_t vkrt_wf_state_bytes(uint32_t pathCapacity, int groups) of csrc/kernels.h: a C++ function of the library, not of the C ABI,
    # so it is found under its Itanium-mangled name; a changed signature has to be followed here
    f = getattr(lib, "_Z19vkrt_wf_state_bytesji", None)
    assert f is not None, "libvkrt.so has no vkrt_wf_state_bytes(unsigned, int): did the signature in csrc/kernels.h change?"
    f.argtypes, f.restype = [C.c_uint32, C.c_int], C.c_size_t
    ctrl = f(0, 1)
    assert ctrl == f(0, 8) == 256 * 8
    for paths in (64, 3200, 2073600):
        for groups in (1, 2, 3, 8):
            without_state = ctrl + groups * paths * 544 + (groups * paths * 16 if groups > 1 else 0)
            assert f(paths, groups) == without_state + 16 * paths * groups, (paths, groups)


def test_option_constant_follows_the_header():
    import os

    import vkrt_amd

    hdr = open(os.path.join(vkrt_amd.REPO_ROOT, "include", "vkrt.h")).read()
    assert abi.VKRT_OPT_WF_SAMPLE_SYNC == 15 and "VKRT_OPT_WF_SAMPLE_SYNC  = 15" in hdr
