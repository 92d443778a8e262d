"""CPU-side checks of the denoiser's C ABI (include/vkrt.h vkrt_denoiser_*, vkrt_denoise_diffuse): declared, exported and mirrored
by abi.py; argument refusals; no CPU fallback; the kernels keep everything in registers."""
import ctypes as C
import os
import re
import subprocess

import vkrt_amd
from vkrt_amd import abi

ROOT = vkrt_amd.REPO_ROOT
NAMES = ["vkrt_denoiser_create", "vkrt_denoiser_destroy", "vkrt_denoiser_reset", "vkrt_denoise_diffuse"]


def _lib():
    from vkrt_amd.renderer import load_library

    return load_library()


def test_denoiser_symbols_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    declared = set(re.findall(r"\b(vkrt_[a-z_]+)\s*\(", header))
    lib = C.CDLL(vkrt_amd.LIB_PATH)
    for n in NAMES:
        assert n in declared and n in abi.VKRT_SYMBOLS and hasattr(lib, n), n
    lib = _lib()
    assert len(lib.vkrt_denoise_diffuse.argtypes) == 7 and lib.vkrt_denoise_diffuse.restype == C.c_int
    assert len(lib.vkrt_denoiser_create.argtypes) == 4
    # additive entry points: the version and the option range stay where they were
    assert "#define VKRT_ABI_VERSION 4" in header and "VKRT_OPT_LAST            = 14" in header


def test_settings_struct_matches_header(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vkrt.h"\nint main(void){printf("%zu %zu %zu\\n", sizeof(vkrt_denoise_settings),'
                   ' offsetof(vkrt_denoise_settings, atrous_iterations), offsetof(vkrt_denoise_settings, max_history)); return 0;}\n')
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(abi.DenoiseSettings), abi.DenoiseSettings.atrous_iterations.offset, abi.DenoiseSettings.max_history.offset]


def test_refusals():
    lib = _lib()
    cam = abi.GlobalUniforms()
    planes = [C.create_string_buffer(64) for _ in range(7)]
    gb = abi.Gbuffer(*(C.addressof(p) for p in planes[:4]))
    nrd = abi.NrdPlanes(None, C.addressof(planes[4]), C.addressof(planes[5]))
    out = C.c_void_p(C.addressof(planes[6]))
    dn = C.c_void_p(0)

    def call(settings, d=dn, g=gb, n=nrd, o=out, c=cam):
        return lib.vkrt_denoise_diffuse(d, C.byref(settings) if settings is not None else None, C.byref(c) if c is not None else None,
                                        C.byref(g) if g is not None else None, C.byref(n) if n is not None else None, o, None)

    ok = abi.DenoiseSettings(C.sizeof(abi.DenoiseSettings), 5, 32)
    assert call(abi.DenoiseSettings(8, 5, 32)) == abi.VKRT_ERR_INVALID_ARGUMENT and b"struct_size" in lib.vkrt_last_error()
    for it, mh, word in ((6, 32, b"atrous_iterations"), (-1, 32, b"atrous_iterations"), (5, 0, b"max_history"), (5, 256, b"max_history")):
        assert call(abi.DenoiseSettings(C.sizeof(abi.DenoiseSettings), it, mh)) == abi.VKRT_ERR_INVALID_ARGUMENT
        assert word in lib.vkrt_last_error()
    # NULL planes are refused before the handle is looked at (so this runs without a device as well)
    for i in range(4):
        bad = abi.Gbuffer(*(None if k == i else C.addressof(planes[k]) for k in range(4)))
        assert call(ok, g=bad) == abi.VKRT_ERR_INVALID_ARGUMENT and b"G-buffer plane" in lib.vkrt_last_error()
    for bad in (abi.NrdPlanes(None, None, C.addressof(planes[5])), abi.NrdPlanes(None, C.addressof(planes[4]), None)):
        assert call(ok, n=bad) == abi.VKRT_ERR_INVALID_ARGUMENT and b"NRD plane" in lib.vkrt_last_error()
    for kw in ({"g": None}, {"n": None}, {"c": None}, {"o": None}):
        assert call(ok, **kw) == abi.VKRT_ERR_INVALID_ARGUMENT and b"NULL argument" in lib.vkrt_last_error()
    assert call(ok) == abi.VKRT_ERR_INVALID_ARGUMENT and b"NULL denoiser" in lib.vkrt_last_error()
    assert call(None) == abi.VKRT_ERR_INVALID_ARGUMENT                                     # defaults, still a NULL handle
    assert lib.vkrt_denoiser_reset(None) == abi.VKRT_ERR_INVALID_ARGUMENT
    lib.vkrt_denoiser_destroy(None)  # no-op
    assert lib.vkrt_denoiser_create(0, 16, 16, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    h = C.c_void_p()
    assert lib.vkrt_denoiser_create(0, 0, 16, C.byref(h)) == abi.VKRT_ERR_INVALID_ARGUMENT and not h.value
    if lib.vkrt_device_count() == 0:
        # no CPU fallback: without a device there is no denoiser
        assert lib.vkrt_denoiser_create(0, 64, 32, C.byref(h)) == abi.VKRT_ERR_NO_DEVICE
        assert b"no HIP device" in lib.vkrt_last_error() and not h.value


def test_denoise_kernels_use_no_scratch(tmp_path):
    csrc = os.path.join(ROOT, "vk-raytracing-engine_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                        "-c", os.path.join(csrc, "denoise.hip"), "-o", str(tmp_path / "dn.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, check=True)
    kernel, scratch = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            kernel = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and kernel:
            scratch[kernel] = int(m.group(1))
    names = {k for k in scratch if re.search(r"k_dn_(temporal|variance|atrous)", k)}
    assert len(names) == 3, scratch
    assert all(scratch[k] == 0 for k in names), scratch
