"""CPU-side checks of vkrt_debug_eval_shade: declared, exported and typed, documented with its record layout, argument-checked without a
device, and its kernel placed and built as the header says (the frame kernels' own functions, not a copy)."""
import ctypes as C
import os
import re

import vkrt_amd
from vkrt_amd import abi

ROOT = vkrt_amd.REPO_ROOT
CSRC = os.path.join(ROOT, "vk-raytracing-engine_amd", "csrc")


def _lib():
    assert os.path.exists(vkrt_amd.LIB_PATH), "run __graft_entry__.build() first"
    return abi.declare_vkrt(C.CDLL(vkrt_amd.LIB_PATH))


def _header_comment():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    end = header.index("int vkrt_debug_eval_shade(")
    return header[header.rindex("/*", 0, end):end]


def test_symbol_is_declared_exported_and_typed():
    header = open(os.path.join(ROOT, "include", "vkrt.h")).read()
    assert re.search(r"int\s+vkrt_debug_eval_shade\(int device, uint32_t n, const float\* in, float\* out\);", header)
    assert header.index("int vkrt_debug_eval_math(") < header.index("int vkrt_debug_eval_shade(")  # beside the math hook
    assert "vkrt_debug_eval_shade" in abi.VKRT_SYMBOLS
    lib = _lib()
    assert hasattr(lib, "vkrt_debug_eval_shade")
    assert lib.vkrt_debug_eval_shade.argtypes == [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p] and lib.vkrt_debug_eval_shade.restype is C.c_int
    # additive: a test hook changes no struct, so the ABI version stays 4
    assert lib.vkrt_abi_version() == 4 == abi.VKRT_ABI_VERSION


def test_header_documents_the_record_layout_and_the_lights_count_range():
    doc = _header_comment()
    for field in ("[0:3] worldPos", "[3:6] worldNrm", "[6:9] tangent", "[9:12] binormal", "[12:15] worldRayDir", "[15:19] baseColorFactor",
                  "[19] metallic", "[20] roughness", "[21:24] emissive", "[24:27] light.position", "[27:30] light.color", "[30] intensity",
                  "[31] light.type", "[32] seed", "[33] depth", "[34] isSpecular", "[35] lightsCount", "[36:40] pad",
                  "[0:3] hitValue", "[3:6] rayOrigin", "[6:9] rayDirection", "[9:12] weight", "[12] isSpecular", "[13] lightDist",
                  "[14:17] shadowRayDir", "[17] seed", "[18:20] pad"):
        assert field in doc, field
    assert "40 floats per record" in doc and "20 floats per record" in doc
    assert re.search(r"lightsCount is[\s*]+1 to 16", doc) and "VKRT_ERR_INVALID_ARGUMENT" in doc and "n == 0: VKRT_OK" in doc
    # the layout is the oracle's, word for word
    oracle = open(os.path.join(ROOT, "oracle", "oracle.cpp")).read()
    odoc = oracle[oracle.index("/* Shading spot-evaluation"):oracle.index("void orc_eval_shade(")]
    fields = re.findall(r"\[\d+(?::\d+)?\] [A-Za-z.]+", odoc)
    assert len(fields) == 27
    for f in fields:
        assert f in doc, f


def test_refusals_without_a_device():
    """NULL with n > 0 is refused before anything else; then (on a machine without a device) VKRT_ERR_NO_DEVICE; n == 0 is VKRT_OK
    where there is a device.  The order is vkrt_debug_eval_math's."""
    lib = _lib()
    rec = (C.c_float * 40)()
    out = (C.c_float * 20)()
    p_rec, p_out = C.addressof(rec), C.addressof(out)
    assert lib.vkrt_debug_eval_shade(0, 1, None, p_out) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert lib.vkrt_debug_eval_shade(0, 1, p_rec, None) == abi.VKRT_ERR_INVALID_ARGUMENT
    assert b"NULL" in lib.vkrt_last_error()
    has_device = lib.vkrt_device_count() > 0
    assert lib.vkrt_debug_eval_shade(0, 0, None, None) == (abi.VKRT_OK if has_device else abi.VKRT_ERR_NO_DEVICE)
    assert lib.vkrt_debug_eval_math(0, 0, 0, None, None, None) == (abi.VKRT_OK if has_device else abi.VKRT_ERR_NO_DEVICE)
    if not has_device:  # lightsCount = 0 in the zeroed record: the device comes first, as for every other argument of a debug hook
        assert lib.vkrt_debug_eval_shade(0, 1, p_rec, p_out) == abi.VKRT_ERR_NO_DEVICE


def test_kernel_sits_after_k_eval_math_and_calls_the_frame_kernels_functions():
    src = open(os.path.join(CSRC, "pathtrace.hip")).read()
    at = src.index("void k_eval_shade(")
    assert src.index("__global__ void k_eval_math") < at  # tests/test_alpha_frames_abi.py slices the file up to k_eval_math
    body = src[at:src.index("// ---- launch wrappers")]
    assert "closestHitLobe(mid, prd)" in body and "closestHitTail(sc, pc, mid, diffuse, prd, st)" in body
    assert re.search(r"if\s*\(i >= n\)\s*return;", body) and "mid.retap = 0u" in body
    # no copy of the bodies: the BRDF helpers and the samplers are reached through the two calls only
    for inner in ("directLight", "computePBR_BRDF", "samplingHemisphere", "samplingNDF_GGXTR", "getSpecularBRDF", "glsl_clamp", "rnd("):
        assert inner not in body, inner
    launch = src[src.index("hipError_t vkrt_launch_eval_shade("):]
    assert "k_eval_shade" in launch and "dim3(VKRT_BLOCK)" in launch and re.search(r"#define VKRT_BLOCK 256\b", src)
    kernels_h = open(os.path.join(CSRC, "kernels.h")).read()
    assert "hipError_t vkrt_launch_eval_shade(unsigned n, const float* in, float4* lights, float* out, hipStream_t stream);" in kernels_h
    assert re.search(r"#define VKRT_EVAL_SHADE_MAX_LIGHTS 16\b", kernels_h)
    # shade.h itself holds the two functions, once
    shade = open(os.path.join(CSRC, "shade.h")).read()
    assert shade.count("VKRT_DEV bool closestHitLobe(") == 1 and shade.count("VKRT_DEV void closestHitTail(") == 1


def test_python_wrapper_shapes_the_records():
    import inspect

    from vkrt_amd import renderer

    src = inspect.getsource(renderer.eval_shade)
    assert "reshape(-1, 40)" in src and "vkrt_debug_eval_shade" in src and list(inspect.signature(renderer.eval_shade).parameters) == ["records", "device"]
