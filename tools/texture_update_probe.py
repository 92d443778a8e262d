"""Times vkrt_scene_update_texture on one 2048 x 2048 sRGB texture from device memory, against its floor and against the only route there
was before it: writes profiles/texture_update_probe.json.  Medians of --calls calls after --warmup, device events around every call, the
variants alternating call by call in one process.

  update_device_ms    vkrt_scene_update_texture with VKRT_MEMORY_DEVICE: level 0 and the footprint records, seven mip launches, one tail
                      launch (prepared arguments at the C ABI, no Python marshalling inside the timed span)
  copy_floor_ms       one stream-ordered device-to-device copy that moves as many bytes as the update reads plus writes (the copy reads
                      and writes each of its bytes once, so it copies half that number): what the memory system alone asks for
  create_and_build_ms vkrt_scene_create + vkrt_accel_build of the same scene with the new image, host wall time: the route of a library
                      without the entry point.  --parent-lib PATH times it on another build of libvkrt.so (the parent commit's) as well

Informational: no ratio is asserted.  The measurement runs in a child process under a time limit of its own (--limit seconds); the
parent never opens the device and stops at the child's first failure.

    python tools/texture_update_probe.py --out profiles/texture_update_probe.json [--parent-lib libvkrt_parent.so]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "oracle", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))

SIDE = 2048


def _scene(image):
    import numpy as np
    from vkrt_amd.flat_scene import LIGHT_DTYPE, MAT_DTYPE, NODE_DTYPE, PRIM_DTYPE, FlatScene

    pos = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32)
    nrm, tan = np.tile(np.array([0, 0, 1], np.float32), (4, 1)), np.tile(np.array([1, 0, 0, 1], np.float32), (4, 1))
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    pm = np.zeros(1, PRIM_DTYPE)
    pm[0] = (0, 6, 0, 4, 0)
    mats = np.zeros(1, MAT_DTYPE)
    mats[0]["pbrBaseColorFactor"] = [1.0, 1.0, 1.0, 1.0]
    mats[0]["pbrBaseColorTexture"] = 0
    mats[0]["metallicRoughnessTexture"] = mats[0]["normalTexture"] = mats[0]["emissiveTexture"] = -1
    mats[0]["roughnessFactor"] = 1.0
    nodes = np.zeros(1, NODE_DTYPE)
    nodes[0]["worldMatrix"] = np.eye(4, dtype=np.float32).ravel()
    lights = np.zeros(1, LIGHT_DTYPE)
    lights[0] = ((0.5, 0.5, 3.0), (1, 1, 1), 20.0, 0)
    return FlatScene(pos, nrm, tan, uv, np.array([0, 1, 2, 0, 2, 3], np.uint32), pm, mats, lights, nodes, [{"rgba8": image, "is_srgb": True}])


def _traffic_bytes(side):
    """bytes the update reads plus writes: level 0 (the image read once, the pool word and the 16-B footprint record written), then every
    mip level reading the level before it and writing itself"""
    n = side * side
    total, w = 4 * n + 4 * n + 16 * n, side
    while w > 1:
        total += 4 * w * w + 4 * (w // 2) * (w // 2)
        w //= 2
    return total


def _create_and_build(lib_path, flat, rounds):
    """host wall ms of vkrt_scene_create + vkrt_accel_build (default flags) per round, through a library handle of its own: only what
    every build of the library exports is declared"""
    import ctypes as C

    from vkrt_amd import abi

    lib = C.CDLL(lib_path)
    lib.vkrt_scene_create.argtypes = [C.POINTER(abi.SceneDesc), C.c_int, C.POINTER(C.c_void_p)]
    lib.vkrt_accel_build.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.vkrt_scene_destroy.argtypes = [C.c_void_p]
    lib.vkrt_scene_destroy.restype = None
    desc, keep = flat.to_desc()
    out = []
    for _ in range(rounds):
        h = C.c_void_p()
        t0 = time.perf_counter()
        rc = lib.vkrt_scene_create(C.byref(desc), 0, C.byref(h))
        rc = rc or lib.vkrt_accel_build(h, 0, None)
        out.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0, rc
        lib.vkrt_scene_destroy(h)
    del keep
    return out


def measure(a):
    import ctypes as C

    import numpy as np
    import torch

    import vkrt_amd
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer

    rng = np.random.default_rng(1)
    first, second = (rng.integers(0, 256, (SIDE, SIDE, 4), dtype=np.uint8) for _ in range(2))
    flat = _scene(first)
    r = Renderer(flat, device=0, build="ploc")
    dev = torch.from_numpy(second).to("cuda:0")
    traffic = _traffic_bytes(SIDE)
    src, dst = (torch.empty(traffic // 2, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    u = abi.TextureUpdate(C.sizeof(abi.TextureUpdate), 0, SIDE, SIDE, abi.VKRT_MEMORY_DEVICE, dev.data_ptr())
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    lib = r.lib

    def update():
        assert lib.vkrt_scene_update_texture(r._h, C.byref(u), st) == 0

    def copy():
        dst.copy_(src, non_blocking=True)

    fns = {"update_device_ms": update, "copy_floor_ms": copy}
    for _ in range(a.warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)] for k in fns}
    for i in range(a.calls):
        for k, f in fns.items():
            ev[k][i][0].record()
            f()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    ms = {k: sorted(x.elapsed_time(y) for x, y in v) for k, v in ev.items()}
    # the result is the image: level 0 reads back as the new texels
    assert np.array_equal(r.read_texture(0, 0), second)
    r.close()
    out = {"texture": f"{SIDE}x{SIDE} sRGB, device memory", "calls": a.calls, "warmup": a.warmup, "traffic_bytes": traffic, "copy_bytes": traffic // 2,
           "launches_per_update": 9}
    for k, v in ms.items():
        out[k] = {"median": statistics.median(v), "min": v[0], "max": v[-1]}
    out["update_over_floor"] = out["update_device_ms"]["median"] / out["copy_floor_ms"]["median"]
    out["update_gb_per_s"] = traffic / out["update_device_ms"]["median"] / 1e6
    routes = {"this_build": vkrt_amd.LIB_PATH}
    if a.parent_lib:
        routes["parent_build"] = os.path.abspath(a.parent_lib)
    target = _scene(second)
    for name, path in routes.items():
        v = sorted(_create_and_build(path, target, a.rebuilds + 1)[1:])  # (the first round warms the library up)
        out["create_and_build_ms_" + name] = {"median": statistics.median(v), "min": v[0], "max": v[-1], "rounds": a.rebuilds}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_update_probe.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rebuilds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return measure(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--warmup", str(a.warmup), "--rebuilds", str(a.rebuilds)]
    if a.parent_lib:
        cmd += ["--parent-lib", a.parent_lib]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    if p.returncode != 0:
        sys.exit(f"the measurement failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    doc = json.loads(p.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
