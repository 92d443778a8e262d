"""Times the two ways of moving instances, for 300 and for 10 000 nodes of the synthetic instance grid (tests/scene_instances.py): writes
profiles/node_update_probe.json.  Medians of --calls calls after --warmup, device events around every call, the variants alternating
call by call in one process (as tools/morph_probe.py does); beside the device time between the two events, the host time the call took.

  a_host_update_nodes     vkrt_scene_update_nodes on a prepared vkrt_node array: records made on the host, sent as kernel arguments, 40
                          per launch (the path of the parent commit, unchanged: the baseline)
  b_device_transforms     vkrt_scene_update_node_transforms from a device array of matrices: one launch

Both are timed at the C ABI (prepared arguments, no Python marshalling inside the timed span).  Informational: no ratio is asserted.
The measurement runs in a child process under a time limit of its own (--limit seconds); the parent never opens the device and stops
at the child's first failure.

    python tools/node_update_probe.py --out profiles/node_update_probe.json
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

SIZES = (300, 10000)


def _timed(fns, calls, warmup):
    """fns: {name: callable}; one call of each per round, in order; returns {name: ([device ms per call], [host ms per call])}"""
    import torch

    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)] for k in fns}
    host = {k: [] for k in fns}
    for i in range(calls):
        for k, f in fns.items():
            ev[k][i][0].record()
            t0 = time.perf_counter()
            f()
            host[k].append((time.perf_counter() - t0) * 1e3)
            ev[k][i][1].record()
    torch.cuda.synchronize()
    return {k: ([a.elapsed_time(b) for a, b in v], host[k]) for k, v in ev.items()}


def measure(a):
    import ctypes as C

    import numpy as np
    import torch

    import vkrt_amd
    from scene_instances import instances_scene
    from vkrt_amd import abi
    from vkrt_amd.renderer import Renderer

    res = {"workload": "tests/scene_instances.py: a grid of quads and boxes, every node moved per call", "source_hash": vkrt_amd.source_hash(),
           "method": f"medians of {a.calls} calls after {a.warmup}, device events around every call (device_ms) and the host's clock around the call "
                     "itself (host_ms), variants alternating call by call; both at the C ABI with prepared arguments"}
    for n in SIZES:
        flat = instances_scene(nodes=n)
        r = Renderer(flat, device=0, build=None)
        rng = np.random.default_rng(5)
        poses = []
        for _ in range(2):
            m = flat.nodes["worldMatrix"].copy()
            m[:, 12:15] += rng.uniform(-0.2, 0.2, (n, 3)).astype(np.float32)
            nd = flat.nodes.copy()
            nd["worldMatrix"] = m
            arr = (abi.Node * n)()
            C.memmove(arr, nd.ctypes.data, C.sizeof(abi.Node) * n)
            t = torch.as_tensor(m, device="cuda:0")
            poses.append((arr, t, abi.NodeUpdate(C.sizeof(abi.NodeUpdate), 0, n, abi.VKRT_MEMORY_DEVICE, t.data_ptr(), None)))
        lib, h, turn = r.lib, r._h, [0]

        def host_update():
            turn[0] += 1
            assert lib.vkrt_scene_update_nodes(h, 0, n, poses[turn[0] & 1][0], None) == 0

        def device_update():
            turn[0] += 1
            assert lib.vkrt_scene_update_node_transforms(h, C.byref(poses[turn[0] & 1][2]), None) == 0

        s = _timed({"a_host_update_nodes": host_update, "b_device_transforms": device_update}, a.calls, a.warmup)
        out = {k: {"device_median_ms": statistics.median(d), "device_min_ms": min(d), "device_max_ms": max(d), "host_median_ms": statistics.median(w),
                   "host_min_ms": min(w), "host_max_ms": max(w), "calls": len(d)} for k, (d, w) in s.items()}
        out["launches"] = {"a_host_update_nodes": (n + 39) // 40, "b_device_transforms": 1}
        out["a_over_b_device"] = out["a_host_update_nodes"]["device_median_ms"] / out["b_device_transforms"]["device_median_ms"]
        out["a_over_b_host"] = out["a_host_update_nodes"]["host_median_ms"] / out["b_device_transforms"]["host_median_ms"]
        out["device_path_is_faster"] = bool(out["a_over_b_device"] > 1.0 and out["a_over_b_host"] > 1.0)
        # both paths leave the same records (the last call of each wrote the same pose or the other one: compare after one more of each)
        host_update()
        want = r.read_instances(0, n).copy()
        turn[0] -= 1
        device_update()
        assert np.array_equal(r.read_instances(0, n).view(np.uint8), want.view(np.uint8))
        res[f"nodes_{n}"] = out
        r.close()
    res["note"] = ("a does not include what a caller with transforms in device memory pays before it: the copy to the host and the wait for it.  "
                   "device_ms spans from the stream reaching the first event to its reaching the second, so for a it includes the gaps between "
                   "its launches, which the host issues one by one.")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds the measuring child process may take")
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert a.calls >= 20, "medians of at least 20 calls"
    if a.child:
        print("NODE_UPDATE_PROBE " + json.dumps(measure(a)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--warmup", str(a.warmup)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    except subprocess.TimeoutExpired:
        print(f"node_update_probe: the measurement did not finish within {a.limit} s", file=sys.stderr)
        return 124
    lines = [x for x in p.stdout.splitlines() if x.startswith("NODE_UPDATE_PROBE ")]
    if p.returncode != 0 or not lines:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        return p.returncode or 1
    line = json.dumps(json.loads(lines[-1][len("NODE_UPDATE_PROBE "):]), indent=1)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
