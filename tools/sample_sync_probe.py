"""Probe of the two schedules of the wavefront path tracer (VKRT_OPT_WF_SAMPLE_SYNC 0 / 1) on the frame bench.py times: the
262 k-triangle atrium at 1920x1080, 16 spp, depth 8, device-built tree.  Per option, in one process: warm-up frames with the option
set, un-overlapped kernel times of single timed frames (VKRT_TRACE_TIME_KERNELS: traverse_ms, shade time per launch) and the frame
time of six-frame calls with the default frames in flight.  One JSON line per option.

PROBE_SYNC="0,1" picks the values ("none": the option is left alone, e.g. for an older build selected with VKRT_LIB that lacks it);
PROBE_OPTION picks the option they are set on (default 15, VKRT_OPT_WF_SAMPLE_SYNC; 16 = VKRT_OPT_WF_CAMERA_ROUNDS: camera rays from
records / from the pixel grid);
PROBE_TIMED=0 leaves the timed frames out, so that a kernel trace of the run holds plain frames only (2 single frames and
1 + PROBE_CALLS calls of six per option)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

W, H, SPP, DEPTH, PER_CALL = 1920, 1080, 16, 8, 6


def main():
    import torch
    import vkrt_amd
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants, uniforms_from_matrices
    from vkrt_amd.renderer import Renderer
    import atrium
    import camera_np

    flat, _ = atrium.build_atrium(262144, seed=1, with_textures=True)
    cam = uniforms_from_matrices(*camera_np.global_uniforms(width=W, height=H, **atrium.DEFAULT_CAMERA))
    lights = len(flat.lights)
    r = Renderer(flat, device=0, build="ploc")
    img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")

    def pc(frame):
        return make_push_constants(samples=SPP, depth=DEPTH, frame=frame, lights_count=lights)

    option = int(os.environ.get("PROBE_OPTION", abi.VKRT_OPT_WF_SAMPLE_SYNC))
    for opt in os.environ.get("PROBE_SYNC", "0,1").split(","):
        if opt != "none":
            r.set_option(option, int(opt))
        for f in range(2):  # warm-up under this option, and frames 0..7 of the image
            r.pathtrace(pc(f), cam, W, H, seed=f, image=img)
        r.pathtrace_frames(pc(2), cam, W, H, PER_CALL, seed=2, image=img)
        torch.cuda.synchronize()
        out = {"sample_sync" if option == abi.VKRT_OPT_WF_SAMPLE_SYNC else f"option_{option}": opt, "lib": os.path.basename(vkrt_amd.LIB_PATH)}
        if os.environ.get("PROBE_TIMED", "1") != "0":
            tr, sh, tot = [], [], []
            for k in range(3):
                r.pathtrace(pc(8 + k), cam, W, H, seed=8 + k, flags=abi.VKRT_TRACE_TIME_KERNELS, image=img)
                torch.cuda.synchronize()
                t = r.last_trace_timing()
                tr.append(t["traverse_ms"]); sh.append(t["shade_ms"] / max(t["shade_launches"], 1)); tot.append(t["total_ms"])
            out.update({"timed_frame_ms": tot, "traverse_ms": tr, "traverse_launches": t["traverse_launches"], "shade_ms_per_launch": sh,
                        "shade_launches": t["shade_launches"]})
        calls = []
        r.reset_counters()
        for k in range(int(os.environ.get("PROBE_CALLS", 3))):
            r.pathtrace_frames(pc(11 + PER_CALL * k), cam, W, H, PER_CALL, seed=11 + PER_CALL * k, image=img)
            torch.cuda.synchronize()
            calls.append(r.last_trace_ms() / PER_CALL)
        c = r.counters()
        out.update({"ms_per_frame_in_calls_of_6": calls, "rays": c["rays_closest"] + c["rays_shadow"], "pair_records": c["pair_records"]})
        print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    main()
