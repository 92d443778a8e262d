"""VKRT_OPT_WF_CAMERA_ROUNDS: in the sample-synchronous schedule the first round of every sample traces and shades its camera rays
straight from the pixel grid (csrc/wf_traverse.hip k_wf_traverse_camera, csrc/wavefront.hip k_wf_shade_camera) instead of from
records that k_wf_init / k_wf_sample_init wrote (option 0, the record path).  The functions, draws and float operations are the
same and only where a value comes from changes, so every case runs with the option at 0 and at 1 and both must leave the same
bits: the oracle's image with its ray and pixel counts where there is an oracle frame, and the same `pair_records` (a tally of the
wavefront pipeline alone)."""
import copy
import os
import sys

import numpy as np
import pytest

from conftest import default_camera

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
THREADS = min(16, os.cpu_count() or 1)
RAYS = ("rays_closest", "rays_shadow", "pixels")


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def scenes(cornell_flat):
    """name -> (flat scene, camera keywords, oracle, renderer): the Cornell box and the small textured atrium"""
    import atrium
    import oracle_py
    from vkrt_amd.renderer import Renderer

    small, _ = atrium.build_atrium(20000, seed=3, with_textures=True)
    out = {}
    for name, flat, camkw in (("cornell", cornell_flat, {}), ("atrium", small, atrium.DEFAULT_CAMERA)):
        out[name] = (flat, camkw, oracle_py.OracleScene(flat), Renderer(flat, device=0, build="ploc"))
    yield out
    for v in out.values():
        v[3].close()


def _both_paths(r, call):
    """call() with the option at 0 (records) and at 1 (pixel grid) -> [(image, counters)] in that order; the default (1) is restored"""
    from vkrt_amd import abi

    got = []
    for camera in (0, 1):
        r.set_option(abi.VKRT_OPT_WF_CAMERA_ROUNDS, camera)
        r.reset_counters()
        img = call().cpu().numpy()
        got.append((img, r.counters()))
    assert r.get_option(abi.VKRT_OPT_WF_CAMERA_ROUNDS) == 1
    return got


def _check_pair(got, ref, cref, what):
    for camera, (img, c) in enumerate(got):
        assert _same_bits(img, ref), (what, camera, float(np.mean(np.any(img.view(np.uint32) != ref.view(np.uint32), axis=-1))))
        assert c["traversal_faults"] == 0
        for k in RAYS:
            assert c[k] == cref[k], (what, camera, k, c[k], cref[k])
    assert got[0][1]["pair_records"] == got[1][1]["pair_records"], what


def _check_equal(got, what, keys=RAYS + ("pair_records", "traversal_faults")):
    assert _same_bits(got[0][0], got[1][0]), what
    for k in keys:
        assert got[0][1][k] == got[1][1][k], (what, k, got[0][1][k], got[1][1][k])


@pytest.mark.parametrize("size", [(75, 40), (64, 40)])
@pytest.mark.parametrize("scene", ["cornell", "atrium"])
def test_both_paths_match_the_oracle_bit_for_bit(scenes, scene, size):
    """Ragged and whole tiles x samples 1, 2, 3, 5 x depth 1, 3, 8 x frame 0 (no jitter) and frame 3 (jitter, blend into a kept image)."""
    import torch
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants

    flat, camkw, orc, r = scenes[scene]
    assert r.get_option(abi.VKRT_OPT_WF_CAMERA_ROUNDS) == 1 and r.get_option(abi.VKRT_OPT_WF_SAMPLE_SYNC) == 1  # the defaults
    W, H = size
    cam = default_camera(W, H, **camkw)
    lights = len(flat.lights)
    kept = np.random.default_rng(5).random((H, W, 4), dtype=np.float32)
    pairs = 0
    for samples in (1, 2, 3, 5):
        for depth in (1, 3, 8):
            for frame in (0, 3):
                pc = make_push_constants(samples=samples, depth=depth, frame=frame, lights_count=lights)
                ref, cref = orc.render(pc, cam, W, H, seed=11 + frame, image=kept.copy() if frame else None, threads=THREADS)
                got = _both_paths(r, lambda: r.pathtrace(pc, cam, W, H, seed=11 + frame, image=torch.from_numpy(kept).cuda() if frame else None))
                _check_pair(got, ref, cref, (samples, depth, frame))
                pairs += got[1][1]["pair_records"]
    assert pairs > 0  # (depth 3 and 8 move pair records)


def test_all_miss_camera_leaves_the_clear_colour(scenes):
    """A camera that looks away from the scene: every sample is one missed camera ray worth clearColor * 0.8 (raytrace.rmiss), which
    ends in the camera shade step itself (finishSegment writes the sample state, or stores the pixel); the image is the binary32
    mean of the samples."""
    from vkrt_amd.flat_scene import make_push_constants

    flat, _, orc, r = scenes["cornell"]
    W, H = 75, 40
    cam = default_camera(W, H, eye=(0, 0, 15), center=(0, 0, 30))
    clear = (0.25, 0.5, 0.7, 1.0)
    for samples in (1, 3, 5):
        pc = make_push_constants(samples=samples, depth=3, frame=0, lights_count=len(flat.lights), clear_color=clear)
        want = np.zeros(3, np.float32)
        for _ in range(samples):
            want = want + np.asarray(clear[:3], np.float32) * np.float32(0.8)
        want = want / np.float32(samples)
        for camera, (img, c) in enumerate(_both_paths(r, lambda: r.pathtrace(pc, cam, W, H, seed=2))):
            assert np.all(img[..., :3] == want) and np.all(img[..., 3] == 1.0), (samples, camera)
            assert (c["rays_closest"], c["rays_shadow"], c["pixels"], c["pair_records"]) == (W * H * samples, 0, W * H, 0), (samples, camera)


@pytest.mark.parametrize("world", [2, 3])
def test_shards_equal_the_whole_image(scenes, world):
    """16-row strips dealt to 2 and 3 shards (the last strip is ragged: 75 x 40): every shard's rows are those of the whole image."""
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.sharding import make_shard, shard_row_indices

    flat, camkw, orc, r = scenes["atrium"]
    W, H = 75, 40
    cam = default_camera(W, H, **camkw)
    pc = make_push_constants(samples=3, depth=3, frame=0, lights_count=len(flat.lights))
    ref, cref = orc.render(pc, cam, W, H, seed=4, threads=THREADS)
    total = [dict.fromkeys(RAYS + ("pair_records",), 0) for _ in range(2)]
    for rank in range(world):
        shard = make_shard(W, H, world, rank)
        rows = shard_row_indices(H, world, rank)
        for camera, (img, c) in enumerate(_both_paths(r, lambda: r.pathtrace(pc, cam, W, H, seed=4, shard=shard))):
            assert _same_bits(img, ref[rows]), (world, rank, camera)
            for k in total[camera]:
                total[camera][k] += c[k]
    assert total[0] == total[1]
    for k in RAYS:
        assert total[1][k] == cref[k], k


def test_subframes_equal_the_whole_frame(scenes):
    """A single-frame call of 256 x 128 (512 tiles: the call splits into two tile ranges, the second with tileFirst = 256) equals
    the same call on the caller's stream (VKRT_OPT_WF_SUBFRAMES 1)."""
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants

    flat, camkw, orc, r = scenes["atrium"]
    W, H = 256, 128
    cam = default_camera(W, H, **camkw)
    pc = make_push_constants(samples=3, depth=3, frame=0, lights_count=len(flat.lights))
    assert r.get_option(abi.VKRT_OPT_WF_SUBFRAMES) == 3
    sub = _both_paths(r, lambda: r.pathtrace(pc, cam, W, H, seed=9))
    r.set_option(abi.VKRT_OPT_WF_SUBFRAMES, 1)
    try:
        whole = _both_paths(r, lambda: r.pathtrace(pc, cam, W, H, seed=9))
    finally:
        r.set_option(abi.VKRT_OPT_WF_SUBFRAMES, 3)
    _check_equal(sub, "sub-framed")
    _check_equal(whole, "whole")
    _check_equal([sub[1], whole[1]], "sub-framed against whole")
    assert sub[1][1]["pixels"] == W * H and sub[1][1]["rays_closest"] >= 3 * W * H and np.any(sub[1][0][..., :3] > 0)


def test_frames_in_flight_equal_single_calls(scenes):
    """vkrt_pathtrace_frames of 4 frames at 64 x 40 (two turns of two lanes, staged pixels and the ordered blend) == four single calls."""
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants

    flat, camkw, orc, r = scenes["atrium"]
    W, H = 64, 40
    cam = default_camera(W, H, **camkw)
    lights = len(flat.lights)
    assert r.get_option(abi.VKRT_OPT_WF_FRAMES_IN_FLIGHT) == 3
    ref, want = None, dict.fromkeys(RAYS, 0)
    for f in range(4):
        ref, cref = orc.render(make_push_constants(samples=2, depth=3, frame=f, lights_count=lights), cam, W, H, seed=20 + f, image=ref, threads=THREADS)
        for k in RAYS:
            want[k] += cref[k]

    def singles():
        img = None
        for f in range(4):
            img = r.pathtrace(make_push_constants(samples=2, depth=3, frame=f, lights_count=lights), cam, W, H, seed=20 + f, image=img)
        return img

    pc = make_push_constants(samples=2, depth=3, frame=0, lights_count=lights)
    one = _both_paths(r, singles)
    call = _both_paths(r, lambda: r.pathtrace_frames(pc, cam, W, H, 4, seed=20))
    _check_pair(one, ref, want, "four single calls")
    _check_pair(call, ref, want, "one call of four frames")
    assert len({c["pair_records"] for _, c in one + call}) == 1


def test_dissolve_stage_sees_the_same_seed(cornell_flat):
    """VKRT_OPT_ANYHIT_DISSOLVE with translucent and invisible materials: the any-hit decision of a camera ray draws from the payload's
    seed when the ray is traced -- the seed after the sample's two jitter draws, which the record path keeps in S0.w and the camera
    kernel takes from startSample.  Both paths leave the same bits (tests/test_gpu_parity.py holds the record path to the oracle), and
    the stage is on: the frame differs from the oracle's opaque one in many pixels."""
    import oracle_py
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Renderer

    flat = copy.deepcopy(cornell_flat)
    for m, a in {1: 0.5, 3: 0.25, 4: 0.0, 6: 0.9}.items():
        flat.materials["pbrBaseColorFactor"][m, 3] = a
    W, H = 75, 40
    cam = default_camera(W, H)
    r = Renderer(flat, device=0, build="ploc", options={abi.VKRT_OPT_ANYHIT_DISSOLVE: 1})
    orc = oracle_py.OracleScene(flat)
    orc.set_dissolve(True)
    try:
        for frame in (0, 2):
            pc = make_push_constants(samples=3, depth=4, frame=frame, lights_count=1)
            got = _both_paths(r, lambda: r.pathtrace(pc, cam, W, H, seed=70 + frame))
            _check_equal(got, ("dissolve", frame))
        orc.set_dissolve(False)
        opaque, _ = orc.render(pc, cam, W, H, seed=70 + frame, threads=THREADS)
        assert np.mean(np.any(got[1][0].view(np.uint32) != opaque.view(np.uint32), axis=-1)) > 0.05  # the stage is on
    finally:
        r.close()


@pytest.mark.parametrize("options", [{2: 0}, {4: 256}, {5: 0}], ids=["bvh2", "trav-block-256", "sharing-off"])
def test_fallbacks_give_the_record_path(scenes, options):
    """Where the sharing wave of the camera kernel does not run -- BVH2 nodes (VKRT_OPT_BVH_LAYOUT 0), traversal workgroups of 256
    (VKRT_OPT_WF_TRAV_BLOCK), sharing off (VKRT_OPT_WF_SHARE 0) -- the option resolves to the record path: the same image and counts."""
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Renderer

    assert (abi.VKRT_OPT_BVH_LAYOUT, abi.VKRT_OPT_WF_TRAV_BLOCK, abi.VKRT_OPT_WF_SHARE) == (2, 4, 5)
    flat, camkw, orc, _ = scenes["atrium"]
    W, H = 75, 40
    cam = default_camera(W, H, **camkw)
    pc = make_push_constants(samples=3, depth=3, frame=0, lights_count=len(flat.lights))
    ref, cref = orc.render(pc, cam, W, H, seed=4, threads=THREADS)
    r = Renderer(flat, device=0, build="ploc", options=options)
    try:
        assert r.get_option(abi.VKRT_OPT_WF_CAMERA_ROUNDS) == 1
        _check_pair(_both_paths(r, lambda: r.pathtrace(pc, cam, W, H, seed=4)), ref, cref, options)
    finally:
        r.close()


def test_counted_launch_tallies_the_same_work(scenes):
    """VKRT_TRACE_COUNT_TRAVERSAL.  Hits, lobes and texture taps are properties of the paths: equal on any frame (75 x 40, ragged
    tiles).  nodes_visited, tris_tested and the wave-step counters also depend on which rays share a wave: on 16 x 16 at depth 1 that
    is fixed on both paths -- four whole tiles, so a camera wave is a tile whether its rays come from records or from the grid, and
    the one shade workgroup compacts the shadow rays in one order -- and there they are equal too."""
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants

    for scene in ("cornell", "atrium"):
        flat, camkw, orc, r = scenes[scene]
        lights = len(flat.lights)
        W, H = 75, 40
        pc = make_push_constants(samples=3, depth=3, frame=0, lights_count=lights)
        got = _both_paths(r, lambda: r.pathtrace(pc, default_camera(W, H, **camkw), W, H, seed=5, flags=abi.VKRT_TRACE_COUNT_TRAVERSAL))
        _check_equal(got, (scene, "ragged"), RAYS + ("pair_records", "traversal_faults", "hits", "diffuse_hits", "tex_taps"))
        assert got[1][1]["hits"] > 0 and got[1][1]["nodes_visited"] > 0
        W = H = 16
        pc = make_push_constants(samples=3, depth=1, frame=0, lights_count=lights)
        got = _both_paths(r, lambda: r.pathtrace(pc, default_camera(W, H, **camkw), W, H, seed=5, flags=abi.VKRT_TRACE_COUNT_TRAVERSAL))
        print(scene, [c for _, c in got])
        _check_equal(got, (scene, "one workgroup"), RAYS + ("pair_records", "traversal_faults", "hits", "diffuse_hits", "tex_taps", "nodes_visited",
                                                            "tris_tested", "wave_node_steps", "wave_tri_steps"))
        assert got[1][1]["nodes_visited"] > 0 and got[1][1]["wave_node_steps"] > 0
