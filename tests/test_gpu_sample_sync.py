"""VKRT_OPT_WF_SAMPLE_SYNC: the sample-synchronous schedule of the wavefront path tracer (all pixels of a frame trace sample s
before any starts sample s + 1; csrc/wavefront.hip k_wf_sample_init) and the schedule it replaces as the default (option 0: a
pixel starts its next sample in the round its sample ends) trace the same paths with the same draws and float operations.  So
both must leave the oracle's image bit for bit, with the oracle's ray and pixel counts; `pair_records` is a tally of the
wavefront pipeline alone (the oracle has no records), so it is compared between the two schedules."""
import hashlib
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


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


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


def _both_schedules(r, call):
    """call() under option 0 and option 1 -> [(image, counters)] in that order; the default (1) is restored"""
    from vkrt_amd import abi

    got = []
    for sync in (0, 1):
        r.set_option(abi.VKRT_OPT_WF_SAMPLE_SYNC, sync)
        r.reset_counters()
        img = call().cpu().numpy()
        got.append((img, r.counters()))
    assert r.get_option(abi.VKRT_OPT_WF_SAMPLE_SYNC) == 1
    return got


def _check_pair(got, ref, cref, what):
    for sync, (img, c) in enumerate(got):
        assert _same_bits(img, ref), (what, sync, float(np.mean(np.any(img.view(np.uint32) != ref.view(np.uint32), axis=-1))))
        assert c["traversal_faults"] == 0
        for k in RAYS:
            assert c[k] == cref[k], (what, sync, k, c[k], cref[k])
    assert got[0][1]["pair_records"] == got[1][1]["pair_records"], what


@pytest.mark.parametrize("size", [(75, 40), (64, 40)])
@pytest.mark.parametrize("scene", ["cornell", "atrium"])
def test_both_schedules_match_the_oracle_bit_for_bit(scenes, scene, size):
    """Ragged and whole tiles x samples 1 (no sample init at all), 2, 3, 5 x depth 1, 3, 8 x frame 0 (no jitter) and frame 3 (jitter,
    blend into a kept image)."""
    import torch
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants

    flat, camkw, orc, r = scenes[scene]
    assert r.get_option(abi.VKRT_OPT_WF_SAMPLE_SYNC) == 1  # the default
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
                got = _both_schedules(r, lambda: r.pathtrace(pc, cam, W, H, seed=11 + frame, image=torch.from_numpy(kept).cuda() if frame else None))
                _check_pair(got, ref, cref, (samples, depth, frame))
                pairs += got[1][1]["pair_records"]
    assert pairs > 0  # (depth 3 and 8 move pair records)


def test_all_miss_camera_leaves_the_clear_colour(scenes):
    """A camera that looks away from the scene: every sample is one missed camera ray worth clearColor * 0.8 (raytrace.rmiss), so a
    pixel goes through sample end and sample init `samples - 1` times and nothing else; the image is the binary32 mean of the samples."""
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
        for sync, (img, c) in enumerate(_both_schedules(r, lambda: r.pathtrace(pc, cam, W, H, seed=2))):
            assert np.all(img[..., :3] == want) and np.all(img[..., 3] == 1.0), (samples, sync)
            assert (c["rays_closest"], c["rays_shadow"], c["pixels"], c["pair_records"]) == (W * H * samples, 0, W * H, 0), (samples, sync)


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
        for sync, (img, c) in enumerate(_both_schedules(r, lambda: r.pathtrace(pc, cam, W, H, seed=4, shard=shard))):
            assert _same_bits(img, ref[rows]), (world, rank, sync)
            for k in total[sync]:
                total[sync][k] += c[k]
    assert total[0] == total[1]
    for k in RAYS:
        assert total[1][k] == cref[k], k


def test_frames_in_flight_and_subframes(scenes):
    """vkrt_pathtrace_frames(4) with the option at three frames in flight (the dealer balances four frames to two turns of two lanes)
    and vkrt_pathtrace_frames(6) (two turns of three lanes) == as many single calls (hash and counters), and a single-frame call
    split into sub-frames (1000 tiles: three tile ranges), all against oracle frames rendered one by one."""
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants

    flat, camkw, orc, r = scenes["atrium"]
    W, H = 316, 200  # 40 x 25 tiles, ragged in x
    cam = default_camera(W, H, **camkw)
    lights = len(flat.lights)
    assert r.get_option(abi.VKRT_OPT_WF_FRAMES_IN_FLIGHT) == 3 and r.get_option(abi.VKRT_OPT_WF_SUBFRAMES) == 3
    ref, want = None, dict.fromkeys(RAYS, 0)
    for f in range(6):
        ref, cref = orc.render(make_push_constants(samples=2, depth=3, frame=f, lights_count=lights), cam, W, H, seed=20 + f, image=ref, threads=THREADS)
        if f == 0:
            ref0, cref0 = ref.copy(), cref
        for k in RAYS:
            want[k] += cref[k]
        if f == 3:
            ref4, want4 = ref.copy(), dict(want)
    pc = make_push_constants(samples=2, depth=3, frame=0, lights_count=lights)

    def singles(n=4):
        img = None
        for f in range(n):
            img = r.pathtrace(make_push_constants(samples=2, depth=3, frame=f, lights_count=lights), cam, W, H, seed=20 + f, image=img)
        return img

    one = _both_schedules(r, singles)  # (each single call is sub-framed)
    call = _both_schedules(r, lambda: r.pathtrace_frames(pc, cam, W, H, 4, seed=20))
    _check_pair(one, ref4, want4, "four single calls")
    _check_pair(call, ref4, want4, "one call of four frames")
    assert len({_sha(img) for img, _ in one + call}) == 1
    assert len({c["pair_records"] for _, c in one + call}) == 1
    one6 = _both_schedules(r, lambda: singles(6))
    call6 = _both_schedules(r, lambda: r.pathtrace_frames(pc, cam, W, H, 6, seed=20))  # three lanes, each with its sample inits
    _check_pair(one6, ref, want, "six single calls")
    _check_pair(call6, ref, want, "one call of six frames")
    assert len({_sha(img) for img, _ in one6 + call6}) == 1
    assert len({c["pair_records"] for _, c in one6 + call6}) == 1
    sub = _both_schedules(r, lambda: r.pathtrace(pc, cam, W, H, seed=20))
    _check_pair(sub, ref0, cref0, "one sub-framed frame")
    r.set_option(abi.VKRT_OPT_WF_SUBFRAMES, 1)
    whole = _both_schedules(r, lambda: r.pathtrace(pc, cam, W, H, seed=20))
    r.set_option(abi.VKRT_OPT_WF_SUBFRAMES, 3)
    _check_pair(whole, ref0, cref0, "one frame on the caller's stream")
    assert whole[1][1]["pair_records"] == sub[1][1]["pair_records"]


def test_hybrid_and_megakernel_frames_do_not_depend_on_the_option(scenes):
    """The hybrid GI path (one sample, its own shade instantiation) and the megakernel (no streams) have no sample init: the same
    frame with the option at either value."""
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Renderer

    flat, camkw, orc, r = scenes["atrium"]
    W, H = 75, 40
    cam = default_camera(W, H, **camkw)
    lights = len(flat.lights)
    g = r.gbuffer_raycast(cam, W, H)
    pc = make_push_constants(samples=1, depth=4, frame=0, lights_count=lights)
    pc.useShadows, pc.useAO, pc.useGI = 1, 1, 1
    hy = _both_schedules(r, lambda: r.hybrid_trace(pc, cam, W, H, g, seed=6))
    assert _same_bits(hy[0][0], hy[1][0]) and hy[0][1]["rays_closest"] == hy[1][1]["rays_closest"] > 0
    assert np.any(hy[1][0][..., :3] > 0)
    pm = make_push_constants(samples=3, depth=3, frame=0, lights_count=lights)
    ref, cref = orc.render(pm, cam, W, H, seed=6, threads=THREADS)
    mega = Renderer(flat, device=0, build="sah", options={abi.VKRT_OPT_MODE: 0})
    got = _both_schedules(mega, lambda: mega.pathtrace(pm, cam, W, H, seed=6))
    mega.close()
    assert _same_bits(got[0][0], got[1][0]) and _same_bits(got[1][0], ref)
    for k in RAYS:
        assert got[0][1][k] == got[1][1][k] == cref[k], k
