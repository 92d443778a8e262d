"""The hit shader forms a texture tap only where some lane of the wave wants it (csrc/shade.h closestHitFront: a wave-uniform test in
front of footprint, loads and blend of each of the four taps), takes the one-record path of the footprint pool without forming the
other three texel indices, and stores a shadow record through one call per stream.  None of this may change a bit: one small frame
pair through vkrt_pathtrace_frames per material set, with the footprint pool and without it (VKRT_TEX_QUADS=0), against the oracle --
image bits, ray counters and the texture() tally.  The material sets make both sides of every wave-uniform branch occur: at 64 x 48
a camera wave is an 8 x 8 tile of the small atrium, and the bounce rounds mix hits of all materials in a wave."""
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
W, H, SAMPLES, DEPTH, FRAMES, SEED = 64, 48, 2, 3, 2, 61
COUNTED = ("rays_closest", "rays_shadow", "pixels", "hits", "diffuse_hits", "tex_taps")
TEXTURE_KEYS = ("pbrBaseColorTexture", "metallicRoughnessTexture", "normalTexture", "emissiveTexture")


def _all_four(flat):
    """every second material has all four textures (an emissive one too), the others none: a tile inside one surface wants all taps
    or none of them, a tile across two surfaces wants them in some lanes"""
    m = flat.materials
    for k in TEXTURE_KEYS:
        m[k][:] = -1
    for i in range(0, len(m), 2):
        m["pbrBaseColorTexture"][i], m["metallicRoughnessTexture"][i] = i % 4, 4 + (i // 2) % 2
        m["normalTexture"][i], m["emissiveTexture"][i] = 6 + (i // 4) % 2, (i // 2) % 4
        m["emissiveFactor"][i] = (0.6, 0.4, 0.3)


def _none(flat):
    for k in TEXTURE_KEYS:
        flat.materials[k][:] = -1


def _emissive_only(flat):
    """emissive textures and no others, on dielectrics and on mirror-like metals: the texture() tally then counts emissive taps alone,
    wanted at depth 0 and after a specular bounce only (raytrace.rchit:83)"""
    m = flat.materials
    for k in TEXTURE_KEYS:
        m[k][:] = -1
    for i in (0, 3, 5, 12, 13, 16, 21):
        m["emissiveTexture"][i] = i % 4
        m["emissiveFactor"][i] = (0.9, 0.55 + 0.02 * i, 0.2 + 0.03 * i)


def _npot(flat):
    """textures 1 (base colour) and 4 (metallic-roughness) become 60 x 37 and 100 x 3: the REPEAT wrap takes its remainder path in the
    lanes that tap them and the mask path in their neighbours"""
    flat.textures[1] = dict(flat.textures[1], rgba8=np.ascontiguousarray(flat.textures[1]["rgba8"][:37, :60]))
    flat.textures[4] = dict(flat.textures[4], rgba8=np.ascontiguousarray(flat.textures[4]["rgba8"][:3, :100]))


CASES = {"all_four": _all_four, "none": _none, "emissive": _emissive_only, "npot": _npot}


@pytest.fixture(scope="module")
def atrium_small():
    import atrium

    flat, _ = atrium.build_atrium(20000, seed=3, with_textures=True)
    return flat, atrium.DEFAULT_CAMERA


@pytest.fixture(scope="module")
def references(atrium_small):
    """case -> (scene, camera, oracle image after FRAMES frames, summed oracle counters), computed once per case"""
    import oracle_py
    from vkrt_amd.flat_scene import make_push_constants

    cache = {}

    def get(case):
        if case not in cache:
            base, camkw = atrium_small
            flat = copy.deepcopy(base)
            CASES[case](flat)
            cam = default_camera(W, H, **camkw)
            orc = oracle_py.OracleScene(flat)
            ref, total = None, dict.fromkeys(COUNTED, 0)
            for f in range(FRAMES):
                pc = make_push_constants(samples=SAMPLES, depth=DEPTH, frame=f, lights_count=len(flat.lights))
                ref, c = orc.render(pc, cam, W, H, seed=SEED + f, image=ref, threads=THREADS)
                for k in COUNTED:
                    total[k] += c[k]
            cache[case] = (flat, cam, orc, ref, total)
        return cache[case]

    return get


@pytest.mark.parametrize("quads", [1, 0], ids=["pool", "texels"])
@pytest.mark.parametrize("case", list(CASES))
def test_frames_match_the_oracle_bit_for_bit(references, monkeypatch, case, quads):
    from vkrt_amd import abi
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Renderer

    flat, cam, _, ref, total = references(case)
    monkeypatch.setenv("VKRT_TEX_QUADS", str(quads))  # read when the scene is created
    r = Renderer(flat, device=0, build="ploc")
    try:
        pc = make_push_constants(samples=SAMPLES, depth=DEPTH, frame=0, lights_count=len(flat.lights))
        r.reset_counters()
        img = r.pathtrace_frames(pc, cam, W, H, FRAMES, seed=SEED, flags=abi.VKRT_TRACE_COUNT_TRAVERSAL).cpu().numpy()
        c = r.counters()
    finally:
        r.close()
    diff = np.any(img.view(np.uint32) != ref.view(np.uint32), axis=-1)
    print(case, quads, "pixels differing", int(diff.sum()), {k: (c[k], total[k]) for k in COUNTED})
    assert not diff.any(), (case, quads, int(diff.sum()))
    assert c["traversal_faults"] == 0
    for k in COUNTED:
        assert c[k] == total[k], (case, quads, k, c[k], total[k])
    if case == "none":
        assert total["tex_taps"] == 0
    else:
        assert total["tex_taps"] > 0


def test_emissive_taps_occur_at_depth_0_and_after_specular_bounces_only(references):
    """What the `emissive` case rests on, from the oracle alone: its tally counts emissive taps only; a depth-1 frame has the camera hits'
    taps, the depth-3 frame has more (hits behind a specular bounce) but fewer than one per hit of a bounce round (the others are
    the lanes that do not want the tap)."""
    from vkrt_amd.flat_scene import make_push_constants

    flat, cam, orc, _, _ = references("emissive")
    taps = {}
    for depth in (1, DEPTH):
        pc = make_push_constants(samples=SAMPLES, depth=depth, frame=0, lights_count=len(flat.lights))
        taps[depth] = orc.render(pc, cam, W, H, seed=SEED, threads=THREADS)[1]
    first, full = taps[1], taps[DEPTH]
    assert 0 < first["tex_taps"] < first["hits"]  # some camera hits lie on emissive-textured materials, some do not
    assert first["tex_taps"] < full["tex_taps"] < first["tex_taps"] + (full["hits"] - first["hits"])


def test_hybrid_frame_matches_the_oracle_bit_for_bit(references):
    """k_wf_shade_hybrid shares the hit shader: the GI pass of one frame at the same size on the all-four material set."""
    from vkrt_amd.flat_scene import make_push_constants
    from vkrt_amd.renderer import Renderer

    flat, cam, orc, _, _ = references("all_four")
    r = Renderer(flat, device=0, build="ploc")
    try:
        g = r.gbuffer_raycast(cam, W, H)
        gnp = {k: v.cpu().numpy() for k, v in g.items()}
        pc = make_push_constants(samples=1, depth=DEPTH, frame=0, lights_count=len(flat.lights))
        pc.useShadows, pc.useAO, pc.useGI = 1, 1, 1
        out = r.hybrid_trace(pc, cam, W, H, g, seed=SEED).cpu().numpy()
    finally:
        r.close()
    ref, _ = orc.hybrid(pc, cam, W, H, gnp, seed=SEED, threads=THREADS)
    diff = np.any(out.view(np.uint32) != ref.view(np.uint32), axis=-1)
    print("hybrid pixels differing", int(diff.sum()))
    assert not diff.any(), int(diff.sum())
