"""The scenes of the scene-edit tests (test_scene_edit_pack.py, test_gpu_scene_edit.py): lod_scene() of test_texture_lod.py -- 1x1, 8x2,
5x3, 37x21, 64x64 linear and 128x32 sRGB textures -- with a 256x256 sRGB noise texture appended and bound (base), and the target every
test edits towards: every image replaced, material slots permuted and factors changed, both lights changed."""
import copy

import numpy as np

from test_texture_lod import lod_scene

NOISE = 6  # the appended texture
SLOTS = ("pbrBaseColorTexture", "metallicRoughnessTexture", "normalTexture", "emissiveTexture")


def base_scene():
    flat = lod_scene()
    rng = np.random.default_rng(23)
    flat.textures.append({"rgba8": rng.integers(0, 256, (256, 256, 4), dtype=np.uint8), "is_srgb": True})
    flat.materials[2]["emissiveTexture"] = NOISE
    flat.materials[1]["pbrBaseColorTexture"] = NOISE  # the second floor strip: in view at every LOD
    return flat


def target_images(flat, seed=71):
    """new texels for every texture of `flat`, same sizes"""
    rng = np.random.default_rng(seed)
    out = []
    for t in flat.textures:
        h, w = t["rgba8"].shape[:2]
        img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        if w >= 32:  # stripes, so that minification changes the colour
            img[:, (np.arange(w) // 3) % 2 == 0, :3] //= 3
        out.append(np.ascontiguousarray(img))
    return out


def target_scene(flat=None):
    """scene B: what scene A must equal after its lights, materials and textures were updated"""
    b = copy.deepcopy(flat or base_scene())
    for t, img in zip(b.textures, target_images(b)):
        t["rgba8"] = img
    slots = [(5, 2, NOISE, 0), (3, NOISE, 1, -1), (NOISE, -1, 4, 5), (2, 0, -1, 1)]  # base, metallicRoughness, normal, emissive
    for k, row in enumerate(slots):
        for name, ti in zip(SLOTS, row):
            b.materials[k][name] = ti
        b.materials[k]["pbrBaseColorFactor"] = [0.9 - 0.1 * k, 0.7, 0.6 + 0.1 * k, 1.0]
        b.materials[k]["metallicFactor"], b.materials[k]["roughnessFactor"] = 0.2 + 0.2 * k, 0.95 - 0.2 * k
        b.materials[k]["emissiveFactor"] = [0.05 * k, 0.25, 0.4 - 0.1 * k]
    b.lights[0] = ((-1.5, 3.0, -6.0), (0.9, 1.0, 0.7), 55.0, 0)
    b.lights[1] = ((-0.2, 1.0, 0.4), (0.8, 0.8, 1.0), 2.5, 1)
    return b
