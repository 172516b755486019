"""Scenes and material edits of the material-edit tests (test_material_edit_cpu.py, test_gpu_material_edit.py).

`edited(sd, ids, mats)` is the reference of every comparison: a new SceneData with the listed materials replaced, whose constructor
runs the host's build_light_list / build_alias_table on the edited description.

An edit is a list of steps, each (ids, materials) as Context.set_materials takes them; the steps are applied in order and the
scene is compared after the last one."""
import functools

import numpy as np


@functools.lru_cache(maxsize=None)
def teapots():
    """16 stand-ins of 864 triangles and a grid of 128 emissive quads, each with a Light material of its own: 14 092 triangles.
    The ceiling light is triangles 10-11 (block 0), the quads are triangles 13 836 - 14 091 (blocks 54 and 55)."""
    from radish_pt_amd import scenes

    return scenes.teapots(segments=24, bands=18, emissive_grid=(8, 16))


@functools.lru_cache(maxsize=None)
def cornell():
    from radish_pt_amd import scenes

    return scenes.cornell_textured(env=True)


SCENES = {"teapots": teapots, "cornell": cornell}


def edited(sd, ids, mats, name=None):
    from radish_pt_amd import scenes

    m = sd.materials.copy()
    m[np.asarray(ids, dtype=np.int64)] = np.asarray(mats, dtype=m.dtype)
    return scenes.SceneData(name or f"{sd.name}_edited", sd.vertices, sd.normals, sd.texcoords, sd.material_ids, m, sd.textures,
                            sd.env_map_tex_id)


def apply_steps(sd, steps):
    """The scene after every step of an edit (cached per edit by the callers)."""
    for ids, mats in steps:
        sd = edited(sd, ids, mats)
    return sd


def _with(sd, ids, **fields):
    from radish_pt_amd import layouts as L

    ids = np.asarray(ids, dtype=np.int32).reshape(-1)
    mats = sd.materials[ids].copy()
    for k, v in fields.items():
        if callable(v):
            mats[k] = v(mats[k])
        else:
            mats[k] = v
    assert mats.dtype == L.MATERIAL_DTYPE
    return ids, mats


def light_ids(sd):
    from radish_pt_amd import layouts as L

    return np.flatnonzero(sd.materials["type"] == L.LIGHT).astype(np.int32)


def half_of_the_lights(sd):
    """Every Light material but those at positions 1 and 2 of each four (in material order): on teapots() that keeps the quads on
    either side of each 64-triangle boundary lit.  A scene with one Light material gives that one."""
    ids = light_ids(sd)
    if len(ids) == 1:
        return ids
    quads = ids[1:] if sd.name.startswith("teapots") else ids  # teapots: the ceiling light stays on
    k = np.arange(len(quads))
    return quads[(k % 4 == 0) | (k % 4 == 3)]


# material ids of the two scenes: a visible Lambertian, the lamp, a non-emissive material with many triangles, and a texture-map change
PICKS = {
    "teapots": {"lambert": 4, "lamp": 3, "many": 9, "maps": (0, {"baseColorMapId": -2})},
    "cornell": {"lambert": 4, "lamp": 5, "many": 7, "maps": ((1, 6), {"baseColorMapId": -2, "normalMapId": -1})},
}

# edits after which the light list differs from the uploaded one in length and placement (test_material_edit_cpu.py checks teapots')
LIST_EDITS = ("half_off", "grow")
EDITS = ("recolour", "to_metal", "to_glass", "lamp_x4", "half_off", "back_on", "grow", "no_lights", "maps")


def steps(scene, edit):
    from radish_pt_amd import layouts as L

    sd, pick = SCENES[scene](), PICKS[scene]
    dark = dict(type=L.LAMBERTIAN, baseColor=(0.5, 0.4, 0.3))
    if edit == "recolour":
        return [_with(sd, pick["lambert"], baseColor=(0.2, 0.3, 0.9))]
    if edit == "to_metal":
        return [_with(sd, pick["lambert"], type=L.METALLIC_WORKFLOW, metallic=1.0, roughness=0.25)]
    if edit == "to_glass":  # Lambertian -> MetallicWorkflow -> Dielectric
        return steps(scene, "to_metal") + [_with(sd, pick["lambert"], type=L.DIELECTRIC, ior=1.5, baseColor=(1.0, 1.0, 1.0))]
    if edit == "lamp_x4":
        return [_with(sd, pick["lamp"], baseColor=lambda c: c * np.float32(4))]
    if edit == "half_off":
        return [_with(sd, half_of_the_lights(sd), **dark)]
    if edit == "back_on":
        ids = half_of_the_lights(sd)
        return steps(scene, "half_off") + [(ids, sd.materials[ids].copy())]
    if edit == "grow":
        return [_with(sd, pick["many"], type=L.LIGHT, baseColor=(3.0, 2.5, 2.0))]
    if edit == "no_lights":
        return [_with(sd, light_ids(sd), **dark)]
    if edit == "maps":
        ids, fields = pick["maps"]
        return [_with(sd, ids, **fields)]
    raise KeyError(edit)


@functools.lru_cache(maxsize=None)
def result(scene, edit):
    """The SceneData after the edit: the reference."""
    return apply_steps(SCENES[scene](), steps(scene, edit))


# ---- the three passes of kernels_materials.h restated ----------------------------------------------------------------------------
def compaction_model(emits, block=256):
    """emits: bool [numPrims] -> the ordered list of set positions, by block totals, their exclusive scan and a scatter at
    offset + rank in the block (rank = waves before + lanes before in the 64-lane wave)."""
    emits = np.asarray(emits, dtype=bool)
    n = len(emits)
    blocks = (n + block - 1) // block
    padded = np.zeros(blocks * block, dtype=bool)
    padded[:n] = emits
    per_block = padded.reshape(blocks, block)
    totals = per_block.sum(axis=1).astype(np.int64)                       # pass 1
    offsets = np.concatenate([[0], np.cumsum(totals)[:-1]]).astype(np.int64) if blocks else np.zeros(0, np.int64)  # pass 2
    total = int(totals.sum())
    out = np.full(total, -1, np.int32)
    waves = per_block.reshape(blocks, block // 64, 64)
    wave_totals = waves.sum(axis=2)
    for b in range(blocks):                                                # pass 3
        for w in range(block // 64):
            lanes = np.flatnonzero(waves[b, w])
            if len(lanes) == 0:
                continue
            rank = np.arange(len(lanes)) + wave_totals[b, :w].sum()       # lanes before + waves before
            out[offsets[b] + rank] = b * block + w * 64 + lanes
    return out, total
