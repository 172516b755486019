"""Scenes and triangle-set edits of the geometry-edit tests (test_geometry_edit_cpu.py, test_gpu_geometry_edit.py).

Every edit is a SceneData with the materials, textures and environment map of the scene it starts from and another triangle set;
its constructor runs the host's build_bvh / build_light_list / build_alias_table, so it is the reference of every comparison.

  remove    stand-ins dropped (teapots: 3, 7 and 12) and every other emissive quad (cornell: one of the lamp's two triangles)
  add       two more stand-ins at the end, one carrying a Light material id: past the uploaded triangle and light capacities
  reassign  the same triangles; one stand-in gets a Light id, one lamp quad a Lambertian id
  reorder   a fixed permutation of the triangles that also changes the emitters' order
  one_light a single triangle, emissive: the root is a leaf
  one_dark  a single triangle that is no emitter: no light left (teapots: length 0; cornell: the environment map alone, length 1)
  back      the original arrays"""
import functools

import numpy as np

import material_edit

EDITS = ("remove", "add", "reassign", "reorder", "one_light", "one_dark", "back")
SCENES = material_edit.SCENES

# per scene: the stand-ins' triangle ranges, the emissive quads' (two triangles each), and the ids the edits hand out
LAYOUT = {
    "teapots": {"standins": [(12 + 864 * k, 864) for k in range(16)], "quads": [(10, 2)] + [(13836 + 2 * q, 2) for q in range(128)],
                "drop": (3, 7, 12), "light_id": 3, "lambert_id": 0, "relit": 5, "unlit_quad": 1},
    "cornell": {"standins": [(12, 384), (396, 384)], "quads": [(10, 2)],
                "drop": (1,), "light_id": 5, "lambert_id": 4, "relit": 0, "unlit_quad": 0},
}


def _scene(sd, name, keep=None, extra=None, ids=None):
    """sd's triangles `keep` (index array; None: all), then the triangles of `extra` = (vertices, normals, texcoords, ids)."""
    from radish_pt_amd import scenes

    n = sd.num_prims
    keep = np.arange(n) if keep is None else np.asarray(keep, dtype=np.int64)
    v = sd.vertices.reshape(n, 9)[keep]
    nr = sd.normals.reshape(n, 9)[keep]
    t = sd.texcoords.reshape(n, 6)[keep]
    m = (sd.material_ids if ids is None else ids)[keep]
    if extra is not None:
        v, nr, t, m = (np.concatenate([a, b]) for a, b in zip((v, nr, t, m), extra))
    return scenes.SceneData(f"{sd.name}_{name}", v.reshape(-1, 3), nr.reshape(-1, 3), t.reshape(-1, 2), m.astype(np.int32), sd.materials,
                            sd.textures, sd.env_map_tex_id)


@functools.lru_cache(maxsize=None)
def result(scene, edit):
    sd, lay = SCENES[scene](), LAYOUT[scene]
    n = sd.num_prims
    if edit == "back":
        return sd
    if edit == "remove":
        gone = np.zeros(n, bool)
        for k in lay["drop"]:
            first, count = lay["standins"][k]
            gone[first:first + count] = True
        quads = lay["quads"]
        if len(quads) > 1:
            for first, count in quads[1::2]:
                gone[first:first + count] = True
        else:
            gone[quads[0][0] + 1] = True
        return _scene(sd, edit, np.flatnonzero(~gone))
    if edit == "add":
        parts = []
        for j, (k, mat, shift) in enumerate(((0, lay["light_id"], (0.35, 0.9, 0.2)), (1, None, (-0.3, 1.0, -0.25)))):
            first, count = lay["standins"][k]
            sl = slice(first, first + count)
            v = sd.vertices.reshape(n, 3, 3)[sl] + np.asarray(shift, np.float32)
            ids = np.full(count, mat, np.int32) if mat is not None else sd.material_ids[sl]
            parts.append((v.reshape(count, 9).astype(np.float32), sd.normals.reshape(n, 9)[sl], sd.texcoords.reshape(n, 6)[sl], ids))
        return _scene(sd, edit, extra=tuple(np.concatenate(a) for a in zip(*parts)))
    if edit == "reassign":
        ids = sd.material_ids.copy()
        first, count = lay["standins"][lay["relit"]]
        ids[first:first + count] = lay["light_id"]
        first, count = lay["quads"][lay["unlit_quad"]]
        ids[first:first + count] = lay["lambert_id"]
        return _scene(sd, edit, ids=ids)
    if edit == "reorder":
        perm = np.random.default_rng(20).permutation(n)
        lit = np.isin(perm, sd.light_prim_ids)
        if np.all(np.diff(perm[lit]) > 0):  # the emitters must change their order too, or the light list (and every frame) stays
            perm = perm[::-1]
        return _scene(sd, edit, perm)
    if edit == "one_light":
        return _scene(sd, edit, [lay["quads"][0][0]])
    if edit == "one_dark":
        return _scene(sd, edit, [0])
    raise KeyError(edit)


def arrays(sd):
    """(vertices, normals, texcoords, material_ids) as Context.set_geometry takes them, still on the host."""
    return sd.vertices.reshape(-1), sd.normals.reshape(-1), sd.texcoords.reshape(-1), sd.material_ids
