"""Deformations of a scene's emissive triangles for the light-rebuild tests: every emissive triangle is scaled about its own
centroid by 10 ** uniform(-1, 1), the two largest by 0.1 instead, so that areas (hence light powers, the alias table and
sumLightPowerInv) change while the triangle count, materials and normals stay."""
import numpy as np


def deformed_vertices(sd, step):
    v = sd.vertices.reshape(-1, 3, 3).astype(np.float64)
    ids = np.asarray(sd.light_prim_ids)
    rng = np.random.default_rng(5 + step)
    scale = 10.0 ** rng.uniform(-1, 1, len(ids))
    tri = v[ids]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    scale[np.argsort(area, kind="stable")[-2:]] = 0.1
    ctr = tri.mean(axis=1, keepdims=True)
    v[ids] = ctr + (tri - ctr) * scale[:, None, None]
    return v.astype(np.float32).reshape(-1, 3)


def deformed_scene(sd, step):
    from radish_pt_amd import scenes

    return scenes.SceneData(f"{sd.name}_deformed{step}", deformed_vertices(sd, step), sd.normals, sd.texcoords, sd.material_ids,
                            sd.materials, sd.textures, sd.env_map_tex_id)


def light_powers(sd, vertices):
    """The power array the light sampler is built over: the emissive triangles', then the environment map's if there is one."""
    from radish_pt_amd import hostlib

    _, _, power = hostlib.build_light_list(vertices, sd.material_ids, sd.materials)
    if sd.env_map_tex_id >= 0:
        power = np.concatenate([power, np.array([sd.env_power], np.float32)]).astype(np.float32)
    return power
