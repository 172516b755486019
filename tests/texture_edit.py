"""Environment maps, texture edits and the numpy float32 model of the texture-edit tests (test_texture_edit_cpu.py,
test_gpu_texture_edit.py).

The model restates what rdh_scene_set_texture derives from an environment map's texels: the pixel weights
luminance * rowSin[row] with rdh_build_envmap_pdf's operations (rowSin from the host's expression, evaluated with the C
library's sinf, as the call does), then alias_model.sweep.  `with_textures(sd, {id: texels})` is the reference of every GPU
comparison: a new SceneData with the listed textures replaced, whose constructor runs the host's build_envmap_sampler and
build_alias_table on the edited description."""
import ctypes
import ctypes.util
import functools

import numpy as np

import alias_model

F = np.float32
PI_F = F(3.1415926535897932384626422832795028841971)

# (width, height): one pixel; odd sizes below a wave; one row of exactly a wave; a wave and one; cornell_textured's own; more than one
# 64-entry tile of both lists and more than one 256-thread block of the weight kernel, neither a multiple of anything
SIZES = ((1, 1), (7, 5), (64, 1), (65, 3), (64, 32), (130, 67))
CONTENTS = ("sky", "moved_sun", "constant", "one_pixel", "black")
EDITS = ("moved_sun", "constant", "one_pixel", "black")  # what the GPU tests edit the uploaded "sky" to

_sinf = None


def sinf(x):
    """The C library's sinf on one binary32 value: the function rdh_build_envmap_pdf and rdh_scene_set_texture call."""
    global _sinf
    if _sinf is None:
        libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        libm.sinf.restype, libm.sinf.argtypes = ctypes.c_float, [ctypes.c_float]
        _sinf = libm.sinf
    return F(_sinf(float(F(x))))


def row_sin(height):
    """float32[height]: sinf((.5f + i) / height * PI), operation for operation."""
    return np.array([sinf(F(F(F(0.5) + F(i)) / F(height)) * PI_F) for i in range(height)], F)


def luminance(texels):
    t = np.ascontiguousarray(texels, dtype=F).reshape(-1, 3)
    return (F(0.2126) * t[:, 0] + F(0.7152) * t[:, 1]).astype(F) + F(0.0722) * t[:, 2]


def weights(texels):
    """texels float32 [h, w, 3] -> float32[h * w]: the model of k_env_weights."""
    h, w = texels.shape[:2]
    return (luminance(texels).reshape(h, w) * row_sin(h)[:, None]).astype(F).reshape(-1)


def sampler(texels):
    """(alias table, sum): the model of an environment edit's table and power."""
    return alias_model.sweep(weights(texels))


def _sky(w, h, sun=(0.3, 0.22)):
    """scenes._sky with the sun where `sun` says (u, v)."""
    v = (np.arange(h, dtype=np.float64) + 0.5) / h
    u = (np.arange(w, dtype=np.float64) + 0.5) / w
    V, U = np.meshgrid(v, u, indexing="ij")
    sky = np.stack([0.25 + 0.3 * (1 - V), 0.4 + 0.35 * (1 - V), 0.7 + 0.3 * (1 - V)], -1) * (V < 0.5)[..., None]
    ground = np.stack([0.12 + 0 * V, 0.1 + 0 * V, 0.08 + 0 * V], -1) * (V >= 0.5)[..., None]
    s = 40.0 * np.exp(-(((U - sun[0]) / 0.03) ** 2 + ((V - sun[1]) / 0.04) ** 2))
    return (sky + ground + s[..., None] * np.array([1.0, 0.9, 0.7])).astype(F)


def _ulps(x, k):
    """float32 [2k + 1]: x and the k floats on either side of it."""
    out = [F(x)]
    for direction in (F(np.inf), F(-np.inf)):
        y = F(x)
        for _ in range(k):
            y = np.nextafter(y, direction)
            out.append(y)
    return np.array(sorted(out), F)


def _texel_of_weight(c, rs):
    """A texel (t, t, b) with luminance(t, t, b) * rs == c in binary32, or None.  The blue channel's coefficient is the smallest, so
    stepping b moves the luminance in steps finer than its own spacing."""
    for lum in _ulps(F(c / rs), 4):
        if F(lum * rs) != c:
            continue
        t, b = np.meshgrid(_ulps(lum, 4), _ulps(lum, 128), indexing="ij")
        tex = np.stack([t.ravel(), t.ravel(), b.ravel()], 1)
        hit = np.flatnonzero(luminance(tex) == lum)
        if len(hit):
            return tex[hit[0]]
    return None


def _constant_weight(w, h):
    """A map whose pixel WEIGHTS are all the same float c, chosen so that the `over` list is empty: row i holds a texel with
    luminance * rowSin[i] == c in binary32.  (A map of constant texels has weights that follow the rows' sines.)  c = 1 + j / 512:
    ten significant bits, so the sequential sum of n <= 16 384 of them is n * c exactly, and j is the first for which the scaled
    value c * float(n / (n c)) is exactly 1 and every row has such a texel."""
    n, rows = w * h, row_sin(h)
    assert n <= 16384
    for j in range(1, 256):
        c = F(1 + j / 512)
        if F(c * F(F(n) / F(n * c))) != F(1):
            continue
        texels = [_texel_of_weight(c, rs) for rs in rows]
        if all(t is not None for t in texels):
            return np.repeat(np.array(texels, F)[:, None, :], w, axis=1)
    raise AssertionError(f"no constant-weight map of {w}x{h}")


@functools.lru_cache(maxsize=None)
def env_map(size, content):
    """float32 [h, w, 3], read-only."""
    w, h = size
    if content == "sky":
        m = _sky(w, h)
    elif content == "moved_sun":
        m = _sky(w, h, sun=(0.62, 0.31))
    elif content == "constant":
        m = _constant_weight(w, h)
    elif content == "one_pixel":  # black except one pixel (the middle one; the only one of a 1x1 map)
        m = np.zeros((h, w, 3), F)
        m[h // 2, (2 * w) // 3] = (30.0, 25.0, 20.0)
    elif content == "black":
        m = np.zeros((h, w, 3), F)
    else:
        raise KeyError(content)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def cornell():
    from radish_pt_amd import scenes

    return scenes.cornell_textured(env=True)


def with_textures(sd, replaced, name=None):
    """A new SceneData: sd with textures {id: texels} replaced (the host's tables of the edited description)."""
    from radish_pt_amd import scenes

    tex = list(sd.textures)
    for k, t in replaced.items():
        tex[k] = np.ascontiguousarray(t, dtype=F)
    out = scenes.SceneData(name or f"{sd.name}_textures", sd.vertices, sd.normals, sd.texcoords, sd.material_ids, sd.materials, tex,
                           sd.env_map_tex_id)
    out.objects, out.rest_vertices, out.rest_normals = sd.objects, sd.rest_vertices, sd.rest_normals
    return out


@functools.lru_cache(maxsize=None)
def scene(size, content="sky"):
    """cornell_textured with its environment map (the last texture) replaced by env_map(size, content)."""
    sd = cornell()
    return with_textures(sd, {sd.env_map_tex_id: env_map(size, content)}, f"cornell_env_{size[0]}x{size[1]}_{content}")


def plain_edits():
    """{texture id: texels}: texture 0 (32x32 base colour) and texture 2 (8x8 roughness) of cornell_textured, replaced."""
    rng = np.random.default_rng(11)
    sd = cornell()
    t0 = np.ascontiguousarray(sd.textures[0][::-1, :, ::-1] * F(0.5) + F(0.25), dtype=F)
    t2 = (0.1 + 0.8 * rng.random((8, 8, 1))).repeat(3, axis=2).astype(F)
    assert t0.shape == sd.textures[0].shape and t2.shape == sd.textures[2].shape
    return {0: t0, 2: t2}
