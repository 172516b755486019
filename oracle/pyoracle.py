"""ctypes loader for oracle/liboracle.so — TEST INFRASTRUCTURE ONLY.

Importable from tests/, from `__graft_entry__.smoke()` and from the `cpu_baseline` leg of bench.py, nowhere else.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RADISH_ORACLE_LIB") or os.path.join(_HERE, "liboracle.so")  # RADISH_ORACLE_LIB: the sanitizer build (tests/tools/sanitize_cpu.sh)

RESERVOIR_BYTES = 36


class SceneDesc(C.Structure):
    _fields_ = [
        ("vertices", C.c_void_p), ("normals", C.c_void_p), ("texcoords", C.c_void_p), ("boundingBoxes", C.c_void_p),
        ("bvhNodes", C.c_void_p * 6), ("bvhSize", C.c_int32), ("numPrims", C.c_int32),
        ("materialIds", C.c_void_p), ("materials", C.c_void_p), ("numMaterials", C.c_int32),
        ("numLights", C.c_int32), ("lightPrimIds", C.c_void_p), ("lightUnitRadiance", C.c_void_p),
        ("sumLightPowerInv", C.c_float), ("lightSamplerLength", C.c_int32), ("lightSampler", C.c_void_p),
        ("sobol", C.c_void_p),
        ("numTextures", C.c_int32), ("textures", C.c_void_p), ("envMapTexId", C.c_int32),
        ("envMapSamplerLength", C.c_int32), ("envMapSampler", C.c_void_p),
    ]


class TextureC(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("data", C.c_void_p)]


class GBufferC(C.Structure):
    _fields_ = [
        ("albedo", C.c_void_p), ("normal", C.c_void_p * 2), ("motion", C.c_void_p), ("depth", C.c_void_p * 2),
        ("primId", C.c_void_p * 2), ("frameIdx", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
    ]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("closestRays", "anyRays", "nodeVisits", "triTests", "closestHits")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run `make -C oracle`")
        l = C.CDLL(LIB_PATH)
        vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
        l.orc_scene_create.restype = vp
        l.orc_scene_create.argtypes = [C.POINTER(SceneDesc)]
        l.orc_scene_destroy.argtypes = [vp]
        l.orc_stats_reset.argtypes = [vp]
        l.orc_stats_get.argtypes = [vp, C.POINTER(Stats)]
        l.orc_trace_closest.argtypes = [vp, vp, i64, vp]
        l.orc_trace_closest_naive.argtypes = [vp, vp, i64, vp]
        l.orc_trace_occluded.argtypes = [vp, vp, i64, vp]
        l.orc_path_trace.argtypes = [vp, vp, vp, vp, i32, i32, i32, i64, i64, i64]
        l.orc_path_trace_direct.argtypes = [vp, vp, vp, i32, i32, i64, i64, i64]
        l.orc_gbuffer_render.argtypes = [vp, vp, vp, C.POINTER(GBufferC)]
        l.orc_restir_direct.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, C.POINTER(GBufferC)] + [i32] * 5
        l.orc_utilhash.restype = C.c_uint32
        l.orc_utilhash.argtypes = [C.c_uint32]
        l.orc_aabb_intersect.restype = i32
        l.orc_aabb_intersect.argtypes = [vp, vp, C.POINTER(f32)]
        l.orc_intersect_triangle.restype = i32
        l.orc_intersect_triangle.argtypes = [vp, vp, vp, C.POINTER(f32)]
        l.orc_sincos.argtypes = [f32, C.POINTER(f32), C.POINTER(f32)]
        l.orc_atan2.restype = f32
        l.orc_atan2.argtypes = [f32, f32]
        l.orc_texture_sample.restype = None
        l.orc_texture_sample.argtypes = [vp, i32, vp, vp]
        l.orc_material_eval.argtypes = [vp, i32, vp, vp, vp, vp]
        l.orc_camera_sample.argtypes = [vp, i32, i32, vp, vp]
        l.orc_sample_direct_light.argtypes = [vp, vp, vp, i32, vp, vp, C.POINTER(f32), C.POINTER(f32)]
        l.orc_sample_direct_light.restype = None
        l.orc_reservoir_op.argtypes, l.orc_reservoir_op.restype = [i32, vp, vp, f32, i32], None
        l.orc_reservoir_W.argtypes, l.orc_reservoir_W.restype = [vp, vp, vp, vp], f32
        l.orc_power_heuristic.argtypes, l.orc_power_heuristic.restype = [f32, f32], f32
        l.orc_copy_image_to_pbo.argtypes = [vp, vp, i32, i32, i32, i32, f32]
        l.orc_copy_image_to_pbo.restype = None
        l.orc_pow_gamma.argtypes = [f32]
        l.orc_pow_gamma.restype = f32
        l.orc_exp.argtypes, l.orc_exp.restype = [f32], f32
        l.orc_pow.argtypes, l.orc_pow.restype = [f32, f32], f32
        G = C.POINTER(GBufferC)
        l.orc_denoise_eaw.argtypes = [vp, vp, G, vp, f32, f32, f32, i32]
        l.orc_denoise_svgf.argtypes = [vp, vp, vp, vp, vp, G, vp, f32, f32, f32, i32]
        l.orc_denoise_modulate.argtypes = [vp, G]
        l.orc_denoise_add.argtypes = [vp, vp, vp, i32, i32]
        l.orc_denoise_temporal_accumulate.argtypes = [vp, vp, vp, vp, vp, G, i32]
        l.orc_denoise_estimate_variance.argtypes = [vp, vp, i32, i32]
        l.orc_denoise_filter_variance.argtypes = [vp, vp, i32, i32]
        for fn in ("orc_denoise_eaw", "orc_denoise_svgf", "orc_denoise_modulate", "orc_denoise_add",
                   "orc_denoise_temporal_accumulate", "orc_denoise_estimate_variance", "orc_denoise_filter_variance"):
            getattr(l, fn).restype = None
        for fn in ("orc_scene_destroy", "orc_stats_reset", "orc_stats_get", "orc_trace_closest", "orc_trace_closest_naive",
                   "orc_trace_occluded", "orc_path_trace", "orc_path_trace_direct", "orc_gbuffer_render",
                   "orc_restir_direct", "orc_sincos", "orc_material_eval", "orc_camera_sample"):
            getattr(l, fn).restype = None
        for fn in ("orc_intersect_triangle_n", "orc_ray_n", "orc_utilhash_n", "orc_sincos_n", "orc_atan2_n", "orc_to_sphere_n",
                   "orc_to_plane_n", "orc_power_heuristic_n", "orc_material_n", "orc_procedural_texture_n", "orc_pow_gamma_n",
                   "orc_tonemap_n", "orc_exp_pow_n", "orc_reservoir_n", "orc_reservoir_w_n"):
            getattr(l, fn).argtypes, getattr(l, fn).restype = [vp, i64, vp], None
        l.orc_aabb_intersect_n.argtypes, l.orc_aabb_intersect_n.restype = [vp, i64, vp, vp], None
        l.orc_linear_sample_n.argtypes, l.orc_linear_sample_n.restype = [vp, i32, i32, vp, i64, vp], None
        _lib = l
    return _lib


HIT_DTYPE = np.dtype([("primId", "<i4"), ("u", "<f4"), ("v", "<f4"), ("t", "<f4")])


class GBufferHost:
    """Host-memory G-buffer with the reference's double-buffer semantics (src/gBuffer.h:24-57)."""

    def __init__(self, width, height):
        n = width * height
        self.width, self.height = width, height
        self.albedo = np.zeros((n, 3), np.float32)
        self.normal = [np.zeros((n, 3), np.float32) for _ in range(2)]
        self.motion = np.zeros(n, np.int32)
        self.depth = [np.zeros(n, np.float32) for _ in range(2)]
        self.primId = [np.zeros(n, np.int32) for _ in range(2)]
        self.frameIdx = 0
        self.lastCam = None

    def c_struct(self):
        g = GBufferC()
        g.albedo = self.albedo.ctypes.data
        g.normal = (C.c_void_p * 2)(*[a.ctypes.data for a in self.normal])
        g.motion = self.motion.ctypes.data
        g.depth = (C.c_void_p * 2)(*[a.ctypes.data for a in self.depth])
        g.primId = (C.c_void_p * 2)(*[a.ctypes.data for a in self.primId])
        g.frameIdx, g.width, g.height = self.frameIdx, self.width, self.height
        return g

    def update(self, cam):  # GBuffer::update (src/gBuffer.cu:78-81)
        self.lastCam = cam.copy()
        self.frameIdx ^= 1


class OracleScene:
    """Owns an orc_scene handle over the arrays of a radish_pt_amd.scenes.SceneData (borrowed)."""

    def __init__(self, sd):
        self.sd = sd
        d = SceneDesc()
        d.vertices, d.normals, d.texcoords = sd.vertices.ctypes.data, sd.normals.ctypes.data, sd.texcoords.ctypes.data
        d.boundingBoxes = sd.boxes.ctypes.data
        d.bvhNodes = (C.c_void_p * 6)(*[a.ctypes.data for a in sd.nodes])
        d.bvhSize, d.numPrims = sd.bvh_size, sd.num_prims
        d.materialIds, d.materials, d.numMaterials = sd.material_ids.ctypes.data, sd.materials.ctypes.data, len(sd.materials)
        d.numLights = sd.num_lights
        d.lightPrimIds = sd.light_prim_ids.ctypes.data
        d.lightUnitRadiance = sd.light_unit_radiance.ctypes.data
        d.sumLightPowerInv = float(sd.sum_light_power_inv)
        d.lightSamplerLength = len(sd.light_sampler)
        d.lightSampler = sd.light_sampler.ctypes.data
        d.sobol = sd.sobol.ctypes.data
        texs = getattr(sd, "textures", [])
        self._tex = (TextureC * max(len(texs), 1))()
        for i, t in enumerate(texs):
            self._tex[i].width, self._tex[i].height, self._tex[i].data = t.shape[1], t.shape[0], t.ctypes.data
        d.numTextures = len(texs)
        d.textures = C.cast(self._tex, C.c_void_p)
        d.envMapTexId = getattr(sd, "env_map_tex_id", -1)
        env = getattr(sd, "env_map_sampler", None)
        d.envMapSamplerLength = 0 if env is None else len(env)
        d.envMapSampler = None if env is None or len(env) == 0 else env.ctypes.data
        self._desc = d
        self.h = lib().orc_scene_create(C.byref(d))
        if not self.h:
            raise RuntimeError("orc_scene_create failed (textured materials are out of scope)")

    def __del__(self):
        if getattr(self, "h", None):
            lib().orc_scene_destroy(self.h)
            self.h = None

    def reset_stats(self):
        lib().orc_stats_reset(self.h)

    def stats(self):
        s = Stats()
        lib().orc_stats_get(self.h, C.byref(s))
        return s.as_dict()

    def sample_direct_light(self, pos, r4, visibility):
        """(pdf, radiance[3], wi[3], dist) of sampleDirectLight / sampleDirectLightNoVisibility at `pos` with draws r4."""
        pos = np.ascontiguousarray(pos, np.float32)
        r4 = np.ascontiguousarray(r4, np.float32)
        rad, wi = np.zeros(3, np.float32), np.zeros(3, np.float32)
        dist, pdf = C.c_float(0), C.c_float(0)
        lib().orc_sample_direct_light(self.h, pos.ctypes.data, r4.ctypes.data, int(visibility), rad.ctypes.data, wi.ctypes.data,
                                      C.byref(dist), C.byref(pdf))
        return pdf.value, rad, wi, dist.value

    def trace_closest(self, rays, naive=False):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        hits = np.zeros(len(rays), HIT_DTYPE)
        fn = lib().orc_trace_closest_naive if naive else lib().orc_trace_closest
        fn(self.h, rays.ctypes.data, len(rays), hits.ctypes.data)
        return hits

    def trace_occluded(self, segments):
        seg = np.ascontiguousarray(segments, np.float32).reshape(-1, 6)
        occ = np.zeros(len(seg), np.int32)
        lib().orc_trace_occluded(self.h, seg.ctypes.data, len(seg), occ.ctypes.data)
        return occ

    @staticmethod
    def _cam_buf(cam):
        return np.frombuffer(cam.tobytes(), np.uint8).copy()

    def path_trace(self, cam, direct, indirect, iter, looper, max_depth, pix=None):
        w, h = (int(v) for v in cam["resolution"])
        b, e, s = pix if pix else (0, w * h, 1)
        cb = self._cam_buf(cam)
        lib().orc_path_trace(self.h, cb.ctypes.data, direct.ctypes.data, indirect.ctypes.data, iter, looper, max_depth,
                             b, e, s)

    def path_trace_direct(self, cam, direct, iter, looper, pix=None):
        w, h = (int(v) for v in cam["resolution"])
        b, e, s = pix if pix else (0, w * h, 1)
        cb = self._cam_buf(cam)
        lib().orc_path_trace_direct(self.h, cb.ctypes.data, direct.ctypes.data, iter, looper, b, e, s)

    def gbuffer_render(self, cam, gb):
        cb = self._cam_buf(cam)
        lb = self._cam_buf(gb.lastCam if gb.lastCam is not None else cam)
        g = gb.c_struct()
        lib().orc_gbuffer_render(self.h, cb.ctypes.data, lb.ctypes.data, C.byref(g))

    def restir_direct(self, cam, direct, iter, looper, res_out, res_in, res_temp, gb, first_frame, reuse_mask,
                      faithful_ris=1, num_spatial=5, ris_count=32):
        cb = self._cam_buf(cam)
        g = gb.c_struct()
        lib().orc_restir_direct(self.h, cb.ctypes.data, direct.ctypes.data, iter, looper, res_out.ctypes.data,
                                res_in.ctypes.data, res_temp.ctypes.data, C.byref(g), int(first_frame), reuse_mask,
                                faithful_ris, num_spatial, ris_count)


def copy_image_to_pbo(image, width, height, kind=0, tone_mapping=0, scale=1.0):
    """sendImageToPBO (pathtrace.cu:32-118) on a host array → uint8 [width*height, 4]."""
    img = np.ascontiguousarray(image)
    pbo = np.zeros((width * height, 4), np.uint8)
    lib().orc_copy_image_to_pbo(pbo.ctypes.data, img.ctypes.data, width, height, kind, tone_mapping, scale)
    return pbo


def pow_gamma(x):
    return float(lib().orc_pow_gamma(float(x)))


# ---- denoisers (denoiser.cu) on host arrays -----------------------------------------------------------------------------
def _cam_bytes(cam):
    return np.frombuffer(np.asarray(cam).tobytes(), np.uint8).copy()


def denoise_eaw(color_in, gb, cam, sig_lumin, sig_normal, sig_depth, level):
    out = np.zeros_like(color_in)
    g, cb = gb.c_struct(), _cam_bytes(cam)
    lib().orc_denoise_eaw(out.ctypes.data, color_in.ctypes.data, C.byref(g), cb.ctypes.data, sig_lumin, sig_normal, sig_depth, level)
    return out


def denoise_svgf(color_in, var_in, var_filtered, gb, cam, sig_lumin, sig_normal, sig_depth, level):
    out, var_out = np.zeros_like(color_in), np.zeros_like(var_in)
    g, cb = gb.c_struct(), _cam_bytes(cam)
    lib().orc_denoise_svgf(out.ctypes.data, color_in.ctypes.data, var_out.ctypes.data, var_in.ctypes.data, var_filtered.ctypes.data,
                           C.byref(g), cb.ctypes.data, sig_lumin, sig_normal, sig_depth, level)
    return out, var_out


def denoise_modulate(image, gb):
    out = image.copy()
    g = gb.c_struct()
    lib().orc_denoise_modulate(out.ctypes.data, C.byref(g))
    return out


def denoise_add(in1, in2, width, height):
    out = np.zeros_like(in1)
    lib().orc_denoise_add(out.ctypes.data, in1.ctypes.data, in2.ctypes.data, width, height)
    return out


def denoise_temporal_accumulate(color_accum_in, moment_accum_in, color_in, gb, first):
    c_out, m_out = np.zeros_like(color_in), np.zeros_like(color_in)
    g = gb.c_struct()
    lib().orc_denoise_temporal_accumulate(c_out.ctypes.data, color_accum_in.ctypes.data, m_out.ctypes.data,
                                          moment_accum_in.ctypes.data, color_in.ctypes.data, C.byref(g), 1 if first else 0)
    return c_out, m_out


def denoise_estimate_variance(moment, width, height):
    var = np.zeros(width * height, np.float32)
    lib().orc_denoise_estimate_variance(var.ctypes.data, moment.ctypes.data, width, height)
    return var


def denoise_filter_variance(var_in, width, height):
    out = np.zeros_like(var_in)
    lib().orc_denoise_filter_variance(out.ctypes.data, var_in.ctypes.data, width, height)
    return out


def reservoir_op(op, r, rhs, rnd, M=20):
    """restir.h's reservoir arithmetic on one-element RESERVOIR_DTYPE arrays (see orc_reservoir_op); returns the new `r`."""
    out = np.array(r, copy=True)
    rhs = np.ascontiguousarray(rhs)
    lib().orc_reservoir_op(int(op), out.ctypes.data, rhs.ctypes.data, float(rnd), int(M))
    return out


def reservoir_W(r, material, n, wo):
    r = np.ascontiguousarray(r)
    m = np.ascontiguousarray(material)
    n = np.ascontiguousarray(n, np.float32)
    wo = np.ascontiguousarray(wo, np.float32)
    return float(lib().orc_reservoir_W(r.ctypes.data, m.ctypes.data, n.ctypes.data, wo.ctypes.data))


def power_heuristic(f, g):
    return float(lib().orc_power_heuristic(float(f), float(g)))


# ---- batch entries (orc_*_n): n records of 32-bit words in, n records out, laid out as in tests/probe/device_probe.hip ----
BATCH_WORDS = {  # name -> (words per input record, words per output record)
    "intersect_triangle": (15, 4), "ray": (6, 8), "utilhash": (1, 1), "sincos": (1, 2), "atan2": (2, 1), "to_sphere": (2, 3),
    "to_plane": (3, 2), "power_heuristic": (2, 1), "material": (20, 12), "procedural_texture": (2, 3), "pow_gamma": (1, 1),
    "tonemap": (3, 6), "exp_pow": (2, 3), "reservoir": (20, 45), "reservoir_w": (24, 1),
}


def batch(name, records):
    """orc_<name>_n over `records` (uint32 [n, words in]) -> uint32 [n, words out]."""
    wi, wo = BATCH_WORDS[name]
    rec = np.ascontiguousarray(records).view(np.uint32).reshape(-1, wi)
    out = np.zeros((len(rec), wo), np.uint32)
    getattr(lib(), f"orc_{name}_n")(rec.ctypes.data, len(rec), out.ctypes.data)
    return out


def aabb_intersect_n(records):
    """orc_aabb_intersect over float32 [n, 12] = box6, ray6 -> (hit int32 [n], tMin float32 [n])."""
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, 12)
    hit, t = np.zeros(len(rec), np.int32), np.zeros(len(rec), np.float32)
    lib().orc_aabb_intersect_n(rec.ctypes.data, len(rec), hit.ctypes.data, t.ctypes.data)
    return hit, t


def linear_sample_n(texels, uv):
    """linearSample of float32 texels [height, width, 3] at FINITE uv float32 [n, 2] -> float32 [n, 3]."""
    tex = np.ascontiguousarray(texels, np.float32)
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    assert np.isfinite(uv).all(), "linearSample's texel index is undefined (out of bounds on the host) for a non-finite uv"
    out = np.zeros((len(uv), 3), np.float32)
    lib().orc_linear_sample_n(tex.ctypes.data, tex.shape[1], tex.shape[0], uv.ctypes.data, len(uv), out.ctypes.data)
    return out
