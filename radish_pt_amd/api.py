"""Host-side mirror of the reference's render API over libradish_hip.so (include/radish_hip.h).

Same names, argument meaning and side effects as the reference's C++ free functions and globals
(`/root/reference/src/pathtrace.h:18-23`, `restir.h:103-106`, `gBuffer.h:24-27`, `common.h:50-72`):

    Settings.traceDepth, Settings.reservoirReuse, State.looper, State.scene
    pathTraceInit() / pathTraceFree()
    pathTrace(directIllum, indirectIllum, iter)          # advances State.looper mod 10000
    pathTraceSamples(directIllum, indirectIllum, iter, samples)   # `samples` pathTrace calls' worth in one call
    pathTraceDirect(directIllum, iter)
    ReSTIRInit() / ReSTIRFree() / ReSTIRDirect(directIllum, iter, gBuffer)
    GBuffer.create(w, h) / destroy() / render(devScene, cam) / update(cam)
    DevScene.create(scene) / destroy()

Images are CUDA (HIP) float32 torch tensors of shape [H*W, 3] — the reference's `glm::vec3*` device buffers.  PyTorch
is plumbing here (device memory, streams, torch.distributed); every computation happens in the HIP library.  There is
no CPU path: importing works without a GPU, calling anything raises.
"""
import ctypes as C
import os

import numpy as np

from . import hostlib
from . import layouts as L

_HERE = os.path.dirname(os.path.abspath(__file__))
# RADISH_HIP_LIB selects an alternative build of the same library (tuning experiments); never a different backend.
HIP_LIB_PATH = os.environ.get("RADISH_HIP_LIB") or os.path.join(_HERE, "csrc", "libradish_hip.so")

RDH_PT_MEGAKERNEL, RDH_PT_WAVEFRONT, RDH_PT_SORT_MATERIAL, RDH_PT_COUNT, RDH_PT_PROFILE = 0, 1, 2, 4, 8
RDH_PT_PERSISTENT = 16
RDH_PT_NO_SCHEDULE = 32
RDH_PT_ONE_LANE_PER_PIXEL = 64
RDH_PT_MEGA_GBUFFER = RDH_PT_ONE_LANE_PER_PIXEL
RDH_PT_NO_DEFER = 128
RDH_PT_WG_PER_RAY = 256
RDH_PT_PARTITION_GBUFFER = 512
RDH_PT_RESTIR_FUSED = 1024
RDH_PT_WF_SUBFRAMES = 2048
RDH_PT_WF_SMALL_LISTS = 4096
RDH_PT_NO_PAIRS = 16384
RDH_PT_NO_PACKETS = 8192
RDH_PT_PAIRS = 32768
RDH_PT_AUTO = 65536
RDH_PT_WALK_ALL = 131072
# BVH builders of rdh_build_bvh_device_ex / rdh_scene_update_geometry_ex (Context.build_bvh_device / update_geometry `builder`)
RDH_BVH_SAH, RDH_BVH_LBVH = 0, 1
BVH_BUILDERS = {"sah": RDH_BVH_SAH, "lbvh": RDH_BVH_LBVH}
# rdh_set_lens (Context.set_lens `mode`)
RDH_LENS_OFF, RDH_LENS_DISK, RDH_LENS_MASK = 0, 1, 2
LENS_MODES = {"off": RDH_LENS_OFF, "disk": RDH_LENS_DISK, "mask": RDH_LENS_MASK}
# rdh_scene_pose_objects: what happens to the tree (Context.pose_objects `tree`) and its flag
RDH_POSE_REFIT, RDH_POSE_SAH, RDH_POSE_LBVH = 0, 1, 2
RDH_POSE_REBUILD_LIGHTS = 1
POSE_TREES = {"refit": RDH_POSE_REFIT, "sah": RDH_POSE_SAH, "lbvh": RDH_POSE_LBVH}
# rdh_object_range[]: the first three fields of hostlib.OBJECT_DTYPE
OBJECT_RANGE_DTYPE = np.dtype([("firstPrim", "<i4"), ("numPrims", "<i4"), ("restFirstPrim", "<i4")])
SOBOL_SAMPLE_NUM = 10000  # SobolSampleNum, src/sampler.h:12

# Every symbol include/radish_hip.h declares (tests check that the library exports all of them).
EXPORTS = [
    "rdh_create", "rdh_destroy", "rdh_last_error", "rdh_set_stream", "rdh_synchronize", "rdh_scene_upload",
    "rdh_scene_free", "rdh_set_camera", "rdh_set_partition", "rdh_tiles_per_rank", "rdh_untile", "rdh_path_trace", "rdh_path_trace_samples",
    "rdh_path_trace_direct", "rdh_gbuffer_render", "rdh_restir_init", "rdh_restir_free", "rdh_restir_direct",
    "rdh_restir_read", "rdh_restir_read_scratch", "rdh_copy_image_to_pbo", "rdh_denoise_eaw", "rdh_denoise_svgf", "rdh_denoise_modulate",
    "rdh_denoise_add", "rdh_denoise_temporal_accumulate", "rdh_denoise_estimate_variance", "rdh_denoise_filter_variance", "rdh_restir_exchange_pack", "rdh_restir_exchange_unpack", "rdh_trace_closest", "rdh_trace_occluded", "rdh_counters_reset", "rdh_counters_read",
    "rdh_last_kernel_ms", "rdh_profile_reset", "rdh_profile_read", "rdh_debug_persist_stamps", "rdh_debug_persist_phases", "rdh_debug_wf_stamps",
    "rdh_debug_wf_counts",
    "rdh_gbuffer_exchange_pack", "rdh_gbuffer_exchange_unpack", "rdh_comm_unique_id", "rdh_comm_init", "rdh_comm_destroy",
    "rdh_dump_rays", "rdh_set_occupancy_share", "rdh_allgather_tiles", "rdh_path_trace_gathered", "rdh_restir_exchange", "rdh_restir_direct_gathered", "rdh_gbuffer_exchange",
    "rdh_comm_init_all", "rdh_path_trace_gathered_all", "rdh_gbuffer_exchange_all", "rdh_restir_direct_gathered_all",
    "rdh_comm_set_overlap", "rdh_comm_join",
    "rdh_build_bvh_device", "rdh_scene_update_geometry", "rdh_debug_read_tree",
    "rdh_scene_refit_geometry", "rdh_scene_tree_cost",
    "rdh_build_bvh_device_ex", "rdh_scene_update_geometry_ex",
    "rdh_scene_track_motion",
    "rdh_build_alias_table_device", "rdh_scene_rebuild_lights", "rdh_debug_read_lights",
    "rdh_scene_set_objects", "rdh_scene_pose_objects", "rdh_debug_read_world",
    "rdh_scene_set_materials", "rdh_build_light_list_device",
    "rdh_scene_set_texture", "rdh_scene_env_power", "rdh_debug_read_textures",
    "rdh_scene_set_geometry", "rdh_debug_read_geometry",
    "rdh_path_trace_adaptive", "rdh_adaptive_plan",
    "rdh_debug_persist_schedule", "rdh_debug_persist_read", "rdh_debug_persist_set_order",
    "rdh_set_lens", "rdh_debug_primary_rays", "rdh_debug_read_lens",
]


class SceneDescC(C.Structure):
    _fields_ = [
        ("vertices", C.c_void_p), ("normals", C.c_void_p), ("texcoords", C.c_void_p), ("boundingBoxes", C.c_void_p),
        ("bvhNodes", C.c_void_p * 6), ("bvhSize", C.c_int32), ("numPrims", C.c_int32),
        ("materialIds", C.c_void_p), ("materials", C.c_void_p), ("numMaterials", C.c_int32),
        ("numLights", C.c_int32), ("lightPrimIds", C.c_void_p), ("lightUnitRadiance", C.c_void_p),
        ("sumLightPowerInv", C.c_float), ("lightSamplerLength", C.c_int32), ("lightSampler", C.c_void_p),
        ("sampleSequence", C.c_void_p),
        ("numTextures", C.c_int32), ("textures", C.c_void_p), ("envMapTexId", C.c_int32),
        ("envMapSamplerLength", C.c_int32), ("envMapSampler", C.c_void_p),
    ]


class LightUpdateC(C.Structure):  # rdh_light_update
    _fields_ = [("lightSampler", C.c_void_p), ("lightSamplerLength", C.c_int32), ("sumLightPowerInv", C.c_float)]


class TextureC(C.Structure):  # rdh_texture
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("data", C.c_void_p)]


class GBufferC(C.Structure):  # == the reference's GBuffer, 272 bytes
    _fields_ = [
        ("albedo", C.c_void_p), ("normal", C.c_void_p * 2), ("motion", C.c_void_p), ("depth", C.c_void_p * 2),
        ("primId", C.c_void_p * 2), ("frameIdx", C.c_int32), ("lastCam", C.c_uint8 * 196), ("width", C.c_int32),
        ("height", C.c_int32),
    ]


assert C.sizeof(GBufferC) == 272


class CountersC(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("closestRays", "anyRays", "nodeVisits", "triTests", "closestHits")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class AdaptiveStatsC(C.Structure):  # rdh_adaptive_stats
    _fields_ = [("samplesRequested", C.c_int64), ("activeBlocks", C.c_int32), ("wantingPixels", C.c_int32)]


RDH_ADAPTIVE_MAX_REQUEST = 16


class RestirParamsC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("reuseMask", "risCount", "numSpatial", "temporalClamp", "faithfulRIS")]


_lib = None


def lib():
    """Load libradish_hip.so; raises if it has not been built — there is no fallback implementation."""
    global _lib
    if _lib is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise RuntimeError(
                f"{HIP_LIB_PATH} is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'`. "
                "radish_pt_amd has no CPU or PyTorch fallback for the render path."
            )
        l = C.CDLL(HIP_LIB_PATH)
        vp, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
        sig = {
            "rdh_create": ([C.POINTER(vp), i32], i32),
            "rdh_destroy": ([vp], None),
            "rdh_last_error": ([vp], C.c_char_p),
            "rdh_set_stream": ([vp, vp], i32),
            "rdh_synchronize": ([vp], i32),
            "rdh_scene_upload": ([vp, C.POINTER(SceneDescC)], i32),
            "rdh_scene_free": ([vp], i32),
            "rdh_set_camera": ([vp, vp], i32),
            "rdh_set_partition": ([vp, i32, i32, i32], i32),
            "rdh_tiles_per_rank": ([vp], i32),
            "rdh_untile": ([vp, vp, vp], i32),
            "rdh_path_trace": ([vp, vp, vp, i32, i32, i32, u32], i32),
            "rdh_path_trace_samples": ([vp, vp, vp, i32, i32, i32, i32, i32, u32], i32),
            "rdh_path_trace_direct": ([vp, vp, i32, i32, u32], i32),
            "rdh_gbuffer_render": ([vp, C.POINTER(GBufferC), u32], i32),
            "rdh_restir_init": ([vp], i32),
            "rdh_restir_free": ([vp], i32),
            "rdh_restir_direct": ([vp, vp, i32, i32, C.POINTER(GBufferC), C.POINTER(RestirParamsC), u32], i32),
            "rdh_restir_read": ([vp, i32, vp], i32),
            "rdh_restir_read_scratch": ([vp, i32, vp, i64], i64),
            "rdh_copy_image_to_pbo": ([vp, vp, vp, i32, i32, i32, i32, C.c_float], i32),
            "rdh_denoise_eaw": ([vp, vp, vp, C.POINTER(GBufferC), vp] + [C.c_float] * 3 + [i32], i32),
            "rdh_denoise_svgf": ([vp, vp, vp, vp, vp, vp, C.POINTER(GBufferC), vp] + [C.c_float] * 3 + [i32], i32),
            "rdh_denoise_modulate": ([vp, vp, C.POINTER(GBufferC)], i32),
            "rdh_denoise_add": ([vp, vp, vp, vp, i32, i32], i32),
            "rdh_denoise_temporal_accumulate": ([vp, vp, vp, vp, vp, vp, C.POINTER(GBufferC), i32], i32),
            "rdh_denoise_estimate_variance": ([vp, vp, vp, i32, i32], i32),
            "rdh_denoise_filter_variance": ([vp, vp, vp, i32, i32], i32),
            "rdh_restir_exchange_pack": ([vp, vp], i32),
            "rdh_restir_exchange_unpack": ([vp, vp], i32),
            "rdh_trace_closest": ([vp, vp, i64, vp, u32], i32),
            "rdh_trace_occluded": ([vp, vp, i64, vp, u32], i32),
            "rdh_counters_reset": ([vp], i32),
            "rdh_counters_read": ([vp, C.POINTER(CountersC)], i32),
            "rdh_last_kernel_ms": ([vp, C.POINTER(C.c_float)], i32),
            "rdh_profile_reset": ([vp], i32),
            "rdh_profile_read": ([vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)], i32),
            "rdh_debug_persist_stamps": ([vp, vp], i32),
            "rdh_debug_persist_phases": ([vp, vp], i32),
            "rdh_gbuffer_exchange_pack": ([vp, C.POINTER(GBufferC), vp], i32),
            "rdh_gbuffer_exchange_unpack": ([vp, C.POINTER(GBufferC), vp], i32),
            "rdh_comm_unique_id": ([vp], i32),
            "rdh_comm_init": ([vp, vp, i32, i32], i32),
            "rdh_comm_destroy": ([vp], i32),
            "rdh_comm_init_all": ([C.POINTER(vp), i32], i32),
            "rdh_path_trace_gathered_all": ([C.POINTER(vp), i32, C.POINTER(vp), C.POINTER(vp), i32, i32, i32, u32], i32),
            "rdh_gbuffer_exchange_all": ([C.POINTER(vp), i32, C.POINTER(GBufferC)], i32),
            "rdh_restir_direct_gathered_all": ([C.POINTER(vp), i32, C.POINTER(vp), i32, i32, C.POINTER(GBufferC), C.POINTER(RestirParamsC), u32], i32),
            "rdh_comm_set_overlap": ([vp, i32], i32),
            "rdh_comm_join": ([vp], i32),
            "rdh_allgather_tiles": ([vp, vp, vp], i32),
            "rdh_path_trace_gathered": ([vp, vp, vp, i32, i32, i32, u32], i32),
            "rdh_restir_exchange": ([vp], i32),
            "rdh_restir_direct_gathered": ([vp, vp, i32, i32, C.POINTER(GBufferC), C.POINTER(RestirParamsC), u32], i32),
            "rdh_gbuffer_exchange": ([vp, C.POINTER(GBufferC)], i32),
            "rdh_dump_rays": ([vp, i32, i32, vp, i64, vp, i64, C.POINTER(i64), C.POINTER(i64)], i32),
            "rdh_set_occupancy_share": ([vp, i32], i32),
            "rdh_build_bvh_device": ([vp, vp, i32, vp, C.POINTER(vp)], i32),
            "rdh_scene_update_geometry": ([vp, vp, vp, C.POINTER(LightUpdateC)], i32),
            "rdh_debug_read_tree": ([vp, i32, vp, i64], i64),
            "rdh_scene_refit_geometry": ([vp, vp, vp, C.POINTER(LightUpdateC)], i32),
            "rdh_scene_tree_cost": ([vp, C.POINTER(C.c_double), C.POINTER(C.c_double)], i32),
            "rdh_build_bvh_device_ex": ([vp, vp, i32, i32, vp, C.POINTER(vp)], i32),
            "rdh_scene_update_geometry_ex": ([vp, vp, vp, C.POINTER(LightUpdateC), i32], i32),
            "rdh_scene_track_motion": ([vp, i32], i32),
            "rdh_build_alias_table_device": ([vp, vp, i32, vp, vp], i32),
            "rdh_scene_rebuild_lights": ([vp, C.c_float], i32),
            "rdh_debug_read_lights": ([vp, i32, vp, i64], i64),
            "rdh_scene_set_objects": ([vp, vp, i32, vp, vp, i32], i32),
            "rdh_scene_pose_objects": ([vp, vp, vp, i32, i32, u32, C.c_float], i32),
            "rdh_debug_read_world": ([vp, vp, vp], i32),
            "rdh_scene_set_materials": ([vp, vp, vp, i32, C.c_float], i32),
            "rdh_build_light_list_device": ([vp, vp, vp, i32, vp, i32, vp, vp, vp, vp], i32),
            "rdh_scene_set_texture": ([vp, i32, vp, i32, i32], i32),
            "rdh_scene_env_power": ([vp, C.POINTER(C.c_float)], i32),
            "rdh_debug_read_textures": ([vp, i32, vp, i64], i64),
            "rdh_scene_set_geometry": ([vp, vp, vp, vp, vp, i32, i32, C.c_float], i32),
            "rdh_debug_read_geometry": ([vp, i32, vp, i64], i64),
        }
        for name, (args, res) in sig.items():
            fn = getattr(l, name)
            fn.argtypes, fn.restype = args, res
        _lib = l
    return _lib


def adaptive_entries():
    """(rdh_path_trace_adaptive, rdh_adaptive_plan) with their signatures.  Bound here, at first use, not in lib(): RADISH_HIP_LIB
    may name a build from before these entries (the parent's library of an A/B run), which everything else must still load."""
    vp, i32 = C.c_void_p, C.c_int32
    trace, plan = lib().rdh_path_trace_adaptive, lib().rdh_adaptive_plan
    trace.argtypes, trace.restype = [vp, vp, vp, vp, vp, vp, i32, i32, C.c_uint32, C.POINTER(C.c_int64)], i32
    plan.argtypes, plan.restype = [vp, vp, vp, vp, i32, i32, i32, C.c_float, C.POINTER(AdaptiveStatsC)], i32
    return trace, plan


def persist_entries():
    """(rdh_debug_persist_schedule, rdh_debug_persist_read, rdh_debug_persist_set_order) with their signatures; bound at first use
    for the same reason as adaptive_entries."""
    vp, i32 = C.c_void_p, C.c_int32
    sched, read, set_order = lib().rdh_debug_persist_schedule, lib().rdh_debug_persist_read, lib().rdh_debug_persist_set_order
    sched.argtypes, sched.restype = [vp, vp, vp, vp, i32], i32
    read.argtypes, read.restype = [vp, vp, vp, vp, vp, i32], i32
    set_order.argtypes, set_order.restype = [vp, vp, i32], i32
    return sched, read, set_order


def lens_entries():
    """(rdh_set_lens, rdh_debug_primary_rays, rdh_debug_read_lens) with their signatures; bound at first use for the same reason
    as adaptive_entries."""
    vp, i32 = C.c_void_p, C.c_int32
    set_lens, rays, read = lib().rdh_set_lens, lib().rdh_debug_primary_rays, lib().rdh_debug_read_lens
    set_lens.argtypes, set_lens.restype = [vp, i32, i32], i32
    rays.argtypes, rays.restype = [vp, i32, vp], i32
    read.argtypes, read.restype = [vp, i32, vp, C.c_int64], C.c_int64
    return set_lens, rays, read


class RadishError(RuntimeError):
    pass


def _torch():
    import torch

    return torch


def _builder(what, builder):
    """A builder name of BVH_BUILDERS -> its RDH_BVH_* value."""
    if builder not in BVH_BUILDERS:
        raise RadishError(f"{what}: builder must be one of {sorted(BVH_BUILDERS)}, got {builder!r}")
    return BVH_BUILDERS[builder]


class Context:
    """One rdh_ctx (one device, one stream)."""

    def __init__(self, device=0, use_torch_stream=True):
        torch = _torch()  # imported first so that the HIP runtime torch ships is the one the library binds to
        if not torch.cuda.is_available():
            raise RadishError("radish_pt_amd needs a HIP device; there is no CPU fallback")
        h = C.c_void_p()
        rc = lib().rdh_create(C.byref(h), device)
        if rc != 0:
            raise RadishError(f"rdh_create failed with code {rc} (no usable HIP device?)")
        self.h = h
        self.device = device
        self.rank, self.world, self.tile = 0, 1, 64
        self.width = self.height = 0
        if use_torch_stream:
            self.check(lib().rdh_set_stream(self.h, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))

    # ---- argument checks: the C ABI takes raw device pointers, so a wrongly shaped tensor would be a silent out-of-bounds
    # device write; every image-like argument is checked here (dtype, device, contiguity, minimum element count) ----
    def _ptr(self, t, min_elems, what, dtype=None):
        torch = _torch()
        dtype = dtype or torch.float32
        if not isinstance(t, torch.Tensor):
            raise RadishError(f"{what}: expected a torch tensor, got {type(t).__name__}")
        if not t.is_cuda or t.device.index != self.device:
            raise RadishError(f"{what}: tensor is on {t.device}, the context is on cuda:{self.device}")
        if t.dtype != dtype:
            raise RadishError(f"{what}: dtype {t.dtype}, expected {dtype}")
        if not t.is_contiguous():
            raise RadishError(f"{what}: tensor is not contiguous")
        if t.numel() < min_elems:
            raise RadishError(f"{what}: {t.numel()} elements, the call writes/reads {min_elems}")
        return t.data_ptr()

    def _image_elems(self, gathered=False):
        """floats of one vec3 image argument: the frame, or this rank's packed tiles on a partition"""
        if getattr(self, "world", 1) > 1 and not gathered:
            return self.tiles_per_rank() * self.tile * self.tile * 3
        return self.width * self.height * 3

    def check(self, rc):
        if rc != 0:
            msg = lib().rdh_last_error(self.h)
            raise RadishError(f"libradish_hip error {rc}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "h", None):
            lib().rdh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- scene / camera ----
    def upload_scene(self, sd):
        d = SceneDescC()
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
        d.sampleSequence = sd.sobol.ctypes.data
        texs = getattr(sd, "textures", [])
        tex_c = (TextureC * max(len(texs), 1))()
        for i, t in enumerate(texs):
            tex_c[i].width, tex_c[i].height, tex_c[i].data = t.shape[1], t.shape[0], t.ctypes.data
        d.numTextures = len(texs)
        d.textures = C.cast(tex_c, C.c_void_p)
        d.envMapTexId = getattr(sd, "env_map_tex_id", -1)
        env = getattr(sd, "env_map_sampler", None)
        d.envMapSamplerLength = 0 if env is None else len(env)
        d.envMapSampler = None if env is None or len(env) == 0 else env.ctypes.data
        self.check(lib().rdh_scene_upload(self.h, C.byref(d)))
        self._num_prims = int(sd.num_prims)

    # ---- moving geometry: the device BVH builder ----
    def build_bvh_device(self, vertices, builder="sah"):
        """vertices: float32 cuda tensor [3N, 3] (or [N, 3, 3]) -> (boxes float32 [2N-1, 6], nodes int32 [6, 2N-1, 3]) on the device.
        builder "sah": bit for bit hostlib.build_bvh of the same soup; "lbvh": the linear BVH (rdh_build_bvh_device_ex).
        Asynchronous on the context's stream."""
        b = _builder("build_bvh_device", builder)
        torch = _torch()
        if not isinstance(vertices, torch.Tensor) or vertices.numel() == 0 or vertices.numel() % 9:
            raise RadishError("build_bvh_device: vertices must be a tensor of 9*N floats (N >= 1)")
        n = vertices.numel() // 9
        vp = self._ptr(vertices, 9 * n, "build_bvh_device vertices")
        size = 2 * n - 1
        boxes = torch.empty(size, 6, dtype=torch.float32, device=vertices.device)
        nodes = torch.empty(6, size, 3, dtype=torch.int32, device=vertices.device)
        ptrs = (C.c_void_p * 6)(*[nodes[k].data_ptr() for k in range(6)])
        if b == RDH_BVH_SAH:
            self.check(lib().rdh_build_bvh_device(self.h, vp, n, boxes.data_ptr(), ptrs))
        else:
            self.check(lib().rdh_build_bvh_device_ex(self.h, vp, n, b, boxes.data_ptr(), ptrs))
        return boxes, nodes

    def _geometry_args(self, what, vertices, normals, lights):
        n = getattr(self, "_num_prims", None)
        if n is None:
            raise RadishError(f"{what}: no scene uploaded")
        torch = _torch()
        for t, name in ((vertices, "vertices"), (normals, "normals")):
            if t is not None and (not isinstance(t, torch.Tensor) or t.numel() != 9 * n):
                got = t.numel() if isinstance(t, torch.Tensor) else type(t).__name__
                raise RadishError(f"{what}: {name} must hold 9*{n} floats (the uploaded triangle count), got {got}")
        vp = self._ptr(vertices, 9 * n, f"{what} vertices")
        np_ = None if normals is None else self._ptr(normals, 9 * n, f"{what} normals")
        lu = None
        if lights is not None:
            table, inv = lights
            table = np.ascontiguousarray(table, dtype=L.BINOMIAL_DTYPE)
            lu = LightUpdateC(table.ctypes.data if len(table) else None, len(table), float(inv))
        # the LightUpdateC keeps no reference to the table: return it so that it lives through the call
        return vp, np_, lu, lights if lights is None else table

    def update_geometry(self, vertices, normals=None, lights=None, builder="sah"):
        """New positions for the uploaded scene's triangles (same count and order): vertices / normals float32 cuda tensors of
        9*numPrims floats; lights None (keep the light table) or (light_sampler, sum_light_power_inv) with light_sampler a
        layouts.BINOMIAL_DTYPE array of the scene's length.  Rebuilds the tree on the device with `builder` ("sah": the host
        builder's tree; "lbvh": the linear BVH); does not block."""
        b = _builder("update_geometry", builder)
        vp, np_, lu, _keep = self._geometry_args("update_geometry", vertices, normals, lights)
        if b == RDH_BVH_SAH:
            self.check(lib().rdh_scene_update_geometry(self.h, vp, np_, None if lu is None else C.byref(lu)))
        else:
            self.check(lib().rdh_scene_update_geometry_ex(self.h, vp, np_, None if lu is None else C.byref(lu), b))

    def refit_geometry(self, vertices, normals=None, lights=None):
        """update_geometry's arguments, but the tree keeps its topology and only its boxes are recomputed (rdh_scene_refit_geometry).
        The first refit after an upload or update_geometry derives the refit plan and blocks; later ones do not block."""
        vp, np_, lu, _keep = self._geometry_args("refit_geometry", vertices, normals, lights)
        self.check(lib().rdh_scene_refit_geometry(self.h, vp, np_, None if lu is None else C.byref(lu)))

    def track_motion(self, enable=True):
        """Keep the triangle records as this context's last gbuffer_render saw them (48 B per triangle), so that a render after
        update_geometry / refit_geometry writes motion indices that follow the moved geometry (rdh_scene_track_motion, DESIGN
        11d).  Needs an uploaded scene; upload_scene switches it off again.  False frees the buffer."""
        self.check(lib().rdh_scene_track_motion(self.h, 1 if enable else 0))

    def tree_cost(self):
        """(now, at_build): the SAH cost of the tree as it stands and before the first refit since the last upload / update_geometry
        (rdh_scene_tree_cost).  Blocking."""
        now, at_build = C.c_double(0), C.c_double(0)
        self.check(lib().rdh_scene_tree_cost(self.h, C.byref(now), C.byref(at_build)))
        return now.value, at_build.value

    def debug_read_tree(self, which):
        """Blocking test access (rdh_debug_read_tree): 0 -> NodeRec bytes, 1 -> PairRec bytes, 2 -> the 48-byte header."""
        n = lib().rdh_debug_read_tree(self.h, which, None, 0)
        if n < 0:
            self.check(int(n))
        out = np.zeros(n, np.uint8)
        if n:
            rc = lib().rdh_debug_read_tree(self.h, which, out.ctypes.data, n)
            if rc < 0:
                self.check(int(rc))
        return out

    # ---- moving geometry: the light sampler ----
    def build_alias_table_device(self, values):
        """values: float32 cuda tensor [n] -> (table int32 [n, 2], sum float32 [1]) on the device: row i of table is
        layouts.BINOMIAL_DTYPE's {prob (its bits), failId}, bit for bit hostlib.build_alias_table of the same values
        (rdh_build_alias_table_device).  Asynchronous on the context's stream."""
        torch = _torch()
        if not isinstance(values, torch.Tensor) or values.dim() != 1:
            raise RadishError("build_alias_table_device: values must be a one-dimensional tensor")
        n = values.numel()
        vp = self._ptr(values, n, "build_alias_table_device values")
        table = torch.empty(n, 2, dtype=torch.int32, device=values.device)
        total = torch.zeros(1, dtype=torch.float32, device=values.device)
        self.check(lib().rdh_build_alias_table_device(self.h, vp, n, table.data_ptr(), total.data_ptr()))
        return table, total

    def rebuild_lights(self, env_power=0.0):
        """The uploaded scene's alias table, sumLightPowerInv and per-light constants again, from the emissive triangles as the last
        update_geometry / refit_geometry left them (rdh_scene_rebuild_lights).  env_power: SceneData.env_power of a scene with an
        environment map (ignored without one).  Does not block."""
        self.check(lib().rdh_scene_rebuild_lights(self.h, float(env_power)))

    def debug_read_lights(self, which):
        """Blocking test access (rdh_debug_read_lights): 0 -> the alias table (layouts.BINOMIAL_DTYPE), 1 -> {float32 sum,
        sumLightPowerInv; int32 lightSamplerLength, numLights} as 16 bytes, 2 -> the LightPre records' bytes, 4 -> the current
        lightPrimIds (int32)."""
        n = lib().rdh_debug_read_lights(self.h, which, None, 0)
        if n < 0:
            self.check(int(n))
        out = np.zeros(n, np.uint8)
        if n:
            rc = lib().rdh_debug_read_lights(self.h, which, out.ctypes.data, n)
            if rc < 0:
                self.check(int(rc))
        if which == 4:
            return out.view(np.int32)
        return out.view(L.BINOMIAL_DTYPE) if which == 0 else out

    # ---- materials edited on the device ----
    def set_materials(self, ids, materials, env_power=0.0):
        """Replace the listed materials of the uploaded scene (rdh_scene_set_materials): ids int32 (each at most once), materials an
        array of layouts.MATERIAL_DTYPE, one per id.  Triangles keep their material ids.  When the edit changes which materials
        are lights, or a light's colour, the emissive-triangle list, the alias table, sumLightPowerInv and the per-light constants
        are derived again on the device (env_power as for rebuild_lights).  The scene then renders like a fresh upload_scene of the
        edited description.  Does not block in the steady state."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        mats = np.asarray(materials)
        if mats.dtype != L.MATERIAL_DTYPE:
            raise RadishError(f"set_materials: materials must be an array of layouts.MATERIAL_DTYPE, got dtype {mats.dtype}")
        mats = np.ascontiguousarray(mats).reshape(-1)
        if len(mats) != len(ids):
            raise RadishError(f"set_materials: {len(ids)} ids but {len(mats)} materials")
        self.check(lib().rdh_scene_set_materials(self.h, ids.ctypes.data if len(ids) else None, mats.ctypes.data if len(ids) else None,
                                                 len(ids), float(env_power)))

    def build_light_list_device(self, vertices, material_ids, materials):
        """vertices float32 cuda tensor of 9*N floats, material_ids int32 cuda tensor [N], materials uint8 cuda tensor holding M
        layouts.MATERIAL_DTYPE records (44 B each) -> (light_prim_ids int32 [N], light_unit_radiance float32 [N, 3], light_power
        float32 [N], count int32 [1]) on the device: the first `count` rows are hostlib.build_light_list's, bit for bit; count is
        -1 when a material id is out of range (rdh_build_light_list_device).  Asynchronous on the context's stream."""
        torch = _torch()
        for t, name in ((vertices, "vertices"), (material_ids, "material_ids"), (materials, "materials")):
            if not isinstance(t, torch.Tensor):
                raise RadishError(f"build_light_list_device: {name} must be a torch tensor, got {type(t).__name__}")
        n = material_ids.numel()
        if vertices.numel() != 9 * n:
            raise RadishError(f"build_light_list_device: {n} material ids but {vertices.numel()} vertex floats (9 per triangle)")
        if materials.numel() % L.MATERIAL_DTYPE.itemsize:
            raise RadishError(f"build_light_list_device: materials must hold whole {L.MATERIAL_DTYPE.itemsize}-byte records")
        m = materials.numel() // L.MATERIAL_DTYPE.itemsize
        vp = self._ptr(vertices, 9 * n, "build_light_list_device vertices") if n else None
        ip = self._ptr(material_ids, n, "build_light_list_device material_ids", torch.int32) if n else None
        mp = self._ptr(materials, materials.numel(), "build_light_list_device materials", torch.uint8) if n else None
        dev = f"cuda:{self.device}"
        prims = torch.empty(n, dtype=torch.int32, device=dev)
        radiance = torch.empty(n, 3, dtype=torch.float32, device=dev)
        power = torch.empty(n, dtype=torch.float32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.check(lib().rdh_build_light_list_device(self.h, vp, ip, n, mp, m, prims.data_ptr() if n else None,
                                                     radiance.data_ptr() if n else None, power.data_ptr() if n else None, count.data_ptr()))
        return prims, radiance, power, count

    # ---- textures and the environment map edited on the device ----
    def set_texture(self, tex_id, texels):
        """Replace the texels of texture tex_id of the uploaded scene (rdh_scene_set_texture): texels a float32 cuda tensor
        [height, width, 3] of the uploaded texture's size.  When tex_id is the environment map, its pixel alias table, its power
        and with it the light sampler (alias table, sumLightPowerInv, per-light constants) are derived again on the device.  The
        scene then renders like a fresh upload_scene of the edited description.  Does not block."""
        torch = _torch()
        if not isinstance(texels, torch.Tensor) or texels.dim() != 3 or texels.shape[2] != 3:
            raise RadishError("set_texture: texels must be a tensor [height, width, 3]")
        h, w = int(texels.shape[0]), int(texels.shape[1])
        self.check(lib().rdh_scene_set_texture(self.h, int(tex_id), self._ptr(texels, 3 * w * h, "set_texture texels"), w, h))

    def env_power(self):
        """The environment entry's power as the scene holds it, np.float32 (rdh_scene_env_power): SceneData.env_power of the scene
        as it stands, also after set_texture changed the environment map.  The env_power argument of a later rebuild_lights,
        set_materials or pose_objects.  Blocking; raises on a scene without an environment map."""
        out = C.c_float(0)
        self.check(lib().rdh_scene_env_power(self.h, C.byref(out)))
        return np.float32(out.value)

    def debug_read_textures(self, which):
        """Blocking test access (rdh_debug_read_textures): 0 -> every texture's texels (float32, upload order), 1 -> the
        environment map's alias table (layouts.BINOMIAL_DTYPE), 2 -> {float32 envPower; int32 envMapTexId, envMapSamplerLength,
        numTextures} as 16 bytes."""
        n = lib().rdh_debug_read_textures(self.h, which, None, 0)
        if n < 0:
            self.check(int(n))
        out = np.zeros(n, np.uint8)
        if n:
            rc = lib().rdh_debug_read_textures(self.h, which, out.ctypes.data, n)
            if rc < 0:
                self.check(int(rc))
        if which == 0:
            return out.view(np.float32)
        return out.view(L.BINOMIAL_DTYPE) if which == 1 else out

    # ---- the lens: depth of field ----
    def set_lens(self, mode, mask_tex_id=-1):
        """How primary rays pick their point on the lens (rdh_set_lens): "off" (the pinhole, the default and the state after
        every upload_scene), "disk" (a round aperture) or "mask" (texture mask_tex_id of the uploaded scene is the aperture's
        shape, e.g. SceneData.aperture_mask_tex_id; its alias table is built on the device in this call, which waits for it
        once).  The camera's lens_radius and focal_dist (hostlib.make_camera) are the aperture's size and the focal plane; with
        lens_radius 0 frames are the pinhole's.  path_trace, path_trace_samples, path_trace_adaptive, path_trace_direct and
        dump_rays follow the lens; the G-buffer and the denoisers do not, and restir_direct raises while a lens is active.  A
        scene file's LensRadius / ApertureMask switch nothing on: the caller does.  The reference-style shim (Camera / pathTrace)
        has no counterpart: the reference leaves its lens dead."""
        if mode not in LENS_MODES:
            raise RadishError(f"set_lens: mode must be one of {sorted(LENS_MODES)}, got {mode!r}")
        self.check(lens_entries()[0](self.h, LENS_MODES[mode], int(mask_tex_id)))

    def debug_primary_rays(self, looper):
        """Test access (rdh_debug_primary_rays): every pixel's primary ray at Sobol row `looper`, a float32 cuda tensor
        [height, width, 6] = {origin, direction}, from the draw and the camera function the tracers use."""
        torch = _torch()
        if getattr(self, "width", None) is None:
            raise RadishError("debug_primary_rays: no camera set")
        w, h = self.width, self.height
        rays = torch.zeros(h, w, 6, dtype=torch.float32, device=f"cuda:{self.device}")
        self.check(lens_entries()[1](self.h, int(looper), rays.data_ptr()))
        return rays

    def debug_read_lens(self):
        """Blocking test access (rdh_debug_read_lens): (mode name, mask texture id, width, height, the mask's alias table as
        layouts.BINOMIAL_DTYPE — empty unless the mode is "mask")."""
        read = lens_entries()[2]
        head = np.zeros(4, np.int32)
        rc = read(self.h, 0, head.ctypes.data, 16)
        if rc < 0:
            self.check(int(rc))
        n = read(self.h, 1, None, 0)
        if n < 0:
            self.check(int(n))
        table = np.zeros(n, np.uint8)
        if n:
            rc = read(self.h, 1, table.ctypes.data, n)
            if rc < 0:
                self.check(int(rc))
        names = {v: k for k, v in LENS_MODES.items()}
        return names[int(head[0])], int(head[1]), int(head[2]), int(head[3]), table.view(L.BINOMIAL_DTYPE)

    # ---- the triangle set replaced on the device ----
    def set_geometry(self, vertices, normals, texcoords, material_ids, builder="sah", env_power=0.0):
        """Replace the uploaded scene's triangles (rdh_scene_set_geometry): vertices / normals float32 cuda tensors of 9*N floats,
        texcoords of 6*N floats, material_ids an int32 cuda tensor [N]; N >= 1 may differ from the uploaded count.  Materials,
        textures, the environment map and the camera stay; the tree is built on the device with `builder`, and the light list and
        sampler are derived again (env_power as for rebuild_lights).  With "sah" the scene then equals, bit for bit, a fresh
        upload_scene of the edited description; with "lbvh" that upload followed by update_geometry(..., builder="lbvh").  The
        object table is dropped (call set_objects again before a pose).  Waits once for the check of the arrays.  The
        reference-style shim (DevScene / Scene) has no counterpart: it uploads."""
        b = _builder("set_geometry", builder)
        torch = _torch()
        if getattr(self, "_num_prims", None) is None:
            raise RadishError("set_geometry: no scene uploaded")
        if not isinstance(material_ids, torch.Tensor) or material_ids.numel() == 0:
            raise RadishError("set_geometry: material_ids must be a tensor of N >= 1 int32")
        n = material_ids.numel()
        for t, name, per in ((vertices, "vertices", 9), (normals, "normals", 9), (texcoords, "texcoords", 6)):
            if not isinstance(t, torch.Tensor) or t.numel() != per * n:
                got = t.numel() if isinstance(t, torch.Tensor) else type(t).__name__
                raise RadishError(f"set_geometry: {name} must hold {per}*{n} floats ({n} material ids), got {got}")
        vp = self._ptr(vertices, 9 * n, "set_geometry vertices")
        np_ = self._ptr(normals, 9 * n, "set_geometry normals")
        tp = self._ptr(texcoords, 6 * n, "set_geometry texcoords")
        ip = self._ptr(material_ids, n, "set_geometry material_ids", torch.int32)
        self.check(lib().rdh_scene_set_geometry(self.h, vp, np_, tp, ip, n, b, float(env_power)))
        self._num_prims = int(n)

    def debug_read_geometry(self, which):
        """Blocking test access (rdh_debug_read_geometry): 0 -> TriRec bytes, 1 -> AttrRec bytes, 2 -> the shading classes (uint8),
        3 -> the per-material triangle counts (int32)."""
        n = lib().rdh_debug_read_geometry(self.h, which, None, 0)
        if n < 0:
            self.check(int(n))
        out = np.zeros(n, np.uint8)
        if n:
            rc = lib().rdh_debug_read_geometry(self.h, which, out.ctypes.data, n)
            if rc < 0:
                self.check(int(rc))
        return out.view(np.int32) if which == 3 else out

    # ---- moving geometry: objects posed on the device ----
    def set_objects(self, sd=None, objects=None, rest_vertices=None, rest_normals=None):
        """The uploaded scene's object table and rest pose (rdh_scene_set_objects): a SceneData from scenes.load_scene_file (its
        .objects / .rest_vertices / .rest_normals), or explicit arrays — objects with fields firstPrim, numPrims, restFirstPrim
        (or an int [n, 3] array in that order), rest_vertices / rest_normals float32 of 9 floats per rest triangle.  An empty
        table clears it.  Blocking."""
        if sd is not None:
            if getattr(sd, "objects", None) is None:
                raise RadishError("set_objects: this SceneData has no object table (only scenes.load_scene_file makes one)")
            objects, rest_vertices, rest_normals = sd.objects, sd.rest_vertices, sd.rest_normals
        if objects is None:
            raise RadishError("set_objects: give a SceneData or objects, rest_vertices and rest_normals")
        objects = np.asarray(objects)
        table = np.zeros(len(objects), OBJECT_RANGE_DTYPE)
        if objects.dtype.names:
            for f in OBJECT_RANGE_DTYPE.names:
                table[f] = objects[f]
        elif len(objects):
            cols = objects.reshape(len(objects), 3)
            for k, f in enumerate(OBJECT_RANGE_DTYPE.names):
                table[f] = cols[:, k]
        if len(table) == 0:
            self.check(lib().rdh_scene_set_objects(self.h, None, 0, None, None, 0))
            return
        if rest_vertices is None or rest_normals is None:
            raise RadishError("set_objects: rest_vertices and rest_normals are needed")
        rv = np.ascontiguousarray(rest_vertices, dtype=np.float32).reshape(-1)
        rn = np.ascontiguousarray(rest_normals, dtype=np.float32).reshape(-1)
        if rv.size % 9 or rv.size != rn.size:
            raise RadishError(f"set_objects: rest_vertices ({rv.size} floats) and rest_normals ({rn.size}) must hold 9 floats per triangle each")
        self.check(lib().rdh_scene_set_objects(self.h, table.ctypes.data, len(table), rv.ctypes.data, rn.ctypes.data, rv.size // 9))

    def pose_objects(self, ids, trs=None, xforms=None, tree="refit", rebuild_lights=False, env_power=0.0):
        """Move the listed objects of the table (rdh_scene_pose_objects).  trs: (count, 9) translate, rotate in degrees, scale —
        turned into matrices by hostlib.object_transform, so that the posed scene holds the floats a scene file with these values
        loads to (a singular transform raises ValueError before any device call); or xforms: (count, 32) float32, X column-major
        then inverse(X), for callers with their own matrices.  tree: "refit" keeps the topology, "sah" / "lbvh" rebuild it.
        rebuild_lights: rebuild the light sampler from the moved emissive triangles (env_power as for rebuild_lights).  Does
        not block in the steady state."""
        if tree not in POSE_TREES:
            raise RadishError(f"pose_objects: tree must be one of {sorted(POSE_TREES)}, got {tree!r}")
        if (trs is None) == (xforms is None):
            raise RadishError("pose_objects: give exactly one of trs and xforms")
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        if trs is not None:
            t = np.asarray(trs, dtype=np.float32).reshape(-1, 9)
            xf = np.stack([hostlib.object_transform(r[0:3], r[3:6], r[6:9]) for r in t]) if len(t) else np.zeros((0, 32), np.float32)
        else:
            xf = np.ascontiguousarray(xforms, dtype=np.float32).reshape(-1, 32)
        if len(xf) != len(ids):
            raise RadishError(f"pose_objects: {len(ids)} ids but {len(xf)} transforms")
        xf = np.ascontiguousarray(xf, dtype=np.float32)
        flags = RDH_POSE_REBUILD_LIGHTS if rebuild_lights else 0
        self.check(lib().rdh_scene_pose_objects(self.h, ids.ctypes.data if len(ids) else None, xf.ctypes.data if len(ids) else None,
                                                len(ids), POSE_TREES[tree], flags, float(env_power)))

    def debug_read_world(self):
        """Blocking test access (rdh_debug_read_world): (vertices, normals), float32 [3*numPrims, 3] each — the world arrays the
        poses write."""
        n = getattr(self, "_num_prims", None)
        if n is None:
            raise RadishError("debug_read_world: no scene uploaded")
        v = np.zeros((3 * n, 3), np.float32)
        nr = np.zeros((3 * n, 3), np.float32)
        self.check(lib().rdh_debug_read_world(self.h, v.ctypes.data, nr.ctypes.data))
        return v, nr

    def set_camera(self, cam):
        buf = np.frombuffer(np.asarray(cam, dtype=L.CAMERA_DTYPE).tobytes(), np.uint8).copy()
        self.check(lib().rdh_set_camera(self.h, buf.ctypes.data))
        self.width, self.height = (int(v) for v in cam["resolution"])

    def set_partition(self, rank, world, tile=64):
        self.check(lib().rdh_set_partition(self.h, rank, world, tile))
        self.rank, self.world, self.tile = rank, world, tile

    def tiles_per_rank(self):
        n = lib().rdh_tiles_per_rank(self.h)
        if n < 0:
            self.check(n)
        return n

    def untile(self, gathered, frame):
        shard = self.tiles_per_rank() * self.tile * self.tile * 3
        self.check(lib().rdh_untile(self.h, self._ptr(gathered, shard * self.world, "untile: gathered"),
                                    self._ptr(frame, self.width * self.height * 3, "untile: frame")))

    # ---- hot path ----
    def path_trace(self, direct, indirect, iter, looper, max_depth, flags=RDH_PT_PERSISTENT):
        n = self._image_elems() if self.width else 0
        self.check(lib().rdh_path_trace(self.h, self._ptr(direct, n, "pathTrace: directIllum"),
                                        self._ptr(indirect, n, "pathTrace: indirectIllum"), iter, looper, max_depth, flags))

    def path_trace_samples(self, direct, indirect, iter, looper, samples, max_depth, flags=RDH_PT_PERSISTENT, samples_per_pass=0):
        """`samples` samples per pixel (rdh_path_trace_samples): the images afterwards are those of path_trace at iter + s, looper
        (looper + s) % 10000 for s = 0..samples-1.  Wavefront: samples_per_pass samples share one pipeline pass (0: the library picks)."""
        n = self._image_elems()
        self.check(lib().rdh_path_trace_samples(self.h, self._ptr(direct, n, "pathTraceSamples: directIllum"),
                                                self._ptr(indirect, n, "pathTraceSamples: indirectIllum"), iter, looper, samples,
                                                samples_per_pass, max_depth, flags))

    # ---- adaptive sampling (rdh_path_trace_adaptive, rdh_adaptive_plan): planes in frame layout ----
    def path_trace_adaptive(self, direct, indirect, counts, requests, looper, max_depth, flags, moments=None):
        """requests[p] more samples of every pixel p (0..16) in one wavefront pass: pixel p's images afterwards are those of path_trace
        at iter counts[p] + j, looper (looper + counts[p] + j) % 10000, j = 0..requests[p]-1; counts[p] grows by requests[p] and the
        moments (float32 [H*W, 2], running means of the samples' luminance and its square; may be None) are folded alike.  Pixels
        without a request are not written.  Returns the samples traced (the plane's sum).  One host synchronisation."""
        torch = _torch()
        px = self.width * self.height
        traced = C.c_int64(0)
        self.check(adaptive_entries()[0](
            self.h, self._ptr(direct, 3 * px, "pathTraceAdaptive: directIllum"), self._ptr(indirect, 3 * px, "pathTraceAdaptive: indirectIllum"),
            self._ptr(counts, px, "pathTraceAdaptive: counts", torch.int32), self._ptr(requests, px, "pathTraceAdaptive: requests", torch.int32),
            None if moments is None else self._ptr(moments, 2 * px, "pathTraceAdaptive: moments"), looper, max_depth, flags,
            C.byref(traced)))
        return int(traced.value)

    def adaptive_plan(self, counts, moments, requests, min_samples, max_samples, step, threshold):
        """Fill requests (int32 [H*W]) from counts and moments (rdh_adaptive_plan): every pixel of an 8x8 block in which some pixel
        has fewer than min_samples samples, or a relative standard error of its mean luminance above threshold, gets
        min(step, max_samples - count), every other pixel 0.  Returns {"samplesRequested", "activeBlocks", "wantingPixels"}."""
        torch = _torch()
        px = self.width * self.height
        st = AdaptiveStatsC()
        self.check(adaptive_entries()[1](
            self.h, self._ptr(counts, px, "adaptivePlan: counts", torch.int32), self._ptr(moments, 2 * px, "adaptivePlan: moments"),
            self._ptr(requests, px, "adaptivePlan: requests", torch.int32), min_samples, max_samples, step, threshold, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in st._fields_}

    def converge(self, direct, indirect, counts, moments, looper, max_depth, flags, min_samples, max_samples, step, threshold, max_passes):
        """Plan and trace in turn, at most max_passes times, until the plan asks for nothing.  Returns the plans' statistics, one dict
        per plan made (the last one has samplesRequested == 0 when the frame has converged within max_passes)."""
        torch = _torch()
        requests = torch.zeros(self.width * self.height, dtype=torch.int32, device=counts.device)
        passes = []
        for _ in range(max_passes):
            passes.append(self.adaptive_plan(counts, moments, requests, min_samples, max_samples, step, threshold))
            if passes[-1]["samplesRequested"] == 0:
                break
            self.path_trace_adaptive(direct, indirect, counts, requests, looper, max_depth, flags, moments=moments)
        return passes

    def path_trace_direct(self, direct, iter, looper, flags=0):
        n = self._image_elems() if self.width else 0
        self.check(lib().rdh_path_trace_direct(self.h, self._ptr(direct, n, "pathTraceDirect: directIllum"), iter, looper, flags))

    def gbuffer_render(self, gb_c, flags=0):
        self.check(lib().rdh_gbuffer_render(self.h, C.byref(gb_c), flags))

    def restir_init(self):
        self.check(lib().rdh_restir_init(self.h))

    def restir_free(self):
        self.check(lib().rdh_restir_free(self.h))

    def restir_direct(self, direct, iter, looper, gb_c, reuse_mask, ris_count=32, num_spatial=5, temporal_clamp=20,
                      faithful_ris=1, flags=0):
        p = RestirParamsC(reuse_mask, ris_count, num_spatial, temporal_clamp, faithful_ris)
        n = self._image_elems() if self.width else 0
        self.check(lib().rdh_restir_direct(self.h, self._ptr(direct, n, "ReSTIRDirect: directIllum"), iter, looper, C.byref(gb_c),
                                           C.byref(p), flags))

    def copy_image_to_pbo(self, pbo, image, width, height, kind=0, tone_mapping=0, scale=1.0):
        torch = _torch()
        n = width * height
        if pbo.numel() * pbo.element_size() < 4 * n or not pbo.is_cuda or not pbo.is_contiguous():
            raise RadishError("copyImageToPBO: PBO must be a contiguous device buffer of 4 bytes per pixel")
        want = {0: (3 * n, torch.float32), 1: (2 * n, torch.float32), 2: (n, torch.float32), 3: (n, torch.int32)}.get(kind)
        if want is None:
            raise RadishError(f"copyImageToPBO: kind {kind}")
        self.check(lib().rdh_copy_image_to_pbo(self.h, pbo.data_ptr(), self._ptr(image, want[0], "copyImageToPBO: image", want[1]),
                                               width, height, kind, tone_mapping, scale))

    # ---- denoisers (src/denoiser.cu) ----
    @staticmethod
    def _cam_buf(cam):
        return np.frombuffer(np.asarray(cam, dtype=L.CAMERA_DTYPE).tobytes(), np.uint8).copy()

    def denoise_eaw(self, color_out, color_in, gb_c, cam, sig_lumin, sig_normal, sig_depth, level):
        cb = self._cam_buf(cam)
        self.check(lib().rdh_denoise_eaw(self.h, color_out.data_ptr(), color_in.data_ptr(), C.byref(gb_c), cb.ctypes.data,
                                         sig_lumin, sig_normal, sig_depth, level))

    def denoise_svgf(self, color_out, color_in, var_out, var_in, var_filtered, gb_c, cam, sig_lumin, sig_normal, sig_depth, level):
        cb = self._cam_buf(cam)
        self.check(lib().rdh_denoise_svgf(self.h, color_out.data_ptr(), color_in.data_ptr(), var_out.data_ptr(), var_in.data_ptr(),
                                          var_filtered.data_ptr(), C.byref(gb_c), cb.ctypes.data, sig_lumin, sig_normal,
                                          sig_depth, level))

    def denoise_modulate(self, image, gb_c):
        self.check(lib().rdh_denoise_modulate(self.h, image.data_ptr(), C.byref(gb_c)))

    def denoise_add(self, out, in1, in2, width, height):
        self.check(lib().rdh_denoise_add(self.h, out.data_ptr(), in1.data_ptr(), in2.data_ptr(), width, height))

    def denoise_temporal_accumulate(self, color_out, color_in_accum, moment_out, moment_in_accum, color_in, gb_c, first):
        self.check(lib().rdh_denoise_temporal_accumulate(self.h, color_out.data_ptr(), color_in_accum.data_ptr(),
                                                         moment_out.data_ptr(), moment_in_accum.data_ptr(),
                                                         color_in.data_ptr(), C.byref(gb_c), 1 if first else 0))

    def denoise_estimate_variance(self, variance, moment, width, height):
        self.check(lib().rdh_denoise_estimate_variance(self.h, variance.data_ptr(), moment.data_ptr(), width, height))

    def denoise_filter_variance(self, var_out, var_in, width, height):
        self.check(lib().rdh_denoise_filter_variance(self.h, var_out.data_ptr(), var_in.data_ptr(), width, height))

    def restir_exchange_pack(self, packed):
        shard = self.tiles_per_rank() * self.tile * self.tile * 9
        self.check(lib().rdh_restir_exchange_pack(self.h, self._ptr(packed, shard, "restir_exchange_pack")))

    def restir_exchange_unpack(self, gathered):
        shard = self.tiles_per_rank() * self.tile * self.tile * 9
        self.check(lib().rdh_restir_exchange_unpack(self.h, self._ptr(gathered, shard * self.world, "restir_exchange_unpack")))

    def gbuffer_exchange_pack(self, gb_c, packed):
        shard = self.tiles_per_rank() * self.tile * self.tile * 9
        self.check(lib().rdh_gbuffer_exchange_pack(self.h, C.byref(gb_c), self._ptr(packed, shard, "gbuffer_exchange_pack")))

    def gbuffer_exchange_unpack(self, gb_c, gathered):
        shard = self.tiles_per_rank() * self.tile * self.tile * 9
        self.check(lib().rdh_gbuffer_exchange_unpack(self.h, C.byref(gb_c), self._ptr(gathered, shard * self.world, "gbuffer_exchange_unpack")))

    # ---- collectives inside the library (RCCL, bound at run time) ----
    @staticmethod
    def comm_unique_id():
        """128 bytes (ncclUniqueId): made on rank 0, handed to every rank's comm_init."""
        buf = (C.c_uint8 * 128)()
        rc = lib().rdh_comm_unique_id(C.cast(buf, C.c_void_p))
        if rc != 0:
            raise RadishError(f"rdh_comm_unique_id failed with code {rc} (RCCL not loadable?)")
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        buf = (C.c_uint8 * 128)(*unique_id)
        self.check(lib().rdh_comm_init(self.h, C.cast(buf, C.c_void_p), rank, world))
        self.rank, self.world = rank, world

    def comm_destroy(self):
        self.check(lib().rdh_comm_destroy(self.h))

    # ---- ONE process, n GPUs: the reference's host model (one frame loop, main.cpp:163-202) ----
    @staticmethod
    def comm_init_all(ctxs):
        """ctxs[i] (one Context per DEVICE) becomes rank i of len(ctxs): rdh_comm_init_all (grouped ncclCommInitRank)."""
        n = len(ctxs)
        arr = (C.c_void_p * n)(*[c.h for c in ctxs])
        rc = lib().rdh_comm_init_all(arr, n)
        if rc != 0:
            ctxs[0].check(rc)
        for i, c in enumerate(ctxs):
            c.rank, c.world = i, n

    @staticmethod
    def path_trace_gathered_all(ctxs, direct_frames, indirect_frames, iter, looper, max_depth, flags=RDH_PT_PERSISTENT):
        """pathTrace on every context of this process (rdh_path_trace_gathered_all): whole-frame images in and out per device."""
        n = len(ctxs)
        arr = (C.c_void_p * n)(*[c.h for c in ctxs])
        px = ctxs[0].width * ctxs[0].height * 3
        d = (C.c_void_p * n)(*[c._ptr(t, px, "path_trace_gathered_all: direct") for c, t in zip(ctxs, direct_frames)])
        i = (C.c_void_p * n)(*[c._ptr(t, px, "path_trace_gathered_all: indirect") for c, t in zip(ctxs, indirect_frames)])
        rc = lib().rdh_path_trace_gathered_all(arr, n, d, i, iter, looper, max_depth, flags)
        if rc != 0:
            msgs = [lib().rdh_last_error(c.h) for c in ctxs]
            raise RadishError(f"libradish_hip error {rc}: " + "; ".join(f"ctx {k}: {m.decode()}" for k, m in enumerate(msgs) if m))

    def allgather_tiles(self, packed, frame):
        shard = self.tiles_per_rank() * self.tile * self.tile * 3
        self.check(lib().rdh_allgather_tiles(self.h, self._ptr(packed, shard, "allgather_tiles: packed"),
                                             self._ptr(frame, self.width * self.height * 3, "allgather_tiles: frame")))

    def path_trace_gathered(self, direct_frame, indirect_frame, iter, looper, max_depth, flags=RDH_PT_PERSISTENT):
        n = self.width * self.height * 3
        self.check(lib().rdh_path_trace_gathered(self.h, self._ptr(direct_frame, n, "path_trace_gathered: direct"),
                                                 self._ptr(indirect_frame, n, "path_trace_gathered: indirect"), iter, looper,
                                                 max_depth, flags))

    def restir_exchange(self):
        self.check(lib().rdh_restir_exchange(self.h))

    def comm_set_overlap(self, enable):
        """ReSTIR's exchanges on a communication stream beside rendering (default on) or on the render stream (off)."""
        self.check(lib().rdh_comm_set_overlap(self.h, 1 if enable else 0))

    def comm_join(self):
        """The render stream waits for the exchanges in flight (before anything else reads G-buffer planes they complete)."""
        self.check(lib().rdh_comm_join(self.h))

    @staticmethod
    def _all_error(ctxs, rc):
        msgs = [lib().rdh_last_error(c.h) for c in ctxs]
        raise RadishError(f"libradish_hip error {rc}: " + "; ".join(f"ctx {k}: {m.decode()}" for k, m in enumerate(msgs) if m))

    @staticmethod
    def gbuffer_exchange_all(ctxs, gb_cs):
        n = len(ctxs)
        arr = (C.c_void_p * n)(*[c.h for c in ctxs])
        gbs = (GBufferC * n)(*gb_cs)
        rc = lib().rdh_gbuffer_exchange_all(arr, n, gbs)
        if rc != 0:
            Context._all_error(ctxs, rc)

    @staticmethod
    def restir_direct_gathered_all(ctxs, direct_frames, iter, looper, gb_cs, reuse_mask, ris_count=32, num_spatial=5, temporal_clamp=20,
                                   faithful_ris=1, flags=0):
        n = len(ctxs)
        arr = (C.c_void_p * n)(*[c.h for c in ctxs])
        px = ctxs[0].width * ctxs[0].height * 3
        d = (C.c_void_p * n)(*[c._ptr(t, px, "restir_direct_gathered_all") for c, t in zip(ctxs, direct_frames)])
        gbs = (GBufferC * n)(*gb_cs)
        p = RestirParamsC(reuse_mask, ris_count, num_spatial, temporal_clamp, faithful_ris)
        rc = lib().rdh_restir_direct_gathered_all(arr, n, d, iter, looper, gbs, C.byref(p), flags)
        if rc != 0:
            Context._all_error(ctxs, rc)

    def restir_direct_gathered(self, direct_frame, iter, looper, gb_c, reuse_mask, ris_count=32, num_spatial=5, temporal_clamp=20,
                               faithful_ris=1, flags=0):
        p = RestirParamsC(reuse_mask, ris_count, num_spatial, temporal_clamp, faithful_ris)
        self.check(lib().rdh_restir_direct_gathered(self.h, self._ptr(direct_frame, self.width * self.height * 3, "restir_direct_gathered"),
                                                    iter, looper, C.byref(gb_c), C.byref(p), flags))

    def gbuffer_exchange(self, gb_c):
        self.check(lib().rdh_gbuffer_exchange(self.h, C.byref(gb_c)))

    def restir_read(self, which):
        out = np.zeros(self.width * self.height, dtype=L.RESERVOIR_DTYPE)
        self.check(lib().rdh_restir_read(self.h, which, out.ctypes.data))
        return out

    def restir_read_scratch(self, which):
        """What the last split pass 1 left per slot: 0 primary rays [slots, 6], 1 shadow segments [slots, 6], 2 the set-aside
        lists as int32 {count[4], primarySlots[256], shadowSlots[256]} (rdh_restir_read_scratch)."""
        nbytes = int(lib().rdh_restir_read_scratch(self.h, which, None, 0))
        if nbytes < 0:
            self.check(nbytes)
        out = np.zeros(nbytes // 4, np.int32 if which == 2 else np.float32)
        got = int(lib().rdh_restir_read_scratch(self.h, which, out.ctypes.data, nbytes))
        if got < 0:
            self.check(got)
        return out if which == 2 else out.reshape(-1, 6)

    def trace_closest(self, rays, hits, flags=RDH_PT_PERSISTENT):  # flags without RDH_PT_PERSISTENT: one lane per ray
        n = rays.numel() // 6  # n == 0 still reaches the library (it returns at once)
        self.check(lib().rdh_trace_closest(self.h, self._ptr(rays, 6 * n, "trace_closest: rays"), n,
                                           self._ptr(hits, 4 * n, "trace_closest: hits", _torch().int32), flags))

    def trace_occluded(self, segments, out, flags=RDH_PT_PERSISTENT):
        n = segments.numel() // 6
        self.check(lib().rdh_trace_occluded(self.h, self._ptr(segments, 6 * n, "trace_occluded: segments"), n,
                                            self._ptr(out, n, "trace_occluded: out", _torch().int32), flags))

    def dump_rays(self, looper, max_depth):
        """The frame's own ray lists (see rdh_dump_rays): (closest rays float32 [n,6], occlusion segments float32 [m,6]) on the device."""
        torch = _torch()
        nc, na = C.c_int64(0), C.c_int64(0)
        self.check(lib().rdh_dump_rays(self.h, looper, max_depth, None, 0, None, 0, C.byref(nc), C.byref(na)))
        dev = torch.device("cuda", self.device)
        closest = torch.zeros(max(nc.value, 1), 6, device=dev)
        segs = torch.zeros(max(na.value, 1), 6, device=dev)
        n2, a2 = C.c_int64(0), C.c_int64(0)
        self.check(lib().rdh_dump_rays(self.h, looper, max_depth, closest.data_ptr(), nc.value, segs.data_ptr(), na.value,
                                       C.byref(n2), C.byref(a2)))
        assert (n2.value, a2.value) == (nc.value, na.value)
        return closest[:nc.value], segs[:na.value]

    def set_occupancy_share(self, share):
        self.check(lib().rdh_set_occupancy_share(self.h, share))

    def counters_reset(self):
        self.check(lib().rdh_counters_reset(self.h))

    def counters(self):
        c = CountersC()
        self.check(lib().rdh_counters_read(self.h, C.byref(c)))
        return c.as_dict()

    def synchronize(self):
        self.check(lib().rdh_synchronize(self.h))

    def profile_reset(self):
        self.check(lib().rdh_profile_reset(self.h))

    def profile_read(self):
        """(total ms, launches) of the traversal-kernel launches made with RDH_PT_PROFILE since the last reset."""
        ms, n = C.c_double(0), C.c_int64(0)
        self.check(lib().rdh_profile_read(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def debug_persist_stamps(self):
        out = np.zeros((5, 4096), dtype=np.uint64)
        self.check(lib().rdh_debug_persist_stamps(self.h, out.ctypes.data))
        return out

    def debug_persist_schedule(self, cost, ema, order, n):
        """k_persist_schedule alone over the caller's arrays (rdh_debug_persist_schedule): cost / ema / order are int32 cuda tensors
        holding the kernel's 32-bit words (torch has no unsigned 32-bit arithmetic; view them), at least n each.  Asynchronous."""
        torch = _torch()
        n = int(n)
        ptrs = [self._ptr(t, max(n, 1), f"debug_persist_schedule {name}", torch.int32) for t, name in ((cost, "cost"), (ema, "ema"), (order, "order"))]
        self.check(persist_entries()[0](self.h, *ptrs, n))

    def debug_persist_read(self):
        """The block-order sequence as it stands (rdh_debug_persist_read; blocking): a dict of frame (persistent launches since the
        last restart), valid, blocks, pending (block count of an order set with debug_persist_set_order, or 0), orders int32
        [2, blocks], costs uint32 [2, blocks], ema uint32 [blocks]."""
        read = persist_entries()[1]
        state = np.zeros(4, np.int32)
        n = read(self.h, state.ctypes.data, None, None, None, 0)
        if n < 0:
            self.check(n)
        orders, costs, ema = np.zeros((2, n), np.int32), np.zeros((2, n), np.uint32), np.zeros(n, np.uint32)
        if n:
            rc = read(self.h, state.ctypes.data, orders.ctypes.data, costs.ctypes.data, ema.ctypes.data, n)
            if rc < 0:
                self.check(rc)
            assert rc == n
        return {"frame": int(state[0]), "valid": bool(state[1]), "blocks": int(state[2]), "pending": int(state[3]),
                "orders": orders, "costs": costs, "ema": ema}

    def debug_persist_set_order(self, order):
        """The next persistent launch, and only that one, visits its blocks in `order` (rdh_debug_persist_set_order): a permutation
        of range(blocks of the current camera and partition).  Raises on anything else, nothing changed."""
        order = np.ascontiguousarray(order, dtype=np.int32).reshape(-1)
        self.check(persist_entries()[2](self.h, order.ctypes.data if len(order) else None, len(order)))

    def debug_wf_stamps(self):
        """uint64 [stages, waves, 6] of the last wavefront pass's trace stages: entry, queue dry, exit, list loop left (100 MHz
        ticks), 1 + the reserved items the wave held unstarted when the shared head was dry, and 1 + the stage's list entries
        (kernels_wave.h, kWfStampKinds): a
        -DRD_WF_STAMPS build of this tree via RADISH_HIP_LIB.  (Bound here, not in lib(): RADISH_HIP_LIB may name a build from
        before this entry.)"""
        fn = lib().rdh_debug_wf_stamps
        fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)], C.c_int32
        stages, waves = C.c_int32(0), C.c_int32(0)
        self.check(fn(self.h, None, 0, C.byref(stages), C.byref(waves)))
        out = np.zeros((stages.value, waves.value, 6), dtype=np.uint64)
        self.check(fn(self.h, out.ctypes.data, out.size, C.byref(stages), C.byref(waves)))
        return out

    def debug_wf_counts(self):
        """(rays, shadows): int32 [maxDepth + 1] each, what the last wavefront pass queued per stage — rays[k] the entries of
        trace(k)'s ray queue, shadows[k] the shadow rays shade(k) queued for trace(k + 1) (include/radish_hip.h).  (Bound here,
        not in lib(): RADISH_HIP_LIB may name a build from before this entry.)"""
        fn = lib().rdh_debug_wf_counts
        fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)], C.c_int32
        stages = C.c_int32(0)
        self.check(fn(self.h, None, None, 0, C.byref(stages)))
        rays, shadows = np.zeros(stages.value, dtype=np.int32), np.zeros(stages.value, dtype=np.int32)
        if stages.value:
            self.check(fn(self.h, rays.ctypes.data, shadows.ctypes.data, stages.value, C.byref(stages)))
        return rays, shadows

    def debug_persist_phases(self):
        out = np.zeros(16, dtype=np.uint64)
        self.check(lib().rdh_debug_persist_phases(self.h, out.ctypes.data))
        return out

    def last_kernel_ms(self):
        ms = C.c_float(0)
        self.check(lib().rdh_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value


# ======================================================================================================================
# The reference's globals and free functions
# ======================================================================================================================
class ReservoirReuse:  # src/common.h:41-48
    NONE, Temporal, Spatial, TemporalSpatial = 0, 1, 2, 3


class Settings:  # src/common.h:50-66, defaults src/common.cpp:3-15
    traceDepth = 0
    useReservoir = True
    reservoirReuse = ReservoirReuse.Temporal
    accumulate = False
    # knobs that exist only here (not in the reference)
    ptFlags = RDH_PT_PERSISTENT  # the fastest pathTrace kernel (RDH_PT_MEGAKERNEL = the reference's one-lane-per-pixel structure)
    restirNumSpatial = 5      # src/restir.cu:87
    restirRISCount = 32       # RESERVOIR_SIZE, src/restir.h:9
    restirTemporalClamp = 20  # src/restir.cu:168
    restirFaithfulRIS = 1     # src/restir.h:21


class State:  # src/common.h:68-72
    camChanged = True
    looper = 0
    scene = None  # a `Scene` below


class DevScene:
    """`DevScene::create/destroy` (src/scene.h:74-75): owns the device copy of a scene (inside an rdh_ctx)."""

    def __init__(self):
        self.ctx = None

    def create(self, scene_data, device=0):
        self.ctx = Context(device)
        self.ctx.upload_scene(scene_data)

    def destroy(self):
        if self.ctx:
            self.ctx.close()
            self.ctx = None


class Scene:
    """The slice of the reference's `Scene` the render API reads: `camera` and `devScene` (src/scene.h:520-577)."""

    def __init__(self, scene_data, camera, device=0):
        self.data = scene_data
        self.camera = camera
        self.devScene = DevScene()
        self.devScene.create(scene_data, device)

    def clear(self):  # Scene::clear (src/scene.cpp:251-254)
        self.devScene.destroy()


def _ctx():
    if State.scene is None or State.scene.devScene.ctx is None:
        raise RadishError("State.scene is not set")
    ctx = State.scene.devScene.ctx
    ctx.set_camera(State.scene.camera)
    return ctx


def _advance_looper():
    State.looper = (State.looper + 1) % SOBOL_SAMPLE_NUM  # src/pathtrace.cu:380-381


def pathTraceInit():  # src/pathtrace.cu:28
    _ctx().synchronize()


def pathTraceFree():  # src/pathtrace.cu:30
    pass


def pathTrace(directIllum, indirectIllum, iter):
    """src/pathtrace.cu:351-385.  Blocking, like the reference (checkCUDAError = device sync)."""
    ctx = _ctx()
    ctx.path_trace(directIllum, indirectIllum, iter, State.looper, Settings.traceDepth, Settings.ptFlags)
    ctx.synchronize()
    _advance_looper()


def pathTraceSamples(directIllum, indirectIllum, iter, samples):
    """`samples` samples per pixel in one call: the images and State.looper afterwards are those of pathTrace at iter,
    iter + 1, ..., iter + samples - 1 (the reference's `accumulate` loop).  Blocking."""
    ctx = _ctx()
    ctx.path_trace_samples(directIllum, indirectIllum, iter, State.looper, samples, Settings.traceDepth, Settings.ptFlags)
    ctx.synchronize()
    State.looper = (State.looper + samples) % SOBOL_SAMPLE_NUM


def pathTraceDirect(directIllum, iter):
    """src/pathtrace.cu:387-407."""
    ctx = _ctx()
    ctx.path_trace_direct(directIllum, iter, State.looper, Settings.ptFlags & RDH_PT_COUNT)
    ctx.synchronize()
    _advance_looper()


class ToneMapping:  # src/common.h:23-25
    NONE, Filmic, ACES = 0, 1, 2


def copyImageToPBO(devPBO, devImage, width, height, toneMapping=ToneMapping.NONE, scale=1.0):
    """copyImageToPBO's four overloads (src/pathtrace.h:25-29, src/pathtrace.cu:120-147), selected the way C++ overload
    resolution does — by the image's element type: float32 [n,3] → vec3 (tone-mapped), float32 [n,2] → vec2, float32 [n] →
    float, int32 [n] → pixel indices.  devPBO: uint8 [n,4]."""
    torch = _torch()
    n = width * height
    if devImage.dtype == torch.int32:
        kind = 3
    elif devImage.dtype == torch.float32:
        kind = {3 * n: 0, 2 * n: 1, n: 2}.get(devImage.numel())
    else:
        kind = None
    if kind is None or devPBO.numel() * devPBO.element_size() != 4 * n:
        raise RadishError("copyImageToPBO: image/PBO shape does not match width*height")
    _ctx().copy_image_to_pbo(devPBO, devImage, width, height, kind, toneMapping, scale)


def ReSTIRInit():  # src/restir.cu:235-245
    _ctx().restir_init()


def ReSTIRFree():  # src/restir.cu:247-251
    if State.scene is not None and State.scene.devScene.ctx is not None:
        State.scene.devScene.ctx.restir_free()


def ReSTIRDirect(directIllum, iter, gBuffer):
    """src/restir.cu:205-233 (swap of the reservoir buffers and the first-frame flag happen inside the library)."""
    ctx = _ctx()
    ctx.restir_direct(directIllum, iter, State.looper, gBuffer.c_struct(), Settings.reservoirReuse,
                      Settings.restirRISCount, Settings.restirNumSpatial, Settings.restirTemporalClamp,
                      Settings.restirFaithfulRIS, Settings.ptFlags & RDH_PT_COUNT)
    ctx.synchronize()
    _advance_looper()


class GBuffer:
    """src/gBuffer.h:15-58.  Planes are torch CUDA tensors; `c_struct()` is the 272-byte reference layout."""

    def __init__(self):
        self.width = self.height = 0
        self.frameIdx = 0
        self.lastCam = None

    def create(self, width, height, device=0):  # src/denoiser.cu:329-344
        torch = _torch()
        n = width * height
        dev = torch.device("cuda", device)
        self.width, self.height = width, height
        self.albedo = torch.zeros(n, 3, dtype=torch.float32, device=dev)
        self.normal = [torch.zeros(n, 3, dtype=torch.float32, device=dev) for _ in range(2)]
        self.motion = torch.zeros(n, dtype=torch.int32, device=dev)
        self.depth = [torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(2)]
        self.primId = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2)]
        self.frameIdx = 0
        self.lastCam = None

    def destroy(self):  # src/denoiser.cu:346-359
        for name in ("albedo", "normal", "motion", "depth", "primId"):
            if hasattr(self, name):
                delattr(self, name)

    def c_struct(self, cam_fallback=None):
        g = GBufferC()
        g.albedo = self.albedo.data_ptr()
        g.normal = (C.c_void_p * 2)(*[t.data_ptr() for t in self.normal])
        g.motion = self.motion.data_ptr()
        g.depth = (C.c_void_p * 2)(*[t.data_ptr() for t in self.depth])
        g.primId = (C.c_void_p * 2)(*[t.data_ptr() for t in self.primId])
        g.frameIdx = self.frameIdx
        last = self.lastCam if self.lastCam is not None else cam_fallback
        if last is not None:
            raw = np.asarray(last, dtype=L.CAMERA_DTYPE).tobytes()
            g.lastCam = (C.c_uint8 * 196)(*raw)
        g.width, g.height = self.width, self.height
        return g

    def render(self, devScene, cam):
        """GBuffer::render (src/gBuffer.cu:83-103).  On the very first frame the reference's lastCam is
        uninitialised memory; here it is defined to be `cam`."""
        ctx = devScene.ctx
        ctx.set_camera(cam)
        ctx.gbuffer_render(self.c_struct(cam_fallback=cam), Settings.ptFlags & RDH_PT_COUNT)
        ctx.synchronize()

    def update(self, cam):  # src/gBuffer.cu:78-81
        self.lastCam = np.asarray(cam, dtype=L.CAMERA_DTYPE).copy()
        self.frameIdx ^= 1


# ======================================================================================================================
# Denoisers: the reference's filter classes (src/denoiser.h:16-77, src/denoiser.cu:388-558) over the rdh_denoise_* entries
# ======================================================================================================================
def modulateAlbedo(devImage, gBuffer):  # src/denoiser.cu:363-371
    _ctx().denoise_modulate(devImage, gBuffer.c_struct())


def addImage(out, in1, in2=None, width=None, height=None):
    """addImage(devImage, in, w, h) and addImage(out, in1, in2, w, h) (src/denoiser.cu:373-386)."""
    if in2 is None or isinstance(in2, int):  # two-image overload: addImage(devImage, in, width, height)
        width, height = (in2, width) if isinstance(in2, int) else (width, height)
        in1, in2 = out, in1
    _ctx().denoise_add(out, in1, in2, width, height)


class EAWaveletFilter:  # src/denoiser.h:16-36
    def __init__(self, width=0, height=0, sigLumin=0.0, sigNormal=0.0, sigDepth=0.0):
        self.width, self.height = width, height
        self.sigLumin, self.sigNormal, self.sigDepth = sigLumin, sigNormal, sigDepth

    def filter(self, colorOut, colorIn, gBuffer, cam, level, varianceOut=None, varianceIn=None, filteredVar=None):
        ctx = _ctx()
        if varianceOut is None:  # src/denoiser.cu:388-397
            ctx.denoise_eaw(colorOut, colorIn, gBuffer.c_struct(), cam, self.sigLumin, self.sigNormal, self.sigDepth, level)
        else:  # src/denoiser.cu:399-409
            ctx.denoise_svgf(colorOut, colorIn, varianceOut, varianceIn, filteredVar, gBuffer.c_struct(), cam, self.sigLumin,
                             self.sigNormal, self.sigDepth, level)


class LeveledEAWFilter:  # src/denoiser.h:38-49, src/denoiser.cu:411-434
    def create(self, width, height, level, device=0):
        torch = _torch()
        self.level = level
        self.waveletFilter = EAWaveletFilter(width, height, 64.0, 0.2, 1.0)
        self.tmpImg = torch.zeros(width * height, 3, device=torch.device("cuda", device))

    def destroy(self):
        self.tmpImg = None

    def filter(self, colorOut, colorIn, gBuffer, cam):
        """Five à-trous passes (levels 0..4, as in the reference, whatever `level` says).  `colorOut` is `glm::vec3 *&` in the
        reference — the result ends up in what was tmpImg; returns the tensor that holds it."""
        f = self.waveletFilter
        f.filter(colorOut, colorIn, gBuffer, cam, 0)
        for lv in (1, 2, 3, 4):
            f.filter(self.tmpImg, colorOut, gBuffer, cam, lv)
            colorOut, self.tmpImg = self.tmpImg, colorOut
        return colorOut


class SpatioTemporalFilter:  # src/denoiser.h:51-77, src/denoiser.cu:436-560
    def create(self, width, height, level, device=0):
        torch = _torch()
        dev = torch.device("cuda", device)
        self.level = level
        self.accumColor = [torch.zeros(width * height, 3, device=dev) for _ in range(2)]
        self.accumMoment = [torch.zeros(width * height, 3, device=dev) for _ in range(2)]
        self.variance = torch.zeros(width * height, device=dev)
        self.waveletFilter = EAWaveletFilter(width, height, 4.0, 128.0, 1.0)
        self.tmpColor = torch.zeros(width * height, 3, device=dev)
        self.tmpVar = torch.zeros(width * height, device=dev)
        self.filteredVar = torch.zeros(width * height, device=dev)
        self.firstTime = True
        self.frameIdx = 0

    def destroy(self):
        self.accumColor = self.accumMoment = self.variance = self.tmpColor = self.tmpVar = self.filteredVar = None

    def temporalAccumulate(self, colorIn, gBuffer):  # :461-485
        f = self.frameIdx
        _ctx().denoise_temporal_accumulate(self.accumColor[f], self.accumColor[f ^ 1], self.accumMoment[f], self.accumMoment[f ^ 1],
                                           colorIn, gBuffer.c_struct(), self.firstTime)
        self.firstTime = False

    def estimateVariance(self):  # :487-509
        w = self.waveletFilter
        _ctx().denoise_estimate_variance(self.variance, self.accumMoment[self.frameIdx], w.width, w.height)

    def filterVariance(self):  # :511-523
        w = self.waveletFilter
        _ctx().denoise_filter_variance(self.filteredVar, self.variance, w.width, w.height)

    def filter(self, colorOut, colorIn, gBuffer, cam):
        """src/denoiser.cu:525-558, swap for swap.  Returns the tensor that holds the result (`colorOut` is `glm::vec3 *&`)."""
        f, w = self.frameIdx, self.waveletFilter
        self.temporalAccumulate(colorIn, gBuffer)
        self.estimateVariance()
        self.filterVariance()
        w.filter(colorOut, self.accumColor[f], gBuffer, cam, 0, self.tmpVar, self.variance, self.filteredVar)
        colorOut, self.accumColor[f] = self.accumColor[f], colorOut
        self.tmpVar, self.variance = self.variance, self.tmpVar
        self.filterVariance()
        w.filter(colorOut, self.accumColor[f], gBuffer, cam, 1, self.tmpVar, self.variance, self.filteredVar)
        self.tmpVar, self.variance = self.variance, self.tmpVar
        for lv in (2, 3, 4):
            self.filterVariance()
            w.filter(self.tmpColor, colorOut, gBuffer, cam, lv, self.tmpVar, self.variance, self.filteredVar)
            self.tmpColor, colorOut = colorOut, self.tmpColor
            self.tmpVar, self.variance = self.variance, self.tmpVar
        return colorOut

    def nextFrame(self):  # :560
        self.frameIdx ^= 1
