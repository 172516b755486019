"""The reference-signature C++ shim, radish_pt_amd/csrc/radish_shim.hpp, RUN on the GPU and held to the oracle by bits.

Every other GPU test goes through the Python mirror (radish_pt_amd/api.py), a second, separately written copy of the shim's host
logic.  Here tests/shim/shim_runner (built by _build.build_shim_runner from tests/shim/ref_decls.h + the shim, in its plain,
RADISH_SHIM_MULTI_GPU and RADISH_SHIM_ONE_PROCESS_GPUS form) executes a plan through the shim's free functions and classes only:
devSceneCreate's scene hand-over, toC's G-buffer copy, the positional ReSTIR parameters, the four State::looper updates, the SVGF
ping-pong, RDH_PT_AUTO, commInit / commInitAll with one GPU, and check()'s exit.  Each test writes its inputs under tmp_path, starts
ONE child, replays the same plan on the CPU oracle (Replay below) and compares every dump bit for bit and State::looper after every
step.  The child never loads the oracle.

A child that ends on a signal or its time limit stops the file: every later test fails at once without starting another child.
RADISH_SHIM_RUNNER_DIR selects scratch binaries (build_shim_runner(out_dir=, shim=)) built against a changed copy of the header,
to show that these tests can fail.
"""
import functools
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300  # seconds (the convention of test_gpu_samples_subframes.py); a child takes a few: start-up, upload, small frames
_child_ended_badly = None  # why, once a child has ended on a signal or its time limit: no further child is started


# ---------------------------------------------------------------------------------------------------------------------
# The runner binaries and the child's environment
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runners():
    from radish_pt_amd import _build

    scratch = os.environ.get("RADISH_SHIM_RUNNER_DIR")
    where = scratch or os.path.dirname(_build.SHIM_RUNNER_SOURCE)
    paths = {name: os.path.join(where, name) for name in _build.SHIM_RUNNER_FORMS}
    if not scratch:
        if os.path.exists(_build.HIPCC) or shutil.which("hipcc"):
            _build.build_shim_runner()  # a no-op when the binaries are current
        elif not all(os.path.exists(p) for p in paths.values()):
            pytest.fail(f"the shim runner binaries are missing from {where} and there is no hipcc to build them: run build() "
                        "(radish_pt_amd._build.build_shim_runner) where hipcc is installed")
    missing = [p for p in paths.values() if not os.path.exists(p)]
    if missing:
        pytest.fail(f"shim runner binaries missing: {missing}")
    return paths


def _needed_hip_soname(runner):
    with open(runner, "rb") as f:
        names = set(re.findall(rb"libamdhip64\.so(?:\.\d+)*(?=\x00)", f.read()))
    assert len(names) == 1, f"{runner}: expected one libamdhip64 name in its dynamic strings, found {names}"
    return names.pop().decode()


def child_env(tmp_path, runner):
    """Exactly one HIP runtime in the child, and the RCCL that was built against it.  libradish_hip.so and the runner carry a
    RUNPATH (not RPATH), so LD_LIBRARY_PATH decides.  When torch ships libamdhip64.so and librccl.so, the child gets torch's pair,
    the runtime every other GPU test runs on: torch's file is named libamdhip64.so but the runner needs its SONAME
    (libamdhip64.so.N), so the directory alone would not be searched successfully and the RUNPATH's copy would load, and torch's
    librccl.so (NEEDED libamdhip64.so, RPATH $ORIGIN) would then bring torch's runtime in as a SECOND one.  A link named by the
    SONAME, first on LD_LIBRARY_PATH, makes the runner load torch's file; librccl.so's own request then resolves to the same
    file, which the loader recognises.  Without torch's pair nothing is set: the RUNPATH's runtime, and the librccl.so.1 found
    the same way."""
    env = {k: v for k, v in os.environ.items() if k not in ("RADISH_RCCL_LIB", "RADISH_HIP_LIB")}
    spec = importlib.util.find_spec("torch")
    lib_dir = os.path.join(list(spec.submodule_search_locations)[0], "lib") if spec and spec.submodule_search_locations else ""
    hip, rccl = os.path.join(lib_dir, "libamdhip64.so"), os.path.join(lib_dir, "librccl.so")
    if lib_dir and os.path.exists(hip) and os.path.exists(rccl):
        links = tmp_path / "hip_runtime"
        links.mkdir(exist_ok=True)
        link = links / _needed_hip_soname(runner)
        if not link.exists():
            link.symlink_to(hip)
        env["LD_LIBRARY_PATH"] = os.pathsep.join([str(links), lib_dir] + [p for p in env.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p])
        env["RADISH_RCCL_LIB"] = rccl
    return env


def run_child(tmp_path, runner, plan, expect_status=0):
    """Write the plan, run ONE child, return (looper log [(step name, looper)], loaded objects {tag: [real paths]}, result)."""
    global _child_ended_badly
    if _child_ended_badly:
        pytest.fail(f"an earlier runner child ended abnormally ({_child_ended_badly}); no further child is started")
    (tmp_path / "plan.txt").write_text("".join(" ".join(str(t) for t in step) + "\n" for step in plan))
    try:
        r = subprocess.run([runner, str(tmp_path)], env=child_env(tmp_path, runner), cwd=ROOT, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _child_ended_badly = f"time limit of {CHILD_TIMEOUT} s"
        pytest.fail(f"runner child exceeded {CHILD_TIMEOUT} s")
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _child_ended_badly = f"exit status {r.returncode}"
    assert r.returncode == expect_status, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    steps, loaded = [], {}
    for line in (tmp_path / "log.txt").read_text().splitlines():
        w = line.split()
        if w[0] == "loaded":
            loaded.setdefault(w[1], []).append(os.path.realpath(w[2]))
        elif w[0] == "step":
            steps.append((w[2], int(w[4])))
    hip = {p for paths in loaded.values() for p in paths if "amdhip64" in os.path.basename(p)}
    assert len(hip) == 1, f"the child must hold exactly one HIP runtime, it loaded {loaded}"
    print(f"child loaded {loaded}")
    return steps, loaded, r


# ---------------------------------------------------------------------------------------------------------------------
# Inputs
# ---------------------------------------------------------------------------------------------------------------------
def write_inputs(tmp_path, sd, cams):
    from radish_pt_amd import hostlib, layouts as L

    def put(name, a, dtype):
        np.ascontiguousarray(a, dtype=dtype).tofile(tmp_path / name)

    put("vertices.bin", sd.vertices, "<f4")
    put("normals.bin", sd.normals, "<f4")
    put("texcoords.bin", sd.texcoords, "<f4")
    put("material_ids.bin", sd.material_ids, "<i4")
    put("materials.bin", sd.materials, L.MATERIAL_DTYPE)
    put("boxes.bin", sd.boxes, "<f4")
    for k in range(6):
        put(f"nodes{k}.bin", sd.nodes[k], L.MTBVH_NODE_DTYPE)
    put("light_ids.bin", sd.light_prim_ids, "<i4")
    put("light_radiance.bin", sd.light_unit_radiance, "<f4")
    put("light_sampler.bin", sd.light_sampler, L.BINOMIAL_DTYPE)
    # Scene::lightSampler.sum, from which the shim computes 1.f / sum (SceneData keeps only the reciprocal)
    power = sd.light_power if sd.env_map_tex_id < 0 else np.concatenate([sd.light_power, [sd.env_power]]).astype(np.float32)
    light_sum = hostlib.build_alias_table(power)[1] if len(power) else np.float32(0)
    if len(power):
        assert np.float32(1.0) / light_sum == sd.sum_light_power_inv
    put("light_sum.bin", [light_sum], "<f4")
    put("env_sampler.bin", sd.env_map_sampler, L.BINOMIAL_DTYPE)
    put("env_map_tex_id.bin", [sd.env_map_tex_id], "<i4")
    put("texture_sizes.bin", [[t.shape[1], t.shape[0]] for t in sd.textures], "<i4")
    for k, t in enumerate(sd.textures):
        put(f"texture_{k}.bin", t, "<f4")
    put("sobol.bin", sd.sobol, "<u4")
    put("cameras.bin", np.array(cams, dtype=L.CAMERA_DTYPE), L.CAMERA_DTYPE)
    return light_sum


@functools.lru_cache(maxsize=None)
def teapots_scene():
    from radish_pt_amd import scenes

    return scenes.teapots(segments=12, bands=8, grid=2, emissive_grid=(4, 8))


def degenerate_scene(case):
    """The scenes of test_gpu_parity.py::test_degenerate_scenes_bit_exact."""
    from radish_pt_amd import layouts as L, scenes

    white = L.make_material(L.LAMBERTIAN, (0.8, 0.7, 0.6))
    lamp = L.make_material(L.LIGHT, (6.0, 5.0, 4.0))
    tri = np.array([[-1, 0, 0], [1, 0, 0], [0, 1.5, 0]], np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (3, 1))
    uv = np.array([[0, 0], [1, 0], [0, 1]], np.float32)
    if case == "one_triangle":
        v, n, t, ids, mats = tri, nrm, uv, [0], [white]
    else:
        quad = np.array([[-2, -0.5, -2], [2, -0.5, -2], [2, -0.5, 2], [-2, -0.5, -2], [2, -0.5, 2], [-2, -0.5, 2]], np.float32)
        v = np.concatenate([tri, tri + np.array([0.3, 0.2, -0.7], np.float32), quad])
        n = np.concatenate([nrm, nrm, np.tile(np.array([0, 1, 0], np.float32), (6, 1))])
        t = np.concatenate([uv, uv, uv, uv])
        ids = [0, 0, 0, 0] if case == "no_lights" else [1, 1, 1, 1]
        mats = [white, lamp]
    return scenes.SceneData(case, v, n, t, np.array(ids, np.int32), np.array(mats, dtype=L.MATERIAL_DTYPE))


# ---------------------------------------------------------------------------------------------------------------------
# The same plan on the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------
class Replay:
    """Executes a plan on oracle/pyoracle.py the way test_mirror_frame_loop_like_runCuda and test_denoisers_bit_exact drive it.
    Buffers are values here (uint8 arrays viewed as the step needs them); the runner's are pointer variables the shim swaps."""

    def __init__(self, tmp_path, sd, cams):
        from oracle import pyoracle

        self.po, self.dir, self.sd, self.cams = pyoracle, tmp_path, sd, cams
        self.o = pyoracle.OracleScene(sd)
        self.cam, self.depth, self.reuse, self.looper = cams[0], 0, 0, 0
        self.b, self.dumps, self.steps = {}, {}, []
        self.gb = None

    def f32(self, name, cols):
        a = self.b[name].view(np.float32)
        return a if cols == 1 else a.reshape(-1, cols)

    def put(self, name, a):
        self.b[name] = np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()

    def advance(self, n=1):
        self.looper = (self.looper + n) % 10000  # src/pathtrace.cu:380-381

    def run(self, plan):
        for step in plan:
            getattr(self, "do_" + step[0])(*step[1:])
            self.steps.append((step[0], self.looper))
        return self

    def do_alloc(self, name, nbytes):
        self.b[name] = np.zeros(nbytes, np.uint8)

    def do_load(self, name, file):
        self.b[name] = np.fromfile(self.dir / file, np.uint8)

    def do_camera(self, k):
        self.cam = self.cams[k]

    def do_depth(self, n):
        self.depth = n

    def do_reuse(self, n):
        self.reuse = n

    def do_looper(self, n):
        self.looper = n

    def do_gbuffer_create(self, w, h):
        self.gb = self.po.GBufferHost(w, h)
        self.gb.lastCam = self.cams[0].copy()

    def do_gbuffer_render(self):
        self.o.gbuffer_render(self.cam, self.gb)

    def do_gbuffer_update(self):
        self.gb.update(self.cam)

    def do_gbuffer_destroy(self):
        pass

    def do_restir_init(self):
        from radish_pt_amd import layouts as L

        w, h = (int(v) for v in self.cam["resolution"])
        self.res = [np.zeros(w * h, L.RESERVOIR_DTYPE) for _ in range(3)]
        self.restir_first = True

    def do_restir_direct(self, img, it):
        # the shim's fixed parameters: RESERVOIR_SIZE 32, 5 spatial neighbours, the reference's (faithful) Reservoir::update
        self.o.restir_direct(self.cam, self.f32(img, 3), it, self.looper, self.res[0], self.res[1], self.res[2], self.gb,
                             self.restir_first, self.reuse, 1, 5, 32)
        self.res[0], self.res[1] = self.res[1], self.res[0]
        self.restir_first = False
        self.advance()

    def do_restir_free(self):
        pass

    def do_path_trace_init(self):
        pass

    def do_path_trace_free(self):
        pass

    def do_path_trace(self, d, i, it):
        self.o.path_trace(self.cam, self.f32(d, 3), self.f32(i, 3), it, self.looper, self.depth)
        self.advance()

    def do_path_trace_samples(self, d, i, it, samples):
        for s in range(samples):  # the reference's `accumulate` loop: one pathTrace per sample
            self.o.path_trace(self.cam, self.f32(d, 3), self.f32(i, 3), it + s, (self.looper + s) % 10000, self.depth)
        self.advance(samples)

    def do_path_trace_direct(self, d, it):
        self.o.path_trace_direct(self.cam, self.f32(d, 3), it, self.looper)
        self.advance()

    def do_pbo_vec3(self, pbo, img, w, h, tone, scale):
        self.put(pbo, self.po.copy_image_to_pbo(self.f32(img, 3), w, h, 0, tone, float(np.float32(scale))))  # the plan carries 9 digits

    def do_pbo_vec3_default_scale(self, pbo, img, w, h, tone):
        self.do_pbo_vec3(pbo, img, w, h, tone, 1.0)

    def do_pbo_vec2(self, pbo, img, w, h):
        self.put(pbo, self.po.copy_image_to_pbo(self.f32(img, 2), w, h, 1))

    def do_pbo_float(self, pbo, img, w, h):
        self.put(pbo, self.po.copy_image_to_pbo(self.f32(img, 1), w, h, 2))

    def do_pbo_int(self, pbo, img, w, h):
        self.put(pbo, self.po.copy_image_to_pbo(self.b[img].view(np.int32), w, h, 3))

    def do_eaw_create(self, w, h):
        pass

    def do_eaw_filter(self, out, inp):  # LeveledEAWFilter::filter: five a-trous levels (denoiser.cu:419-434), sigmas of ::create
        ref = self.po.denoise_eaw(self.f32(inp, 3), self.gb, self.cam, 64.0, 0.2, 1.0, 0)
        for lv in (1, 2, 3, 4):
            ref = self.po.denoise_eaw(ref, self.gb, self.cam, 64.0, 0.2, 1.0, lv)
        self.put(out, ref)

    def do_eaw_destroy(self):
        pass

    def do_svgf_create(self, w, h):
        n = w * h
        self.accC = [np.zeros((n, 3), np.float32) for _ in range(2)]
        self.accM = [np.zeros((n, 3), np.float32) for _ in range(2)]
        self.svgf_first, self.fidx, self.var = True, 0, np.zeros(n, np.float32)

    def do_svgf_filter(self, out, inp):  # SpatioTemporalFilter::filter (denoiser.cu:525-558)
        po, gb, cam, f = self.po, self.gb, self.cam, self.fidx
        W, H = gb.width, gb.height
        noisy = self.f32(inp, 3)
        self.accC[f], self.accM[f] = po.denoise_temporal_accumulate(self.accC[f ^ 1], self.accM[f ^ 1], noisy, gb, self.svgf_first)
        self.svgf_first = False
        var = po.denoise_estimate_variance(self.accM[f], W, H)
        fvar = po.denoise_filter_variance(var, W, H)
        color, var = po.denoise_svgf(self.accC[f], var, fvar, gb, cam, 4.0, 128.0, 1.0, 0)
        color, self.accC[f] = self.accC[f], color  # std::swap(colorOut, accumColor[frameIdx]): level 0 feeds next frame's history
        fvar = po.denoise_filter_variance(var, W, H)
        color, var = po.denoise_svgf(self.accC[f], var, fvar, gb, cam, 4.0, 128.0, 1.0, 1)
        for lv in (2, 3, 4):
            fvar = po.denoise_filter_variance(var, W, H)
            color, var = po.denoise_svgf(color, var, fvar, gb, cam, 4.0, 128.0, 1.0, lv)
        self.var = var
        self.put(out, color)

    def do_svgf_next_frame(self):
        self.fidx ^= 1

    def do_svgf_destroy(self):
        pass

    def do_modulate(self, img):
        self.put(img, self.po.denoise_modulate(self.f32(img, 3), self.gb))

    def do_add2(self, img, inp, w, h):
        self.put(img, self.po.denoise_add(self.f32(img, 3), self.f32(inp, 3), w, h))

    def do_add3(self, out, in1, in2, w, h):
        self.put(out, self.po.denoise_add(self.f32(in1, 3), self.f32(in2, 3), w, h))

    def do_dump(self, what, file):
        gb = self.gb
        if what.startswith("gb."):
            a = getattr(gb, what[3:-1])[int(what[-1])] if what[-1] in "01" else getattr(gb, what[3:])
        elif what == "svgf.variance":
            a = self.var
        elif what == "svgf.accumColor":
            a = self.accC[self.fidx]
        else:
            a = self.b[what]
        self.dumps[file] = np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()

    def do_scene_destroy(self):
        pass


def compare(tmp_path, replay, steps):
    """Every dump against the oracle's (float files bit for bit with the first difference named, the rest as bytes), and the looper log."""
    assert replay.dumps, "the plan dumps nothing"
    for file, want in replay.dumps.items():
        got = np.fromfile(tmp_path / file, np.uint8)
        assert got.size == want.size, f"{file}: {got.size} bytes, the oracle has {want.size}"
        if file.endswith(".f32"):
            assert_bit_equal(got.view(np.float32), want.view(np.float32), file)
        else:
            assert np.array_equal(got, want), f"{file}: {(got != want).sum()} of {got.size} bytes differ"
    assert steps == replay.steps, f"State::looper after each step: the shim's {steps}, expected {replay.steps}"


def f32(replay, file, cols=3):
    a = replay.dumps[file].view(np.float32)
    return a if cols == 1 else a.reshape(-1, cols)


def dump_gbuffer(plan, cur, tag):
    for plane, ext in (("albedo", "f32"), (f"normal{cur}", "f32"), (f"depth{cur}", "f32"), (f"primId{cur}", "i32"), ("motion", "i32")):
        plan.append(("dump", "gb." + plane, f"{tag}_{plane.rstrip('01')}.{ext}"))


def assert_gbuffer_hits_and_misses(replay, tag):
    prim = replay.dumps[f"{tag}_primId.i32"].view(np.int32)
    assert (prim != -1).any() and (prim == -1).any(), "the G-buffer should hold hits (a material id, -2 for a light) and misses (-1)"


def animated_camera(W, H, f):  # Settings::animateCamera of test_mirror_frame_loop_like_runCuda: the eye moves, then Camera::update
    from radish_pt_amd import hostlib

    return hostlib.make_camera(W, H, eye=(0.3 + 0.06 * np.cos(0.4 * f), 1.9, 7.4 + 0.06 * np.sin(0.4 * f)), rotation=(-91.5, -11.0, 0.0),
                               fovy=19.0)


# ---------------------------------------------------------------------------------------------------------------------
# 1. The frame loop, across the Sobol table's wrap
# ---------------------------------------------------------------------------------------------------------------------
def test_frame_loop_with_looper_wrap(runners, tmp_path):
    """runCuda's loop (src/main.cpp:163-202) through the shim: per frame camera, GBuffer::render, one of ReSTIRDirect
    (TemporalSpatial) / pathTraceDirect / pathTrace / pathTraceSamples(iter, 3) / ReSTIRDirect, the ACES preview, GBuffer::update.
    State::looper starts at 9998: ReSTIR runs on row 9998, pathTraceDirect on the table's LAST row 9999 and takes the looper
    9999 -> 0; the looper is then set back to 9999 so that the batch of three samples starts on the last row and spans the wrap
    (rows 9999, 0, 1), after which the looper must stand at 2.

    Row 9999 is the end of the 10000 x 200 table, so nothing on it may draw past column 199: ReSTIR with the shim's fixed 32
    candidates and 5 neighbours draws, by rdh_restir_direct's own count, 4 + 32*5 + 1 + 1 + (5*3 + 1) = 182 numbers, and pathTrace at
    depth 3 draws 4 + 7*3 = 25.  The depth on that row must stay that small."""
    sd = teapots_scene()
    W, H = 56, 40
    n = W * H
    modes = ("restir", "direct", "pt", "samples", "restir")
    cams = [animated_camera(W, H, f) for f in range(len(modes))]
    write_inputs(tmp_path, sd, cams)
    plan = [("alloc", "direct", 12 * n), ("alloc", "indirect", 12 * n), ("alloc", "pbo", 4 * n), ("depth", 3), ("reuse", 3),
            ("looper", 9998), ("path_trace_init",), ("restir_init",), ("gbuffer_create", W, H)]
    for f, mode in enumerate(modes):
        plan += [("camera", f), ("gbuffer_render",)]
        if mode == "restir":
            plan.append(("restir_direct", "direct", 0))
        elif mode == "direct":
            plan.append(("path_trace_direct", "direct", 0))
        elif mode == "pt":
            plan.append(("path_trace", "direct", "indirect", 0))
        else:
            plan += [("looper", 9999), ("path_trace_samples", "direct", "indirect", 0, 3)]
        plan.append(("dump", "direct", f"frame{f}_direct.f32"))
        if mode in ("pt", "samples"):
            plan.append(("dump", "indirect", f"frame{f}_indirect.f32"))
        plan += [("pbo_vec3_default_scale", "pbo", "direct", W, H, 2), ("dump", "pbo", f"frame{f}_preview.u8"), ("gbuffer_update",)]
    plan += [("restir_free",), ("path_trace_free",), ("gbuffer_destroy",), ("scene_destroy",)]
    steps, _, _ = run_child(tmp_path, runners["shim_runner"], plan)
    rp = Replay(tmp_path, sd, cams).run(plan)
    loopers = [l for _, l in rp.steps]
    assert 9999 in loopers and loopers[loopers.index(9999) + 1:].count(0) > 0 and loopers[-1] == 3  # 9998 .. 9999 -> 0 .. 9999 -> 2 -> 3
    assert dict(rp.steps)["path_trace_samples"] == 2
    for f in range(len(modes)):  # lit pixels in every frame and every preview
        assert (f32(rp, f"frame{f}_direct.f32") > 0).mean() > 0.2 and rp.dumps[f"frame{f}_preview.u8"].max() > 50, f
    assert f32(rp, "frame2_indirect.f32").max() > 0 and f32(rp, "frame3_indirect.f32").max() > 0
    compare(tmp_path, rp, steps)


# ---------------------------------------------------------------------------------------------------------------------
# 2. Textures and the environment map through devSceneCreate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [True, False])
def test_textures_and_environment_map(runners, tmp_path, env):
    """devSceneCreate's texture table (width, height, texels per Image), envMapTexId, the environment sampler and
    sumLightPowerInv = 1.f / sum with the environment entry last in the light sampler; the vertex normals matter to every
    shaded pixel and the G-buffer's normal plane.  Two pathTrace iterations at depth 5, then a G-buffer and two ReSTIR frames."""
    from radish_pt_amd import scenes

    sd = scenes.cornell_textured(segments=12, bands=8, env=env)
    W, H = 56, 40
    n = W * H
    cams = [scenes.cornell_camera(W, H)]
    write_inputs(tmp_path, sd, cams)
    assert len(sd.textures) == (5 if env else 4) and sd.env_map_tex_id == (4 if env else -1)
    assert len(sd.light_sampler) == sd.num_lights + (1 if env else 0) and len(sd.env_map_sampler) == (64 * 32 if env else 0)
    plan = [("alloc", "direct", 12 * n), ("alloc", "indirect", 12 * n), ("alloc", "restir", 12 * n), ("depth", 5), ("looper", 60),
            ("path_trace", "direct", "indirect", 0), ("path_trace", "direct", "indirect", 1),
            ("dump", "direct", "pt_direct.f32"), ("dump", "indirect", "pt_indirect.f32"),
            ("reuse", 3), ("looper", 80), ("restir_init",), ("gbuffer_create", W, H)]
    for f in range(2):
        plan.append(("gbuffer_render",))
        dump_gbuffer(plan, f & 1, f"gb{f}")
        plan += [("restir_direct", "restir", 0), ("dump", "restir", f"restir{f}.f32"), ("gbuffer_update",)]
    plan += [("restir_free",), ("gbuffer_destroy",), ("scene_destroy",)]
    steps, _, _ = run_child(tmp_path, runners["shim_runner"], plan)
    rp = Replay(tmp_path, sd, cams).run(plan)
    assert (f32(rp, "pt_direct.f32") > 0).mean() > 0.3 and f32(rp, "pt_indirect.f32").max() > 0
    assert (f32(rp, "restir0.f32") > 0).mean() > 0.2 and (f32(rp, "restir1.f32") > 0).mean() > 0.2
    assert_gbuffer_hits_and_misses(rp, "gb0")
    if env:
        assert f32(rp, "pt_direct.f32")[0].max() > 0  # the corner pixel misses the box and sees the environment map
    compare(tmp_path, rp, steps)


# ---------------------------------------------------------------------------------------------------------------------
# 3. Degenerate scenes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["one_triangle", "no_lights", "only_lights"])
def test_degenerate_scenes(runners, tmp_path, case):
    """A single triangle, a scene without emitters, a scene of emitters only.  Without emitters Scene::lightSampler.sum is 0 and the
    shim hands over sumLightPowerInv = 1.f / 0 = inf, as the reference does (src/scene.cpp:527), where the mirror and the oracle
    are given 0: the device code reads the value only behind lightSamplerLength != 0 (pickLightPoint's callers, kernels_pt.h /
    path_step.h / kernels_restir.h / lights.h:128), with an environment map, or on a hit of a Light material, none of which
    exists in such a scene, so the results must be equal."""
    from radish_pt_amd import hostlib

    sd = degenerate_scene(case)
    W, H = 40, 24
    n = W * H
    cams = [hostlib.make_camera(W, H, eye=(0.1, 0.6, 4.0), rotation=(-90.0, 0.0, 0.0), fovy=19.5)]
    light_sum = write_inputs(tmp_path, sd, cams)
    if case != "only_lights":
        assert sd.num_lights == 0 and light_sum == 0 and sd.sum_light_power_inv == 0  # the shim sends 1.f / 0, the oracle gets 0
    plan = [("alloc", "direct", 12 * n), ("alloc", "indirect", 12 * n), ("alloc", "dd", 12 * n), ("alloc", "restir", 12 * n),
            ("depth", 4), ("looper", 3), ("path_trace", "direct", "indirect", 0), ("path_trace", "direct", "indirect", 1),
            ("dump", "direct", "pt_direct.f32"), ("dump", "indirect", "pt_indirect.f32"),
            ("looper", 11), ("path_trace_direct", "dd", 0), ("dump", "dd", "direct_only.f32"),
            ("reuse", 3), ("looper", 20), ("restir_init",), ("gbuffer_create", W, H)]
    for f in range(2):
        plan.append(("gbuffer_render",))
        dump_gbuffer(plan, f & 1, f"gb{f}")
        plan += [("restir_direct", "restir", 0), ("dump", "restir", f"restir{f}.f32"), ("gbuffer_update",)]
    plan += [("restir_free",), ("gbuffer_destroy",), ("scene_destroy",)]
    steps, _, _ = run_child(tmp_path, runners["shim_runner"], plan)
    rp = Replay(tmp_path, sd, cams).run(plan)
    assert_gbuffer_hits_and_misses(rp, "gb0")
    if case == "only_lights":
        assert (f32(rp, "pt_direct.f32") > 0).any() and (f32(rp, "restir0.f32") > 0).any()
    else:  # nothing emits: every image is black, and the albedo plane shows that the triangles were hit
        assert f32(rp, "gb0_albedo.f32").max() > 0
    compare(tmp_path, rp, steps)


# ---------------------------------------------------------------------------------------------------------------------
# 4. The denoiser classes
# ---------------------------------------------------------------------------------------------------------------------
def test_denoiser_classes(runners, tmp_path):
    """LeveledEAWFilter::filter, SpatioTemporalFilter::filter + nextFrame (the swap-for-swap ping-pong of colorOut / accumColor,
    tmpVar / variance, tmpColor / colorOut and frameIdx ^ 1), modulateAlbedo and both addImage overloads over three frames: the
    scene, 70 x 45 size, cameras and seeded noisy input with fireflies of test_denoisers_bit_exact.  colorOut is a pointer the
    shim swaps; what it points to afterwards is dumped, with the filter's variance and accumColor[frameIdx]."""
    from radish_pt_amd import hostlib

    sd = teapots_scene()
    W, H = 70, 45  # not multiples of the 32x8 workgroup footprint
    n = W * H
    cams = [hostlib.make_camera(W, H, eye=(0.3 + 0.07 * f, 1.9, 7.4), rotation=(-91.5, -11.0, 0.0), fovy=19.0) for f in range(3)]
    write_inputs(tmp_path, sd, cams)
    rng = np.random.default_rng(2)
    noisy = []
    for f in range(3):
        a = (rng.random((n, 3)).astype(np.float32) ** 2) * 2.0
        a[rng.integers(0, n, 5)] = 40.0  # fireflies
        a.tofile(tmp_path / f"noisy{f}.f32")
        noisy.append(a)
    plan = [("alloc", "eaw_out", 12 * n), ("alloc", "svgf_out", 12 * n), ("alloc", "sum3", 12 * n), ("gbuffer_create", W, H),
            ("eaw_create", W, H), ("svgf_create", W, H)]
    for f in range(3):
        plan += [("camera", f), ("gbuffer_render",), ("load", f"noisy{f}", f"noisy{f}.f32"),
                 ("eaw_filter", "eaw_out", f"noisy{f}"), ("dump", "eaw_out", f"eaw{f}.f32"),
                 ("svgf_filter", "svgf_out", f"noisy{f}"), ("dump", "svgf_out", f"svgf{f}.f32"),
                 ("dump", "svgf.variance", f"variance{f}.f32"), ("dump", "svgf.accumColor", f"accum{f}.f32"), ("svgf_next_frame",),
                 ("modulate", "svgf_out"), ("dump", "svgf_out", f"modulated{f}.f32"),
                 ("add2", "svgf_out", f"noisy{f}", W, H), ("dump", "svgf_out", f"add2_{f}.f32"),
                 ("add3", "sum3", "svgf_out", f"noisy{f}", W, H), ("dump", "sum3", f"add3_{f}.f32"), ("gbuffer_update",)]
    plan += [("eaw_destroy",), ("svgf_destroy",), ("gbuffer_destroy",), ("scene_destroy",)]
    steps, _, _ = run_child(tmp_path, runners["shim_runner"], plan)
    rp = Replay(tmp_path, sd, cams).run(plan)
    for f in range(3):  # the filters really changed the input, the history really changes the result, nothing is trivial
        for name in ("eaw", "svgf"):
            out = f32(rp, f"{name}{f}.f32")
            assert np.isfinite(out).all() and np.abs(out - noisy[f]).max() > 0.1, (name, f)
        assert f32(rp, f"variance{f}.f32", 1).max() > 0 and not np.array_equal(f32(rp, f"accum{f}.f32"), noisy[f])
        assert not np.array_equal(f32(rp, f"modulated{f}.f32"), f32(rp, f"svgf{f}.f32"))
        assert not np.array_equal(f32(rp, f"add3_{f}.f32"), f32(rp, f"add2_{f}.f32"))
    assert not np.array_equal(f32(rp, "accum1.f32"), f32(rp, "accum0.f32"))
    compare(tmp_path, rp, steps)


# ---------------------------------------------------------------------------------------------------------------------
# 5. copyImageToPBO's four overloads
# ---------------------------------------------------------------------------------------------------------------------
def test_copy_image_to_pbo_overloads(runners, tmp_path):
    """vec3 (tone maps 0 / 1 / 2, an explicit scale and the default argument), vec2, float and int at 37 x 29, with the
    special-value rows of test_copy_image_to_pbo_bit_exact; every overload writes over a PBO preset to 77."""
    from radish_pt_amd import hostlib

    sd = degenerate_scene("one_triangle")  # the shim's context comes with a scene
    W, H = 37, 29
    n = W * H
    cams = [hostlib.make_camera(W, H, eye=(0.1, 0.6, 4.0), rotation=(-90.0, 0.0, 0.0), fovy=19.5)]
    write_inputs(tmp_path, sd, cams)
    rng = np.random.default_rng(7)
    img = (rng.random((n, 3)).astype(np.float32) ** 3) * 6.0
    special = np.array([0.0, -0.0, -1.5, np.nan, np.inf, -np.inf, 1e-42, 1.0, 255.0, 1e30], np.float32)
    img[: len(special), 0] = special
    img[: len(special), 1] = special[::-1]
    img.tofile(tmp_path / "img.f32")
    (rng.random((n, 2)).astype(np.float32) * 1.5 - 0.2).astype(np.float32).tofile(tmp_path / "rg.f32")
    (rng.random(n).astype(np.float32) * 3.0).astype(np.float32).tofile(tmp_path / "grey.f32")
    rng.integers(-1, n, n).astype(np.int32).tofile(tmp_path / "motion.i32")
    np.full(4 * n, 77, np.uint8).tofile(tmp_path / "pbo77.u8")
    scale = np.float32(0.37)
    plan = [("load", "img", "img.f32"), ("load", "rg", "rg.f32"), ("load", "grey", "grey.f32"), ("load", "motion", "motion.i32")]
    for tone in (0, 1, 2):
        plan += [("load", "pbo", "pbo77.u8"), ("pbo_vec3_default_scale", "pbo", "img", W, H, tone), ("dump", "pbo", f"vec3_tone{tone}.u8"),
                 ("load", "pbo", "pbo77.u8"), ("pbo_vec3", "pbo", "img", W, H, tone, f"{scale:.9g}"), ("dump", "pbo", f"vec3_tone{tone}_scaled.u8")]
    for kind, src in (("vec2", "rg"), ("float", "grey"), ("int", "motion")):
        plan += [("load", "pbo", "pbo77.u8"), ("pbo_" + kind, "pbo", src, W, H), ("dump", "pbo", f"{kind}.u8")]
    plan.append(("scene_destroy",))
    steps, _, _ = run_child(tmp_path, runners["shim_runner"], plan)
    rp = Replay(tmp_path, sd, cams).run(plan)
    outs = [rp.dumps[k] for k in sorted(rp.dumps)]
    assert len(outs) == 9 and all(o.reshape(-1, 4)[:, 3].max() == 0 and o.max() > 100 for o in outs)  # alpha 0: the 77s are gone
    assert len({o.tobytes() for o in outs}) == 9  # tone maps, scales and kinds all show
    compare(tmp_path, rp, steps)


# ---------------------------------------------------------------------------------------------------------------------
# 6. The multi-GPU forms, on one GPU
# ---------------------------------------------------------------------------------------------------------------------
def _multi_gpu_form(runners, tmp_path, binary):
    sd = teapots_scene()
    W, H = 56, 40
    n = W * H
    cams = [animated_camera(W, H, f) for f in range(2)]
    write_inputs(tmp_path, sd, cams)
    plan = [("alloc", "direct", 12 * n), ("alloc", "indirect", 12 * n), ("alloc", "pbo", 4 * n), ("depth", 3), ("reuse", 3),
            ("looper", 9998), ("path_trace_init",), ("restir_init",), ("gbuffer_create", W, H), ("camera", 0), ("gbuffer_render",)]
    dump_gbuffer(plan, 0, "gb0")
    plan += [("restir_direct", "direct", 0), ("dump", "direct", "restir.f32"), ("pbo_vec3_default_scale", "pbo", "direct", W, H, 2),
             ("dump", "pbo", "preview.u8"), ("gbuffer_update",), ("camera", 1), ("path_trace", "direct", "indirect", 0),
             ("dump", "direct", "pt_direct.f32"), ("dump", "indirect", "pt_indirect.f32"),
             ("restir_free",), ("path_trace_free",), ("gbuffer_destroy",), ("scene_destroy",)]
    steps, loaded, _ = run_child(tmp_path, runners[binary], plan)
    rccl = {p for p in loaded.get("comm", []) if "rccl" in os.path.basename(p)}
    assert len(rccl) == 1, f"the communicator should come from exactly one RCCL, the child loaded {loaded}"
    rp = Replay(tmp_path, sd, cams).run(plan)
    assert (f32(rp, "restir.f32") > 0).mean() > 0.2 and (f32(rp, "pt_direct.f32") > 0).mean() > 0.2 and f32(rp, "pt_indirect.f32").max() > 0
    assert_gbuffer_hits_and_misses(rp, "gb0")
    assert [l for _, l in rp.steps][-1] == 0  # 9998 -> 9999 -> 0
    compare(tmp_path, rp, steps)


def test_multi_gpu_form_world_of_one(runners, tmp_path):
    """RADISH_SHIM_MULTI_GPU with commInit(id, 0, 1): the partitioned G-buffer with its exchange, rdh_restir_direct_gathered and
    rdh_path_trace_gathered over RCCL with one rank give the single-GPU frames."""
    _multi_gpu_form(runners, tmp_path, "shim_runner_multi_gpu")


def test_one_process_form_with_one_gpu(runners, tmp_path):
    """RADISH_SHIM_ONE_PROCESS_GPUS with commInitAll(scene, sobol, 1): no peers, the *_all entries with one context."""
    _multi_gpu_form(runners, tmp_path, "shim_runner_one_process")


# ---------------------------------------------------------------------------------------------------------------------
# 7. check(): print and exit, like checkCUDAError
# ---------------------------------------------------------------------------------------------------------------------
def test_error_path_prints_and_exits(runners, tmp_path):
    """A null image pointer to pathTrace: rdh_path_trace refuses it on the host (RDH_ERR_ARGS, `rdh_path_trace: bad arguments`)
    before it selects the device or enqueues anything, so this is a refusal, not a fault.  check() must print
    `HIP error (file:line): pathTrace: <rdh_last_error>` and exit(EXIT_FAILURE); the steps before it run, the one after does not."""
    from radish_pt_amd import hostlib

    sd = degenerate_scene("one_triangle")
    W, H = 16, 8
    write_inputs(tmp_path, sd, [hostlib.make_camera(W, H, eye=(0.1, 0.6, 4.0), rotation=(-90.0, 0.0, 0.0), fovy=19.5)])
    plan = [("alloc", "indirect", 12 * W * H), ("depth", 2), ("looper", 7), ("path_trace", "null", "indirect", 0), ("looper", 8)]
    steps, _, r = run_child(tmp_path, runners["shim_runner"], plan, expect_status=1)
    assert steps == [("alloc", 0), ("depth", 0), ("looper", 7)]
    lines = [l for l in r.stderr.splitlines() if l.startswith("HIP error")]
    assert len(lines) == 1, r.stderr
    m = re.fullmatch(r"HIP error \((.*radish_shim\.hpp):(\d+)\): pathTrace: rdh_path_trace: bad arguments", lines[0])
    assert m, lines[0]
    if not os.environ.get("RADISH_SHIM_RUNNER_DIR"):  # the line lies inside pathTrace's body of the committed header
        src = open(os.path.join(ROOT, "radish_pt_amd", "csrc", "radish_shim.hpp")).read().splitlines()
        first = next(i for i, l in enumerate(src, 1) if l.startswith("inline void pathTrace(glm::vec3 *directIllum"))
        last = next(i for i, l in enumerate(src, 1) if i > first and l == "}")
        assert first < int(m.group(2)) < last, lines[0]
