"""The scene, cameras, loopers, tolerance, cap and coverage floor shared by tests/test_path_model_cpu.py (the oracle against
tests/path_model.py) and tests/test_gpu_path_model.py (the HIP kernels against the same model).

Inputs, frozen: 48x36 (1728 pixels: no multiple of the 8x8 packet nor of 64), maxDepth 3, loopers 3001 and 3002 as iterations 0 and 1
(consecutive, so that path_trace_samples can take both in one pass), three cameras that translate and turn, build_scene()'s 62
triangles.  Tolerance: restir_model_checks' 2e-4 relative with a floor of 1e-3.  Cap: 6 of 1728 pixels (0.4 %) per image and per
step.  Coverage floor: 30 pixels per image, five times the cap.

How the inputs were chosen (the cap and the tolerance were never touched).  The first scene had the metal as 15- and 9-cell sheets
under a random 8x8 normal map with uv spans of 2, the second of them at a grazing angle to the camera: 5 to 12 pixels of each
G-buffer and 7 of an indirect image differed, every one by 2e-4 to 2e-2 RELATIVE, none grossly.  The cause is the conditioning of
intersectTriangle (intersections.h:20-68) in binary32: bary = dot(origin - v0, pvec) / det with an origin 5 units away and
det = 2 * area * cos, so a small or grazing triangle carries 3e-6 of error in bary, hence in uv, hence — times the normal map's
gradient — 1e-5 in the mapped normal, which is 2e-4 of any cosine below 0.05.  Larger triangles (2 x 3 and 1 x 1 cells), a smooth
normal map, uv spans below 1 on the metal and a shelf tilted toward the camera brought that below the tolerance.  A sun 1000 times
its neighbour texel was given a halo for the same reason (linearSample's weights carry the direction's error).  The procedural
panel's uv stays below 0.3: sin(uv * 20 pi + ...) in binary32 has an absolute error of half an ulp of its ARGUMENT, and the product
of two such sines near zero then misses 2e-4 relative at arguments of 60.

The oracle against the model (tests/test_path_model_cpu.py; the GPU tests assert the same sets for every kernel structure):

    path_trace        iteration 0: direct {} indirect {}      iteration 1: direct {} indirect {}
    path_trace_direct iteration 0: {}                         iteration 1: {}
    gbuffer_render    camera 0: {537}      camera 1: {}       camera 2: {}
    restir_direct     reuse 0 and 3, the reference's update:  frame 0: gbuffer {537} pass 1 {994} pass 2 {};  frames 1, 2: none
    sample_direct_light, 3000 positions: 0 shadow rays classified differently

Of fourteen other loopers tried on the frozen scene none left out more than 1 direct and 4 indirect pixels.  Explanations, by
count: 0 pixels by a discrete choice (a triangle edge, an alias `r < prob`, the Fresnel or lobe threshold, a texel's `fract > 0.5`,
a procedural cell boundary, the 0.9999 frame switch); 2 pixels by a component BELOW THE TOLERANCE'S FLOOR, which is no discrete
choice and is named as what it is: pixel 537's mapped normal has x = 4.04e-4 (the model's 4.0406e-4, the oracle's 4.0441e-4) and
pixel 994's kept `wi` has z = 2.55e-5 (2.5496e-5 against 2.5820e-5); the absolute differences, 3.5e-7 and 3.2e-7, are binary32's
rounding of the hit position and exceed 2e-4 * 1e-3 = 2e-7.  tests/test_restir_model_cpu.py accounts for its pixels the same way.

Coverage, from the model's event masks, pixels per image (iteration 0, iteration 1), each at least 30:

    environment NEE accepted at depth 1 (direct)      404, 408     refraction entering                        362, 384
    environment NEE accepted at depth >= 2 (indirect)  65,  79     refraction leaving                         235, 260
    environment NEE rejected by occlusion             171, 161     total internal reflection (reflects)       185, 190
    a bounce missing into the map, MIS weight < 1     770, 751     metallic sample from the diffuse lobe       74,  95
    a bounce missing into the map after a specular one 83,  99     metallic sample from the GGX lobe          179, 158
    a primary miss                                    381, 379     metallic sample below the horizon           36,  35
    an emitter seen directly                           79,  79     normal-mapped hit, flip test differs        62,  65
    an emitter collected by a BSDF ray                 75,  92     base-colour lookup with wrapped uv          59,  52
    an emitter refused by the single-sided test        49,  40     procedural lookup at depth >= 2             40,  40
                                                                   draw cursor behind 4 + 7 (depth - 1) at 3  317, 331

"Total internal reflection ending a path" does not exist in the reference: `fresnel()` returns 1 under total internal reflection
(material.h:55-57), `r.z < pdfRefl` (:165) is then true for every draw but 1.0f itself, and the sample is the mirror direction.
The `Invalid` of :170-174 is reached only by that one draw; the model has it, counts it (0 here) and the test asserts the 0.

Planted mistakes (each in the model alone; the oracle's pixels outside the tolerance in the worst image, cap 6): uv weights
swapped 1025, normal map decoded without its offset 303, dielectric normal flipped 439, a cosine on a specular throughput 276, NEE
draws consumed for a dielectric 193, 1 / pi^2 dropped from the environment NEE pdf 541, a sine on environmentMapPdf 946, the map's
colour on a primary miss 398, the pixel's corner for its centre 545.  Two switches one might expect are not there.  `mapped * 2 - 1`
is the SAME rule as the reference's `mapped * 1 - 0.5`: one is twice the other and the decode normalises (scene.h:107-108), so no
input can tell them apart; the test asserts that it changes nothing.  `metallicMapId != NullTextureId` needs a material with -2
in that field, which both the scene loader and rdh_scene_upload (and the oracle) refuse."""
import numpy as np

import path_model as P
import restir_model_checks as RC
from radish_pt_amd import hostlib, layouts as L, scenes

W, H = 48, 36  # 1728 pixels: not a multiple of the 8x8 packet nor of 64
N = W * H
MAX_DEPTH = 3
LOOPERS = (3001, 3002)  # iterations 0 and 1
RESTIR_LOOPERS = (40, 977, 5003)  # frames 0-2
CAP = 6  # 0.4 % of 1728 pixels, per image and per step
COVERAGE_FLOOR = 30  # five times the cap
far = RC.far


# ---------------------------------------------------------------------------------------------------------------------
# textures
# ---------------------------------------------------------------------------------------------------------------------
def _textures():
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:16, 0:16]
    checker = ((x // 2 + y // 2) % 2)[..., None]
    base = (np.array([0.85, 0.8, 0.7]) * (1 - checker) + np.array([0.2, 0.3, 0.65]) * checker) * (0.8 + 0.2 * rng.random((16, 16, 1)))
    metallic = (0.15 + 0.8 * rng.random((8, 8, 1))).repeat(3, 2)  # lobe threshold 1 / (2 - m) between 0.54 and 0.95
    roughness = (0.62 + 0.36 * rng.random((8, 8, 1))).repeat(3, 2)  # >= 0.25: ggxDistribution's cancellation stays small
    ph = 2 * np.pi * np.arange(8) / 8  # smooth and periodic: a uv error of 1e-6 moves the normal by about as much
    normal = np.stack([0.5 + 0.4 * np.sin(ph[None, :] + 0.5 * np.cos(ph[:, None])), 0.5 + 0.4 * np.cos(ph[:, None] + 0.7 * np.sin(ph[None, :])),
                       0.85 + 0.1 * np.sin(ph[None, :] + ph[:, None])], 2)  # `- 0.5` leaves tilts up to 50 degrees
    # environment: a dim sky that brightens toward the zenith, a dimmer ground, a sun of 2 x 2 texels with a halo
    h, w = 16, 32
    v = ((np.arange(h) + 0.5) / h)[:, None, None]
    uu = ((np.arange(w) + 0.5) / w)[None, :, None]
    env = np.where(v < 0.5, np.array([0.05, 0.07, 0.11]) * (1.2 - v) * (1.0 + 0.3 * np.sin(2 * np.pi * uu)), np.array([0.03, 0.028, 0.02]) + 0 * uu)
    # The sun falls off by a factor of 6 per texel over three rings: linearSample's weights carry binary32's error in the
    # direction (about 1e-6 of a texel), and next to a texel 1000 times its neighbour that alone would exceed 2e-4 relative.
    for ring in (3, 2, 1, 0):
        env[3 - ring:5 + ring, 5 - ring:7 + ring] = np.array([60.0, 54.0, 40.0]) / 6.0 ** ring
    return [t.astype(np.float32) for t in (base, metallic, roughness, normal, env)]


# ---------------------------------------------------------------------------------------------------------------------
# scene
# ---------------------------------------------------------------------------------------------------------------------
def _patch(pos, nrm, uv, nu, nv):
    """A grid of nu x nv cells, two triangles each, over the parameter square: per-vertex positions, normals and texcoords from
    the three functions of (s, t) in [0, 1]."""
    p, n, t = [], [], []
    g = lambda i, j: (i / nu, j / nv)
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = g(i, j), g(i + 1, j), g(i + 1, j + 1), g(i, j + 1)
            for tri in ((a, b, c), (a, c, d)):
                for st in tri:
                    p.append(pos(*st)), n.append(nrm(*st)), t.append(uv(*st))
    return np.array(p, np.float64), np.array(n, np.float64), np.array(t, np.float64)


def _flat(tris, outward_from):
    """Flat-shaded triangles [k, 3, 3] wound and given normals that face away from the point `outward_from`."""
    p, n = [], []
    for a, b, c in np.asarray(tris, np.float64):
        nn = np.cross(b - a, c - a)
        if np.dot(nn, a - outward_from) < 0:
            b, c, nn = c, b, -nn
        p += [a, b, c]
        n += [nn / np.linalg.norm(nn)] * 3
    return np.array(p), np.array(n), np.zeros((len(p), 2))


def _prism(x0, x1, y0, y1, z_back, z_front):
    """A closed glass body with flat faces: the right-angled triangle (x0, z_back) (x1, z_back) (x0, z_front) extruded from y0 to
    y1.  A ray that enters the front hypotenuse meets a leg from inside beyond the critical angle."""
    A, B, Cc = (x0, z_back), (x1, z_back), (x0, z_front)
    lo = [np.array([q[0], y0, q[1]]) for q in (A, B, Cc)]
    hi = [np.array([q[0], y1, q[1]]) for q in (A, B, Cc)]
    tris = [(lo[0], lo[1], lo[2]), (hi[0], hi[1], hi[2])]
    for i, j in ((0, 1), (1, 2), (2, 0)):
        tris += [(lo[i], lo[j], hi[j]), (lo[i], hi[j], hi[i])]
    return _flat(tris, np.mean(lo + hi, axis=0))


def build_scene():
    """About 100 triangles under an open sky.

      ground   3 x 3 cells of an undulating Lambertian sheet with a base-colour map; uv from -0.7 to 1.9
      panel    2 x 2 cells of a leaning Lambertian sheet with the procedural colour; uv inside [0.04, 0.96]
      metal    5 x 3 cells of a quarter cylinder, MetallicWorkflow with metallic, roughness and normal maps; uv from -0.6 to 1.7
      glass    two right-angled prisms (ior 1.5), flat faces, hovering
      lamps    three emissive quads wound toward the ground: two with authored normals pointing up (a BSDF ray from below
               collects them, pathtrace.cu:252-256), one with normals pointing down (refused); the third hangs in view
      sky      32 x 16 map, a sun of four texels

    Every sheet's three vertex normals differ within a triangle, and no triangle is axis-aligned."""
    tex = _textures()
    mats = []

    def mat(**kw):
        maps = {k: kw.pop(k) for k in list(kw) if k.endswith("MapId")}
        m = L.make_material(**kw)
        for k, v in maps.items():
            m[k] = v
        mats.append(m)
        return len(mats) - 1

    ground = mat(type=L.LAMBERTIAN, baseColor=(1, 1, 1), baseColorMapId=0)
    panel = mat(type=L.LAMBERTIAN, baseColor=(1, 1, 1), baseColorMapId=-2)
    metal = mat(type=L.METALLIC_WORKFLOW, baseColor=(0.95, 0.8, 0.45), metallic=1.0, roughness=0.5, metallicMapId=1, roughnessMapId=2,
                normalMapId=3)
    glass = mat(type=L.DIELECTRIC, baseColor=(0.95, 1.0, 0.97), ior=1.5)
    lamp_up = mat(type=L.LIGHT, baseColor=(9.0, 8.0, 6.0))
    lamp_up2 = mat(type=L.LIGHT, baseColor=(5.0, 8.0, 10.0))
    lamp_down = mat(type=L.LIGHT, baseColor=(9.0, 5.0, 4.0))
    P_, N_, T_, ids = [], [], [], []

    def add(p, n, t, m):
        P_.append(p), N_.append(n), T_.append(t), ids.extend([m] * (len(p) // 3))

    # ground: y = 0.09 sin(1.3 x + 0.4) cos(1.1 z), normals from its gradient
    gx = lambda s: -2.3 + 4.6 * s
    gz = lambda t: -2.7 + 4.6 * t
    gy = lambda x, z: 0.09 * np.sin(1.3 * x + 0.4) * np.cos(1.1 * z)
    add(*_patch(lambda s, t: (gx(s), gy(gx(s), gz(t)), gz(t)),
                lambda s, t: (-0.09 * 1.3 * np.cos(1.3 * gx(s) + 0.4) * np.cos(1.1 * gz(t)), 1.0,
                              0.09 * 1.1 * np.sin(1.3 * gx(s) + 0.4) * np.sin(1.1 * gz(t))),
                lambda s, t: (-0.7 + 2.6 * s, 1.9 - 2.4 * t), 3, 3), ground)
    # panel: leaning back, bowed
    add(*_patch(lambda s, t: (-2.3 + 3.6 * s, 0.1 + 1.9 * t, -2.45 - 0.5 * t + 0.25 * (s - 0.5) ** 2),
                lambda s, t: (-0.5 * (s - 0.5), 0.27 + 0.08 * t, 1.0),
                lambda s, t: (0.02 + 0.28 * s, 0.03 + 0.25 * t), 2, 2), panel)
    # metal: a quarter cylinder about the axis x in [0.5, 1.9] at (y, z) = (0.12, -1.2), radius 0.85, seen from its convex side
    ang = lambda t: np.radians(20.0 + 95.0 * t)
    add(*_patch(lambda s, t: (0.45 + 1.5 * s, 0.12 + 0.85 * np.sin(ang(t)) + 0.1 * s, -1.2 + 0.85 * np.cos(ang(t))),
                lambda s, t: (-0.07 + 0.16 * (s - 0.5), np.sin(ang(t)), np.cos(ang(t))),
                lambda s, t: (-0.35 + 0.8 * s, 1.3 - 0.7 * t), 2, 3), metal)
    # metal: a bowed shelf seen at a grazing angle, where the mapped normal and the interpolated one face opposite ways often
    add(*_patch(lambda s, t: (1.0 + 1.3 * s, 0.62 + 0.1 * (s - 0.5) ** 2 - 0.3 * t, -0.1 + 1.5 * t),
                lambda s, t: (-0.2 * (s - 0.5), 1.0, 0.22 + 0.1 * t - 0.05 * s),
                lambda s, t: (0.35 - 0.7 * s, -0.3 + 0.6 * t), 1, 1), metal)
    # glass
    add(*_prism(-1.55, -0.35, 0.25, 1.05, -0.9, 0.35), glass)
    add(*_prism(0.15, 0.95, 0.3, 0.8, 0.55, 1.25), glass)

    def lamp(cx, cz, hx, hz, y, tilt, normal_y, m, lean=0.0):
        c = [(cx - hx, y - tilt + lean, cz - hz), (cx + hx, y + lean, cz - hz), (cx + hx, y + tilt - lean, cz + hz),
             (cx - hx, y - lean, cz + hz)]  # wound toward -y
        p = np.array([c[0], c[1], c[2], c[0], c[2], c[3]], np.float64)
        add(p, np.tile(np.array([0.0, normal_y, 0.0]), (6, 1)), np.zeros((6, 2)), m)

    lamp(-0.9, -0.2, 0.75, 0.6, 2.05, 0.06, 1.0, lamp_up)
    lamp(1.1, 0.4, 0.6, 0.65, 2.25, -0.05, 1.0, lamp_up2)
    lamp(0.1, -1.75, 0.8, 0.5, 1.2, 0.04, -1.0, lamp_down, lean=0.33)  # its back edge up: the camera sees its upper side
    return scenes.SceneData("path_model", np.concatenate(P_).astype(np.float32), np.concatenate(N_).astype(np.float32),
                            np.concatenate(T_).astype(np.float32), np.array(ids, np.int32), np.array(mats, dtype=L.MATERIAL_DTYPE), tex, 4)


def cameras():
    """Frame f's camera; the path tracer and the direct kernel use the first, the G-buffer and ReSTIR all three."""
    return [hostlib.make_camera(W, H, eye=(0.25 + 0.2 * f, 1.45, 4.3 - 0.1 * f), rotation=(-92.0 + 2.5 * f, -16.0 - 1.5 * f, 0.0), fovy=19.0)
            for f in range(3)]


# ---------------------------------------------------------------------------------------------------------------------
# the model's evaluations, once per process
# ---------------------------------------------------------------------------------------------------------------------
_MEMO = {}


def setup(plant=None):
    """(scene data, model scene, cameras); the unplanted one is shared."""
    key = ("setup", plant)
    if key not in _MEMO:
        sd = _MEMO[("setup", None)][0] if ("setup", None) in _MEMO else build_scene()
        _MEMO[key] = (sd, P.PathScene(sd, plant), cameras())
    return _MEMO[key]


def model_path_trace(plant=None):
    """single_kernel_pt over iterations 0 and 1: a list of its dicts, the second accumulated on the first."""
    key = ("pt", plant)
    if key not in _MEMO:
        _, ms, cams = setup(plant)
        out, prev = [], None
        for it, looper in enumerate(LOOPERS):
            out.append(P.single_kernel_pt(ms, cams[0], looper, MAX_DEPTH, it, prev))
            prev = (out[-1]["direct"], out[-1]["indirect"])
        _MEMO[key] = out
    return _MEMO[key]


def model_pt_direct(plant=None):
    key = ("ptd", plant)
    if key not in _MEMO:
        _, ms, cams = setup(plant)
        out, prev = [], None
        for it, looper in enumerate(LOOPERS):
            prev = P.pt_direct(ms, cams[0], looper, it, prev)
            out.append(prev)
        _MEMO[key] = out
    return _MEMO[key]


def model_gbuffer(plant=None):
    key = ("gb", plant)
    if key not in _MEMO:
        _, ms, cams = setup(plant)
        _MEMO[key] = [P.gbuffer(ms, cams[f], cams[f - 1] if f else None) for f in range(len(cams))]
    return _MEMO[key]


# ---------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------
def path_trace_excluded(tested, plant=None):
    """tested: per iteration (direct, indirect) as the code under test accumulates them.  Per iteration {"direct": pixels,
    "indirect": pixels} outside the tolerance.  Iteration 1 is compared on the model's mean over the MODEL's iteration 0, so a
    pixel left out at iteration 0 is, as a rule, left out at iteration 1 too: the cap holds per image."""
    model = model_path_trace(plant)
    return [{"direct": np.flatnonzero(far(d, m["direct"])), "indirect": np.flatnonzero(far(i, m["indirect"]))}
            for (d, i), m in zip(tested, model)]


def images_excluded(tested, model):
    return [np.flatnonzero(far(t, m)) for t, m in zip(tested, model)]


def gbuffer_excluded(tested, plant=None):
    return [np.flatnonzero(RC.gbuffer_bad(m, t)) for t, m in zip(tested, model_gbuffer(plant))]


def assert_within_cap(px, what):
    assert len(px) <= CAP, f"{what}: {len(px)} pixels differ from the float64 model (cap {CAP}); first {np.asarray(px)[:12]}"


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's runs
# ---------------------------------------------------------------------------------------------------------------------
def oracle_path_trace(sd, cam):
    from oracle import pyoracle

    o = pyoracle.OracleScene(sd)
    d, i = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32)
    out = []
    for it, looper in enumerate(LOOPERS):
        o.path_trace(cam, d, i, it, looper, MAX_DEPTH)
        out.append((d.copy(), i.copy()))
    return out


def oracle_pt_direct(sd, cam):
    from oracle import pyoracle

    o = pyoracle.OracleScene(sd)
    d = np.zeros((N, 3), np.float32)
    out = []
    for it, looper in enumerate(LOOPERS):
        o.path_trace_direct(cam, d, it, looper)
        out.append(d.copy())
    return out


def oracle_gbuffer(sd, cams):
    from oracle import pyoracle

    o = pyoracle.OracleScene(sd)
    gb = pyoracle.GBufferHost(W, H)
    out = []
    for cam in cams:
        o.gbuffer_render(cam, gb)
        out.append(RC.host_planes(gb, gb.frameIdx))
        gb.update(cam)
    return out


def oracle_excluded():
    """What the oracle's runs leave out, once per process: {"path_trace": [...], "pt_direct": [...], "gbuffer": [...]}."""
    if "oracle" not in _MEMO:
        sd, _, cams = setup()
        _MEMO["oracle"] = {"path_trace": path_trace_excluded(oracle_path_trace(sd, cams[0])),
                           "pt_direct": images_excluded(oracle_pt_direct(sd, cams[0]), model_pt_direct()),
                           "gbuffer": gbuffer_excluded(oracle_gbuffer(sd, cams))}
    return _MEMO["oracle"]


# ---------------------------------------------------------------------------------------------------------------------
# ReSTIR DI on this scene: restir_model's three steps through restir_model_checks' sequence, frames 0-2
# ---------------------------------------------------------------------------------------------------------------------
RESTIR_CASES = ((0, 1), (3, 1))  # (reuse mask, the reference's `update`)
assert RC.LOOPERS[:3] == RESTIR_LOOPERS


def oracle_restir_excluded(reuse, faithful):
    """Per frame what RC.check_frame returns for the oracle's run: ({step: excluded pixels}, pass 1, pass 2)."""
    key = ("restir", reuse, faithful)
    if key not in _MEMO:
        sd, ms, cams = setup()
        frames = RC.run_oracle(sd, cams, reuse, faithful)
        _MEMO[key] = [RC.check_frame(ms, f, cams, reuse, faithful, t) for f, t in enumerate(frames)]
    return _MEMO[key]
