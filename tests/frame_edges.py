"""Inputs for the frame kernels at the ends of their two axes: tiny frames and the 28-bounce depth limit
(tests/test_frame_edges_cpu.py holds these inputs to their conditions with the oracle alone, tests/test_gpu_frame_edges.py compares
the kernels with the oracle on them).  Scenes, one camera per shape, the partitions, and oracle references cached per process.

The closed scene: the Cornell room with a sixth, metallic wall at z = 1 and the camera inside, so a path ends only on the lamp, on an
invalid BSDF sample or at the depth bound.  At 16x12 and looper 5 the oracle traces 192, 191, ..., 177 extension rays at bounces
1..28 (test_frame_edges_cpu.py pins the decay).  The glass-free variant has a Lambertian in the glass object's place: a dielectric
bounce draws 3 Sobol values, every other 7, so there a path alive at bounce 28 has drawn exactly 4 + 7 * 28 = 200; its sixth wall
is half metallic, which makes the last of the 200 values decide something (closed_scene).
"""
import functools

import numpy as np

from helpers import oracle_path_trace_mt

COUNTER_KEYS = ("closestRays", "anyRays", "nodeVisits", "triTests", "closestHits")
MAX_DEPTH = 28        # 4 + 7 * 28 = 200 Sobol dimensions: rdh_path_trace refuses 29
LAST_ROW = 9999       # the last row of the 10000 x 200 Sobol table; State::looper wraps to 0 after it
BASE = (16, 12)       # the dense base: 192 pixels, 2 x 2 blocks with the lower ones half empty

# shape -> what it edges
SHAPES = {
    (1, 1): "single pixel",
    (1, 65): "one pixel wide: every block 7/8 empty, aspect 1/65 in cameraSample",
    (65, 1): "one pixel high: every block 7/8 empty, aspect 65 in cameraSample",
    (7, 9): "narrower than an 8x8 block (one wave), two blocks high",
    (8, 8): "exactly one block",
    (9, 8): "one pixel over a block",
    (16, 8): "128 slots = kPacket",
    (16, 16): "256 slots = kShadePacket",
    (32, 32): "1024 slots = kSortPacket",
    (40, 32): "1280 slots = 1024 + 256",
    (63, 65): "one short of / one over the 64-pixel tile",
    (16, 12): "the dense base",
}
SHAPE_IDS = {s: f"{s[0]}x{s[1]}" for s in SHAPES}

# Closed scene: vertical field of view (the half angle in degrees, as make_camera takes it) and the first of the two consecutive
# loopers of each shape.  The room is closed, so every fovy keeps every primary ray inside; the wide frames get a narrow one so that
# aspect * tan(fovy) stays a view of the room's back half and not a fan over 170 degrees.
CLOSED_FOVY = {(65, 1): 0.8, (1, 65): 35.0}
CLOSED_LOOPER = {}          # default 5 (the looper the base counts were measured at)
# Teapots stand-in: fovy 19 is the view of test_restir_sequence_bit_exact.  65x1 at fovy 19 would span atan(65 tan 19) = 87 degrees
# to either side and see the room in 6 % of its pixels; 0.36 degrees gives it the 48x40 frame's horizontal extent.
TEAPOTS_FOVY = {(65, 1): 0.36}

# (shape, tile, world): partitions in which some rank's share of the tiles reaches past numTiles.  In all but (65, 1) world 4
# (9 tiles: 3 / 2 / 2 / 2 real ones) world exceeds the tile count and the last rank gets no pixel at all.
PARTITIONS = (((7, 9), 8, 3), ((1, 1), 8, 2), ((63, 65), 64, 3), ((65, 1), 8, 4), ((65, 1), 8, 10))


def _materials(b):
    from radish_pt_amd import layouts as L

    return {"white": b.material(L.make_material(L.LAMBERTIAN, (0.73, 0.73, 0.73))),
            "red": b.material(L.make_material(L.LAMBERTIAN, (0.63, 0.065, 0.05))),
            "green": b.material(L.make_material(L.LAMBERTIAN, (0.14, 0.45, 0.091))),
            "light": b.material(L.make_material(L.LIGHT, (17.0, 12.0, 4.0))),
            "diffuse": b.material(L.make_material(L.LAMBERTIAN, (0.9, 0.9, 0.9))),
            "metal": b.material(L.make_material(L.METALLIC_WORKFLOW, (0.95, 0.8, 0.45), metallic=1.0, roughness=0.3)),
            "glass": b.material(L.make_material(L.DIELECTRIC, (1.0, 1.0, 1.0), ior=1.5))}


@functools.lru_cache(maxsize=None)
def closed_scene(glass=True):
    """The closed room: 12 wall and 2 lamp triangles, 3 x 16 x 12 x 2 = 1152 of the three objects."""
    from radish_pt_amd import layouts as L, scenes

    b = scenes._Builder()
    m = _materials(b)
    b.room(-1, 1, 0, 2, -1, 1, m["white"], m["red"], m["green"])
    # the sixth wall, facing -z.  Glass-free variant: half metallic, so that metallicSample's lobe choice `r.z > 1 / (2 - metallic)`
    # depends on the third value of its draw (at metallic 1 it never does, and a Lambertian ignores it): without that, the last word
    # of a row, table[looper][199], is read at bounce 28 and changes nothing
    wall = m["metal"] if glass else b.material(L.make_material(L.METALLIC_WORKFLOW, (0.95, 0.8, 0.45), metallic=0.5, roughness=0.3))
    b.add(*scenes._quad((1, 0, 1), (-1, 0, 1), (-1, 2, 1), (1, 2, 1), (0, 0, -1)), wall)
    b.ceiling_light(0.0, 0.0, 0.1, 1.999, m["light"])
    third = m["glass"] if glass else m["diffuse"]
    for k, (mat, pos) in enumerate(((m["diffuse"], (-0.5, 0.0, -0.35)), (m["metal"], (0.45, 0.0, -0.1)), (third, (-0.05, 0.0, 0.3)))):
        p, n, uv = scenes._revolved(16, 12, 0.3, 0.55, k)
        b.add(p, n, uv, mat, pos)
    return b.finish("closed_room" if glass else "closed_room_no_glass")


def closed_camera(shape, glass=True):
    """Glass-free variant at 1x1: turned 5 degrees, so that at looper 9999 the pixel's one path is alive at bounce 28 and takes
    that bounce on the half-metallic wall (straight ahead it dies at bounce 24)."""
    from radish_pt_amd import hostlib

    w, h = shape
    yaw = 5.0 if (not glass and shape == (1, 1)) else 0.0
    return hostlib.make_camera(w, h, eye=(0.0, 1.0, 0.9), rotation=(-90.0, yaw, 0.0), fovy=CLOSED_FOVY.get(shape, 35.0))


def closed_looper(shape):
    return CLOSED_LOOPER.get(shape, 5)


@functools.lru_cache(maxsize=None)
def teapots_scene():
    from radish_pt_amd import scenes

    return scenes.teapots(segments=12, bands=8, grid=2, emissive_grid=(4, 8))


def teapots_cameras(shape, frames=3):
    """The moving camera of test_restir_sequence_bit_exact at this shape."""
    from radish_pt_amd import hostlib

    w, h = shape
    return [hostlib.make_camera(w, h, eye=(0.3 + 0.05 * f, 1.9, 7.4), rotation=(-91.5, -11.0, 0.0), fovy=TEAPOTS_FOVY.get(shape, 19.0))
            for f in range(frames)]


# ---------------------------------------------------------------------------------------------------------------------------------
# oracle references (computed once per process, read-only)
# ---------------------------------------------------------------------------------------------------------------------------------
def _frozen(a):
    a.setflags(write=False)
    return a


def oracle_frames(sd, cam, depth, looper, frames=1, iter0=0):
    """`frames` oracle frames folded into one pair of images (iter iter0.., looper, looper + 1, .. mod 10000) and their summed
    counters, as _oracle_frame of test_gpu_wf_compact.py."""
    w, h = (int(v) for v in cam["resolution"])
    d, i = np.zeros((w * h, 3), np.float32), np.zeros((w * h, 3), np.float32)
    stats = {k: 0 for k in COUNTER_KEYS}
    for f in range(frames):
        _, st = oracle_path_trace_mt(sd, cam, d, i, iter0 + f, (looper + f) % (LAST_ROW + 1), depth)
        for k in COUNTER_KEYS:
            stats[k] += st[k]
    return {"cam": cam, "d": _frozen(d), "i": _frozen(i), "stats": stats}


@functools.lru_cache(maxsize=None)
def closed_ref(shape, depth=MAX_DEPTH, looper=None, frames=1, glass=True):
    return oracle_frames(closed_scene(glass), closed_camera(shape, glass), depth, closed_looper(shape) if looper is None else looper,
                         frames)


@functools.lru_cache(maxsize=None)
def bounce_rays(shape, looper=None, glass=True, upto=MAX_DEPTH):
    """Extension rays the oracle traces at bounce 0 (the primary rays), 1, ..., `upto` of one frame: the closest-hit rays of depth k
    minus those of depth k - 1."""
    counts = [closed_ref(shape, depth, looper, 1, glass)["stats"]["closestRays"] for depth in range(upto + 1)]
    return tuple(counts[0:1] + [b - a for a, b in zip(counts, counts[1:])])


@functools.lru_cache(maxsize=None)
def direct_ref(shape, looper0=100, iters=2):
    from oracle import pyoracle

    w, h = shape
    cam = closed_camera(shape)
    o = pyoracle.OracleScene(closed_scene())
    ref = np.zeros((w * h, 3), np.float32)
    for it in range(iters):
        o.path_trace_direct(cam, ref, it, looper0 + it)
    return {"cam": cam, "d": _frozen(ref), "looper0": looper0, "iters": iters}


def _gb_planes(gb):
    cur = gb.frameIdx
    return {"albedo": gb.albedo.copy(), "normal": gb.normal[cur].copy(), "depth": gb.depth[cur].copy(), "primId": gb.primId[cur].copy(),
            "motion": gb.motion.copy()}


def _delta(after, before):
    return {k: after[k] - before[k] for k in COUNTER_KEYS}


@functools.lru_cache(maxsize=None)
def gbuffer_ref(shape, frames=2):
    """Per frame of the moving camera: the oracle's planes (the current ones and motion) and the work of that render."""
    from oracle import pyoracle

    w, h = shape
    cams = teapots_cameras(shape, frames)
    o = pyoracle.OracleScene(teapots_scene())
    gb = pyoracle.GBufferHost(w, h)
    out = []
    for cam in cams:
        before = o.stats()
        o.gbuffer_render(cam, gb)
        out.append({"cam": cam, "planes": {k: _frozen(v) for k, v in _gb_planes(gb).items()}, "stats": _delta(o.stats(), before)})
        gb.update(cam)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def restir_ref(shape, reuse, faithful):
    """The three-frame sequence of test_restir_sequence_bit_exact: per frame the image, the reservoirs that frame wrote, the counters
    of restir_direct, and the primId plane it ran on."""
    from oracle import pyoracle
    from radish_pt_amd import layouts as L

    w, h = shape
    n = w * h
    cams = teapots_cameras(shape)
    o = pyoracle.OracleScene(teapots_scene())
    gb = pyoracle.GBufferHost(w, h)
    res = [np.zeros(n, L.RESERVOIR_DTYPE) for _ in range(3)]  # cur, last, temp
    img = np.zeros((n, 3), np.float32)
    out = []
    for f, cam in enumerate(cams):
        o.gbuffer_render(cam, gb)
        before = o.stats()
        o.restir_direct(cam, img, 0, 40 + f, res[0], res[1], res[2], gb, f == 0, reuse, faithful)
        st = _delta(o.stats(), before)
        res[0], res[1] = res[1], res[0]
        out.append({"cam": cam, "img": _frozen(img.copy()), "reservoirs": res[1].tobytes(), "stats": st,
                    "primId": _frozen(gb.primId[gb.frameIdx].copy())})
        gb.update(cam)
    return tuple(out)
