"""Stage 0 of the wavefront path as packets (kernels_wave.h, k_wf_trace_primary): the primary rays of every 64-slot group
walked by one wave with one scalar record load per visit, the stage's literal-class list traced by the first workgroups of the same
launch.  RDH_PT_NO_PACKETS keeps k_wf_trace for stage 0.

Every case renders four frames — packets and RDH_PT_NO_PACKETS, each with RDH_PT_COUNT and without — and asks that all four images
are bit-equal to the CPU oracle's, that both counting frames' five work counters equal the oracle's, and (which follows, and names
the layer when it fails) that the two builds of stage 0 agree with each other.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_bit_equal, oracle_path_trace_mt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTER_KEYS = ("closestRays", "anyRays", "nodeVisits", "triTests", "closestHits")
LOOPER = 23
SHAPES = [(1, 1), (8, 8), (37, 29), (64, 48)]  # one pixel; one group, one workgroup; edge blocks with off-frame lanes; 48 groups
STRUCTURES = {"sorted_pairs": (True, True), "sorted_threaded": (True, False), "unsorted_pairs": (False, True), "unsorted_threaded": (False, False)}


def _torch():
    import torch

    return torch


def _flags(api, structure="sorted_pairs"):
    sort, pairs = STRUCTURES[structure]
    return api.RDH_PT_WAVEFRONT | (api.RDH_PT_SORT_MATERIAL if sort else 0) | (api.RDH_PT_PAIRS if pairs else api.RDH_PT_NO_PAIRS)


@pytest.fixture(scope="module")
def teapots_small():
    from radish_pt_amd import scenes

    return scenes.teapots(segments=12, bands=8, grid=2, emissive_grid=(4, 8))


_oracle_cache = {}


def _oracle(sd, cam, depth, samples=1, pix=None, key=None):
    """{'d', 'i', 'stats'} of `samples` accumulated oracle samples (iter s, looper LOOPER + s), once per key and read-only;
    pix = (begin, end): those pixels of the frame only.  key: what names the scene AND its tree (default: the scene's name)."""
    from oracle import pyoracle

    key = (key or sd.name, cam.tobytes(), depth, samples, pix)
    if key not in _oracle_cache:
        w, h = (int(v) for v in cam["resolution"])
        d, i = np.zeros((w * h, 3), np.float32), np.zeros((w * h, 3), np.float32)
        stats = {k: 0 for k in COUNTER_KEYS}
        for s in range(samples):
            if pix is None:
                _, st = oracle_path_trace_mt(sd, cam, d, i, s, LOOPER + s, depth)
            else:
                o = pyoracle.OracleScene(sd)
                o.path_trace(cam, d, i, s, LOOPER + s, depth, pix=(pix[0], pix[1], 1))
                st = o.stats()
            for k in COUNTER_KEYS:
                stats[k] += st[k]
        d.setflags(write=False)
        i.setflags(write=False)
        _oracle_cache[key] = {"d": d, "i": i, "stats": stats}
    return _oracle_cache[key]


def _use(ctx, sd, cam):
    ctx.set_partition(0, 1, 64)
    ctx.upload_scene(sd)
    ctx.set_camera(cam)


def _render(ctx, depth, flags, samples=1, elems=None):
    torch = _torch()
    n = elems if elems is not None else ctx.width * ctx.height
    d, i = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda")
    ctx.counters_reset()
    if samples == 1:
        ctx.path_trace(d, i, 0, LOOPER, depth, flags)
    else:
        ctx.path_trace_samples(d, i, 0, LOOPER, samples, depth, flags, samples_per_pass=samples)
    return d.cpu().numpy(), i.cpu().numpy(), ctx.counters()


def _four_frames(ctx, depth, base, ref, what, samples=1, elems=None, select=None):
    """The four frames of the module's docstring on the scene and camera the context holds.  select = (frame pixels, packed pixels)
    of a rank's share."""
    from radish_pt_amd import api

    got = {}
    for packets in (True, False):
        for count in (True, False):
            flags = base | (0 if packets else api.RDH_PT_NO_PACKETS) | (api.RDH_PT_COUNT if count else 0)
            d, i, ct = _render(ctx, depth, flags, samples, elems)
            name = f"{what}, {'packets' if packets else 'no packets'}, {'count' if count else 'no count'}"
            if select is not None:
                d, i = d[select[1]], i[select[1]]
            assert_bit_equal(d, ref["d"] if select is None else ref["d"][select[0]], f"{name}: direct vs oracle")
            assert_bit_equal(i, ref["i"] if select is None else ref["i"][select[0]], f"{name}: indirect vs oracle")
            if count:
                for k in COUNTER_KEYS:
                    assert ct[k] == ref["stats"][k], (name, k, ct[k], ref["stats"][k])
            got[packets, count] = (d, i, ct)
    for count in (True, False):
        a, b = got[True, count], got[False, count]
        assert_bit_equal(a[0], b[0], f"{what}: direct, packets vs none")
        assert_bit_equal(a[1], b[1], f"{what}: indirect, packets vs none")
        assert a[2] == b[2], (what, a[2], b[2])
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# frame shapes, depths, structures
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("structure", list(STRUCTURES))
@pytest.mark.parametrize("depth", (0, 1, 3))
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_cornell(gpu_ctx, cornell_small, shape, depth, structure):
    from radish_pt_amd import api, scenes

    cam = scenes.cornell_camera(*shape)
    ref = _oracle(cornell_small, cam, depth)
    _use(gpu_ctx, cornell_small, cam)
    got = _four_frames(gpu_ctx, depth, _flags(api, structure), ref, f"cornell {shape} depth {depth} {structure}")
    assert got[True, True][2]["closestRays"] >= shape[0] * shape[1]


@pytest.mark.parametrize("structure", ("sorted_pairs", "unsorted_threaded"))
@pytest.mark.parametrize("shape,depth", [((37, 29), 3), ((64, 48), 1), ((8, 8), 0)], ids=["37x29-d3", "64x48-d1", "8x8-d0"])
def test_teapots(gpu_ctx, teapots_small, shape, depth, structure):
    from radish_pt_amd import api, scenes

    cam = scenes.teapots_camera(*shape)
    ref = _oracle(teapots_small, cam, depth)
    _use(gpu_ctx, teapots_small, cam)
    _four_frames(gpu_ctx, depth, _flags(api, structure), ref, f"teapots {shape} depth {depth} {structure}")


@pytest.mark.parametrize("scene", ("cornell", "teapots"))
def test_packet_budget_of_four_hands_every_block_over(gpu_ctx, cornell_small, teapots_small, scene):
    """RDH_PT_WF_SMALL_LISTS: packets of 4 visits, so every block's lanes go on each on its own (the end of packetWalk)."""
    from radish_pt_amd import api, scenes

    sd, cam = (cornell_small, scenes.cornell_camera(64, 48)) if scene == "cornell" else (teapots_small, scenes.teapots_camera(37, 29))
    ref = _oracle(sd, cam, 3)
    assert ref["stats"]["nodeVisits"] > 4 * 64 * 48
    _use(gpu_ctx, sd, cam)
    _four_frames(gpu_ctx, 3, _flags(api) | api.RDH_PT_WF_SMALL_LISTS, ref, f"{scene}, small lists")


# ---------------------------------------------------------------------------------------------------------------------------------
# literal-class primary rays
# ---------------------------------------------------------------------------------------------------------------------------------
# The path tracer's primary rays are jittered inside their pixels, so an axis-aligned camera alone (test_gbuffer_literal_rays_bit_exact's)
# does not put a zero into a direction: the field of view is made a few millionths as well, so that the image plane's extent is of the
# order of the box test's Eps.  The rays of a frame are then next to parallel and hit one spot; what is tested is who traces them.
#   all_listed   the plane is 1.7e-7 wide: every ray has |d.x|, |d.y| < 1.1e-6 (listed) and |d.z| > 1 - Eps (class 3)
#   mixed        8e-6: the middle columns and rows are listed, every other ray is of class 3 and NOT listed (its wave traces it whole)
#   hint_fails   the camera turned by 45 degrees about y, 4e-6: d.y is the only small component; |d.y| < 1e-6 is class 4 and listed,
#                1e-6 <= |d.y| < 1.1e-6 is listed and of class 0 — the hint does not hold, and the ray is walked in its packet
LITERAL_CAMERAS = {
    "all_listed": dict(eye=(0.0, 1.0, 4.2), rotation=(-90.0, 0.0, 0.0), fovy=1e-5),
    "mixed": dict(eye=(0.0, 1.0, 4.2), rotation=(-90.0, 0.0, 0.0), fovy=float(np.degrees(2 * np.arctan(8e-6)))),
    "hint_fails": dict(eye=(-2.2, 1.0, 2.6), rotation=(-45.0, 0.0, 0.0), fovy=float(np.degrees(2 * np.arctan(4e-6)))),
}


def _primary_classes(ctx):
    """(listed, class) of the frame's primary rays as k_wf_raygen and makeRaySlab decide them, from the frame's own ray list."""
    rays, _ = ctx.dump_rays(LOOPER, 0)
    d = rays[:, 3:6].cpu().numpy().astype(np.float32)
    assert len(d) == ctx.width * ctx.height
    a = np.abs(d)
    eps = np.float32(1e-6)
    one = np.float32(1.0) - eps
    cls = np.where(a[:, 0] > one, 1, np.where(a[:, 1] > one, 2, np.where(a[:, 2] > one, 3, np.where((a < eps).any(axis=1), 4, 0))))
    return (a < np.float32(1.1e-6)).any(axis=1), cls


@pytest.mark.parametrize("small_lists", (False, True), ids=("lists", "small_lists"))
@pytest.mark.parametrize("camera,shape", [("all_listed", (8, 8)), ("all_listed", (24, 16)), ("mixed", (8, 8)), ("mixed", (37, 29)),
                                          ("hint_fails", (37, 29))],
                         ids=["all_listed-8x8", "all_listed-24x16", "mixed-8x8", "mixed-37x29", "hint_fails-37x29"])
def test_literal_class_primary_rays(gpu_ctx, cornell_small, camera, shape, small_lists):
    """8x8 is one workgroup: its list entries are traced by the stride loop, one after the other; 24x16 and 37x29 are 2 and 5
    workgroups with more entries than workgroups.  small_lists: the list holds 4 entries; what looks literal beyond them stays in
    the queue as a plain slot, and its own wave traces it whole."""
    from radish_pt_amd import api, hostlib

    w, h = shape
    cam = hostlib.make_camera(w, h, **LITERAL_CAMERAS[camera])
    _use(gpu_ctx, cornell_small, cam)
    listed, cls = _primary_classes(gpu_ctx)
    groups = ((w + 7) // 8) * ((h + 7) // 8)
    print(f"{camera} {w}x{h}: {int(listed.sum())} listed, {int((listed & (cls == 0)).sum())} of them of class 0, "
          f"{int((~listed & (cls != 0)).sum())} literal-class and not listed, {(groups + 3) // 4} workgroups")
    assert int((listed & (cls != 0)).sum()) > (groups + 3) // 4  # more entries to trace than workgroups
    if camera == "all_listed":
        assert listed.all() and (cls == 3).all()
    elif camera == "mixed":
        assert (cls == 3).all() and 0 < listed.sum() < w * h
    else:
        assert int((listed & (cls == 0)).sum()) > 0 and int((listed & (cls == 4)).sum()) > 0 and int((~listed & (cls == 0)).sum()) > 0
    ref = _oracle(cornell_small, cam, 1)
    assert ref["stats"]["closestHits"] >= w * h  # every primary ray hits the room
    flags = _flags(api) | (api.RDH_PT_WF_SMALL_LISTS if small_lists else 0)
    _four_frames(gpu_ctx, 1, flags, ref, f"{camera} {w}x{h}{' small lists' if small_lists else ''}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the entries that share the stage loop
# ---------------------------------------------------------------------------------------------------------------------------------
def test_three_samples_in_one_pass(gpu_ctx, cornell_small):
    from radish_pt_amd import api, scenes

    cam = scenes.cornell_camera(37, 29)
    ref = _oracle(cornell_small, cam, 3, samples=3)
    _use(gpu_ctx, cornell_small, cam)
    _four_frames(gpu_ctx, 3, _flags(api), ref, "three samples", samples=3)


def test_rank_one_of_two(gpu_ctx, cornell_small):
    """64x96 in tiles of 64: rank 1 of 2 renders the rows from 64 on, which the oracle takes as a pixel range."""
    from radish_pt_amd import api, partition, scenes

    w, h, depth = 64, 96, 1
    cam = scenes.cornell_camera(w, h)
    frame_idx, packed_idx = partition.rank_pixels(w, h, 1, 2, 64)
    assert np.array_equal(frame_idx, np.arange(64 * 64, 64 * 96))
    ref = _oracle(cornell_small, cam, depth, pix=(64 * 64, 64 * 96))
    _use(gpu_ctx, cornell_small, cam)
    try:
        gpu_ctx.set_partition(1, 2, 64)
        _four_frames(gpu_ctx, depth, _flags(api), ref, "rank 1 of 2", elems=gpu_ctx.tiles_per_rank() * 64 * 64, select=(frame_idx, packed_idx))
    finally:
        gpu_ctx.set_partition(0, 1, 64)


def test_adaptive_call_with_scattered_blocks(gpu_ctx, cornell_small):
    """One rdh_path_trace_adaptive over counts of zero: requests of 0..3 samples with whole blocks at 0 and blocks of one pixel, so a
    64-slot group of stage 0 holds several samples of a pixel and the pixels of more than one block."""
    import adaptive_oracle as ao
    from radish_pt_amd import api, scenes

    torch = _torch()
    w, h, depth, num = 37, 29, 2, 3
    p = w * h
    cam = scenes.cornell_camera(w, h)
    fr = ao.frames(cornell_small, cam, LOOPER, num, depth)
    rng = np.random.default_rng(5)
    request = rng.integers(0, num + 1, p).astype(np.int32)
    y, x = np.divmod(np.arange(p), w)
    block = (y // 8) * ((w + 7) // 8) + x // 8
    blocks = rng.permutation(block.max() + 1)
    for b in blocks[:6]:
        request[block == b] = 0
    for b in blocks[6:10]:
        keep = rng.choice(np.flatnonzero(block == b))
        request[(block == b) & (np.arange(p) != keep)] = 0
        request[keep] = num
    count = np.zeros(p, np.int32)
    on = request > 0
    assert on.sum() > 200 and (~on).sum() > 200 and request.sum() % 64 != 0
    counters = ao.pair_counters(cornell_small, cam, LOOPER, count, request, depth)
    ed, ei = ao.means_at(fr, request)
    _use(gpu_ctx, cornell_small, cam)
    got = {}
    for packets in (True, False):
        flags = _flags(api) | api.RDH_PT_COUNT | (0 if packets else api.RDH_PT_NO_PACKETS)
        d, i = torch.zeros(p, 3, device="cuda"), torch.zeros(p, 3, device="cuda")
        c, r = torch.zeros(p, dtype=torch.int32, device="cuda"), torch.from_numpy(request).cuda()
        gpu_ctx.counters_reset()
        traced = gpu_ctx.path_trace_adaptive(d, i, c, r, LOOPER, depth, flags)
        ct = gpu_ctx.counters()
        what = f"adaptive, {'packets' if packets else 'no packets'}"
        assert traced == int(request.sum()), what
        assert_bit_equal(d.cpu().numpy()[on], ed[on], f"{what}: direct vs oracle")
        assert_bit_equal(i.cpu().numpy()[on], ei[on], f"{what}: indirect vs oracle")
        assert not d.cpu().numpy()[~on].any() and np.array_equal(c.cpu().numpy(), request), what
        for k in COUNTER_KEYS:
            assert ct[k] == counters[k], (what, k, ct[k], counters[k])
        got[packets] = (d.cpu().numpy(), i.cpu().numpy(), ct)
    assert_bit_equal(got[True][0], got[False][0], "adaptive: direct, packets vs none")
    assert_bit_equal(got[True][1], got[False][1], "adaptive: indirect, packets vs none")
    assert got[True][2] == got[False][2]


CHILD_TIMEOUT = 300  # seconds; the child takes a few (start-up, the oracle's 131 072 pixels at depth 1, 4 wavefront frames)
CHILD = r"""
import numpy as np
import torch
from helpers import assert_bit_equal, oracle_path_trace_mt
from radish_pt_amd import api, scenes

W, H, depth, looper = 512, 256, 1, 23
keys = ("closestRays", "anyRays", "nodeVisits", "triTests", "closestHits")
sd = scenes.cornell(segments=16, bands=12)
cam = scenes.cornell_camera(W, H)
rd, ri = np.zeros((W * H, 3), np.float32), np.zeros((W * H, 3), np.float32)
_, st = oracle_path_trace_mt(sd, cam, rd, ri, 0, looper, depth)
ctx = api.Context(0)
ctx.set_partition(0, 1, 64)
ctx.upload_scene(sd)
ctx.set_camera(cam)
base = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_WF_SUBFRAMES
for packets in (True, False):
    for count in (True, False):
        flags = base | (0 if packets else api.RDH_PT_NO_PACKETS) | (api.RDH_PT_COUNT if count else 0)
        d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
        ctx.counters_reset()
        ctx.path_trace(d, i, 0, looper, depth, flags)
        ct = ctx.counters()
        what = f"two pipelines packets={packets} count={count}"
        assert_bit_equal(d.cpu().numpy(), rd, what + ": direct vs oracle")
        assert_bit_equal(i.cpu().numpy(), ri, what + ": indirect vs oracle")
        if count:
            assert all(ct[k] == st[k] for k in keys), (what, ct, st)
        print(what + ": ok", flush=True)
ctx.close()
"""


def test_two_subframe_pipelines():
    """RADISH_WF_PARTS is read once per process: a child renders Cornell at 512x256 (2 048 blocks, where sub-frames engage) as two
    pipelines of 1 024 blocks, each with its own stage-0 launch on its own stream (the pattern of test_gpu_samples_subframes.py)."""
    env = dict(os.environ, RADISH_WF_PARTS="2")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    print(r.stdout)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert r.stdout.count(": ok") == 4


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes and trees
# ---------------------------------------------------------------------------------------------------------------------------------
def test_environment_map(gpu_ctx):
    from radish_pt_amd import api, scenes

    sd = scenes.cornell_textured(segments=16, bands=12, env=True)
    cam = scenes.cornell_camera(37, 29)
    ref = _oracle(sd, cam, 3)
    _use(gpu_ctx, sd, cam)
    _four_frames(gpu_ctx, 3, _flags(api), ref, "environment map")


def test_no_emitters(gpu_ctx, cornell_small):
    from radish_pt_amd import api, layouts as L, scenes

    mats = cornell_small.materials.copy()
    for m in range(len(mats)):
        if mats[m]["type"] == L.LIGHT:
            mats[m] = L.make_material(L.LAMBERTIAN, (0.73, 0.73, 0.73))
    sd = scenes.SceneData("cornell_unlit", cornell_small.vertices, cornell_small.normals, cornell_small.texcoords,
                          cornell_small.material_ids, mats)
    assert sd.num_lights == 0
    cam = scenes.cornell_camera(37, 29)
    ref = _oracle(sd, cam, 3)
    assert ref["stats"]["anyRays"] == 0
    _use(gpu_ctx, sd, cam)
    _four_frames(gpu_ctx, 3, _flags(api), ref, "no emitters")


@pytest.mark.parametrize("case", ("lbvh_cornell", "refit_scrambled"))
def test_lbvh_and_refitted_trees(case):
    """The tree of the LBVH builder, and the SAH tree refitted to scrambled teapots, whose primary rays go past the packet budget of
    256 visits (test_gpu_tree_shapes.py); the oracle walks the restated tree."""
    from radish_pt_amd import api
    from test_gpu_tree_shapes import _camera, _device_with_tree
    from test_tree_shapes_cpu import tree_case

    sd, calls, target = tree_case(case)
    cam = _camera(case, 37, 29)
    ref = _oracle(target, cam, 3, key=case)
    ctx = _device_with_tree(sd, calls, target, case)
    try:
        ctx.set_camera(cam)
        for structure in ("sorted_pairs", "unsorted_threaded"):
            _four_frames(ctx, 3, _flags(api, structure), ref, f"{case} {structure}")
    finally:
        ctx.close()
