"""Motion vectors that follow moved geometry (rdh_scene_track_motion).

Scene: cornell_small with one stand-in (the dielectric one, material id motion_model.MOVED_MATERIAL) deformed per frame by a
translation plus a twist, three frames, a camera that also moves.  The expected motion plane is motion_model.motion_plane, which
test_motion_model_cpu.py pins to the oracle; every other plane and the work counters are the oracle's own, on the tree the update
leaves (the host builder's, the LBVH restatement's, or the uploaded topology with refitted boxes)."""
import ctypes as C
import functools

import numpy as np
import pytest

import lbvh_model
import motion_model
import refit_model
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

W, H = 151, 91  # odd: an axis-aligned camera's centre row and column are literal-class rays
METHODS = ["sah", "lbvh", "refit"]
RDH_REUSE_TEMPORAL, RDH_REUSE_SPATIAL = 1, 2


def _torch():
    import torch

    return torch


def _cuda(a):
    return _torch().from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _kernel_flags(kernel):
    from radish_pt_amd import api

    return {"packets": 0, "persistent": api.RDH_PT_NO_PACKETS, "one_lane_per_pixel": api.RDH_PT_ONE_LANE_PER_PIXEL,
            "no_defer": api.RDH_PT_NO_DEFER}[kernel]


KERNELS = ["packets", "persistent", "one_lane_per_pixel", "no_defer"]


@functools.lru_cache(maxsize=None)
def _base():
    from radish_pt_amd import scenes

    return scenes.cornell(segments=16, bands=12)


@functools.lru_cache(maxsize=None)
def _frame_scene(method, step):
    """The scene of deformation `step` carrying the tree that `method` leaves on the device: the host builder's (update_geometry's
    SAH builder gives it bit for bit), the LBVH restatement's, or the uploaded topology with the restatement's refitted boxes."""
    sd = _base()
    m = motion_model.deformed(sd, step)
    if method == "lbvh":
        m.boxes, m.nodes = lbvh_model.build(m.vertices)
    elif method == "refit":
        m.nodes = [n.copy() for n in sd.nodes]
        m.boxes = refit_model.refit_boxes(m.vertices, sd.nodes)
    return m


def _apply(ctx, method, m):
    v, n, lights = _cuda(m.vertices), _cuda(m.normals), (m.light_sampler, m.sum_light_power_inv)
    if method == "refit":
        ctx.refit_geometry(v, n, lights)
    else:
        ctx.update_geometry(v, n, lights, builder=method)


def _start(ctx, sd, track):
    ctx.set_partition(0, 1, 64)
    ctx.upload_scene(sd)
    if track:
        ctx.track_motion(True)


def _render(ctx, gb, cam, flags=0):
    ctx.set_camera(cam)
    ctx.counters_reset()
    ctx.gbuffer_render(gb.c_struct(cam_fallback=cam), flags)
    ctx.synchronize()
    k = gb.frameIdx
    return {"albedo": gb.albedo.cpu().numpy().copy(), "normal": gb.normal[k].cpu().numpy().copy(), "depth": gb.depth[k].cpu().numpy().copy(),
            "primId": gb.primId[k].cpu().numpy().copy(), "motion": gb.motion.cpu().numpy().copy()}


def _oracle_render(o, gb_ref, cam):
    before = o.stats()
    o.gbuffer_render(cam, gb_ref)
    after = o.stats()
    return {k: after[k] - before[k] for k in ("closestRays", "nodeVisits", "triTests", "closestHits")}


def _assert_planes(got, gb_ref, what, motion=None):
    k = gb_ref.frameIdx
    assert np.array_equal(got["primId"], gb_ref.primId[k]), f"{what}: primId"
    assert_bit_equal(got["albedo"], gb_ref.albedo, f"{what}: albedo")
    assert_bit_equal(got["normal"], gb_ref.normal[k], f"{what}: normal")
    assert_bit_equal(got["depth"], gb_ref.depth[k], f"{what}: depth")
    want = gb_ref.motion if motion is None else motion
    bad = np.flatnonzero(got["motion"] != want)
    assert len(bad) == 0, f"{what}: motion differs at {len(bad)} pixels, first {bad[:4].tolist()}: {got['motion'][bad[:4]].tolist()} vs {want[bad[:4]].tolist()}"


def _gbuffers():
    from oracle import pyoracle
    from radish_pt_amd import api

    gb = api.GBuffer()
    gb.create(W, H)
    return gb, pyoracle.GBufferHost(W, H)


def _last(gb_ref, cam):
    return gb_ref.lastCam if gb_ref.lastCam is not None else cam


# ---- 1. moved geometry, exact ----

@pytest.mark.parametrize("literal", [False, True])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("method", METHODS)
def test_moved_geometry_exact(gpu_ctx, method, kernel, literal):
    from oracle import pyoracle
    from radish_pt_amd import api

    sd = _base()
    _start(gpu_ctx, sd, track=True)
    gb, gb_ref = _gbuffers()
    prev = sd
    for f, cam in enumerate(motion_model.moving_cameras(W, H, literal=literal)):
        cur = _frame_scene(method, f + 1)
        _apply(gpu_ctx, method, cur)
        o = pyoracle.OracleScene(cur)
        work = _oracle_render(o, gb_ref, cam)
        want = motion_model.motion_plane(o, cur.vertices, prev.vertices, cam, _last(gb_ref, cam))
        got = _render(gpu_ctx, gb, cam, _kernel_flags(kernel) | api.RDH_PT_COUNT)
        _assert_planes(got, gb_ref, f"{method} {kernel} frame {f}", motion=want)
        ct = gpu_ctx.counters()
        for k, v in work.items():
            assert ct[k] == v, f"{method} {kernel} frame {f}: {k} {ct[k]} vs {v}"
        moved = gb_ref.primId[gb_ref.frameIdx] == motion_model.MOVED_MATERIAL
        share = (want[moved] != gb_ref.motion[moved]).mean()
        print(f"{method} {kernel} literal={literal} frame {f}: {moved.sum()} moved pixels, {share:.2f} with a tracked index of their own")
        assert moved.sum() >= 30 and share >= 0.2, "the case cannot tell tracking from none"
        assert np.array_equal(want[~moved], gb_ref.motion[~moved])
        gb_ref.update(cam)
        gb.update(cam)
        prev = cur


# ---- 2. equal vertices, equal bits ----

@pytest.mark.parametrize("literal", [False, True])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("method", METHODS)
def test_equal_vertices_equal_bits(gpu_ctx, method, kernel, literal):
    """An update with the uploaded vertices while tracking: the kernels interpolate the kept records, and every plane, motion
    included, equals the untracked render bit for bit (the interpolation is fetchSurface's expression, operand for operand)."""
    sd = _base()
    cams = motion_model.moving_cameras(W, H, literal=literal)
    own = _frame_scene(method, 0)
    planes = {}
    for track in (False, True):
        _start(gpu_ctx, sd, track)
        gb, _ = _gbuffers()
        _render(gpu_ctx, gb, cams[0], _kernel_flags(kernel))
        gb.update(cams[0])
        _apply(gpu_ctx, method, own)
        planes[track] = _render(gpu_ctx, gb, cams[1], _kernel_flags(kernel))
    for name in planes[True]:
        assert np.array_equal(planes[True][name].view(np.uint32), planes[False][name].view(np.uint32)), f"{method} {kernel}: {name}"
    assert (planes[True]["motion"] > 0).mean() > 0.05


# ---- 3. off means off ----

@pytest.mark.parametrize("mode", ["never", "disabled"])
@pytest.mark.parametrize("method", METHODS)
def test_off_means_off(gpu_ctx, method, mode):
    from oracle import pyoracle

    sd = _base()
    _start(gpu_ctx, sd, track=(mode == "disabled"))
    gb, gb_ref = _gbuffers()
    for f, cam in enumerate(motion_model.moving_cameras(W, H)):
        if mode == "disabled" and f == 1:
            gpu_ctx.track_motion(False)
            gpu_ctx.track_motion(False)  # twice: a no-op
        cur = _frame_scene(method, f + 1)
        _apply(gpu_ctx, method, cur)
        o = pyoracle.OracleScene(cur)
        _oracle_render(o, gb_ref, cam)
        got = _render(gpu_ctx, gb, cam)
        if mode == "never" or f >= 1:
            _assert_planes(got, gb_ref, f"{method} {mode} frame {f}")  # the static rule: the oracle's own plane
        gb_ref.update(cam)
        gb.update(cam)


# ---- 4. the flag's state machine ----

def test_flag_state_machine(gpu_ctx):
    from oracle import pyoracle
    from radish_pt_amd import api

    sd = _base()
    cams = motion_model.moving_cameras(W, H, frames=5)
    fresh = api.Context(0)
    try:
        with pytest.raises(api.RadishError):
            fresh.track_motion(True)  # RDH_ERR_NO_SCENE
        assert api.lib().rdh_scene_track_motion(fresh.h, 1) == -2
    finally:
        fresh.close()
    _start(gpu_ctx, sd, track=True)
    gpu_ctx.track_motion(True)  # twice: a no-op
    gb, gb_ref = _gbuffers()
    steps = [_frame_scene("sah", s) for s in range(4)]

    def frame(cam, cur, prev, what):
        o = pyoracle.OracleScene(cur)
        _oracle_render(o, gb_ref, cam)
        want = motion_model.motion_plane(o, cur.vertices, prev.vertices, cam, _last(gb_ref, cam))
        got = _render(gpu_ctx, gb, cam)
        _assert_planes(got, gb_ref, what, motion=want)
        moved = gb_ref.primId[gb_ref.frameIdx] == motion_model.MOVED_MATERIAL
        differs = (want[moved] != gb_ref.motion[moved]).mean()
        gb_ref.update(cam)
        gb.update(cam)
        return differs

    # no update yet: the static rule
    assert frame(cams[0], steps[0], steps[0], "before any update") == 0.0
    # two updates, then one render: "previous" is what the last render saw (step 0), not what the first update left (step 1)
    # (three in fact, through each entry: an update, a refit of its tree, and an update whose tree is the oracle's)
    _apply(gpu_ctx, "sah", steps[1])
    _apply(gpu_ctx, "refit", steps[2])
    _apply(gpu_ctx, "lbvh", steps[3])
    _apply(gpu_ctx, "sah", steps[2])
    assert frame(cams[1], steps[2], steps[0], "two updates, one render") >= 0.2
    # a second render with no update in between: zero object motion, the static rule
    assert frame(cams[2], steps[2], steps[2], "render, render") == 0.0
    # a refused update between a good one and the render changes nothing
    _apply(gpu_ctx, "sah", steps[3])
    v = _cuda(steps[1].vertices)
    assert api.lib().rdh_scene_update_geometry_ex(gpu_ctx.h, C.c_void_p(v.data_ptr()), None, None, 7) == -1
    assert api.lib().rdh_scene_refit_geometry(gpu_ctx.h, None, None, None) == -1
    assert frame(cams[3], steps[3], steps[2], "a refused update in between") >= 0.2
    # rdh_scene_upload switches tracking off
    gpu_ctx.upload_scene(sd)
    _apply(gpu_ctx, "sah", steps[1])
    o = pyoracle.OracleScene(steps[1])
    _oracle_render(o, gb_ref, cams[4])
    _assert_planes(_render(gpu_ctx, gb, cams[4]), gb_ref, "after a new upload")


# ---- 5. the consumers, end to end ----

@pytest.mark.parametrize("method", METHODS)
def test_restir_follows_tracked_motion(gpu_ctx, method):
    """update -> tracked render -> rdh_restir_direct with temporal and spatial reuse, against the oracle's restir_direct on its own
    G-buffer whose motion plane is the model's: image and the three reservoir buffers bit-equal on every frame."""
    from oracle import pyoracle
    from radish_pt_amd import layouts as L

    torch = _torch()
    sd = _base()
    n = W * H
    reuse = RDH_REUSE_TEMPORAL | RDH_REUSE_SPATIAL
    cams = motion_model.moving_cameras(W, H)
    _start(gpu_ctx, sd, track=True)
    gb, gb_ref = _gbuffers()
    res = [np.zeros(n, L.RESERVOIR_DTYPE) for _ in range(3)]  # cur, last, temp (restir.cu:4-7)
    ref_img = np.zeros((n, 3), np.float32)
    img = torch.zeros(n, 3, device="cuda")
    gpu_ctx.set_camera(cams[0])
    gpu_ctx.restir_init()
    try:
        prev = sd
        for f, cam in enumerate(cams):
            cur = _frame_scene(method, f + 1)
            _apply(gpu_ctx, method, cur)
            o = pyoracle.OracleScene(cur)
            _oracle_render(o, gb_ref, cam)
            gb_ref.motion[:] = motion_model.motion_plane(o, cur.vertices, prev.vertices, cam, _last(gb_ref, cam))
            _assert_planes(_render(gpu_ctx, gb, cam), gb_ref, f"{method} frame {f}")
            o.restir_direct(cam, ref_img, 0, 40 + f, res[0], res[1], res[2], gb_ref, f == 0, reuse, 1)
            res[0], res[1] = res[1], res[0]  # std::swap(directReservoir, lastDirectReservoir)
            gpu_ctx.restir_direct(img, 0, 40 + f, gb.c_struct(cam), reuse)
            gpu_ctx.synchronize()
            assert_bit_equal(img.cpu().numpy(), ref_img, f"{method}: ReSTIR image, frame {f}")
            for which, name in ((1, "last"), (0, "cur"), (2, "temp")):
                same = gpu_ctx.restir_read(which).tobytes() == res[which].tobytes()
                print(f"{method} frame {f}: reservoirs `{name}` equal: {same}")
                assert same, f"{method}: reservoirs `{name}`, frame {f}"
            gb_ref.update(cam)
            gb.update(cam)
            prev = cur
        assert ref_img.max() > 0
    finally:
        gpu_ctx.restir_free()


@pytest.mark.parametrize("method", METHODS)
def test_temporal_accumulate_follows_tracked_motion(gpu_ctx, method):
    """SVGF's temporal accumulation over the three frames: colour and moment planes bit-equal against the oracle fed the model's
    motion plane."""
    from oracle import pyoracle

    torch = _torch()
    sd = _base()
    n = W * H
    rng = np.random.default_rng(5)
    _start(gpu_ctx, sd, track=True)
    gb, gb_ref = _gbuffers()
    acc_c, acc_m = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    prev = sd
    for f, cam in enumerate(motion_model.moving_cameras(W, H)):
        cur = _frame_scene(method, f + 1)
        _apply(gpu_ctx, method, cur)
        o = pyoracle.OracleScene(cur)
        _oracle_render(o, gb_ref, cam)
        gb_ref.motion[:] = motion_model.motion_plane(o, cur.vertices, prev.vertices, cam, _last(gb_ref, cam))
        _assert_planes(_render(gpu_ctx, gb, cam), gb_ref, f"{method} frame {f}")
        noisy = rng.uniform(0.0, 2.0, (n, 3)).astype(np.float32)
        want_c, want_m = pyoracle.denoise_temporal_accumulate(acc_c, acc_m, noisy, gb_ref, f == 0)
        co, mo = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda")
        gpu_ctx.denoise_temporal_accumulate(co, _cuda(acc_c), mo, _cuda(acc_m), _cuda(noisy), gb.c_struct(cam), f == 0)
        gpu_ctx.synchronize()
        assert_bit_equal(co.cpu().numpy(), want_c, f"{method}: accumulated colour, frame {f}")
        assert_bit_equal(mo.cpu().numpy(), want_m, f"{method}: accumulated moments, frame {f}")
        acc_c, acc_m = want_c, want_m
        gb_ref.update(cam)
        gb.update(cam)
        prev = cur


# ---- 6. it does what it is for ----

@pytest.mark.parametrize("method", METHODS)
def test_more_of_the_moved_object_finds_its_temporal_neighbour(gpu_ctx, method):
    """On frames 1 and 2, over the moved object's pixels: how many indices pass findTemporalNeighbor's tests against last frame's
    planes, with tracking and, on a second context, without.  Tracking must win; the counts go to DESIGN 11d."""
    from radish_pt_amd import api

    sd = _base()
    other = api.Context(0)
    try:
        _start(gpu_ctx, sd, track=True)
        _start(other, sd, track=False)
        gbs = {True: _gbuffers()[0], False: _gbuffers()[0]}
        count = {True: 0, False: 0}
        last = {}
        total = 0
        for f, cam in enumerate(motion_model.moving_cameras(W, H)):
            cur = _frame_scene(method, f + 1)
            for track, ctx in ((True, gpu_ctx), (False, other)):
                _apply(ctx, method, cur)
                p = _render(ctx, gbs[track], cam)
                if f >= 1:
                    moved = p["primId"] == motion_model.MOVED_MATERIAL
                    ok = motion_model.passes_temporal_test(p["motion"], p["primId"], last[track]["primId"], p["normal"], last[track]["normal"])
                    count[track] += int((ok & moved).sum())
                    total += int(moved.sum()) if track else 0
                last[track] = p
                gbs[track].update(cam)
        print(f"{method}: of {total} pixels of the moved object on frames 1 and 2, {count[True]} find their temporal neighbour with tracking, "
              f"{count[False]} without")
        assert count[True] > count[False]
    finally:
        other.close()


# ---- 7. partition ----

def test_partitioned_tracked_render(gpu_ctx):
    """Two virtual ranks, each tracking the whole scene: the partitioned tracked render plus pack / unpack equals the
    single-context tracked planes."""
    from radish_pt_amd import api

    torch = _torch()
    sd = _base()
    world, tile = 2, 32
    cams = motion_model.moving_cameras(W, H)
    _start(gpu_ctx, sd, track=True)
    ref_gb, _ = _gbuffers()
    ctxs, gbs = [], []
    try:
        for rank in range(world):
            c = api.Context(0)
            c.upload_scene(sd)
            c.track_motion(True)
            c.set_camera(cams[0])
            c.set_partition(rank, world, tile)
            ctxs.append(c)
            gbs.append(_gbuffers()[0])
        tpr = ctxs[0].tiles_per_rank()
        for f, cam in enumerate(cams):
            cur = _frame_scene("lbvh", f + 1)
            _apply(gpu_ctx, "lbvh", cur)
            want = _render(gpu_ctx, ref_gb, cam)
            ref_gb.update(cam)
            packs = []
            for c, g in zip(ctxs, gbs):
                _apply(c, "lbvh", cur)
                c.set_camera(cam)
                c.gbuffer_render(g.c_struct(cam_fallback=cam), api.RDH_PT_PARTITION_GBUFFER)
                pk = torch.zeros(tpr * tile * tile, 9, device="cuda")
                c.gbuffer_exchange_pack(g.c_struct(cam_fallback=cam), pk)
                c.synchronize()
                packs.append(pk)
            gathered = torch.cat(packs).contiguous()
            for r, (c, g) in enumerate(zip(ctxs, gbs)):
                c.gbuffer_exchange_unpack(g.c_struct(cam_fallback=cam), gathered)
                c.synchronize()
                k = g.frameIdx
                got = {"albedo": g.albedo, "normal": g.normal[k], "depth": g.depth[k], "primId": g.primId[k], "motion": g.motion}
                for name, t in got.items():
                    assert np.array_equal(t.cpu().numpy().view(np.uint32), want[name].view(np.uint32)), f"rank {r} frame {f}: {name}"
                g.update(cam)
    finally:
        for c in ctxs:
            c.close()
        gpu_ctx.set_partition(0, 1, 64)
