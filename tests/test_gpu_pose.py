"""Objects posed on the device (rdh_scene_set_objects, rdh_scene_pose_objects, kernels_pose.h).

Everything hangs on one equality: the arrays k_pose_objects writes equal, bit for bit, what the host loader produces for a scene file
that carries the same Translate / Rotate / Scale.  test_pose_cpu.py pins pose_model to the loader; here the device is pinned to
pose_model and to a second scene file, and the posed scene's trees, frames and counters to contexts that were given the same arrays
through the entries the rest of the suite pins to the oracle (upload, update_geometry, refit_geometry)."""
import ctypes as C

import numpy as np
import pytest

import motion_model
import pose_model
import pose_scene
import test_gpu_motion as tgm
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

W, H = 64, 48
DEPTH = 3
TREES = ["refit", "sah", "lbvh"]


def _torch():
    import torch

    return torch


def _cuda(a):
    return _torch().from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The scene file, a second file carrying pose_scene.POSED, and the model's arrays for POSED (computed once, never changed)."""
    from radish_pt_amd import scenes

    d = str(tmp_path_factory.mktemp("pose_gpu"))
    pose_scene.write_meshes(d)
    sd, cam, _ = scenes.load_scene_file(pose_scene.write_scene(d, "scene.txt"))
    sd2, cam2, _ = scenes.load_scene_file(pose_scene.write_scene(d, "posed.txt", pose_scene.POSED))
    assert (int(cam["resolution"][0]), int(cam["resolution"][1])) == (W, H) and cam.tobytes() == cam2.tobytes()
    v, n = pose_model.pose(sd.rest_vertices, sd.rest_normals, sd.objects, pose_scene.xforms(pose_scene.POSED))
    for a in (v, n, sd.vertices, sd.normals, sd2.vertices, sd2.normals):
        a.setflags(write=False)
    return {"dir": d, "sd": sd, "cam": cam, "sd2": sd2, "model": (v, n), "trs": pose_scene.trs_array(pose_scene.POSED)}


@pytest.fixture
def make_ctx():
    """Contexts of a test's own, closed when it ends."""
    from radish_pt_amd import api

    made = []

    def make(sd=None, cam=None, objects=False):
        c = api.Context(0)
        made.append(c)
        if sd is not None:
            c.upload_scene(sd)
            if objects:
                c.set_objects(sd)
        if cam is not None:
            c.set_camera(cam)
        return c

    yield make
    for c in made:
        c.close()


def _with_vertices(sd, v, n, name="moved"):
    from radish_pt_amd import scenes

    return scenes.SceneData(name, v, n, sd.texcoords, sd.material_ids, sd.materials, sd.textures, sd.env_map_tex_id)


def _frames(ctx, cam):
    """The persistent path-trace frame (depth 3), every G-buffer plane and the work counters of both."""
    from radish_pt_amd import api

    torch = _torch()
    out = {}
    d = torch.zeros(W * H, 3, device="cuda")
    i = torch.zeros(W * H, 3, device="cuda")
    ctx.set_camera(cam)
    ctx.counters_reset()
    ctx.path_trace(d, i, 0, 2, DEPTH, api.RDH_PT_PERSISTENT | api.RDH_PT_COUNT)
    ctx.synchronize()
    out["direct"], out["indirect"], out["pt counters"] = d.cpu().numpy(), i.cpu().numpy(), ctx.counters()
    gb = api.GBuffer()
    gb.create(W, H)
    ctx.counters_reset()
    ctx.gbuffer_render(gb.c_struct(cam_fallback=cam), api.RDH_PT_COUNT)
    ctx.synchronize()
    k = gb.frameIdx
    for name, t in (("albedo", gb.albedo), ("normal", gb.normal[k]), ("depth", gb.depth[k]), ("primId", gb.primId[k]), ("motion", gb.motion)):
        out[name] = t.cpu().numpy().copy()
    out["gbuffer counters"] = ctx.counters()
    gb.destroy()
    return out


def _assert_same_frames(a, b, what):
    assert a["direct"].max() > 0 and (a["primId"] >= 0).sum() > 200, f"{what}: the frame shows nothing"
    for name in a:
        if isinstance(a[name], dict):
            assert a[name] == b[name], f"{what}: {name} {a[name]} vs {b[name]}"
        else:
            assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), f"{what}: {name} differs"


def _assert_world(ctx, v, n, what):
    gv, gn = ctx.debug_read_world()
    assert_bit_equal(gv, v, f"{what}: world vertices")
    assert_bit_equal(gn, n, f"{what}: world normals")


# ---- 1. pose on the device == load the posed file ----

def test_posed_scene_equals_the_posed_file(files, make_ctx):
    sd, sd2, cam = files["sd"], files["sd2"], files["cam"]
    a = make_ctx(sd, cam, objects=True)
    _assert_world(a, sd.vertices, sd.normals, "after set_objects")
    a.pose_objects(np.arange(6), trs=files["trs"], tree="sah", rebuild_lights=True)
    _assert_world(a, *files["model"], "posed, against the model")
    _assert_world(a, sd2.vertices, sd2.normals, "posed, against the second file")
    b = make_ctx(sd2, cam)
    for which in (0, 1, 2):
        assert np.array_equal(a.debug_read_tree(which), b.debug_read_tree(which)), f"tree part {which}"
        assert np.array_equal(a.debug_read_lights(which), b.debug_read_lights(which)), f"light part {which}"
    _assert_same_frames(_frames(a, cam), _frames(b, cam), "posed vs fresh upload of the posed file")


# ---- 2. each tree path == the caller's own arrays through the existing entry ----

@pytest.mark.parametrize("tree", TREES)
def test_pose_equals_existing_entry(files, make_ctx, tree):
    sd, cam = files["sd"], files["cam"]
    v, n = files["model"]
    a = make_ctx(sd, cam, objects=True)
    a.pose_objects(np.arange(6), trs=files["trs"], tree=tree)
    b = make_ctx(sd, cam)
    if tree == "refit":
        b.refit_geometry(_cuda(v), _cuda(n))
    else:
        b.update_geometry(_cuda(v), _cuda(n), builder=tree)
    _assert_world(a, v, n, tree)
    for which in (0, 1, 2):
        ta, tb = a.debug_read_tree(which), b.debug_read_tree(which)
        assert len(ta) > 0 and np.array_equal(ta, tb), f"{tree}: tree part {which}"
    _assert_same_frames(_frames(a, cam), _frames(b, cam), tree)


# ---- 3. subsets ----

@pytest.mark.parametrize("which", [0, 5, 2], ids=["first", "last", "one-triangle"])
def test_pose_of_one_object(files, make_ctx, which):
    sd, cam = files["sd"], files["cam"]
    ctx = make_ctx(sd, cam, objects=True)
    o = sd.objects[which]
    lo, hi = 3 * int(o["firstPrim"]), 3 * (int(o["firstPrim"]) + int(o["numPrims"]))
    assert (which == 2) == (hi - lo == 3)
    trs = files["trs"][which:which + 1]
    want = pose_model.pose(sd.rest_vertices, sd.rest_normals, sd.objects, pose_scene.xforms([pose_scene.POSED[which]]), ids=[which],
                           world=(sd.vertices, sd.normals))
    assert not np.array_equal(want[0][lo:hi], sd.vertices[lo:hi])
    outside = np.ones(len(sd.vertices), bool)
    outside[lo:hi] = False
    assert np.array_equal(want[0][outside], sd.vertices[outside]) and np.array_equal(want[1][outside], sd.normals[outside])
    ctx.pose_objects([which], trs=trs)
    _assert_world(ctx, *want, "one object")
    ctx.pose_objects([which], trs=trs)  # idempotent: the rest pose is the source, not the world arrays
    _assert_world(ctx, *want, "the same pose again")
    before = ctx.debug_read_tree(0).copy()
    ctx.pose_objects([], trs=np.zeros((0, 9), np.float32))  # count == 0
    _assert_world(ctx, *want, "count == 0")
    assert np.array_equal(ctx.debug_read_tree(0), before)
    b = make_ctx(sd, cam)
    b.refit_geometry(_cuda(want[0]), _cuda(want[1]))
    _assert_same_frames(_frames(ctx, cam), _frames(b, cam), "one object")


# ---- 4. many tiny objects ----

def test_many_tiny_objects(make_ctx):
    """70 objects of one triangle and one of 150 over a soup of 220 triangles: more prefix entries than a wave has lanes, workgroups
    that serve a single row of three vertices, and a partial tail workgroup (450 vertices = 256 + 194).  The ids are listed in a
    shuffled order, and some objects share a rest range."""
    from radish_pt_amd import hostlib, scenes

    sd = scenes.tiny(n_tris=218)
    assert sd.num_prims == 220
    table = np.zeros(71, [("firstPrim", "<i4"), ("numPrims", "<i4"), ("restFirstPrim", "<i4")])
    table["firstPrim"] = np.arange(71)
    table["numPrims"] = 1
    table["numPrims"][70] = 150
    table["restFirstPrim"] = np.arange(71)
    table["restFirstPrim"][10:20] = 3  # ten instances of triangle 3
    rng = np.random.default_rng(11)
    ids = rng.permutation(71)
    rows = [(rng.uniform(-0.5, 0.5, 3), rng.uniform(-180, 180, 3), rng.uniform(0.5, 1.5, 3) * rng.choice([-1.0, 1.0], 3)) for _ in ids]
    xf = np.stack([hostlib.object_transform(*r) for r in rows])
    want = pose_model.pose(sd.vertices, sd.normals, table, xf, ids=ids, world=(sd.vertices, sd.normals))
    for tree in ("lbvh", "refit"):
        ctx = make_ctx(sd)
        ctx.set_objects(objects=table, rest_vertices=sd.vertices, rest_normals=sd.normals)
        ctx.pose_objects(ids, xforms=xf, tree=tree)
        _assert_world(ctx, *want, f"many tiny objects, {tree}")
    assert not np.array_equal(want[0][:3 * 220], sd.vertices) and np.isfinite(want[1]).all()


# ---- 5. lights ----

def test_emissive_object_scaled_and_moved(files, make_ctx):
    from radish_pt_amd import api

    torch = _torch()
    sd, cam = files["sd"], files["cam"]
    _, _, t, r, s = pose_scene.OBJECTS[4]
    row = ((t[0] - 0.5, t[1] - 0.25, t[2] + 0.25), r, tuple(3.0 * x for x in s))
    v, n = pose_model.pose(sd.rest_vertices, sd.rest_normals, sd.objects, pose_scene.xforms([row]), ids=[4], world=(sd.vertices, sd.normals))
    moved = _with_vertices(sd, v, n)
    assert not np.array_equal(moved.light_sampler, sd.light_sampler) and moved.num_lights == 21

    def restir(ctx):
        gb = api.GBuffer()
        gb.create(W, H)
        dev = api.DevScene()
        dev.ctx = ctx
        gb.render(dev, cam)
        img = torch.zeros(W * H, 3, device="cuda")
        ctx.restir_init()
        ctx.restir_direct(img, 0, 1, gb.c_struct(cam), 3)
        ctx.synchronize()
        ctx.restir_free()
        gb.destroy()
        return img.cpu().numpy()

    a = make_ctx(sd, cam, objects=True)
    a.pose_objects([4], trs=pose_scene.trs_array([row]), rebuild_lights=True)
    b = make_ctx(sd, cam)
    b.refit_geometry(_cuda(v), _cuda(n), (moved.light_sampler, moved.sum_light_power_inv))
    assert np.array_equal(b.debug_read_lights(0), moved.light_sampler)
    for which in (0, 1, 2):
        assert np.array_equal(a.debug_read_lights(which), b.debug_read_lights(which)), f"light part {which}"
    ia, ib = restir(a), restir(b)
    assert ia.max() > 0
    assert_bit_equal(ia, ib, "ReSTIR frame")
    stale = make_ctx(sd, cam, objects=True)
    stale.pose_objects([4], trs=pose_scene.trs_array([row]))  # without the flag the table is the upload's
    assert np.array_equal(stale.debug_read_lights(0), sd.light_sampler)
    assert not np.array_equal(stale.debug_read_lights(0), a.debug_read_lights(0))


# ---- 6. motion ----

def test_motion_plane_follows_a_posed_object(files, make_ctx):
    from oracle import pyoracle
    from radish_pt_amd import api

    sd = files["sd"]
    cams = [files["cam"], files["cam"].copy()]  # the same camera twice: every motion index that changes is the object's
    ctx = make_ctx(sd, cams[0], objects=True)
    ctx.track_motion(True)
    gb, gb_ref = api.GBuffer(), pyoracle.GBufferHost(W, H)
    gb.create(W, H)
    o0 = pyoracle.OracleScene(sd)
    tgm._oracle_render(o0, gb_ref, cams[0])
    tgm._assert_planes(tgm._render(ctx, gb, cams[0]), gb_ref, "before the pose")
    gb_ref.update(cams[0])
    gb.update(cams[0])
    which = 0
    v, n = pose_model.pose(sd.rest_vertices, sd.rest_normals, sd.objects, pose_scene.xforms([pose_scene.POSED[which]]), ids=[which],
                           world=(sd.vertices, sd.normals))
    cur = _with_vertices(sd, v, n)
    ctx.pose_objects([which], trs=files["trs"][which:which + 1], tree="sah")
    o1 = pyoracle.OracleScene(cur)
    work = tgm._oracle_render(o1, gb_ref, cams[1])
    want = motion_model.motion_plane(o1, cur.vertices, sd.vertices, cams[1], tgm._last(gb_ref, cams[1]))
    got = tgm._render(ctx, gb, cams[1], api.RDH_PT_COUNT)
    tgm._assert_planes(got, gb_ref, "after the pose", motion=want)
    ct = ctx.counters()
    for k, x in work.items():
        assert ct[k] == x, f"{k}: {ct[k]} vs {x}"
    seen = gb_ref.primId[gb_ref.frameIdx] == int(sd.objects[which]["materialId"])
    tracked = (want[seen] != gb_ref.motion[seen]).mean()
    print(f"{seen.sum()} pixels of the posed object, {tracked:.2f} with a tracked index of their own")
    assert seen.sum() >= 30 and tracked >= 0.2, "the case cannot tell tracking from none"
    gb.destroy()


# ---- 7. state and errors ----

def _raw_pose(ctx, ids, xf, tree=0, flags=0):
    from radish_pt_amd import api

    ids = np.ascontiguousarray(ids, np.int32)
    xf = np.ascontiguousarray(xf, np.float32)
    return api.lib().rdh_scene_pose_objects(ctx.h, C.c_void_p(ids.ctypes.data), C.c_void_p(xf.ctypes.data), len(ids), tree, flags, 0.0)


def test_state_and_errors(files, make_ctx):
    from radish_pt_amd import api

    sd, cam = files["sd"], files["cam"]
    xf = pose_scene.xforms(pose_scene.POSED)
    ctx = make_ctx(sd, cam)
    assert _raw_pose(ctx, [0], xf[:1]) == -5  # RDH_ERR_STATE: no table
    with pytest.raises(api.RadishError):
        ctx.debug_read_world()
    ctx.set_objects(sd)
    tree0 = ctx.debug_read_tree(0).copy()
    assert _raw_pose(ctx, [0, 3, 0], xf[:3]) == -1       # listed twice
    assert _raw_pose(ctx, [0, 6], xf[:2]) == -1          # out of range
    assert _raw_pose(ctx, [-1], xf[:1]) == -1
    assert _raw_pose(ctx, [0], xf[:1], tree=7) == -1     # unknown tree
    assert _raw_pose(ctx, [0], xf[:1], flags=2) == -1    # unknown flag
    assert api.lib().rdh_scene_pose_objects(ctx.h, None, None, 1, 0, 0, 0.0) == -1
    assert api.lib().rdh_scene_pose_objects(ctx.h, None, None, 0, 0, 0, 0.0) == 0  # count == 0
    with pytest.raises(api.RadishError):
        ctx.pose_objects([0], trs=files["trs"][:1], tree="bvh")
    with pytest.raises(ValueError):  # singular: refused on the host, before any device call
        ctx.pose_objects([0], trs=np.array([[0, 0, 0, 0, 0, 0, 1, 0, 1]], np.float32))
    _assert_world(ctx, sd.vertices, sd.normals, "after refused calls")
    assert np.array_equal(ctx.debug_read_tree(0), tree0)
    # set_objects: overlapping ranges, ranges out of bounds
    rng3 = lambda rows: np.array(rows, np.int32)
    for bad in ([[0, 10, 0], [9, 5, 0]], [[640, 4, 0]], [[0, 5, 220]], [[-1, 2, 0]]):
        with pytest.raises(api.RadishError):
            ctx.set_objects(objects=rng3(bad), rest_vertices=sd.rest_vertices, rest_normals=sd.rest_normals)
    assert _raw_pose(ctx, [1], xf[1:2]) == 0  # a refused set_objects leaves the table in force
    # disjoint ranges that do not cover the scene are fine; an empty table clears it
    ctx.set_objects(objects=rng3([[200, 21, 200]]), rest_vertices=sd.rest_vertices, rest_normals=sd.rest_normals)
    assert _raw_pose(ctx, [1], xf[1:2]) == -1 and _raw_pose(ctx, [0], xf[1:2]) == 0
    ctx.set_objects(objects=np.zeros((0, 3), np.int32))
    assert _raw_pose(ctx, [0], xf[:1]) == -5
    # upload_scene drops the table
    ctx.set_objects(sd)
    ctx.upload_scene(sd)
    assert _raw_pose(ctx, [0], xf[:1]) == -5


def test_callers_own_refit_in_between(files, make_ctx):
    """pose all, then the caller's refit_geometry with noise-moved vertices, then a pose of one object: the listed object is the
    model's, every other triangle keeps the caller's vertices (and, the caller having passed no normals, the normals it had)."""
    sd, cam = files["sd"], files["cam"]
    v, n = files["model"]
    ctx = make_ctx(sd, cam, objects=True)
    ctx.pose_objects(np.arange(6), trs=files["trs"])
    noise = (v + np.random.default_rng(5).uniform(-0.01, 0.01, v.shape)).astype(np.float32)
    ctx.refit_geometry(_cuda(noise))
    row = pose_scene.OBJECTS[1][2:5]
    ctx.pose_objects([1], trs=pose_scene.trs_array([row]))
    want = pose_model.pose(sd.rest_vertices, sd.rest_normals, sd.objects, pose_scene.xforms([row]), ids=[1], world=(noise, n))
    o = sd.objects[1]
    lo, hi = 3 * int(o["firstPrim"]), 3 * (int(o["firstPrim"]) + int(o["numPrims"]))
    assert_bit_equal(want[0][lo:hi], sd.vertices[lo:hi], "the object's own transform gives the uploaded vertices")
    _assert_world(ctx, *want, "pose after the caller's refit")
    b = make_ctx(sd, cam)
    b.refit_geometry(_cuda(want[0]), _cuda(want[1]))
    _assert_same_frames(_frames(ctx, cam), _frames(b, cam), "pose after the caller's refit")


def test_eight_poses_and_frames_without_a_host_wait(files, make_ctx):
    """Eight pose + frame steps enqueued back to back (nothing reads back, nothing synchronises), then the last frame against a
    fresh upload of the file that carries the last pose."""
    from radish_pt_amd import api

    torch = _torch()
    sd, sd2, cam = files["sd"], files["sd2"], files["cam"]
    start, end = pose_scene.trs_array([o[2:5] for o in pose_scene.OBJECTS]), files["trs"]
    ctx = make_ctx(sd, cam, objects=True)
    d = torch.zeros(W * H, 3, device="cuda")
    i = torch.zeros(W * H, 3, device="cuda")
    for step in range(1, 9):
        f = np.float32(step / 8.0)
        trs = end if step == 8 else (start + (end - start) * f).astype(np.float32)
        ctx.pose_objects(np.arange(6), trs=trs, tree="sah", rebuild_lights=True)
        ctx.path_trace(d, i, 0, 2, DEPTH, api.RDH_PT_PERSISTENT)
    ctx.synchronize()
    b = make_ctx(sd2, cam)
    d2 = torch.zeros(W * H, 3, device="cuda")
    i2 = torch.zeros(W * H, 3, device="cuda")
    b.path_trace(d2, i2, 0, 2, DEPTH, api.RDH_PT_PERSISTENT)
    b.synchronize()
    assert d2.max().item() > 0
    assert_bit_equal(d.cpu().numpy(), d2.cpu().numpy(), "direct")
    assert_bit_equal(i.cpu().numpy(), i2.cpu().numpy(), "indirect")
    _assert_world(ctx, sd2.vertices, sd2.normals, "after eight poses")
