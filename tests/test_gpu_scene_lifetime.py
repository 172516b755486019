"""What lives and dies with an uploaded scene (rdh_scene_upload, rdh_scene_free, rdh_destroy).

One context gathers every kind of scene state the edit entries make — an object table, motion tracking, an LBVH tree with a light
rebuild, a refit (hence a refit plan), an emitter list grown beyond the upload's capacity, a tree header and a light sum still
pending — and is then given a new scene, freed or destroyed.  What follows must be what a fresh context gives: frames and the
bytes of rdh_debug_read_tree / rdh_debug_read_lights are compared bit for bit, always between two contexts that were given the same
calls, so the alias table's NaN payloads need no special case."""
import ctypes as C
import types

import numpy as np
import pytest

import light_deform
import material_edit
import pose_scene

pytestmark = pytest.mark.gpu

SIZES = ((37, 29), (64, 48))
DEPTH = 4


def _torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    """The scenes (never changed): the pose tests' file (643 triangles, 21 of them emissive), its first three objects without the
    lamp (222 triangles, no lights), and the file with two more objects, one of them a lamp (864 triangles, 221 emitters)."""
    from radish_pt_amd import hostlib, layouts as L, scenes

    d = str(tmp_path_factory.mktemp("scene_lifetime"))
    pose_scene.write_meshes(d)
    sd, _, _ = scenes.load_scene_file(pose_scene.write_scene(d, "scene.txt"))
    extra = pose_scene.object_block(6, "rev.obj", "lamp", (0.75, 1.0, -0.75), (0.0, 45.0, 20.0), (0.5, 0.5, 0.5)) + \
        pose_scene.object_block(7, "cone.obj", "green", (-0.5, 0.25, 1.0), (0.0, 0.0, 0.0), (1.0, 2.0, 1.0))
    big, _, _ = scenes.load_scene_file(pose_scene.write_scene(d, "big.txt", extra_objects=extra))
    n = int(sd.objects[2]["firstPrim"]) + int(sd.objects[2]["numPrims"])
    small = scenes.SceneData("small", sd.vertices[:3 * n], sd.normals[:3 * n], sd.texcoords[:3 * n], sd.material_ids[:n], sd.materials)
    assert (sd.num_prims, sd.num_lights) == (643, 21) and (small.num_prims, small.num_lights) == (222, 0)
    assert (big.num_prims, big.num_lights) == (864, 221) and len(big.objects) == 8
    mat = lambda t, red: int(np.flatnonzero((sd.materials["type"] == t) & np.isclose(sd.materials["baseColor"][:, 0], red))[0])
    cams = [hostlib.make_camera(w, h, eye=(0.2, 1.6, 5.0), rotation=(-92.0, -12.0, 0.0), fovy=20.0) for w, h in SIZES]  # the file's view
    return types.SimpleNamespace(sd=sd, small=small, big=big, cams=cams, red=mat(L.LAMBERTIAN, 0.63), steel=mat(L.METALLIC_WORKFLOW, 0.9))


@pytest.fixture
def make_ctx():
    """Contexts of a test's own, closed when it ends."""
    from radish_pt_amd import api

    made = []

    def make(sd=None):
        c = api.Context(0)
        made.append(c)
        if sd is not None:
            c.upload_scene(sd)
        return c

    yield make
    for c in made:
        c.close()


def _lit(sd, mat_id, colour):
    """(ids, materials) for Context.set_materials: material mat_id becomes a Light."""
    from radish_pt_amd import layouts as L

    mats = sd.materials[[mat_id]].copy()
    mats["type"] = L.LIGHT
    mats["baseColor"] = colour
    return np.array([mat_id], np.int32), mats


def _load(ctx, S):
    """Every kind of scene state on ctx; nothing waits at the end: the refit's tree header and the rebuild's light sum are pending."""
    sd = S.sd
    ctx.upload_scene(sd)
    ctx.set_objects(sd)
    ctx.track_motion(True)
    ctx.pose_objects(np.arange(6), trs=pose_scene.trs_array(pose_scene.POSED), tree="lbvh", rebuild_lights=True)
    ctx.pose_objects([0, 4], trs=pose_scene.trs_array([pose_scene.OBJECTS[0][2:5], pose_scene.OBJECTS[4][2:5]]), tree="refit")
    ctx.set_materials(*_lit(sd, S.red, (3.0, 2.5, 2.0)))  # 21 -> 221 emitters: beyond what the upload allocated
    # the lamp's triangles change their areas under the table and the tracked records (a refit from outside the object table), so
    # that the rebuild has new powers to sum; the tensor stays with the context: nothing has waited for the refit to read it
    ctx.moved = _torch().from_numpy(light_deform.deformed_vertices(sd, 0)).cuda()
    ctx.refit_geometry(ctx.moved)
    ctx.rebuild_lights()
    return ctx


def _snap(ctx, S):
    """Frames of two kernel families at both sizes (device tensors) and the bytes of both debug readers."""
    from radish_pt_amd import api

    torch = _torch()
    out = {}
    for (w, h), cam in zip(SIZES, S.cams):
        ctx.set_camera(cam)
        for name, flags in (("persistent", api.RDH_PT_PERSISTENT), ("wavefront", api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL)):
            img = torch.zeros(2, w * h, 3, device="cuda")
            ctx.path_trace(img[0], img[1], 0, 2, DEPTH, flags)
            out[f"{name} {w}x{h}"] = img
    ctx.synchronize()
    for which in (0, 1, 2):
        out[f"tree {which}"] = ctx.debug_read_tree(which).tobytes()
    for which in (0, 1, 2, 4):
        out[f"lights {which}"] = ctx.debug_read_lights(which).tobytes()
    return out


def _assert_same(a, b, what):
    torch = _torch()
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], bytes):
            assert a[k] == b[k], f"{what}: {k} differs"
        else:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: {k} differs"


def _lights_show(snap):
    return all(v.max().item() > 0 for k, v in snap.items() if not isinstance(v, bytes))


def _gbuffer(ctx, cam, w, h):
    from radish_pt_amd import api

    gb = api.GBuffer()
    gb.create(w, h)
    ctx.set_camera(cam)
    ctx.gbuffer_render(gb.c_struct(cam_fallback=cam), 0)
    ctx.synchronize()
    out = {"motion": gb.motion.clone(), "primId": gb.primId[gb.frameIdx].clone(), "depth": gb.depth[gb.frameIdx].clone()}
    gb.destroy()
    return out


def _raw_pose(ctx, ids):
    from radish_pt_amd import api

    ids = np.ascontiguousarray(ids, np.int32)
    xf = np.ascontiguousarray(pose_scene.xforms(pose_scene.POSED[:len(ids)]), np.float32)
    return api.lib().rdh_scene_pose_objects(ctx.h, C.c_void_p(ids.ctypes.data), C.c_void_p(xf.ctypes.data), len(ids), 0, 0, 0.0)


def _last_error(ctx):
    from radish_pt_amd import api

    return api.lib().rdh_last_error(ctx.h).decode()


def test_the_loaded_context_holds_what_it_claims(S, make_ctx):
    """The state the other cases start from: 221 emitters where the upload had 21, a refit plan (the tree's cost has moved since it
    was built), and frames of the edited scene."""
    ctx = _load(make_ctx(), S)
    hdr = ctx.debug_read_lights(1)
    assert tuple(hdr.view(np.int32)[2:]) == (221, 221)
    ids = ctx.debug_read_lights(4)
    assert len(ids) == 221 and len(np.unique(ids)) == 221
    now, at_build = ctx.tree_cost()
    assert now != at_build
    edited = material_edit.edited(S.sd, *_lit(S.sd, S.red, (3.0, 2.5, 2.0)))
    assert np.array_equal(ids, edited.light_prim_ids)
    assert _lights_show(_snap(ctx, S))


def test_reupload_of_a_smaller_scene_without_lights(S, make_ctx):
    torch = _torch()
    a, b = _load(make_ctx(), S), make_ctx(S.small)
    a.upload_scene(S.small)
    sa, sb = _snap(a, S), _snap(b, S)
    _assert_same(sa, sb, "small scene after the loaded one")
    assert sa["lights 0"] == b"" and len(sa["tree 0"]) == 6 * 2 * S.small.num_prims * 32
    # what must be gone: the object table, the refit plan, motion tracking
    assert _raw_pose(a, [0]) == -5  # RDH_ERR_STATE
    assert _last_error(a) == "rdh_scene_pose_objects: the scene has no object table (rdh_scene_set_objects)"
    now, at_build = a.tree_cost()
    assert now == at_build
    # Tracking: the loaded context's geometry moved after its last G-buffer render (it never rendered one), so had the upload kept
    # prevTris and the "moved since the render" flag, this render would take its motion vectors from the old scene's 643 records.
    # The check relies on that flag: records that survived with the flag cleared would not show here.
    (w, h), cam = SIZES[1], S.cams[1]
    ga, gb = _gbuffer(a, cam, w, h), _gbuffer(b, cam, w, h)
    assert (ga["primId"] >= 0).sum().item() > 200, "the G-buffer shows nothing"
    for k in ga:
        assert torch.equal(ga[k].view(torch.int32), gb[k].view(torch.int32)), f"G-buffer {k} differs"


def test_reupload_of_a_larger_scene_then_edits(S, make_ctx):
    big = S.big
    a, b = _load(make_ctx(), S), make_ctx(big)
    a.upload_scene(big)
    first = _snap(a, S)
    _assert_same(first, _snap(b, S), "large scene after the loaded one")
    assert _lights_show(first)
    rows = pose_scene.trs_array([pose_scene.POSED[1], ((0.5, 1.25, -0.5), (10.0, 30.0, 0.0), (0.75, 0.5, 0.5))])
    steps = (("set_objects", lambda c: c.set_objects(big)),
             ("pose with refit", lambda c: c.pose_objects([1, 6], trs=rows, tree="refit", rebuild_lights=True)),
             ("material edit", lambda c: c.set_materials(*_lit(big, S.steel, (9.0, 7.0, 5.0)))))  # 221 -> 242 emitters: grows again
    last = first
    for what, step in steps:
        step(a)
        step(b)
        sa = _snap(a, S)
        _assert_same(sa, _snap(b, S), what)
        if what != "set_objects":
            assert sa["lights 0"] != last["lights 0"] and sa["persistent 64x48"].ne(last["persistent 64x48"]).any().item(), f"{what} changed nothing"
        last = sa
    assert np.frombuffer(last["lights 1"], np.int32)[3] == 242


def test_free_then_upload(S, make_ctx):
    """The codes and texts are those the library had before the scene's state moved into one struct."""
    from radish_pt_amd import api

    torch = _torch()
    lib = api.lib()
    a = _load(make_ctx(), S)
    a.set_camera(S.cams[1])
    assert lib.rdh_scene_free(a.h) == 0
    img = torch.zeros(2, 64 * 48, 3, device="cuda")
    ids = np.zeros(1, np.int32)
    mats = S.sd.materials[:1].copy()
    refused = (
        (lambda: lib.rdh_path_trace(a.h, img[0].data_ptr(), img[1].data_ptr(), 0, 2, DEPTH, api.RDH_PT_PERSISTENT), -2,
         "no scene uploaded (rdh_scene_upload)"),
        (lambda: lib.rdh_scene_set_materials(a.h, ids.ctypes.data, mats.ctypes.data, 1, 0.0), -2, "rdh_scene_set_materials: no scene uploaded"),
        (lambda: lib.rdh_scene_rebuild_lights(a.h, 0.0), -1, "rdh_scene_rebuild_lights: no scene uploaded"),
        (lambda: lib.rdh_scene_refit_geometry(a.h, img.data_ptr(), None, None), -1, "rdh_scene_refit_geometry: no scene uploaded"),
        (lambda: lib.rdh_scene_track_motion(a.h, 1), -2, "rdh_scene_track_motion: no scene uploaded"),
        (lambda: lib.rdh_debug_read_lights(a.h, 1, None, 0), -2, "no scene uploaded"),
    )
    for call, code, text in refused:
        assert call() == code, text
        assert _last_error(a) == text
    a.upload_scene(S.sd)
    sa = _snap(a, S)
    _assert_same(sa, _snap(make_ctx(S.sd), S), "upload after rdh_scene_free")
    assert _lights_show(sa)


def test_close_of_a_loaded_context(S, make_ctx):
    """Twice in one process: destroy the loaded context, then a new context renders the reference frames.  Nothing more is claimed
    than that this ends without an error."""
    ref = _snap(make_ctx(S.sd), S)
    for k in range(2):
        _load(make_ctx(), S).close()
        _assert_same(_snap(make_ctx(S.sd), S), ref, f"a new context after close {k}")
