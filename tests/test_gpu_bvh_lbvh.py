"""The LBVH builder on the device (kernels_lbvh.h; rdh_build_bvh_device_ex / rdh_scene_update_geometry_ex with RDH_BVH_LBVH).

The builder must give the numpy restatement's tree (lbvh_model.py) byte for byte.  Everything behind it is checked against a
second context that uploads the same vertices carrying that tree: the upload derives the threaded arrays, pairs and root box from
them, and the rest of the suite pins uploads to the oracle."""
import ctypes as C

import numpy as np
import pytest

import lbvh_model
import refit_model
from helpers import assert_bit_equal, oracle_path_trace_mt
from test_bvh_lbvh_cpu import CASES, case_vertices
from test_gpu_bvh_build import _frames, _moved
from test_gpu_bvh_refit import _assert_same_state, _cuda, _render, _scene, _tree_state, _with_vertices

pytestmark = pytest.mark.gpu


def _lbvh(ctx, m, builder="lbvh"):
    ctx.update_geometry(_cuda(m.vertices), _cuda(m.normals), (m.light_sampler, m.sum_light_power_inv), builder=builder)


def _refit(ctx, m):
    ctx.refit_geometry(_cuda(m.vertices), _cuda(m.normals), (m.light_sampler, m.sum_light_power_inv))


def _with_model_tree(m):
    """m carrying the restatement's LBVH tree of its own vertices."""
    m.boxes, m.nodes = lbvh_model.build(m.vertices)
    return m


# ---- 1. the builder equals the restatement ----

@pytest.mark.parametrize("name", CASES + ["config5"])
def test_build_equals_restatement(gpu_ctx, name):
    v = _scene("config5").vertices if name == "config5" else case_vertices(name)
    hb, hn = lbvh_model.build(v)
    boxes, nodes = gpu_ctx.build_bvh_device(_cuda(np.ascontiguousarray(v, np.float32).reshape(-1, 3)), builder="lbvh")
    gpu_ctx.synchronize()
    db, dn = boxes.cpu().numpy(), nodes.cpu().numpy()
    assert_bit_equal(db, hb, f"{name}: boxes")
    for k in range(6):
        ref = np.stack([hn[k]["primitiveId"], hn[k]["boundingBoxId"], hn[k]["nextNodeIfMiss"]], axis=1).astype(np.int32)
        assert np.array_equal(dn[k], ref), f"{name}: ordering {k} differs at {np.argwhere(dn[k] != ref)[:3].tolist()}"


# ---- 2. update_geometry(lbvh): the derived state equals an upload of the model tree ----

@pytest.mark.parametrize("case", ["cornell", "teapots", "cornell_moved", "teapots_moved"])
def test_update_equals_upload_of_model_tree(case):
    from radish_pt_amd import api

    sd = _scene(case.split("_")[0])
    m = _moved(sd, 1) if case.endswith("moved") else _with_vertices(sd, sd.vertices)
    a, b = api.Context(0), api.Context(0)
    try:
        a.upload_scene(sd)
        _lbvh(a, m)
        b.upload_scene(_with_model_tree(m))
        sa, sb = _tree_state(a), _tree_state(b)
        assert sa[2].view(np.int32)[1] == 1, "an LBVH tree always has pairs"
        _assert_same_state(sa, sb, case)
    finally:
        a.close()
        b.close()


# ---- 3. frames after an LBVH update ----

@pytest.mark.parametrize("scene", ["cornell", "teapots"])
def test_frames_after_lbvh_update_equal_upload(scene):
    from radish_pt_amd import api, scenes

    W, H = 512, 320
    sd = _scene(scene)
    cam = scenes.cornell_camera(W, H) if scene == "cornell" else scenes.teapots_camera(W, H)
    target = _with_model_tree(_moved(sd, 0))
    a, b = api.Context(0), api.Context(0)
    try:
        a.upload_scene(sd)
        a.set_camera(cam)
        _lbvh(a, target)
        b.upload_scene(target)
        b.set_camera(cam)
        fa, fb = _frames(a, cam, W, H), _frames(b, cam, W, H)
        for name in fa:
            for k, (x, y) in enumerate(zip(fa[name][0], fb[name][0])):
                assert_bit_equal(x.view(np.float32), y.view(np.float32), f"{scene} {name} output {k}")
            assert fa[name][1] == fb[name][1], f"{scene} {name}: counters {fa[name][1]} vs {fb[name][1]}"
        if scene == "cornell":
            d, i = fa["persistent"][0]
            ref_d = np.zeros((W * H, 3), np.float32)
            ref_i = np.zeros((W * H, 3), np.float32)
            idx, _ = oracle_path_trace_mt(target, cam, ref_d, ref_i, 0, 3, 4, stride=61)
            assert_bit_equal(d[idx], ref_d[idx], "LBVH frame vs oracle sample, direct")
            assert_bit_equal(i[idx], ref_i[idx], "LBVH frame vs oracle sample, indirect")
    finally:
        a.close()
        b.close()


# ---- 4. refit after an LBVH update ----

@pytest.mark.parametrize("scene", ["cornell", "teapots"])
def test_refit_after_lbvh_update(scene):
    from radish_pt_amd import api

    sd = _scene(scene)
    a, b = api.Context(0), api.Context(0)
    try:
        a.upload_scene(sd)
        _lbvh(a, sd)
        built = _tree_state(a)
        _refit(a, sd)
        _assert_same_state(_tree_state(a), built, f"{scene}: refit with unchanged vertices")
        lb = _with_model_tree(_with_vertices(sd, sd.vertices))
        moved = _moved(sd, 2)
        moved.nodes = [n.copy() for n in lb.nodes]
        moved.boxes = refit_model.refit_boxes(moved.vertices, lb.nodes)
        _refit(a, moved)
        b.upload_scene(moved)
        _assert_same_state(_tree_state(a), _tree_state(b), f"{scene}: refit of the LBVH tree to moved vertices")
    finally:
        a.close()
        b.close()


def test_tree_cost_after_lbvh_update():
    from radish_pt_amd import api

    sd = _scene("teapots")
    ctx = api.Context(0)
    try:
        ctx.upload_scene(sd)
        m = _moved(sd, 0)
        _lbvh(ctx, m)
        ref = refit_model.tree_cost(lbvh_model.build(m.vertices)[0])
        now, at_build = ctx.tree_cost()
        assert now == at_build
        assert abs(now - ref) <= 1e-12 * ref, (now, ref)
    finally:
        ctx.close()


# ---- 5. a sequence without host synchronisation ----

def test_sequence_without_synchronisation():
    from radish_pt_amd import api, scenes

    W, H = 256, 192
    sd, cam = _scene("cornell"), scenes.cornell_camera(W, H)
    m1, m2, m3, m4 = (_moved(sd, s) for s in range(4))
    a, ref = api.Context(0), api.Context(0)
    try:
        a.upload_scene(sd)
        a.set_camera(cam)
        # SAH update, LBVH update, refit, refit, LBVH update to new vertices, SAH update, LBVH update, render
        _lbvh(a, m1, builder="sah")
        _lbvh(a, m2)
        for mv in (m3, m1):
            _refit(a, mv)
        _lbvh(a, m4)
        _lbvh(a, m3, builder="sah")
        _lbvh(a, m2)
        got = _render(a, W, H)
        a.synchronize()
        target = _with_model_tree(m2)
        ref.upload_scene(target)
        ref.set_camera(cam)
        rd, ri = _render(ref, W, H)
        ref.synchronize()
        assert_bit_equal(got[0].cpu().numpy(), rd.cpu().numpy(), "sequence: direct")
        assert_bit_equal(got[1].cpu().numpy(), ri.cpu().numpy(), "sequence: indirect")
        _assert_same_state(_tree_state(a), _tree_state(ref), "sequence: tree")
    finally:
        a.close()
        ref.close()


# ---- 6. the _ex entries with RDH_BVH_SAH, and rejections ----

@pytest.mark.parametrize("scene", ["cornell", "teapots"])
def test_ex_with_sah_equals_update_geometry(scene):
    from radish_pt_amd import api

    sd = _scene(scene)
    m = _moved(sd, 1)
    a, b = api.Context(0), api.Context(0)
    try:
        a.upload_scene(sd)
        b.upload_scene(sd)
        a.update_geometry(_cuda(m.vertices), _cuda(m.normals), (m.light_sampler, m.sum_light_power_inv))
        vp, np_ = _cuda(m.vertices), _cuda(m.normals)
        table = np.ascontiguousarray(m.light_sampler)
        lu = api.LightUpdateC(table.ctypes.data, len(table), float(m.sum_light_power_inv))
        assert api.lib().rdh_scene_update_geometry_ex(b.h, C.c_void_p(vp.data_ptr()), C.c_void_p(np_.data_ptr()), C.byref(lu),
                                                      api.RDH_BVH_SAH) == 0
        _assert_same_state(_tree_state(a), _tree_state(b), f"{scene}: _ex with RDH_BVH_SAH")
    finally:
        a.close()
        b.close()


def test_rejections_leave_scene_usable():
    from radish_pt_amd import api, scenes

    W, H = 64, 48
    sd, cam = _scene("cornell"), scenes.cornell_camera(W, H)
    ctx = api.Context(0)
    try:
        lib = api.lib()
        v = _cuda(sd.vertices)
        ctx.upload_scene(sd)
        ctx.set_camera(cam)
        before = _render(ctx, W, H)
        ctx.synchronize()
        for bad in (2, -1, 7):
            assert lib.rdh_scene_update_geometry_ex(ctx.h, C.c_void_p(v.data_ptr()), None, None, bad) == -1
            assert "builder" in lib.rdh_last_error(ctx.h).decode()
        boxes = _cuda(np.zeros((2 * sd.num_prims - 1, 6), np.float32))
        nodes = _torch_nodes(sd.num_prims)
        ptrs = (C.c_void_p * 6)(*[nodes[k].data_ptr() for k in range(6)])
        assert lib.rdh_build_bvh_device_ex(ctx.h, C.c_void_p(v.data_ptr()), sd.num_prims, 5, C.c_void_p(boxes.data_ptr()), ptrs) == -1
        assert lib.rdh_build_bvh_device_ex(ctx.h, C.c_void_p(v.data_ptr()), 0, api.RDH_BVH_LBVH, C.c_void_p(boxes.data_ptr()), ptrs) == -1
        with pytest.raises(api.RadishError):
            ctx.update_geometry(v[:-3], builder="lbvh")
        with pytest.raises(api.RadishError):
            ctx.update_geometry(v, builder="ploc")
        with pytest.raises(api.RadishError):
            ctx.build_bvh_device(v, builder="median")
        after = _render(ctx, W, H)
        ctx.synchronize()
        assert_bit_equal(after[0].cpu().numpy(), before[0].cpu().numpy(), "direct after rejected calls")
        assert_bit_equal(after[1].cpu().numpy(), before[1].cpu().numpy(), "indirect after rejected calls")
    finally:
        ctx.close()


def _torch_nodes(n):
    import torch

    return torch.zeros(6, 2 * n - 1, 3, dtype=torch.int32, device="cuda")
