"""Materials and the light list edited on the device (rdh_scene_set_materials, rdh_build_light_list_device, kernels_materials.h;
DESIGN 11g).

One equality carries everything: a scene edited on the device is, bit for bit, the scene a fresh upload_scene of the edited
description gives (material_edit.edited: the host's build_light_list / build_alias_table), which the rest of the suite pins to the
oracle.  The alias table's NaN payloads are left aside as in test_gpu_light_rebuild.py; there is no tolerance anywhere."""
import ctypes as C
import tempfile

import numpy as np
import pytest

import light_deform
import material_edit
import pose_scene
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

W, H, DEPTH = 52, 36, 4


def _torch():
    import torch

    return torch


def _cuda(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _cam(scene):
    from radish_pt_amd import scenes

    return scenes.teapots_camera(W, H) if scene == "teapots" else scenes.cornell_camera(W, H)


def _env(sd):
    return float(sd.env_power)


@pytest.fixture
def make_ctx():
    """Contexts of a test's own, closed when it ends."""
    from radish_pt_amd import api

    made = []

    def make(sd=None, cam=None):
        c = api.Context(0)
        made.append(c)
        if sd is not None:
            c.upload_scene(sd)
        if cam is not None:
            c.set_camera(cam)
        return c

    yield make
    for c in made:
        c.close()


# ---- 1. the light list twin ----------------------------------------------------------------------------------------------------------
def _random_case(n, seed, num_mats=11, num_lights=3):
    from radish_pt_amd import layouts as L

    rng = np.random.default_rng(seed)
    mats = np.zeros(num_mats, L.MATERIAL_DTYPE)
    mats["type"] = rng.integers(0, 4, num_mats)
    mats["type"][rng.choice(num_mats, num_lights, replace=False)] = L.LIGHT
    mats["baseColor"] = rng.uniform(0.1, 9, (num_mats, 3))
    return rng.uniform(-1, 1, (3 * n, 3)).astype(np.float32), rng.integers(0, num_mats, n).astype(np.int32), mats


def _device_list(ctx, v, ids, mats):
    torch = _torch()
    mt = _cuda(np.frombuffer(mats.tobytes(), np.uint8).copy()) if len(mats) else torch.zeros(0, dtype=torch.uint8, device="cuda")
    prims, rad, power, count = ctx.build_light_list_device(_cuda(v.reshape(-1)), _cuda(ids), mt)
    ctx.synchronize()
    return prims.cpu().numpy(), rad.cpu().numpy(), power.cpu().numpy(), int(count.cpu().numpy()[0])


def _assert_same_list(ctx, v, ids, mats, what):
    from radish_pt_amd import hostlib

    hp, hr, hw = hostlib.build_light_list(v, ids, mats)
    dp, dr, dw, n = _device_list(ctx, v, ids, mats)
    assert n == len(hp), f"{what}: count {n} vs {len(hp)}"
    assert np.array_equal(dp[:n], hp), f"{what}: lightPrimIds differ at {np.flatnonzero(dp[:n] != hp)[:5]}"
    assert_bit_equal(dr[:n].reshape(-1), np.asarray(hr, np.float32).reshape(-1), f"{what}: lightUnitRadiance")
    assert_bit_equal(dw[:n], hw, f"{what}: lightPower")
    return n


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 5000])
def test_light_list_equals_host_at_the_boundaries(gpu_ctx, n):
    from radish_pt_amd import layouts as L

    v, ids, mats = _random_case(n, 100 + n)
    _assert_same_list(gpu_ctx, v, ids, mats, f"{n} random")
    every = mats.copy()
    every["type"] = L.LIGHT
    assert _assert_same_list(gpu_ctx, v, ids, every, f"{n} all emissive") == n
    none = mats.copy()
    none["type"][none["type"] == L.LIGHT] = L.LAMBERTIAN
    assert _assert_same_list(gpu_ctx, v, ids, none, f"{n} none emissive") == 0


def test_light_list_of_300_000_triangles(gpu_ctx):
    """1 172 block totals: more than one 256-entry tile of the scan."""
    v, ids, mats = _random_case(300_000, 7, num_mats=37, num_lights=9)
    n = _assert_same_list(gpu_ctx, v, ids, mats, "300 000 random")
    assert 40_000 < n < 120_000


def test_light_list_out_of_range_and_empty(gpu_ctx):
    torch = _torch()
    v, ids, mats = _random_case(700, 3)
    for bad, where in ((11, 0), (-1, 350), (1 << 20, 699)):
        broken = ids.copy()
        broken[where] = bad
        assert _device_list(gpu_ctx, v, broken, mats)[3] == -1, (bad, where)
    assert _device_list(gpu_ctx, v, ids, mats)[3] >= 0  # the error flag does not stick
    empty = gpu_ctx.build_light_list_device(torch.zeros(0, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
                                            _cuda(np.frombuffer(mats.tobytes(), np.uint8).copy()))
    gpu_ctx.synchronize()
    assert int(empty[3].cpu()[0]) == 0 and empty[0].numel() == 0


# ---- 2. scene edits ---------------------------------------------------------------------------------------------------------------
def _lights(ctx):
    return [ctx.debug_read_lights(k) for k in (0, 1, 2, 4)]


def _assert_same_lights(a, b, what):
    la, lb = _lights(a), _lights(b)
    assert np.array_equal(la[0]["failId"], lb[0]["failId"]), f"{what}: alias failId differs"
    assert_bit_equal(la[0]["prob"], lb[0]["prob"], f"{what}: alias prob")
    assert np.array_equal(la[1], lb[1]), f"{what}: header {la[1].view(np.float32)[:2]} {la[1].view(np.int32)[2:]} vs " \
                                         f"{lb[1].view(np.float32)[:2]} {lb[1].view(np.int32)[2:]}"
    assert np.array_equal(la[2], lb[2]), f"{what}: LightPre records differ"
    assert np.array_equal(la[3], lb[3]), f"{what}: lightPrimIds differ"


def _outputs(ctx, cam):
    """{name: arrays or counters}: four path-trace kernels' frames, path_trace_direct, every G-buffer plane, one ReSTIR frame."""
    from radish_pt_amd import api

    torch = _torch()
    out = {}
    ctx.set_camera(cam)
    for name, flags in (("persistent", api.RDH_PT_PERSISTENT), ("wavefront", api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL),
                        ("mega", api.RDH_PT_MEGAKERNEL), ("auto", api.RDH_PT_AUTO)):
        d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
        ctx.counters_reset()
        ctx.path_trace(d, i, 0, 3, DEPTH, flags | api.RDH_PT_COUNT)
        ctx.synchronize()
        out[name], out[name + " counters"] = np.concatenate([d.cpu().numpy(), i.cpu().numpy()]), ctx.counters()
    d = torch.zeros(W * H, 3, device="cuda")
    ctx.counters_reset()
    ctx.path_trace_direct(d, 0, 3, api.RDH_PT_COUNT)
    ctx.synchronize()
    out["direct only"], out["direct only counters"] = d.cpu().numpy(), ctx.counters()
    gb = api.GBuffer()
    gb.create(W, H)
    ctx.counters_reset()
    ctx.gbuffer_render(gb.c_struct(cam_fallback=cam), api.RDH_PT_COUNT)
    ctx.synchronize()
    k = gb.frameIdx
    for name, t in (("albedo", gb.albedo), ("normal", gb.normal[k]), ("depth", gb.depth[k]), ("primId", gb.primId[k]), ("motion", gb.motion)):
        out[name] = t.cpu().numpy().copy()
    out["gbuffer counters"] = ctx.counters()
    img = torch.zeros(W * H, 3, device="cuda")
    ctx.restir_init()
    ctx.counters_reset()
    ctx.restir_direct(img, 0, 1, gb.c_struct(cam), 3)
    ctx.synchronize()
    out["restir"], out["restir counters"] = img.cpu().numpy(), ctx.counters()
    ctx.restir_free()
    gb.destroy()
    return out


def _assert_same_outputs(a, b, what):
    assert a["persistent"].max() > 0, f"{what}: the frame shows nothing"
    for name in a:
        if isinstance(a[name], dict):
            assert a[name] == b[name], f"{what}: {name} {a[name]} vs {b[name]}"
        else:
            assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), f"{what}: {name} differs"


def _differs(a, b):
    return any(not isinstance(a[k], dict) and not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


@pytest.fixture(scope="module")
def uploaded():
    """The outputs of the two scenes as uploaded, computed once."""
    from radish_pt_amd import api

    out = {}
    for scene, make in material_edit.SCENES.items():
        c = api.Context(0)
        try:
            c.upload_scene(make())
            out[scene] = (_outputs(c, _cam(scene)), [x.copy() for x in _lights(c)])
        finally:
            c.close()
    return out


@pytest.mark.parametrize("edit", material_edit.EDITS)
@pytest.mark.parametrize("scene", list(material_edit.SCENES))
def test_edited_scene_equals_fresh_upload(scene, edit, make_ctx, uploaded):
    sd, ed, cam = material_edit.SCENES[scene](), material_edit.result(scene, edit), _cam(scene)
    a = make_ctx(sd, cam)
    for ids, mats in material_edit.steps(scene, edit):
        a.set_materials(ids, mats, _env(sd))
    b = make_ctx(ed, cam)
    what = f"{scene} {edit}"
    _assert_same_lights(a, b, what)
    hdr = a.debug_read_lights(1).view(np.int32)
    assert (hdr[2], hdr[3]) == (len(ed.light_sampler), ed.num_lights)
    assert np.array_equal(a.debug_read_lights(4), ed.light_prim_ids)
    fa, fb = _outputs(a, cam), _outputs(b, cam)
    _assert_same_outputs(fa, fb, what)
    before, lights_before = uploaded[scene]
    if edit == "back_on":  # the original upload again
        _assert_same_outputs(fa, before, what + " against the first upload")
        for k, (x, y) in enumerate(zip(_lights(a), lights_before)):
            if k == 0:
                assert np.array_equal(x["failId"], y["failId"])
                assert_bit_equal(x["prob"], y["prob"], "alias prob")
            else:
                assert np.array_equal(x, y), k
    else:  # without the edit the frames differ: the comparison above is not vacuous
        assert _differs(fb, before), f"{what}: the edit does not show"
        if edit in ("to_metal", "to_glass"):  # primClass changed: the material sort bins differently
            assert not np.array_equal(fb["wavefront"].view(np.uint32), before["wavefront"].view(np.uint32))
        if edit in ("half_off", "grow", "no_lights") and scene == "teapots":
            assert not np.array_equal(fb["primId"], before["primId"]), "emitters' primId must flip"
    if edit == "grow":
        assert ed.num_lights > sd.num_lights
    if edit == "no_lights":
        assert len(a.debug_read_lights(0)) == (1 if sd.env_map_tex_id >= 0 else 0)
        if sd.env_map_tex_id < 0:
            assert a.debug_read_lights(1).view(np.float32)[1] == 0.0


# ---- 3. interplay -----------------------------------------------------------------------------------------------------------------
def test_edit_then_refit_and_rebuild(make_ctx):
    """Emitters switched, then deformed vertices through refit_geometry(lights=None) + rebuild_lights: a fresh upload of the edited,
    deformed scene with the refit's boxes."""
    import copy

    import refit_model

    sd, ed, cam = material_edit.teapots(), material_edit.result("teapots", "half_off"), _cam("teapots")
    moved = light_deform.deformed_scene(ed, 0)
    target = copy.copy(moved)
    target.nodes = [n.copy() for n in sd.nodes]
    target.boxes = refit_model.refit_boxes(moved.vertices, sd.nodes)
    a = make_ctx(sd, cam)
    for ids, mats in material_edit.steps("teapots", "half_off"):
        a.set_materials(ids, mats)
    a.refit_geometry(_cuda(moved.vertices))
    a.rebuild_lights()
    b = make_ctx(target, cam)
    _assert_same_lights(a, b, "edit + refit + rebuild")
    _assert_same_outputs(_outputs(a, cam), _outputs(b, cam), "edit + refit + rebuild")


def test_edit_then_pose_with_rebuild(make_ctx):
    from radish_pt_amd import hostlib, layouts as L, scenes

    with tempfile.TemporaryDirectory() as d:
        pose_scene.write_meshes(d)
        sd, _, _ = scenes.load_scene_file(pose_scene.write_scene(d, "scene.txt"))
        sd2, _, _ = scenes.load_scene_file(pose_scene.write_scene(d, "posed.txt", pose_scene.POSED))
    lamp = int(material_edit.light_ids(sd)[0])
    steel = int(np.flatnonzero(sd.materials["type"] == L.METALLIC_WORKFLOW)[0])
    ids = np.array([lamp, steel], np.int32)
    mats = sd.materials[ids].copy()
    mats["type"] = [L.LAMBERTIAN, L.LIGHT]  # the lamp goes out, the other cone lights up
    mats["baseColor"][1] = (9.0, 7.0, 5.0)
    a = make_ctx(sd, None)
    a.set_objects(sd)
    a.set_materials(ids, mats)
    a.pose_objects(np.arange(6), trs=pose_scene.trs_array(pose_scene.POSED), tree="sah", rebuild_lights=True)
    b = make_ctx(material_edit.edited(sd2, ids, mats), None)
    cam_small = hostlib.make_camera(W, H, eye=(0.2, 1.6, 5.0), rotation=(-92.0, -12.0, 0.0), fovy=20.0)  # the file's view
    _assert_same_lights(a, b, "edit + pose")
    _assert_same_outputs(_outputs(a, cam_small), _outputs(b, cam_small), "edit + pose")


def test_edit_with_motion_tracking_keeps_the_motion_plane(make_ctx):
    from radish_pt_amd import api

    sd, ed, cam = material_edit.teapots(), material_edit.result("teapots", "half_off"), _cam("teapots")
    a, b = make_ctx(sd, cam), make_ctx(ed, cam)
    a.track_motion(True)
    planes = []
    for ctx in (a, b):
        gb = api.GBuffer()
        gb.create(W, H)
        ctx.gbuffer_render(gb.c_struct(cam_fallback=cam), 0)
        ctx.synchronize()
        gb.update(cam)
        if ctx is a:
            for ids, mats in material_edit.steps("teapots", "half_off"):
                a.set_materials(ids, mats)
        ctx.gbuffer_render(gb.c_struct(cam_fallback=cam), 0)
        ctx.synchronize()
        k = gb.frameIdx
        planes.append({"motion": gb.motion.cpu().numpy().copy(), "primId": gb.primId[k].cpu().numpy().copy()})
        gb.destroy()
    assert np.array_equal(planes[0]["motion"], planes[1]["motion"])
    assert np.array_equal(planes[0]["primId"], planes[1]["primId"])
    assert (planes[0]["motion"] >= 0).sum() > 200


def test_five_edits_and_frames_without_a_host_wait(make_ctx):
    from radish_pt_amd import api

    torch = _torch()
    sd, cam = material_edit.teapots(), _cam("teapots")
    a = make_ctx(sd, cam)
    got, state = [], sd
    for edit in ("half_off", "grow", "recolour", "no_lights", "lamp_x4"):  # no host synchronisation in this loop (a list that
        for ids, mats in material_edit.steps("teapots", edit)[-1:]:         # outgrows its arrays reallocates, which waits)
            a.set_materials(ids, mats)
            state = material_edit.edited(state, ids, mats)
        d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
        a.path_trace(d, i, 0, 2, DEPTH, api.RDH_PT_PERSISTENT)
        got.append((edit, state, d, i))
    a.synchronize()
    b = make_ctx(None, cam)
    for edit, state, d, i in got:
        b.upload_scene(state)
        rd, ri = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
        b.path_trace(rd, ri, 0, 2, DEPTH, api.RDH_PT_PERSISTENT)
        b.synchronize()
        assert_bit_equal(d.cpu().numpy(), rd.cpu().numpy(), f"after {edit}: direct")
        assert_bit_equal(i.cpu().numpy(), ri.cpu().numpy(), f"after {edit}: indirect")
    _assert_same_lights(a, b, "after five edits")


def test_host_light_update_takes_the_new_length(make_ctx):
    from radish_pt_amd import api

    sd, ed, cam = material_edit.teapots(), material_edit.result("teapots", "half_off"), _cam("teapots")
    a = make_ctx(sd, cam)
    for ids, mats in material_edit.steps("teapots", "half_off"):
        a.set_materials(ids, mats)
    v = _cuda(sd.vertices)
    with pytest.raises(api.RadishError):
        a.refit_geometry(v, None, (sd.light_sampler, sd.sum_light_power_inv))  # the uploaded length: refused
    a.refit_geometry(v, None, (ed.light_sampler, ed.sum_light_power_inv))
    b = make_ctx(ed, cam)
    assert np.array_equal(a.debug_read_lights(0), ed.light_sampler)
    _assert_same_lights(a, b, "host table of the new length")


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_unchanged(make_ctx, uploaded):
    from radish_pt_amd import api, layouts as L

    lib = api.lib()
    sd, cam = material_edit.cornell(), _cam("cornell")
    ctx = make_ctx()
    one = sd.materials[:2].copy()
    ids = np.array([0, 1], np.int32)

    def raw(ids, mats, count, env=float(sd.env_power)):
        ip = None if ids is None else C.c_void_p(ids.ctypes.data)
        mp = None if mats is None else C.c_void_p(mats.ctypes.data)
        return lib.rdh_scene_set_materials(ctx.h, ip, mp, count, env)

    assert raw(ids, one, 2) == -2  # RDH_ERR_NO_SCENE
    ctx.upload_scene(sd)
    ctx.set_camera(cam)
    for bad in ([0, 8], [-1, 1], [3, 3]):  # out of range, listed twice
        assert raw(np.array(bad, np.int32), one, 2) == -1, bad
    assert raw(None, one, 2) == -1 and raw(ids, None, 2) == -1 and raw(ids, one, -1) == -1
    for field, k, bad in (("baseColorMapId", 0, 5), ("baseColorMapId", 0, -3), ("normalMapId", 1, -2), ("roughnessMapId", 1, 5)):
        m = one.copy()
        m[field][k] = bad
        assert raw(ids, m, 2) == -1, (field, bad)
    for bad in (float("nan"), -1.0, float("inf")):
        assert raw(ids, one, 2, bad) == -1, bad
    assert raw(None, None, 0) == 0  # count == 0
    with pytest.raises(api.RadishError):
        ctx.set_materials([0], one)  # one id, two materials
    with pytest.raises(api.RadishError):
        ctx.set_materials([0], np.zeros(1, np.float32))
    assert lib.rdh_debug_read_lights(ctx.h, 3, None, 0) == -1 and lib.rdh_debug_read_lights(ctx.h, 5, None, 0) == -1
    before, lights_before = uploaded["cornell"]
    _assert_same_outputs(_outputs(ctx, cam), before, "after the refused calls")
    for x, y in zip(_lights(ctx), lights_before):
        assert x.tobytes() == y.tobytes()
    assert L.MATERIAL_DTYPE.itemsize == 44
