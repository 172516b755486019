"""The light sampler rebuilt on the device (kernels_lights.h: rdh_build_alias_table_device, rdh_scene_rebuild_lights).

The alias table must be the host's bit for bit, and a scene whose emissive triangles moved and whose lights were then rebuilt on
the device must render exactly like a fresh rdh_scene_upload of the moved scene, which the rest of the suite pins to the oracle."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import alias_model
import light_deform
import refit_model
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

W, H = 256, 192


def _torch():
    import torch

    return torch


@functools.lru_cache(maxsize=None)
def _teapots(grid):
    from radish_pt_amd import scenes

    return scenes.teapots(segments=24, bands=18, emissive_grid=grid)


@functools.lru_cache(maxsize=None)
def _deformed(grid, step):
    return light_deform.deformed_scene(_teapots(grid), step)


def _cuda(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. the alias table twin ----

def _device_table(ctx, values):
    table, total = ctx.build_alias_table_device(_cuda(values.astype(np.float32)))
    ctx.synchronize()
    return table.cpu().numpy().view(np.uint8).reshape(-1).view(alias_model.TABLE_DTYPE), total.cpu().numpy()


def _assert_same_table(ctx, values, what):
    from radish_pt_amd import hostlib

    ht, hs = hostlib.build_alias_table(values)
    dt, ds = _device_table(ctx, values)
    assert_bit_equal(ds, np.array([hs], np.float32), f"{what}: sum")
    assert np.array_equal(dt["failId"], ht["failId"]), f"{what}: failId differs at {np.flatnonzero(dt['failId'] != ht['failId'])[:5]}"
    assert_bit_equal(dt["prob"], ht["prob"], f"{what}: prob")


def test_alias_table_equals_host(gpu_ctx):
    sets = dict(alias_model.power_sets())
    for g in ((4, 8), (16, 32)):
        for step in (0, 1):
            sets[f"teapots {g} step {step}"] = light_deform.light_powers(_teapots(g), light_deform.deformed_vertices(_teapots(g), step))
    sets["100 000 exponential"] = np.random.default_rng(21).exponential(1.0, 100_000).astype(np.float32)
    for name, values in sets.items():
        _assert_same_table(gpu_ctx, values, name)


def test_alias_table_of_zeros(gpu_ctx):
    from radish_pt_amd import hostlib

    z = np.zeros(65, np.float32)
    ht, hs = hostlib.build_alias_table(z)
    dt, ds = _device_table(gpu_ctx, z)
    assert np.array_equal(dt["failId"], ht["failId"]) and np.array_equal(dt["failId"], np.arange(65))
    assert np.array_equal(np.isnan(dt["prob"]), np.isnan(ht["prob"])) and np.isnan(dt["prob"]).all()
    assert_bit_equal(ds, np.array([hs], np.float32), "sum of zeros")


# ---- 2. deformed lights render like a fresh upload ----

def _check_conditions(grid, step):
    """The deformation must exercise the sweep: entries above the mean, demotions, and a table unlike the undeformed scene's."""
    sd, moved = _teapots(grid), _deformed(grid, step)
    power = light_deform.light_powers(moved, moved.vertices)
    with np.errstate(all="ignore"):
        s = np.float32(0)
        for x in power:
            s = np.float32(s + x)
        val = power * np.float32(np.float32(len(power)) / s)
    above = val > np.float32(1)
    demoted = above & (moved.light_sampler["failId"] != np.arange(len(power)))
    assert above.sum() >= 8, f"{grid} step {step}: {above.sum()} entries above the mean"
    assert demoted.sum() >= 8, f"{grid} step {step}: {demoted.sum()} demotions"
    assert not np.array_equal(moved.light_sampler, sd.light_sampler)


def _frames(ctx, cam):
    """{name: (arrays, counters)} of the persistent, wavefront and RDH_PT_AUTO frames, the G-buffer and one ReSTIR frame."""
    from radish_pt_amd import api

    torch = _torch()
    out = {}
    for name, flags in (("persistent", api.RDH_PT_PERSISTENT),
                        ("wavefront", api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_WF_SUBFRAMES),
                        ("auto", api.RDH_PT_AUTO)):
        d = torch.zeros(W * H, 3, device="cuda")
        i = torch.zeros(W * H, 3, device="cuda")
        ctx.counters_reset()
        ctx.path_trace(d, i, 0, 3, 4, flags | api.RDH_PT_COUNT)
        out[name] = ([d.cpu().numpy(), i.cpu().numpy()], ctx.counters())
    gb = api.GBuffer()
    gb.create(W, H)
    dev = api.DevScene()
    dev.ctx = ctx
    ctx.counters_reset()
    gb.render(dev, cam)
    ctx.synchronize()
    out["gbuffer"] = ([gb.primId[0].cpu().numpy(), gb.depth[0].cpu().numpy(), gb.normal[0].cpu().numpy()], ctx.counters())
    img = torch.zeros(W * H, 3, device="cuda")
    ctx.restir_init()
    ctx.counters_reset()
    ctx.restir_direct(img, 0, 1, gb.c_struct(cam), 3)
    ctx.synchronize()
    out["restir"] = ([img.cpu().numpy()], ctx.counters())
    ctx.restir_free()
    gb.destroy()
    return out


def _move(ctx, mode, moved, lights):
    v = _cuda(moved.vertices)
    if mode == "refit":
        ctx.refit_geometry(v, None, lights)
    else:
        ctx.update_geometry(v, None, lights, mode)


def _pair(mode, grid, step, cam, rebuild=True):
    """Context A: the original scene, moved with lights = None, then rebuild_lights.  Context B: a fresh upload of the deformed
    scene ("sah": the update builds the host builder's tree), or the same move with the host-built light table."""
    from radish_pt_amd import api

    sd, moved = _teapots(grid), _deformed(grid, step)
    a, b = api.Context(0), api.Context(0)
    try:
        a.upload_scene(sd)
        a.set_camera(cam)
        _move(a, mode, moved, None)
        if rebuild:
            a.rebuild_lights()
        if mode == "sah":
            b.upload_scene(moved)
        else:
            b.upload_scene(sd)
            _move(b, mode, moved, (moved.light_sampler, moved.sum_light_power_inv))
        b.set_camera(cam)
    except Exception:
        a.close()
        b.close()
        raise
    return a, b


@pytest.mark.parametrize("mode", ["sah", "lbvh", "refit"])
@pytest.mark.parametrize("grid", [(4, 8), (16, 32)])
def test_deformed_lights_render_like_fresh_upload(grid, mode):
    from radish_pt_amd import scenes

    assert len(_teapots(grid).light_sampler) == {(4, 8): 66, (16, 32): 1026}[grid]
    for step in (0, 1):
        _check_conditions(grid, step)
    cam = scenes.teapots_camera(W, H)
    a, b = _pair(mode, grid, 0, cam)
    try:
        moved = _deformed(grid, 0)
        ta, tb = a.debug_read_lights(0), b.debug_read_lights(0)
        assert np.array_equal(tb, moved.light_sampler)
        assert np.array_equal(ta["failId"], tb["failId"]), f"failId differs at {np.flatnonzero(ta['failId'] != tb['failId'])[:5]}"
        assert_bit_equal(ta["prob"], tb["prob"], "alias table prob")
        ha, hb = a.debug_read_lights(1), b.debug_read_lights(1)
        assert np.array_equal(ha, hb), f"header {ha.view(np.float32)[:2]} {ha.view(np.int32)[2:]} vs {hb.view(np.float32)[:2]} {hb.view(np.int32)[2:]}"
        assert_bit_equal(ha.view(np.float32)[1:2], np.array([moved.sum_light_power_inv], np.float32), "sumLightPowerInv")
        assert np.array_equal(a.debug_read_lights(2), b.debug_read_lights(2)), "LightPre records differ"
        fa, fb = _frames(a, cam), _frames(b, cam)
        for name in fa:
            for k, (x, y) in enumerate(zip(fa[name][0], fb[name][0])):
                assert_bit_equal(x.view(np.float32), y.view(np.float32), f"{grid} {mode} {name} output {k}")
            assert fa[name][1] == fb[name][1], f"{grid} {mode} {name}: counters {fa[name][1]} vs {fb[name][1]}"
    finally:
        a.close()
        b.close()


# ---- 3. without the rebuild the table is stale, and the frame shows it ----

def test_stale_table_is_told_apart():
    from radish_pt_amd import api, scenes

    torch = _torch()
    cam = scenes.teapots_camera(W, H)
    a, b = _pair("sah", (4, 8), 0, cam, rebuild=False)
    try:
        assert not np.array_equal(a.debug_read_lights(0), b.debug_read_lights(0))
        frames = []
        for ctx in (a, b):
            d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
            ctx.path_trace(d, i, 0, 3, 4, api.RDH_PT_PERSISTENT)
            ctx.synchronize()
            frames.append(np.concatenate([d.cpu().numpy(), i.cpu().numpy()]))
        assert not np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32))
    finally:
        a.close()
        b.close()


# ---- 4. the environment map's entry ----

def test_environment_map_entry():
    from radish_pt_amd import api, scenes

    torch = _torch()
    sd = scenes.cornell_textured()
    assert len(sd.light_sampler) == 3 and sd.num_lights == 2 and sd.env_power > 0
    moved = light_deform.deformed_scene(sd, 0)
    assert_bit_equal(np.array([moved.env_power]), np.array([sd.env_power]), "env power")
    assert not np.array_equal(moved.light_sampler, sd.light_sampler)
    Wn, Hn, depth = 56, 40, 5
    n = Wn * Hn
    cam = scenes.cornell_camera(Wn, Hn)
    a, b = api.Context(0), api.Context(0)
    try:
        a.upload_scene(sd)
        a.set_camera(cam)
        a.update_geometry(_cuda(moved.vertices))
        a.rebuild_lights(sd.env_power)
        b.upload_scene(moved)
        b.set_camera(cam)
        ta, tb = a.debug_read_lights(0), b.debug_read_lights(0)
        assert np.array_equal(ta["failId"], tb["failId"])
        assert_bit_equal(ta["prob"], tb["prob"], "alias table prob")
        assert np.array_equal(a.debug_read_lights(1), b.debug_read_lights(1))
        assert np.array_equal(a.debug_read_lights(2), b.debug_read_lights(2))
        for name, flags in (("mega", 0), ("wavefront", api.RDH_PT_WAVEFRONT), ("sort", api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL),
                            ("persistent", api.RDH_PT_PERSISTENT)):
            got = []
            for ctx in (a, b):
                d, i = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda")
                ctx.counters_reset()
                for it in range(2):
                    ctx.path_trace(d, i, it, 60 + it, depth, flags | api.RDH_PT_COUNT)
                got.append((d.cpu().numpy(), i.cpu().numpy(), ctx.counters()))
            assert_bit_equal(got[0][0], got[1][0], f"{name} direct")
            assert_bit_equal(got[0][1], got[1][1], f"{name} indirect")
            assert got[0][2] == got[1][2], name
    finally:
        a.close()
        b.close()


# ---- 5. no synchronisation between refit, rebuild and frame; a host table enqueued after a rebuild wins ----

def _refit_target(sd, moved):
    """`moved` with sd's topology and the restatement's boxes (refit_model.py): what a refit of sd to moved's vertices uploads as."""
    t = copy.copy(moved)
    t.nodes = [n.copy() for n in sd.nodes]
    t.boxes = refit_model.refit_boxes(moved.vertices, sd.nodes)
    return t


def test_eight_rebuilds_without_synchronisation():
    from radish_pt_amd import api, scenes

    torch = _torch()
    grid = (4, 8)
    sd, cam = _teapots(grid), scenes.teapots_camera(W, H)
    steps = [_deformed(grid, s) for s in range(8)]
    a = api.Context(0)
    try:
        a.upload_scene(sd)
        a.set_camera(cam)
        got = []
        for m in steps:  # no host synchronisation between the refits, rebuilds and frames
            a.refit_geometry(_cuda(m.vertices))
            a.rebuild_lights()
            d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
            a.path_trace(d, i, 0, 2, 4, api.RDH_PT_PERSISTENT)
            got.append((m, d, i))
        # settle order: the rebuild is of step 7's lights; the refit enqueued right after it brings step 0's host-built table
        a.rebuild_lights()
        a.refit_geometry(_cuda(steps[0].vertices), None, (steps[0].light_sampler, steps[0].sum_light_power_inv))
        d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
        a.path_trace(d, i, 0, 2, 4, api.RDH_PT_PERSISTENT)
        got.append((steps[0], d, i))
        a.synchronize()
        assert np.array_equal(a.debug_read_lights(0), steps[0].light_sampler)
        assert_bit_equal(a.debug_read_lights(1).view(np.float32)[1:2], np.array([steps[0].sum_light_power_inv], np.float32), "inv")
        b = api.Context(0)
        try:
            b.set_camera(cam)
            for k, (m, d, i) in enumerate(got):
                b.upload_scene(_refit_target(sd, m))
                rd, ri = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
                b.path_trace(rd, ri, 0, 2, 4, api.RDH_PT_PERSISTENT)
                b.synchronize()
                assert_bit_equal(d.cpu().numpy(), rd.cpu().numpy(), f"frame {k} ({m.name}) direct")
                assert_bit_equal(i.cpu().numpy(), ri.cpu().numpy(), f"frame {k} ({m.name}) indirect")
        finally:
            b.close()
    finally:
        a.close()


# ---- 6. argument checks: RDH_ERR_ARGS, nothing enqueued, the scene stays as it was ----

def _persistent(ctx, n):
    from radish_pt_amd import api

    torch = _torch()
    d, i = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda")
    ctx.path_trace(d, i, 0, 0, 4, api.RDH_PT_PERSISTENT)
    ctx.synchronize()
    return np.concatenate([d.cpu().numpy(), i.cpu().numpy()])


def test_argument_checks_leave_scene_usable():
    from radish_pt_amd import api, scenes

    torch = _torch()
    Wn, Hn = 64, 48
    sd, cam = scenes.cornell_textured(), scenes.cornell_camera(Wn, Hn)
    ctx = api.Context(0)
    try:
        lib = api.lib()
        assert lib.rdh_scene_rebuild_lights(ctx.h, 0.0) == -1  # before any upload
        with pytest.raises(api.RadishError):
            ctx.rebuild_lights()
        ctx.upload_scene(sd)
        ctx.set_camera(cam)
        ref = _persistent(ctx, Wn * Hn)
        lights0 = [ctx.debug_read_lights(k).tobytes() for k in range(3)]
        for bad in (float("nan"), -1.0, float("inf")):
            assert lib.rdh_scene_rebuild_lights(ctx.h, bad) == -1, bad
        vals = torch.ones(8, device="cuda")
        table = torch.zeros(8, 2, dtype=torch.int32, device="cuda")
        total = torch.zeros(1, device="cuda")
        vp, tp, sp = (C.c_void_p(t.data_ptr()) for t in (vals, table, total))
        assert lib.rdh_build_alias_table_device(ctx.h, vp, -1, tp, sp) == -1
        assert lib.rdh_build_alias_table_device(ctx.h, None, 8, tp, sp) == -1
        assert lib.rdh_build_alias_table_device(ctx.h, vp, 8, None, sp) == -1
        assert lib.rdh_build_alias_table_device(ctx.h, vp, 8, tp, None) == -1
        assert lib.rdh_build_alias_table_device(ctx.h, None, 0, None, None) == 0
        assert lib.rdh_debug_read_lights(ctx.h, 3, None, 0) == -1
        assert_bit_equal(_persistent(ctx, Wn * Hn), ref, "frame after rejected calls")
        assert [ctx.debug_read_lights(k).tobytes() for k in range(3)] == lights0
    finally:
        ctx.close()


def test_scene_without_lights():
    from radish_pt_amd import api, layouts as L, scenes

    Wn, Hn = 64, 48
    sd = scenes.tiny()
    mats = sd.materials.copy()
    mats["type"][mats["type"] == L.LIGHT] = L.LAMBERTIAN
    dark = scenes.SceneData("dark", sd.vertices, sd.normals, sd.texcoords, sd.material_ids, mats)
    assert len(dark.light_sampler) == 0
    ctx = api.Context(0)
    try:
        ctx.upload_scene(dark)
        ctx.set_camera(scenes.cornell_camera(Wn, Hn))
        ref = _persistent(ctx, Wn * Hn)
        assert api.lib().rdh_scene_rebuild_lights(ctx.h, 0.0) == 0
        assert len(ctx.debug_read_lights(0)) == 0
        assert_bit_equal(_persistent(ctx, Wn * Hn), ref, "frame after a rebuild of no lights")
    finally:
        ctx.close()
