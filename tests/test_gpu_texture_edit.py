"""Textures and the environment map edited on the device (rdh_scene_set_texture, rdh_scene_env_power, kernels_textures.h; DESIGN
11h).

One equality carries everything: a scene whose textures were edited on the device is, bit for bit, the scene a fresh upload_scene
of the edited description gives (texture_edit.with_textures: the host's build_envmap_sampler / build_alias_table), which the rest
of the suite pins to the oracle.  Each case uses two contexts: A uploads a scene and edits it, B uploads the edited description.
The alias tables' NaN payloads are left aside as in test_gpu_light_rebuild.py; there is no tolerance anywhere."""
import ctypes as C
import tempfile

import numpy as np
import pytest

import light_deform
import material_edit
import pose_scene
import texture_edit
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

W, H, DEPTH = 52, 36, 4
ENV_CASES = [(size, edit) for size in texture_edit.SIZES for edit in texture_edit.EDITS]


def _torch():
    import torch

    return torch


def _cuda(a):
    return _torch().from_numpy(np.array(a, copy=True, order="C")).cuda()  # (a copy: the shared maps are read-only)


def _cam():
    from radish_pt_amd import scenes

    return scenes.cornell_camera(W, H)


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


# ---- what is compared ---------------------------------------------------------------------------------------------------------------
def _tables(ctx):
    """{name: array}: the three texture readers and the three light readers."""
    out = {f"textures {k}": ctx.debug_read_textures(k) for k in (0, 1, 2)}
    out.update({f"lights {k}": ctx.debug_read_lights(k) for k in (0, 1, 2)})
    return out


def _same_table(x, y):
    """Two alias tables, NaN payloads aside."""
    nan = np.isnan(x["prob"])
    return np.array_equal(x["failId"], y["failId"]) and np.array_equal(nan, np.isnan(y["prob"])) and \
        np.array_equal(x["prob"][~nan].view(np.uint32), y["prob"][~nan].view(np.uint32))


def _assert_same_tables(ta, tb, what):
    assert ta.keys() == tb.keys()
    for k in ta:
        if ta[k].dtype.names:  # an alias table
            assert _same_table(ta[k], tb[k]), f"{what}: {k} differs"
        elif k == "textures 0":
            assert_bit_equal(ta[k], tb[k], f"{what}: texData")
        else:
            assert ta[k].tobytes() == tb[k].tobytes(), f"{what}: {k}: {ta[k].view(np.float32)} {ta[k].view(np.int32)} vs " \
                                                       f"{tb[k].view(np.float32)} {tb[k].view(np.int32)}"


def _outputs(ctx, cam, w=W, h=H):
    """{name: arrays or counters}: four path-trace kernels' frames, path_trace_direct, every G-buffer plane, and one ReSTIR frame
    after restir_init, each with its work counters."""
    from radish_pt_amd import api

    torch = _torch()
    out = {}
    ctx.set_camera(cam)
    for name, flags in (("persistent", api.RDH_PT_PERSISTENT), ("wavefront", api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL),
                        ("mega", api.RDH_PT_MEGAKERNEL), ("auto", api.RDH_PT_AUTO)):
        d, i = torch.zeros(w * h, 3, device="cuda"), torch.zeros(w * h, 3, device="cuda")
        ctx.counters_reset()
        ctx.path_trace(d, i, 0, 3, DEPTH, flags | api.RDH_PT_COUNT)
        ctx.synchronize()
        out[name], out[name + " counters"] = np.concatenate([d.cpu().numpy(), i.cpu().numpy()]), ctx.counters()
    d = torch.zeros(w * h, 3, device="cuda")
    ctx.counters_reset()
    ctx.path_trace_direct(d, 0, 3, api.RDH_PT_COUNT)
    ctx.synchronize()
    out["direct only"], out["direct only counters"] = d.cpu().numpy(), ctx.counters()
    gb = api.GBuffer()
    gb.create(w, h)
    ctx.counters_reset()
    ctx.gbuffer_render(gb.c_struct(cam_fallback=cam), api.RDH_PT_COUNT)
    ctx.synchronize()
    k = gb.frameIdx
    for name, t in (("albedo", gb.albedo), ("normal", gb.normal[k]), ("depth", gb.depth[k]), ("primId", gb.primId[k]), ("motion", gb.motion)):
        out[name] = t.cpu().numpy().copy()
    out["gbuffer counters"] = ctx.counters()
    img = torch.zeros(w * h, 3, device="cuda")
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


_UPLOADED = {}


def _uploaded(size):
    """(outputs, tables) of texture_edit.scene(size) as uploaded, computed once per size."""
    from radish_pt_amd import api

    if size not in _UPLOADED:
        c = api.Context(0)
        try:
            c.upload_scene(texture_edit.scene(size))
            _UPLOADED[size] = (_outputs(c, _cam()), _tables(c))
        finally:
            c.close()
    return _UPLOADED[size]


def _edit_env(ctx, sd, size, content):
    ctx.set_texture(sd.env_map_tex_id, _cuda(texture_edit.env_map(size, content)))


# ---- 1. plain textures ------------------------------------------------------------------------------------------------------------
def test_plain_textures_equal_fresh_upload(make_ctx):
    sd, cam, edits = texture_edit.cornell(), _cam(), texture_edit.plain_edits()
    ed = texture_edit.with_textures(sd, edits)
    a = make_ctx(sd, cam)
    for tex_id, texels in edits.items():
        a.set_texture(tex_id, _cuda(texels))
    b = make_ctx(ed, cam)
    ta, tb = _tables(a), _tables(b)
    assert_bit_equal(ta["textures 0"], np.concatenate([t.reshape(-1) for t in ed.textures]), "texData against the description")
    _assert_same_tables(ta, tb, "plain textures")
    fa, fb = _outputs(a, cam), _outputs(b, cam)
    _assert_same_outputs(fa, fb, "plain textures")
    before, tables_before = _uploaded((64, 32))  # cornell_textured's own environment map
    assert _differs(fb, before), "the edit does not show"
    assert not np.array_equal(fb["albedo"].view(np.uint32), before["albedo"].view(np.uint32)), "the floor's base colour must change"
    for k in ("textures 1", "textures 2", "lights 0", "lights 1", "lights 2"):  # nothing but the texels changed
        assert ta[k].tobytes() == tables_before[k].tobytes(), f"{k} changed"


# ---- 2. the environment map ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,edit", ENV_CASES, ids=[f"{s[0]}x{s[1]}-{e}" for s, e in ENV_CASES])
def test_environment_edit_equals_fresh_upload(size, edit, make_ctx):
    sd, ed, cam = texture_edit.scene(size), texture_edit.scene(size, edit), _cam()
    a = make_ctx(sd, cam)
    _edit_env(a, sd, size, edit)
    b = make_ctx(ed, cam)
    what = f"{size[0]}x{size[1]} {edit}"
    ta, tb = _tables(a), _tables(b)
    _assert_same_tables(ta, tb, what)
    assert_bit_equal(np.array([a.env_power()]), np.array([ed.env_power]), f"{what}: env_power after the edit")
    assert_bit_equal(ta["textures 2"].view(np.float32)[:1], np.array([ed.env_power]), f"{what}: envPower of the header")
    assert tuple(ta["textures 2"].view(np.int32)[1:]) == (sd.env_map_tex_id, size[0] * size[1], len(sd.textures))
    assert _same_table(ta["textures 1"], ed.env_map_sampler) and _same_table(ta["lights 0"], ed.light_sampler), f"{what}: host tables"
    assert_bit_equal(ta["lights 1"].view(np.float32)[1:2], np.array([ed.sum_light_power_inv]), f"{what}: sumLightPowerInv")
    fa, fb = _outputs(a, cam), _outputs(b, cam)
    _assert_same_outputs(fa, fb, what)
    # Without the edit the scene differs, so the comparison above is not vacuous.  (The one-pixel map sees neither sun: there the
    # "edit" writes the texels it found.)
    if np.array_equal(texture_edit.env_map(size, edit), texture_edit.env_map(size, "sky")):
        assert size == (1, 1) and edit == "moved_sun"
        return
    before, tables_before = _uploaded(size)
    assert ta["textures 0"].tobytes() != tables_before["textures 0"].tobytes(), f"{what}: texData unchanged"
    if ed.env_power.tobytes() != sd.env_power.tobytes():
        # another power is another sumLightPowerInv: every light's selection probability, hence every lit pixel, changes.  (A map
        # whose power keeps its bits, the sun's far tail moving over one row of 64 pixels, changes texels in the last place only.)
        assert not _same_table(ta["lights 0"], tables_before["lights 0"]) or ta["lights 1"].tobytes() != tables_before["lights 1"].tobytes()
        assert ta["lights 2"].tobytes() != tables_before["lights 2"].tobytes(), f"{what}: LightPre unchanged"
        assert _differs(fb, before), f"{what}: the edit does not show"
    else:
        assert (size, edit) == ((64, 1), "moved_sun"), (size, edit)
        assert not _same_table(ta["textures 1"], tables_before["textures 1"]), f"{what}: envAlias unchanged"


# ---- 3. env_power() -----------------------------------------------------------------------------------------------------------------
def test_env_power_of_a_fresh_upload(make_ctx):
    """Computed on the device from the uploaded texels, on a scene no edit has touched; asking changes nothing."""
    ctx = make_ctx()
    for size in texture_edit.SIZES:
        for content in ("sky", "black") if size != (64, 32) else texture_edit.CONTENTS:
            sd = texture_edit.scene(size, content)
            ctx.upload_scene(sd)
            before = _tables(ctx) if size == (65, 3) else None  # (this reader's header asks for the power itself)
            assert_bit_equal(np.array([ctx.env_power()]), np.array([sd.env_power]), f"{size} {content}")
            assert_bit_equal(np.array([ctx.env_power()]), np.array([sd.env_power]), f"{size} {content}, asked again")
            if before is not None:
                _assert_same_tables(_tables(ctx), before, f"{size} {content}: after env_power")
                assert before["textures 1"].tobytes() == sd.env_map_sampler.tobytes()  # the upload's own bytes, NaN payloads included


def _edited_pair(make_ctx, size=(64, 32), edit="moved_sun"):
    sd, ed, cam = texture_edit.scene(size), texture_edit.scene(size, edit), _cam()
    a = make_ctx(sd, cam)
    _edit_env(a, sd, size, edit)
    return a, make_ctx(ed, cam), sd, ed, cam


def _assert_same_scene(a, b, cam, what):
    _assert_same_tables(_tables(a), _tables(b), what)
    assert a.debug_read_lights(4).tobytes() == b.debug_read_lights(4).tobytes()
    fa = _outputs(a, cam)
    _assert_same_outputs(fa, _outputs(b, cam), what)
    return fa


def test_env_power_feeds_set_materials(make_ctx):
    """The lamp x 4 after an environment edit: the edit's power, fetched from the device, is what the host computes for B."""
    a, b, sd, ed, cam = _edited_pair(make_ctx)
    ids, mats = material_edit.steps("cornell", "lamp_x4")[0]
    stale = float(sd.env_power)
    assert stale != float(ed.env_power)
    a.set_materials(ids, mats, a.env_power())
    b.set_materials(ids, mats, float(ed.env_power))
    fa = _assert_same_scene(a, b, cam, "edit + lamp x 4")
    c = make_ctx(ed, cam)
    c.set_materials(ids, mats, stale)  # what a caller who kept the uploaded scene's power would get
    assert _differs(fa, _outputs(c, cam)), "the stale power shows nothing"


def test_env_power_feeds_refit_and_rebuild(make_ctx):
    a, b, sd, ed, cam = _edited_pair(make_ctx, edit="one_pixel")
    moved = _cuda(light_deform.deformed_vertices(sd, 0))
    for ctx, power in ((a, a.env_power()), (b, float(ed.env_power))):
        ctx.refit_geometry(moved)
        ctx.rebuild_lights(power)
    _assert_same_scene(a, b, cam, "edit + refit + rebuild")
    ref = make_ctx(light_deform.deformed_scene(ed, 0), cam)  # the host's sampler of the deformed, edited scene
    assert _same_table(a.debug_read_lights(0), ref.debug_read_lights(0))
    assert a.debug_read_lights(1).tobytes() == ref.debug_read_lights(1).tobytes()


def test_env_power_feeds_pose_with_rebuild(make_ctx):
    """The pose tests' scene file with an environment map of 16x8 pixels."""
    from radish_pt_amd import hostlib, scenes

    size = (16, 8)
    with tempfile.TemporaryDirectory() as d:
        pose_scene.write_meshes(d)
        with open(f"{d}/sky.pfm", "wb") as f:
            f.write(b"PF\n%d %d\n-1.0\n" % size + texture_edit.env_map(size, "sky")[::-1].astype("<f4").tobytes())
        sd, _, _ = scenes.load_scene_file(pose_scene.write_scene(d, "scene.txt", extra_objects="EnvMap sky.pfm\n\n"))
    env = sd.env_map_tex_id
    assert env >= 0 and sd.textures[env].shape == (size[1], size[0], 3) and sd.env_power > 0
    ed = texture_edit.with_textures(sd, {env: texture_edit.env_map(size, "moved_sun")})
    assert ed.env_power.tobytes() != sd.env_power.tobytes()
    cam = hostlib.make_camera(W, H, eye=(0.2, 1.6, 5.0), rotation=(-92.0, -12.0, 0.0), fovy=20.0)  # the file's view
    a, b = make_ctx(sd, cam), make_ctx(ed, cam)
    a.set_objects(sd)
    b.set_objects(ed)
    a.set_texture(env, _cuda(texture_edit.env_map(size, "moved_sun")))
    for ctx, power in ((a, a.env_power()), (b, float(ed.env_power))):
        ctx.pose_objects(np.arange(6), trs=pose_scene.trs_array(pose_scene.POSED), tree="sah", rebuild_lights=True, env_power=power)
    _assert_same_scene(a, b, cam, "edit + pose")


# ---- 4. a sequence without host synchronisation -------------------------------------------------------------------------------------
def test_five_edits_and_frames_without_a_host_wait(make_ctx):
    """Five environment edits, a frame after each; nothing in the loop waits for the device beyond what a frame after a light
    rebuild always waits for (its sumLightPowerInv)."""
    from radish_pt_amd import api

    torch = _torch()
    size, cam = (64, 32), _cam()
    sd = texture_edit.scene(size)
    a = make_ctx(sd, cam)
    maps = [_cuda(texture_edit.env_map(size, c)) for c in ("moved_sun", "constant", "one_pixel", "black", "moved_sun")]
    frames = []
    for m in maps:
        a.set_texture(sd.env_map_tex_id, m)
        img = torch.zeros(2, W * H, 3, device="cuda")
        a.path_trace(img[0], img[1], 0, 2, DEPTH, api.RDH_PT_PERSISTENT)
        frames.append(img)
    a.synchronize()
    b = make_ctx(None, cam)
    for k, content in ((3, "black"), (4, "moved_sun")):
        b.upload_scene(texture_edit.scene(size, content))
        ref = torch.zeros(2, W * H, 3, device="cuda")
        b.path_trace(ref[0], ref[1], 0, 2, DEPTH, api.RDH_PT_PERSISTENT)
        b.synchronize()
        assert_bit_equal(frames[k].cpu().numpy(), ref.cpu().numpy(), f"frame after edit {k + 1} ({content})")
    assert not torch.equal(frames[3], frames[4])
    _assert_same_tables(_tables(a), _tables(b), "after five edits")


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_unchanged(make_ctx):
    from radish_pt_amd import api, scenes

    torch = _torch()
    lib = api.lib()
    size, cam = (64, 32), _cam()
    sd = texture_edit.scene(size)
    env = sd.env_map_tex_id
    texels = _cuda(texture_edit.env_map(size, "moved_sun"))
    small = _cuda(texture_edit.plain_edits()[2])
    ctx = make_ctx()
    power = C.c_float(-1.0)

    def raw(tex_id, t, w, h):
        return lib.rdh_scene_set_texture(ctx.h, tex_id, None if t is None else C.c_void_p(t.data_ptr()), w, h)

    assert raw(env, texels, 64, 32) == -2  # RDH_ERR_NO_SCENE
    assert lib.rdh_scene_env_power(ctx.h, C.byref(power)) == -2 and lib.rdh_debug_read_textures(ctx.h, 0, None, 0) == -2
    ctx.upload_scene(sd)
    ctx.set_camera(cam)

    def frame():
        img = torch.zeros(2, W * H, 3, device="cuda")
        ctx.path_trace(img[0], img[1], 0, 2, DEPTH, api.RDH_PT_PERSISTENT)
        ctx.synchronize()
        return img

    first = frame()
    assert first.max().item() > 0
    refused = (
        ("texId -1", lambda: raw(-1, texels, 64, 32)), ("texId numTextures", lambda: raw(len(sd.textures), texels, 64, 32)),
        ("wrong width", lambda: raw(env, texels, 63, 32)), ("wrong height", lambda: raw(env, texels, 64, 33)),
        ("width and height swapped", lambda: raw(env, texels, 32, 64)), ("null pointer", lambda: raw(env, None, 64, 32)),
        ("a plain texture's size for another", lambda: raw(0, small, 8, 8)), ("null pointer, plain texture", lambda: raw(2, None, 8, 8)),
        ("env_power into a null pointer", lambda: lib.rdh_scene_env_power(ctx.h, None)),
        ("reader 3", lambda: lib.rdh_debug_read_textures(ctx.h, 3, None, 0)),
    )
    for what, call in refused:
        assert call() == -1, what  # RDH_ERR_ARGS
        assert torch.equal(frame().view(torch.int32), first.view(torch.int32)), f"{what}: the frame changed"
    with pytest.raises(api.RadishError):
        ctx.set_texture(env, texels.reshape(-1))  # not [h, w, 3]
    with pytest.raises(api.RadishError):
        ctx.set_texture(env, texels.cpu())
    with pytest.raises(api.RadishError):
        ctx.set_texture(env, texels.double())
    before, tables_before = _uploaded(size)
    _assert_same_outputs(_outputs(ctx, cam), before, "after the refused calls")
    for k, t in _tables(ctx).items():
        assert t.tobytes() == tables_before[k].tobytes(), k
    no_env = make_ctx(scenes.cornell_textured(env=False), cam)  # a scene without an environment map
    assert lib.rdh_scene_env_power(no_env.h, C.byref(power)) == -5 and power.value == -1.0  # RDH_ERR_STATE
    with pytest.raises(api.RadishError):
        no_env.env_power()
    hdr = no_env.debug_read_textures(2)
    assert hdr.view(np.float32)[0] == 0.0 and tuple(hdr.view(np.int32)[1:]) == (-1, 0, 4) and len(no_env.debug_read_textures(1)) == 0
    no_env.set_texture(0, _cuda(texture_edit.plain_edits()[0]))  # plain textures of such a scene can still be edited
    assert no_env.debug_read_lights(0).tobytes() == make_ctx(scenes.cornell_textured(env=False)).debug_read_lights(0).tobytes()


# ---- 6. lifetime --------------------------------------------------------------------------------------------------------------------
def _snap(ctx, cam):
    """Frames of two kernel families (device tensors) and the bytes of the readers."""
    from radish_pt_amd import api

    torch = _torch()
    out = {}
    ctx.set_camera(cam)
    for name, flags in (("persistent", api.RDH_PT_PERSISTENT), ("wavefront", api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL)):
        img = torch.zeros(2, W * H, 3, device="cuda")
        ctx.path_trace(img[0], img[1], 0, 2, DEPTH, flags)
        out[name] = img
    ctx.synchronize()
    out.update(_tables(ctx))
    return out


def _assert_same_snap(a, b, what):
    torch = _torch()
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert _same_table(a[k], b[k]) if a[k].dtype.names else a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"
        else:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: {k} differs"


def test_scene_lifetime_after_an_environment_edit(make_ctx):
    """What an environment edit hangs on the scene (workspace, row factors, a pending light sum) goes with the scene: a smaller
    scene, a larger one that is edited in turn, rdh_scene_free and rdh_destroy behave as on a fresh context."""
    from radish_pt_amd import api

    cam = _cam()
    mid, small, large = (65, 3), (7, 5), (130, 67)
    a = make_ctx(texture_edit.scene(mid), cam)
    _edit_env(a, texture_edit.scene(mid), mid, "one_pixel")  # nothing waits: the light sum is pending when the next scene arrives
    a.upload_scene(texture_edit.scene(small))
    _assert_same_snap(_snap(a, cam), _snap(make_ctx(texture_edit.scene(small)), cam), "a smaller scene after the edited one")
    a.upload_scene(texture_edit.scene(large))
    _edit_env(a, texture_edit.scene(large), large, "moved_sun")  # rows 5 -> 67, pixels 35 -> 8 710: nothing of the old scene's fits
    sa = _snap(a, cam)
    _assert_same_snap(sa, _snap(make_ctx(texture_edit.scene(large, "moved_sun")), cam), "a larger scene, edited")
    assert_bit_equal(np.array([a.env_power()]), np.array([texture_edit.scene(large, "moved_sun").env_power]), "env_power")
    _edit_env(a, texture_edit.scene(large), large, "constant")
    assert api.lib().rdh_scene_free(a.h) == 0  # with the edit in flight
    assert api.lib().rdh_scene_set_texture(a.h, 0, C.c_void_p(_cuda(texture_edit.plain_edits()[0]).data_ptr()), 32, 32) == -2
    a.upload_scene(texture_edit.scene(mid))
    assert_bit_equal(np.array([a.env_power()]), np.array([texture_edit.scene(mid).env_power]), "env_power after free and upload")
    ref = _snap(make_ctx(texture_edit.scene(mid)), cam)
    _assert_same_snap(_snap(a, cam), ref, "upload after rdh_scene_free")
    for k in range(2):  # destroy with an edit in flight, then a new context
        c = make_ctx(texture_edit.scene(mid), cam)
        _edit_env(c, texture_edit.scene(mid), mid, "black")
        c.close()
        _assert_same_snap(_snap(make_ctx(texture_edit.scene(mid)), cam), ref, f"a new context after close {k}")
