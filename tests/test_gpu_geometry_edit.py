"""The uploaded scene's triangle set replaced on the device (rdh_scene_set_geometry, kernels_geometry.h).

One equality carries everything: after set_geometry with the SAH builder the context holds, bit for bit, what a second context
holds after upload_scene of the edited SceneData (geometry_edit.result: the host's build_bvh / build_light_list /
build_alias_table); with the LBVH builder, what that upload followed by update_geometry(..., builder="lbvh") holds.  The alias
table's NaN payloads are left aside as in test_gpu_light_rebuild.py; there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import geometry_edit
import material_edit
from helpers import assert_bit_equal, random_rays

pytestmark = pytest.mark.gpu

W, H, DEPTH = 52, 36, 4
BUILDERS = ("sah", "lbvh")


def _torch():
    import torch

    return torch


def _cuda(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _cam(scene):
    from radish_pt_amd import scenes

    return scenes.teapots_camera(W, H) if scene == "teapots" else scenes.cornell_camera(W, H)


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


def _set(ctx, sd, builder="sah"):
    """The triangle set of sd, from device tensors."""
    v, n, t, m = (_cuda(a) for a in geometry_edit.arrays(sd))
    ctx.set_geometry(v, n, t, m, builder=builder, env_power=float(sd.env_power))


def _fresh(make_ctx, sd, builder, cam=None):
    """The yardstick: a second context that received upload_scene of sd (and, for LBVH, the update that builds that tree)."""
    b = make_ctx(sd, cam)
    if builder == "lbvh":
        b.update_geometry(_cuda(sd.vertices.reshape(-1)), builder="lbvh")
    return b


# ---- every debug read ---------------------------------------------------------------------------------------------------------------
def _state(ctx):
    s = {f"geometry {k}": ctx.debug_read_geometry(k) for k in range(4)}
    s.update({f"tree {k}": ctx.debug_read_tree(k) for k in range(3)})
    s.update({f"lights {k}": ctx.debug_read_lights(k) for k in (0, 1, 2, 4)})
    return s


def _assert_same_state(sa, sb, what):
    assert sa.keys() == sb.keys()
    for name in sa:
        x, y = sa[name], sb[name]
        assert x.shape == y.shape, f"{what}: {name} has {x.shape} vs {y.shape}"
        if name == "lights 0":  # the alias table: NaN where the other has NaN, every other float bit for bit
            assert np.array_equal(x["failId"], y["failId"]), f"{what}: alias failId differs"
            nan = np.isnan(x["prob"])
            assert np.array_equal(nan, np.isnan(y["prob"])), f"{what}: alias NaN entries differ"
            assert_bit_equal(x["prob"][~nan], y["prob"][~nan], f"{what}: alias prob")
        else:
            assert np.array_equal(x, y), f"{what}: {name} differs (first at byte/entry {np.flatnonzero(x != y)[:4]})"


def _assert_matches_description(state, sd, what):
    """What the description itself says, without a second context."""
    n = sd.num_prims
    tri = state["geometry 0"].view(np.float32).reshape(n, 12)
    assert_bit_equal(tri[:, :9], sd.vertices.reshape(n, 9), f"{what}: TriRec vertices")
    assert np.array_equal(tri[:, 9].view(np.int32), sd.material_ids), f"{what}: TriRec material ids"
    attr = state["geometry 1"].view(np.float32).reshape(n, 16)
    assert_bit_equal(attr[:, :9], sd.normals.reshape(n, 9), f"{what}: AttrRec normals")
    assert_bit_equal(attr[:, 9:15], sd.texcoords.reshape(n, 6), f"{what}: AttrRec texcoords")
    assert np.array_equal(state["geometry 3"], np.bincount(sd.material_ids, minlength=len(sd.materials))), f"{what}: counts"
    hdr = state["lights 1"].view(np.int32)
    assert (hdr[2], hdr[3]) == (len(sd.light_sampler), sd.num_lights), f"{what}: light header {hdr[2:]}"
    assert np.array_equal(state["lights 4"], sd.light_prim_ids), f"{what}: lightPrimIds"
    assert len(state["tree 0"]) == 32 * 6 * (2 * n - 1 + 1), f"{what}: node arrays' size"


# ---- 1. boundaries ------------------------------------------------------------------------------------------------------------------
def _soup(n, seed, kind="random"):
    """_random_case's recipe (test_gpu_material_edit.py): a random soup with 11 materials, three of them lights; `kind` picks the
    ids: random, every triangle emissive, none emissive."""
    from radish_pt_amd import layouts as L, scenes

    rng = np.random.default_rng(seed)
    mats = np.zeros(11, L.MATERIAL_DTYPE)
    mats["type"] = rng.integers(0, 4, 11)
    mats["type"][rng.choice(11, 3, replace=False)] = L.LIGHT
    mats["baseColor"] = rng.uniform(0.1, 9, (11, 3))
    for field in ("baseColorMapId", "normalMapId", "metallicMapId", "roughnessMapId"):
        mats[field] = -1  # no textures
    rng = np.random.default_rng(seed * 7919 + n)  # the materials depend on the seed alone, the triangles on n too
    lit = np.flatnonzero(mats["type"] == L.LIGHT)
    pool = {"random": np.arange(11), "all": lit, "none": np.setdiff1d(np.arange(11), lit)}[kind]
    v = rng.uniform(-1, 1, (3 * n, 3)).astype(np.float32)
    nr = rng.normal(size=(3 * n, 3)).astype(np.float32)
    uv = rng.uniform(0, 1, (3 * n, 2)).astype(np.float32)
    return scenes.SceneData(f"soup{n}{kind}", v, nr, uv, rng.choice(pool, n).astype(np.int32), mats)


@pytest.fixture(scope="module")
def fixed_rays():
    return _cuda(random_rays(4096, 11, lo=(-1.5, -1.5, -1.5), hi=(1.5, 1.5, 1.5)))


def _hits(ctx, rays):
    torch = _torch()
    hits = torch.full((rays.shape[0], 4), 0x7fffffff, dtype=torch.int32, device="cuda")
    ctx.trace_closest(rays, hits)
    ctx.synchronize()
    return hits.cpu().numpy()


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 5000])
def test_any_count_equals_fresh_upload(n, builder, make_ctx, fixed_rays):
    a = make_ctx(_soup(700, 5))  # 700 triangles uploaded: 5 000 grows every array, the other counts shrink
    for kind in ("random", "all", "none"):
        sd = _soup(n, 5, kind)
        assert sd.num_lights == {"random": sd.num_lights, "all": n, "none": 0}[kind]
        _set(a, sd, builder)
        b = _fresh(make_ctx, sd, builder)
        what = f"{n} {kind} {builder}"
        sa = _state(a)
        _assert_same_state(sa, _state(b), what)
        _assert_matches_description(sa, sd, what)
        assert np.array_equal(_hits(a, fixed_rays), _hits(b, fixed_rays)), f"{what}: trace_closest differs"
        b.close()


def test_more_materials_than_the_check_keeps_in_lds(make_ctx, fixed_rays):
    """1 100 materials: k_geom_check counts with global atomics instead of its 1 024 LDS bins."""
    from radish_pt_amd import layouts as L, scenes

    rng = np.random.default_rng(77)
    mats = np.zeros(1100, L.MATERIAL_DTYPE)
    mats["type"] = rng.integers(0, 5, 1100)
    mats["baseColor"] = rng.uniform(0.1, 9, (1100, 3))
    for field in ("baseColorMapId", "normalMapId", "metallicMapId", "roughnessMapId"):
        mats[field] = -1

    def soup(n):
        return scenes.SceneData(f"many{n}", rng.uniform(-1, 1, (3 * n, 3)), rng.normal(size=(3 * n, 3)), rng.uniform(0, 1, (3 * n, 2)),
                                rng.integers(0, 1100, n), mats)

    a, sd = make_ctx(soup(300)), soup(3000)
    for builder in BUILDERS:
        _set(a, sd, builder)
        b = _fresh(make_ctx, sd, builder)
        sa = _state(a)
        _assert_same_state(sa, _state(b), f"1 100 materials {builder}")
        _assert_matches_description(sa, sd, f"1 100 materials {builder}")
        assert np.array_equal(_hits(a, fixed_rays), _hits(b, fixed_rays))
    broken = _cuda(sd.material_ids.copy())
    broken[2999] = 1100
    v, n, t, _ = (_cuda(x) for x in geometry_edit.arrays(sd))
    from radish_pt_amd import api
    with pytest.raises(api.RadishError, match="material id"):
        a.set_geometry(v, n, t, broken)


# ---- 2. scene edits -------------------------------------------------------------------------------------------------------------------
def _outputs(ctx, cam):
    """{name: arrays or counters}: the persistent, sorted wavefront, megakernel and RDH_PT_AUTO frames, path_trace_direct, every
    G-buffer plane, one ReSTIR frame after restir_init, and all work counters."""
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
    for name in a:
        if isinstance(a[name], dict):
            assert a[name] == b[name], f"{what}: {name} {a[name]} vs {b[name]}"
        else:
            assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), f"{what}: {name} differs"


def _differs(a, b):
    return any(not isinstance(a[k], dict) and not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


@pytest.fixture(scope="module")
def uploaded():
    """The outputs and debug reads of the two scenes as uploaded, computed once."""
    from radish_pt_amd import api

    out = {}
    for scene, make in geometry_edit.SCENES.items():
        c = api.Context(0)
        try:
            c.upload_scene(make())
            out[scene] = (_outputs(c, _cam(scene)), _state(c))
        finally:
            c.close()
    return out


@pytest.fixture(scope="module")
def chains():
    """One context per (scene, builder) that receives the edits in geometry_edit.EDITS' order.  A test asks for the state after edit
    k: the edits up to k that the context has not seen are applied in order (a context that is already past k starts again from
    the upload), so every test stands on its own and the whole module walks each chain once."""
    from radish_pt_amd import api

    held = {}

    def after(scene, builder, k):
        ctx, done = held.get((scene, builder), (None, -1))
        if ctx is None or done > k:
            if ctx is not None:
                ctx.close()
            ctx, done = api.Context(0), -1
            ctx.upload_scene(geometry_edit.SCENES[scene]())
        for j in range(done + 1, k + 1):
            _set(ctx, geometry_edit.result(scene, geometry_edit.EDITS[j]), builder)
        held[(scene, builder)] = (ctx, k)
        return ctx

    yield after
    for ctx, _ in held.values():
        ctx.close()


@pytest.mark.parametrize("edit", geometry_edit.EDITS)
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("scene", list(geometry_edit.SCENES))
def test_edited_scene_equals_fresh_upload(scene, builder, edit, chains, make_ctx, uploaded):
    sd, ed, cam = geometry_edit.SCENES[scene](), geometry_edit.result(scene, edit), _cam(scene)
    a = chains(scene, builder, geometry_edit.EDITS.index(edit))
    b = _fresh(make_ctx, ed, builder, cam)
    what = f"{scene} {builder} {edit}"
    sa = _state(a)
    _assert_same_state(sa, _state(b), what)
    _assert_matches_description(sa, ed, what)
    fa, fb = _outputs(a, cam), _outputs(b, cam)
    _assert_same_outputs(fa, fb, what)
    before, state_before = uploaded[scene]
    if edit == "back":
        if builder == "sah":  # the first upload again
            _assert_same_outputs(fa, before, what + " against the first upload")
            _assert_same_state(sa, state_before, what + " against the first upload")
    else:  # without the edit the frames differ: the comparison above is not vacuous
        assert _differs(fb, before), f"{what}: the edit does not show"
    if ed.num_lights > 0:
        assert fa["persistent"].max() > 0, f"{what}: the frame shows nothing"
    if edit == "one_dark":
        hdr = sa["lights 1"]
        assert hdr.view(np.int32)[2] == (1 if sd.env_map_tex_id >= 0 else 0)
        if sd.env_map_tex_id < 0:
            assert hdr.view(np.float32)[1] == 0.0


# ---- 3. what follows an edit ----------------------------------------------------------------------------------------------------------
def _deformed(sd, amplitude=0.02):
    v = sd.vertices.astype(np.float64)
    v = v + amplitude * np.sin(3.0 * v[:, [1, 2, 0]] + 0.5)
    return v.astype(np.float32).reshape(-1)


def _frame(ctx, cam=None):
    from radish_pt_amd import api

    torch = _torch()
    if cam is not None:
        ctx.set_camera(cam)
    d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
    ctx.path_trace(d, i, 0, 2, DEPTH, api.RDH_PT_PERSISTENT)
    ctx.synchronize()
    return np.concatenate([d.cpu().numpy(), i.cpu().numpy()])


def _pair(make_ctx, edit, builder="sah"):
    """(a, b, ed, cam): teapots with `edit` applied on the device, and the fresh upload of it."""
    sd, ed, cam = geometry_edit.SCENES["teapots"](), geometry_edit.result("teapots", edit), _cam("teapots")
    a = make_ctx(sd, cam)
    _set(a, ed, builder)
    return a, _fresh(make_ctx, ed, builder, cam), ed, cam


@pytest.mark.parametrize("edit", ["remove", "add"])
def test_refit_after_an_edit_derives_its_plan_at_the_new_count(edit, make_ctx):
    a, b, ed, cam = _pair(make_ctx, edit)
    v = _cuda(_deformed(ed))
    for ctx in (a, b):
        ctx.refit_geometry(v)
        ctx.rebuild_lights()
    _assert_same_state(_state(a), _state(b), f"{edit} + refit")
    assert np.array_equal(_frame(a).view(np.uint32), _frame(b).view(np.uint32))
    assert a.tree_cost() == b.tree_cost()


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("edit", ["remove", "add"])
def test_update_after_an_edit_runs_at_the_new_count(edit, builder, make_ctx):
    a, b, ed, cam = _pair(make_ctx, edit, builder)
    v = _cuda(_deformed(ed))
    for ctx in (a, b):
        ctx.update_geometry(v, builder=builder)
        ctx.rebuild_lights()
    _assert_same_state(_state(a), _state(b), f"{edit} + update {builder}")
    assert np.array_equal(_frame(a).view(np.uint32), _frame(b).view(np.uint32))


def test_shrink_update_and_grow_within_the_capacity(make_ctx):
    """A scene uploaded without pairs would get them from the first update at the count of then; here the count goes down, an update
    runs, and the count comes back up within the uploaded capacity: pairs, node arrays and motion buffer must still fit."""
    sd, cam = geometry_edit.SCENES["teapots"](), _cam("teapots")
    small = geometry_edit.result("teapots", "remove")
    a = make_ctx(sd, cam)
    a.track_motion(True)
    _set(a, small)
    a.update_geometry(_cuda(_deformed(small)))
    _set(a, sd)
    b = make_ctx(sd, cam)
    _assert_same_state(_state(a), _state(b), "shrink, update, grow back")
    assert np.array_equal(_frame(a).view(np.uint32), _frame(b).view(np.uint32))


def test_set_materials_after_reassign_counts_the_new_triangles(make_ctx):
    from radish_pt_amd import layouts as L

    sd = geometry_edit.SCENES["teapots"]()
    a, _, ed, cam = _pair(make_ctx, "reassign")
    ids = np.array([9, 0], np.int32)  # the stand-in's old material, which no triangle carries now, and the one the lamp quad got
    mats = ed.materials[ids].copy()
    mats["type"] = L.LIGHT
    mats["baseColor"] = (3.0, 2.5, 2.0)
    a.set_materials(ids, mats)
    target = material_edit.edited(ed, ids, mats)
    b = make_ctx(target, cam)
    now, then = np.bincount(ed.material_ids, minlength=10), np.bincount(sd.material_ids, minlength=10)
    assert (now[9], then[9], now[0] - then[0]) == (0, 864, 2)
    assert target.num_lights == ed.num_lights + now[0]
    sa = _state(a)
    _assert_same_state(sa, _state(b), "reassign + set_materials")
    assert sa["lights 1"].view(np.int32)[3] == target.num_lights
    assert np.array_equal(_frame(a).view(np.uint32), _frame(b).view(np.uint32))


def test_host_light_update_takes_the_new_length(make_ctx):
    from radish_pt_amd import api

    sd = geometry_edit.SCENES["teapots"]()
    a, b, ed, cam = _pair(make_ctx, "remove")
    v = _cuda(ed.vertices.reshape(-1))
    assert len(ed.light_sampler) != len(sd.light_sampler)
    with pytest.raises(api.RadishError):
        a.refit_geometry(v, None, (sd.light_sampler, sd.sum_light_power_inv))  # the uploaded length: refused
    a.refit_geometry(v, None, (ed.light_sampler, ed.sum_light_power_inv))
    assert np.array_equal(a.debug_read_lights(0), ed.light_sampler)
    _assert_same_state(_state(a), _state(b), "host table of the new length")


def test_pose_needs_the_object_table_again(make_ctx):
    from radish_pt_amd import api

    sd, cam = geometry_edit.SCENES["teapots"](), _cam("teapots")
    ed = geometry_edit.result("teapots", "remove")
    first, count = geometry_edit.LAYOUT["teapots"]["standins"][1]
    table = np.array([[first, count, 0]], np.int32)
    a = make_ctx(sd, cam)

    def rest(s):
        return s.vertices.reshape(-1, 9)[first:first + count], s.normals.reshape(-1, 9)[first:first + count]

    a.set_objects(objects=table, rest_vertices=rest(sd)[0], rest_normals=rest(sd)[1])
    trs = np.array([[0.1, 0.2, -0.1, 0, 30, 0, 1, 1, 1]], np.float32)
    a.pose_objects([0], trs=trs)
    _set(a, ed)
    with pytest.raises(api.RadishError, match="object table"):
        a.pose_objects([0], trs=trs)
    assert api.lib().rdh_scene_pose_objects(a.h, None, None, 0, 0, 0, 0.0) == -5  # RDH_ERR_STATE
    b = make_ctx(ed, cam)
    for ctx in (a, b):
        ctx.set_objects(objects=table, rest_vertices=rest(ed)[0], rest_normals=rest(ed)[1])
        ctx.pose_objects([0], trs=trs, tree="sah", rebuild_lights=True)
    _assert_same_state(_state(a), _state(b), "edit + set_objects + pose")
    va, vb = a.debug_read_world(), b.debug_read_world()
    assert np.array_equal(va[0], vb[0]) and np.array_equal(va[1], vb[1])
    assert np.array_equal(_frame(a).view(np.uint32), _frame(b).view(np.uint32))


def test_motion_plane_after_an_edit_is_a_fresh_uploads(make_ctx):
    """Tracking stays on through the edit, "previous == current": the render right after it writes what a fresh upload's render
    writes, and an update_geometry after that render is followed."""
    from radish_pt_amd import api

    sd, ed, cam = geometry_edit.SCENES["teapots"](), geometry_edit.result("teapots", "add"), _cam("teapots")
    a, b = make_ctx(sd, cam), make_ctx(ed, cam)
    a.track_motion(True)
    b.track_motion(True)
    moved = _cuda(_deformed(ed, 0.3))
    planes = []
    for ctx in (a, b):
        gb = api.GBuffer()
        gb.create(W, H)
        if ctx is a:  # a frame of the old set, a move of it (so the buffer holds the OLD set's records), then the edit
            ctx.gbuffer_render(gb.c_struct(cam_fallback=cam), 0)
            gb.update(cam)
            ctx.update_geometry(_cuda(_deformed(sd)))
            _set(a, ed)
        else:
            ctx.gbuffer_render(gb.c_struct(cam_fallback=cam), 0)
            gb.update(cam)
        got = []
        for step in range(2):
            if step == 1:
                ctx.update_geometry(moved)
            ctx.gbuffer_render(gb.c_struct(cam_fallback=cam), 0)
            ctx.synchronize()
            k = gb.frameIdx
            got.append({"motion": gb.motion.cpu().numpy().copy(), "primId": gb.primId[k].cpu().numpy().copy()})
            gb.update(cam)
        planes.append(got)
        gb.destroy()
    for step in range(2):
        assert np.array_equal(planes[0][step]["primId"], planes[1][step]["primId"]), step
        assert np.array_equal(planes[0][step]["motion"], planes[1][step]["motion"]), step
    assert (planes[0][1]["motion"] >= 0).sum() > 200
    assert not np.array_equal(planes[0][0]["motion"], planes[0][1]["motion"]), "the update after the render is not followed"


def test_five_edits_and_frames_without_a_host_wait(make_ctx):
    from radish_pt_amd import api

    torch = _torch()
    cam = _cam("teapots")
    a = make_ctx(geometry_edit.SCENES["teapots"](), cam)
    got = []
    for k, edit in enumerate(("remove", "add", "reorder", "one_dark", "reassign")):  # the caller never synchronises in this loop
        ed = geometry_edit.result("teapots", edit)
        _set(a, ed, BUILDERS[k % 2])
        d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
        a.path_trace(d, i, 0, 2, DEPTH, api.RDH_PT_PERSISTENT)
        got.append((edit, BUILDERS[k % 2], ed, d, i))
    a.synchronize()
    for edit, builder, ed, d, i in got:
        b = _fresh(make_ctx, ed, builder, cam)
        ref = _frame(b)
        assert_bit_equal(np.concatenate([d.cpu().numpy(), i.cpu().numpy()]), ref, f"after {edit}")
        b.close()
    _assert_same_state(_state(a), _state(_fresh(make_ctx, got[-1][2], got[-1][1], cam)), "after five edits")


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_unchanged(make_ctx, uploaded):
    from radish_pt_amd import api

    torch = _torch()
    lib = api.lib()
    sd, cam = geometry_edit.SCENES["cornell"](), _cam("cornell")
    ed = geometry_edit.result("cornell", "remove")
    n = ed.num_prims
    ctx = make_ctx()
    v, nr, t, m = (_cuda(a) for a in geometry_edit.arrays(ed))
    env = float(sd.env_power)

    def raw(v=v, nr=nr, t=t, m=m, n=n, builder=api.RDH_BVH_SAH, env=env):
        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        return lib.rdh_scene_set_geometry(ctx.h, ptr(v), ptr(nr), ptr(t), ptr(m), n, builder, env)

    assert raw() == -2  # RDH_ERR_NO_SCENE
    ctx.upload_scene(sd)
    ctx.set_camera(cam)
    for k in ("v", "nr", "t", "m"):
        assert raw(**{k: None}) == -1, k
    assert raw(n=0) == -1 and raw(n=-5) == -1
    assert raw(n=(1 << 29) + 1) == -1  # the builders' limit
    assert raw(n=1 << 26) == -1  # six node arrays of 4 GiB or more
    assert raw(builder=7) == -1
    for bad in (float("nan"), -1.0, float("inf")):
        assert raw(env=bad) == -1, bad
    for where in (0, n // 2, n - 1):
        for bad in (-1, len(sd.materials)):
            broken = m.clone()
            broken[where] = bad
            assert raw(m=broken) == -1, (where, bad)
            assert b"material id" in lib.rdh_last_error(ctx.h)
        broken = v.clone()
        broken[9 * where + 4] = float("inf")
        assert raw(v=broken) == -1, where
        assert b"coordinate" in lib.rdh_last_error(ctx.h)
    with pytest.raises(api.RadishError):
        ctx.set_geometry(v, nr, t[:-6], m)  # texcoords of another count
    with pytest.raises(api.RadishError):
        ctx.set_geometry(v, nr, t, m.to(torch.int64))
    with pytest.raises(api.RadishError):
        ctx.set_geometry(v, nr, t, m, builder="median")
    assert lib.rdh_debug_read_geometry(ctx.h, 4, None, 0) == -1 and lib.rdh_debug_read_geometry(ctx.h, -1, None, 0) == -1
    before, state_before = uploaded["cornell"]
    _assert_same_state(_state(ctx), state_before, "after the refused calls")
    _assert_same_outputs(_outputs(ctx, cam), before, "after the refused calls")
    # the error flags do not stick: the same arrays, unbroken, go through
    assert raw() == 0
    _assert_same_state(_state(ctx), _state(make_ctx(ed, cam)), "after the accepted call")


def test_texcoords_beyond_the_bound_are_refused(make_ctx):
    """proceduralTexture's cell index is int(uv * 1024): from |uv| = 2^21 on that conversion is undefined (and differs between the
    host checker and gfx950), so both entries that take texture coordinates refuse them, and what they accept stays usable."""
    from radish_pt_amd import api

    lib = api.lib()
    sd, cam = geometry_edit.SCENES["cornell"](), _cam("cornell")
    ctx = make_ctx(sd, cam)
    v, nr, t, m = (_cuda(a) for a in geometry_edit.arrays(sd))
    n = sd.num_prims
    ptr = lambda x: C.c_void_p(x.data_ptr())
    state = _state(ctx)
    for where in (0, 3 * n + 1, 6 * n - 1):
        for bad in (2.0 ** 21, -(2.0 ** 21), float("nan"), float("inf")):
            broken = t.clone()
            broken[where] = bad
            assert lib.rdh_scene_set_geometry(ctx.h, ptr(v), ptr(nr), ptr(broken), ptr(m), n, api.RDH_BVH_SAH, float(sd.env_power)) == -1
            assert b"texture coordinate" in lib.rdh_last_error(ctx.h)
    _assert_same_state(_state(ctx), state, "after the refused texcoords")
    edge = t.clone()
    edge[0] = float(np.nextafter(np.float32(2.0 ** 21), np.float32(0)))  # the largest accepted value
    ctx.set_geometry(v, nr, edge, m, env_power=float(sd.env_power))
    import copy

    bad_sd = copy.copy(sd)
    bad_sd.texcoords = sd.texcoords.copy()
    bad_sd.texcoords.reshape(-1)[5] = 2.0 ** 21
    with pytest.raises(api.RadishError, match="texcoords"):
        make_ctx(bad_sd, cam)
