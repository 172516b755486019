"""Refit of the uploaded tree in place (rdh_scene_refit_geometry, kernels_refit.h) and its cost figure (rdh_scene_tree_cost).

The comparison target of a refit is a second context that uploads the moved vertices with the ORIGINAL node arrays and the boxes
of the numpy restatement (refit_model.py): the upload derives the threaded arrays, pairs and root box from those, and the rest of
the suite pins uploads to the oracle."""
import ctypes as C

import numpy as np
import pytest

import refit_model
from helpers import assert_bit_equal, oracle_path_trace_mt
from test_gpu_bvh_build import _frames, _moved

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


def _cuda(a):
    return _torch().from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _tree_state(ctx):
    return ctx.debug_read_tree(0), ctx.debug_read_tree(1), ctx.debug_read_tree(2)


def _assert_same_state(a, b, what):
    na, pa, ha = a
    nb, pb, hb = b
    assert np.array_equal(na, nb), f"{what}: NodeRec arrays differ at byte {np.flatnonzero(na != nb)[:4].tolist()}"
    assert np.array_equal(pa, pb), f"{what}: pair records differ at byte {np.flatnonzero(pa != pb)[:4].tolist()}"
    assert np.array_equal(ha, hb), f"{what}: header {ha.view(np.int32)[:4]} {ha[16:].view(np.float32)} vs {hb.view(np.int32)[:4]} {hb[16:].view(np.float32)}"


def _scene_of(verts, name="soup"):
    from radish_pt_amd import scenes

    base = scenes.tiny()
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    n = v.shape[0] // 3
    return scenes.SceneData(name, v, np.tile(base.normals[:3], (n, 1)), np.tile(base.texcoords[:3], (n, 1)),
                            np.full(n, base.material_ids[0], np.int32), base.materials)


def _with_vertices(sd, verts, normals=None):
    """sd's triangles at new positions, as SceneData (its own tree, which the caller replaces)."""
    from radish_pt_amd import scenes

    return scenes.SceneData(sd.name + "_moved", np.asarray(verts, np.float32).reshape(-1, 3),
                            sd.normals if normals is None else normals, sd.texcoords, sd.material_ids, sd.materials, sd.textures,
                            sd.env_map_tex_id)


def _target(sd, moved):
    """`moved` with sd's topology and the restatement's boxes: what a refit of sd to moved's vertices must upload as."""
    moved.nodes = [n.copy() for n in sd.nodes]
    moved.boxes = refit_model.refit_boxes(moved.vertices, sd.nodes)
    return moved


def _refit(ctx, m):
    ctx.refit_geometry(_cuda(m.vertices), _cuda(m.normals), (m.light_sampler, m.sum_light_power_inv))


def _chain(n):
    from radish_pt_amd import scenes

    t = scenes.tiny()
    return scenes.SceneData("chain", np.tile(t.vertices[:3], (n, 1)), np.tile(t.normals[:3], (n, 1)), np.tile(t.texcoords[:3], (n, 1)),
                            np.full(n, t.material_ids[0], np.int32), t.materials)


def _scene(name):
    from radish_pt_amd import scenes

    if name == "cornell":
        return scenes.cornell(segments=16, bands=12)
    if name == "teapots":
        return scenes.teapots(segments=24, bands=18)
    if name == "chain600":
        return _chain(600)
    if name == "config5":
        return scenes.teapots(segments=200, bands=156, emissive_grid=(16, 32))
    raise ValueError(name)


# ---- 1. a refit with the scene's own vertices changes nothing ----

@pytest.mark.parametrize("scene", ["cornell", "teapots", "chain600", "config5"])
def test_refit_with_own_vertices_equals_upload(scene):
    from radish_pt_amd import api

    sd = _scene(scene)
    ctx = api.Context(0)
    try:
        ctx.upload_scene(sd)
        ref = _tree_state(ctx)
        _refit(ctx, sd)
        _assert_same_state(_tree_state(ctx), ref, f"{scene}: refit after upload")
        _refit(ctx, sd)  # the plan is built; a steady-state refit
        _assert_same_state(_tree_state(ctx), ref, f"{scene}: second refit")
        if scene != "config5":  # (the update of the 1-M scene costs half a second and shows nothing new)
            ctx.update_geometry(_cuda(sd.vertices), _cuda(sd.normals), (sd.light_sampler, sd.sum_light_power_inv))
            _refit(ctx, sd)
            _assert_same_state(_tree_state(ctx), ref, f"{scene}: refit after update_geometry")
    finally:
        ctx.close()


# ---- 2. moved vertices: byte-equal to an upload of the restatement ----

def _noise(sd, seed, sigma):
    rng = np.random.default_rng(seed)
    return sd.vertices + rng.normal(0, sigma, sd.vertices.shape).astype(np.float32)


def _flatten(sd):
    """The last non-light object pressed flat onto the plane y = its mean y (zero-width boxes)."""
    from radish_pt_amd import layouts as L

    light = [i for i in range(len(sd.materials)) if sd.materials[i]["type"] == L.LIGHT]
    other = [m for m in np.unique(sd.material_ids) if m not in light][-1]
    v = sd.vertices.reshape(-1, 3, 3).copy()
    sel = sd.material_ids == other
    v[sel, :, 1] = np.float32(v[sel, :, 1].mean())
    return v.reshape(-1, 3)


def _moved_case(case):
    """(scene as uploaded, scene with the moved vertices)."""
    if case == "rigid_cornell":
        sd = _scene("cornell")
        return sd, _moved(sd, 0)
    if case == "rigid_teapots":
        sd = _scene("teapots")
        return sd, _moved(sd, 1)
    if case == "noise":
        sd = _scene("teapots")
        return sd, _with_vertices(sd, _noise(sd, 1, 0.01))
    if case == "flatten":
        sd = _scene("cornell")
        return sd, _with_vertices(sd, _flatten(sd))
    if case == "signed_zeros":
        rng = np.random.default_rng(3)
        sd = _scene_of(refit_model.signed_zeros_soup(rng))
        return sd, _with_vertices(sd, refit_model.signed_zeros_soup(rng))
    if case == "magnitudes":
        rng = np.random.default_rng(11)
        scale = np.repeat(10.0 ** rng.uniform(-3, 3, (20000, 1, 1)), 3, axis=1).reshape(-1, 1)
        sd = _scene_of((refit_model.soup(20000, 12) * scale).astype(np.float32))
        return sd, _with_vertices(sd, (refit_model.soup(20000, 13) * scale).astype(np.float32))
    if case.startswith("soup"):
        n = int(case[4:])
        sd = _scene_of(refit_model.soup(n, n))
        return sd, _with_vertices(sd, refit_model.soup(n, n + 1))
    if case == "chain4096":
        sd = _chain(4096)
        return sd, _with_vertices(sd, _noise(sd, 2, 0.05))
    raise ValueError(case)


@pytest.mark.parametrize("case", ["rigid_cornell", "rigid_teapots", "noise", "flatten", "signed_zeros", "magnitudes", "soup1", "soup2",
                                  "soup17", "soup100003", "chain4096"])
def test_moved_vertices_equal_upload_of_restatement(case):
    from radish_pt_amd import api

    sd, moved = _moved_case(case)
    target = _target(sd, moved)
    a, b = api.Context(0), api.Context(0)
    try:
        a.upload_scene(sd)
        _refit(a, target)
        b.upload_scene(target)
        sa, sb = _tree_state(a), _tree_state(b)
        if case == "chain4096":
            assert sa[2].view(np.int32)[1] == 0 and len(sa[1]) == 0, "a 4 095-level chain has no pairs"
        _assert_same_state(sa, sb, case)
    finally:
        a.close()
        b.close()


# ---- 3. frames after a refit ----

@pytest.mark.parametrize("scene", ["cornell", "teapots"])
def test_frames_after_refit_equal_upload(scene):
    from radish_pt_amd import api, scenes

    W, H = 512, 320
    sd = _scene(scene)
    cam = scenes.cornell_camera(W, H) if scene == "cornell" else scenes.teapots_camera(W, H)
    target = _target(sd, _moved(sd, 0))
    a, b = api.Context(0), api.Context(0)
    try:
        a.upload_scene(sd)
        a.set_camera(cam)
        _refit(a, target)
        b.upload_scene(target)
        b.set_camera(cam)
        fa, fb = _frames(a, cam, W, H), _frames(b, cam, W, H)
        for name in fa:
            for k, (x, y) in enumerate(zip(fa[name][0], fb[name][0])):
                assert_bit_equal(x.view(np.float32), y.view(np.float32), f"{scene} {name} output {k}")
            assert fa[name][1] == fb[name][1], f"{scene} {name}: counters {fa[name][1]} vs {fb[name][1]}"
        if scene == "cornell":  # one structure against the oracle, on the refitted boxes and the original nodes
            d, i = fa["persistent"][0]
            ref_d = np.zeros((W * H, 3), np.float32)
            ref_i = np.zeros((W * H, 3), np.float32)
            idx, _ = oracle_path_trace_mt(target, cam, ref_d, ref_i, 0, 3, 4, stride=61)
            assert_bit_equal(d[idx], ref_d[idx], "refit frame vs oracle sample, direct")
            assert_bit_equal(i[idx], ref_i[idx], "refit frame vs oracle sample, indirect")
    finally:
        a.close()
        b.close()


# ---- 4. sequences without host synchronisation ----

def _render(ctx, W, H):
    from radish_pt_amd import api

    torch = _torch()
    d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
    ctx.path_trace(d, i, 0, 2, 4, api.RDH_PT_PERSISTENT)
    return d, i


def _assert_renders_like_upload(ctx, got, target, W, H, what):
    ctx.upload_scene(target)
    rd, ri = _render(ctx, W, H)
    ctx.synchronize()
    assert_bit_equal(got[0].cpu().numpy(), rd.cpu().numpy(), f"{what} direct")
    assert_bit_equal(got[1].cpu().numpy(), ri.cpu().numpy(), f"{what} indirect")


def test_sequences_without_synchronisation():
    from radish_pt_amd import api, scenes

    W, H = 256, 192
    sd, cam = _scene("cornell"), scenes.cornell_camera(W, H)
    targets = [_target(sd, _moved(sd, s)) for s in range(8)]
    a, ref = api.Context(0), api.Context(0)
    try:
        ref.set_camera(cam)
        a.upload_scene(sd)
        a.set_camera(cam)
        got = []
        for t in targets:  # eight refits, each checked by a render; no host synchronisation in between
            _refit(a, t)
            got.append(_render(a, W, H))
        # update_geometry (a new topology: the moved scene's own tree), then a refit of that tree, then a render
        m = _moved(sd, 3)
        a.update_geometry(_cuda(m.vertices), _cuda(m.normals), (m.light_sampler, m.sum_light_power_inv))
        after_update = _target(m, _moved(sd, 5))
        _refit(a, after_update)
        got_upd = _render(a, W, H)
        a.synchronize()
        for k, (t, g) in enumerate(zip(targets, got)):
            _assert_renders_like_upload(ref, g, t, W, H, f"refit {k}")
        _assert_renders_like_upload(ref, got_upd, after_update, W, H, "update_geometry, then refit")
        # a different scene uploaded: the old plan must not survive
        other = _scene("teapots")
        cam2 = scenes.teapots_camera(W, H)
        a.upload_scene(other)
        a.set_camera(cam2)
        ref.set_camera(cam2)
        ot = _target(other, _moved(other, 2))
        _refit(a, ot)
        got_other = _render(a, W, H)
        a.synchronize()
        _assert_renders_like_upload(ref, got_other, ot, W, H, "upload of another scene, then refit")
        _assert_same_state(_tree_state(a), _tree_state(ref), "upload of another scene, then refit: tree")
    finally:
        a.close()
        ref.close()


# ---- 5. rejections leave the scene usable ----

def _not_one_tree(sd):
    """sd with ordering 1 taken from the tree of other geometry (each triangle's position given to the next triangle): valid
    threaded arrays over the same primitives, but not an ordering of sd's tree."""
    from radish_pt_amd import hostlib

    rolled = np.roll(sd.vertices.reshape(-1, 3, 3), 1, axis=0).reshape(-1, 3)
    _, rn = hostlib.build_bvh(rolled)
    sd.nodes = [sd.nodes[0], rn[1]] + list(sd.nodes[2:])
    return sd


def test_rejections_leave_scene_usable():
    from radish_pt_amd import api, scenes

    W, H = 64, 48
    sd, cam = _scene("cornell"), scenes.cornell_camera(W, H)
    ctx = api.Context(0)
    try:
        lib = api.lib()
        v = _cuda(sd.vertices)
        assert lib.rdh_scene_refit_geometry(ctx.h, C.c_void_p(v.data_ptr()), None, None) == -1  # before any upload
        with pytest.raises(api.RadishError):
            ctx.refit_geometry(v)
        for scene in (sd, _not_one_tree(_scene("cornell"))):
            ctx.upload_scene(scene)
            ctx.set_camera(cam)
            assert ctx.debug_read_tree(2).view(np.int32)[1] == (1 if scene is sd else 0), "one tree <=> the upload made pairs"
            before = _render(ctx, W, H)
            ctx.synchronize()
            assert lib.rdh_scene_refit_geometry(ctx.h, None, None, None) == -1
            table = np.ascontiguousarray(sd.light_sampler)
            lu = api.LightUpdateC(table.ctypes.data, len(table) + 1, 1.0)
            assert lib.rdh_scene_refit_geometry(ctx.h, C.c_void_p(v.data_ptr()), None, C.byref(lu)) == -1
            lu = api.LightUpdateC(None, len(table), 1.0)
            assert lib.rdh_scene_refit_geometry(ctx.h, C.c_void_p(v.data_ptr()), None, C.byref(lu)) == -1
            with pytest.raises(api.RadishError):
                ctx.refit_geometry(v[:-3])
            with pytest.raises(api.RadishError):
                ctx.refit_geometry(v, normals=v[:-1])
            if scene is not sd:
                moved = _cuda(_moved(sd, 0).vertices)
                assert lib.rdh_scene_refit_geometry(ctx.h, C.c_void_p(moved.data_ptr()), None, None) == -5  # RDH_ERR_STATE
                assert "one tree" in api.lib().rdh_last_error(ctx.h).decode()
            after = _render(ctx, W, H)
            ctx.synchronize()
            assert_bit_equal(after[0].cpu().numpy(), before[0].cpu().numpy(), f"{scene.name}: direct after rejected refits")
            assert_bit_equal(after[1].cpu().numpy(), before[1].cpu().numpy(), f"{scene.name}: indirect after rejected refits")
    finally:
        ctx.close()


# ---- 6. tree_cost ----

def test_tree_cost():
    from radish_pt_amd import api

    sd = _scene("teapots")
    ctx = api.Context(0)
    try:
        ctx.upload_scene(sd)
        c0 = refit_model.tree_cost(sd.boxes)
        now, at_build = ctx.tree_cost()
        assert now == at_build, "before any refit both figures are the current cost"
        assert abs(now - c0) <= 1e-12 * c0, (now, c0)
        assert ctx.tree_cost() == (now, at_build), "tree_cost must repeat exactly"
        # spread one object's triangles apart (each moved away from the object's centre, unscaled): its inner boxes grow, the
        # topology stays
        v = sd.vertices.reshape(-1, 3, 3).astype(np.float64)
        sel = sd.material_ids == np.unique(sd.material_ids)[-1]
        ctr = v[sel].reshape(-1, 3).mean(axis=0)
        tri_ctr = v[sel].mean(axis=1, keepdims=True)
        for step, f in enumerate((1.2, 1.4, 1.6)):
            m = v.copy()
            m[sel] = m[sel] + (tri_ctr - ctr) * np.array([1.0, 0.0, 1.0]) * (f - 1.0)  # in x and z: the object stays on the floor
            t = _target(sd, _with_vertices(sd, m.astype(np.float32).reshape(-1, 3)))
            _refit(ctx, t)
            now2, at2 = ctx.tree_cost()
            assert at2 == at_build, f"step {step}: at_build moved ({at2} vs {at_build})"
            ref = refit_model.tree_cost(t.boxes)
            assert abs(now2 - ref) <= 1e-12 * ref, (now2, ref)
            assert now2 > now, f"spreading by {f} did not raise the cost ({now2} vs {now})"
            assert ctx.tree_cost() == (now2, at2)
        # update_geometry rebuilds: both figures are the new tree's
        ctx.update_geometry(_cuda(sd.vertices), _cuda(sd.normals), (sd.light_sampler, sd.sum_light_power_inv))
        assert ctx.tree_cost() == (now, now)
    finally:
        ctx.close()


# ---- a refit's pending header superseded by an update's ----

@pytest.mark.parametrize("n", [600, 3000])
def test_update_right_after_refit_settles_as_update(n):
    """refit, then update_geometry to a differently shaped (much deeper) tree, then render, with no host synchronisation: the
    update's whole header (treeDepth, pairs or their absence past 2 048 levels, root box) must be what the render takes."""
    from radish_pt_amd import api, scenes

    W, H = 128, 96
    sd = _scene_of(refit_model.soup(n, n), "soup")
    chain = _scene_of(np.tile(refit_model.soup(1, 1), (n, 1)), "chain")  # n coincident triangles: n - 1 levels
    cam = scenes.cornell_camera(W, H)
    a, b = api.Context(0), api.Context(0)
    try:
        a.upload_scene(sd)
        a.set_camera(cam)
        _refit(a, _target(sd, _with_vertices(sd, refit_model.soup(n, n + 7))))  # builds the plan (blocking), queues a refit header
        _refit(a, _target(sd, _with_vertices(sd, refit_model.soup(n, n + 8))))  # asynchronous: its header is still pending
        a.update_geometry(_cuda(chain.vertices), _cuda(chain.normals), (chain.light_sampler, chain.sum_light_power_inv))
        got = _render(a, W, H)
        b.upload_scene(chain)
        b.set_camera(cam)
        ref = _render(b, W, H)
        a.synchronize()
        b.synchronize()
        assert_bit_equal(got[0].cpu().numpy(), ref[0].cpu().numpy(), f"{n}: direct")
        assert_bit_equal(got[1].cpu().numpy(), ref[1].cpu().numpy(), f"{n}: indirect")
        sa, sb = _tree_state(a), _tree_state(b)
        has_pairs = n - 1 <= 2048
        assert sb[2].view(np.int32)[1] == (1 if has_pairs else 0)
        if has_pairs:
            _assert_same_state(sa, sb, f"refit then update to a {n - 1}-level chain")
        else:  # without pairs the root box is no launch's argument (an upload leaves it zero, an update as it was): compare the rest
            _assert_same_state((sa[0], sa[1], sa[2][:16]), (sb[0], sb[1], sb[2][:16]), f"refit then update to a {n - 1}-level chain")
    finally:
        a.close()
        b.close()


def test_tree_cost_of_degenerate_root_is_node_count():
    from radish_pt_amd import api

    v = np.zeros((3 * 50, 3), np.float32)
    v[:, 0] = np.arange(3 * 50, dtype=np.float32) * np.float32(0.01)  # every triangle on the x axis
    sd = _scene_of(v, "segment")
    ctx = api.Context(0)
    try:
        ctx.upload_scene(sd)
        assert ctx.tree_cost() == (float(sd.bvh_size), float(sd.bvh_size))
        moved = sd.vertices.copy()
        moved[:, 0] *= np.float32(2.0)  # stretched along the x axis: still a zero-area root after the refit
        t = _target(sd, _with_vertices(sd, moved))
        _refit(ctx, t)
        assert refit_model.tree_cost(t.boxes) == float(sd.bvh_size)
        assert ctx.tree_cost() == (float(sd.bvh_size), float(sd.bvh_size))
        moved[:, 1] = moved[:, 0]  # onto a diagonal of the xy plane: the root gains area, the ordinary definition applies
        t = _target(sd, _with_vertices(sd, moved))
        _refit(ctx, t)
        now, at_build = ctx.tree_cost()
        ref = refit_model.tree_cost(t.boxes)
        assert at_build == float(sd.bvh_size) and abs(now - ref) <= 1e-12 * ref, (now, ref)
    finally:
        ctx.close()
