"""The device BVH builder (kernels_bvh.h, rdh_build_bvh_device) and moving geometry (rdh_scene_update_geometry).

The builder must give the host builder's tree bit for bit: every parity test pins the frame to that tree.  Moving geometry is
checked against a fresh rdh_scene_upload of the moved scene, which the rest of the suite already pins to the oracle."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


def _device_tree(ctx, verts):
    torch = _torch()
    v = torch.from_numpy(np.ascontiguousarray(verts, np.float32).reshape(-1, 3)).cuda()
    boxes, nodes = ctx.build_bvh_device(v)
    ctx.synchronize()
    return boxes.cpu().numpy(), nodes.cpu().numpy()


def _assert_same_tree(ctx, verts, what):
    from radish_pt_amd import hostlib

    hb, hn = hostlib.build_bvh(verts)
    db, dn = _device_tree(ctx, verts)
    assert_bit_equal(db, hb, f"{what}: boxes")
    for k in range(6):
        ref = np.stack([hn[k]["primitiveId"], hn[k]["boundingBoxId"], hn[k]["nextNodeIfMiss"]], axis=1).astype(np.int32)
        assert np.array_equal(dn[k], ref), f"{what}: ordering {k} differs at {np.argwhere(dn[k] != ref)[:3].tolist()}"


def _soup(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 1, 3)) * scale
    return (c + rng.normal(0, 0.05 * scale, (n, 3, 3))).astype(np.float32).reshape(-1, 3)


@pytest.mark.parametrize("n", [1, 2, 3, 17, 100_003])
def test_random_soups(gpu_ctx, n):
    _assert_same_tree(gpu_ctx, _soup(n, n), f"soup of {n}")


def test_chain_of_coincident_triangles(gpu_ctx):
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    _assert_same_tree(gpu_ctx, np.tile(tri, (4096, 1)), "4 096 coincident triangles")


def test_zero_width_axis(gpu_ctx):
    v = _soup(5000, 7)
    v[:, 1] = 0.25  # every vertex, hence every centroid, on the plane y = 0.25
    _assert_same_tree(gpu_ctx, v, "centroids on one plane")


def test_signed_zeros(gpu_ctx):
    rng = np.random.default_rng(3)
    v = rng.choice(np.array([0.0, -0.0, 1.0, -1.0, 0.5], np.float32), size=(3 * 3000, 3)).astype(np.float32)
    assert (np.signbit(v) & (v == 0)).any() and (~np.signbit(v) & (v == 0)).any()
    _assert_same_tree(gpu_ctx, v, "+0.0 / -0.0 coordinates")


def test_magnitude_spread(gpu_ctx):
    rng = np.random.default_rng(11)
    v = _soup(20000, 12) * np.repeat(10.0 ** rng.uniform(-3, 3, (20000, 1, 1)), 3, axis=1).reshape(-1, 1)
    _assert_same_tree(gpu_ctx, v.astype(np.float32), "1e6 spread of magnitudes")


def test_scenes(gpu_ctx, cornell_full):
    from radish_pt_amd import scenes

    _assert_same_tree(gpu_ctx, cornell_full.vertices, "cornell")
    _assert_same_tree(gpu_ctx, scenes.teapots().vertices, "teapots")


def test_config5_scene(gpu_ctx):
    from radish_pt_amd import scenes

    sd = scenes.teapots(segments=200, bands=156, emissive_grid=(16, 32))
    _assert_same_tree(gpu_ctx, sd.vertices, "config 5 scene")


# ---- upload derivatives ----

def _tree_state(ctx):
    return ctx.debug_read_tree(0), ctx.debug_read_tree(1), ctx.debug_read_tree(2)


@pytest.mark.parametrize("scene", ["cornell", "teapots", "chain"])
def test_update_with_own_vertices_equals_upload(scene):
    from radish_pt_amd import api, scenes

    torch = _torch()
    if scene == "cornell":
        sd = scenes.cornell(segments=16, bands=12)
    elif scene == "teapots":
        sd = scenes.teapots(segments=24, bands=18)
    else:  # a chain 600 levels deep: pairs exist (depth <= 2 048)
        sd = scenes.tiny()
        tri = sd.vertices[:3].copy()
        sd = scenes.SceneData("chain", np.tile(tri, (600, 1)), np.tile(sd.normals[:3], (600, 1)), np.tile(sd.texcoords[:3], (600, 1)),
                              np.full(600, sd.material_ids[0], np.int32), sd.materials)
    ctx = api.Context(0)
    try:
        ctx.upload_scene(sd)
        nodes0, pairs0, hdr0 = _tree_state(ctx)
        assert hdr0.view(np.int32)[1] == 1, "the upload made no pairs"
        ctx.update_geometry(torch.from_numpy(sd.vertices).cuda(), torch.from_numpy(sd.normals).cuda(),
                            (sd.light_sampler, sd.sum_light_power_inv))
        nodes1, pairs1, hdr1 = _tree_state(ctx)
        assert np.array_equal(nodes1, nodes0), "NodeRec arrays differ"
        assert np.array_equal(pairs1, pairs0), "pair records differ"
        assert np.array_equal(hdr1, hdr0), f"treeDepth / root box differ: {hdr1.view(np.int32)[:4]} vs {hdr0.view(np.int32)[:4]}"
    finally:
        ctx.close()


# ---- moving geometry renders like a fresh upload ----

def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


def _moved(sd, step):
    """One object and the (first) emissive material's triangles turned about y and translated; normals turned with them."""
    from radish_pt_amd import layouts as L, scenes

    mats = sd.materials
    light_mats = [i for i in range(len(mats)) if mats[i]["type"] == L.LIGHT]
    other = [m for m in np.unique(sd.material_ids) if m not in light_mats][-1]
    sel = np.isin(sd.material_ids, [light_mats[0], other])
    v = sd.vertices.reshape(-1, 3, 3).astype(np.float64)
    n = sd.normals.reshape(-1, 3, 3).astype(np.float64)
    R = _rot_y(0.15 * (step + 1))
    ctr = v[sel].reshape(-1, 3).mean(axis=0)
    v[sel] = (v[sel] - ctr) @ R.T + ctr + np.array([0.03, -0.01, 0.02]) * (step + 1)
    n[sel] = n[sel] @ R.T
    return scenes.SceneData(sd.name + f"_moved{step}", v.astype(np.float32).reshape(-1, 3), n.astype(np.float32).reshape(-1, 3),
                            sd.texcoords, sd.material_ids, sd.materials, sd.textures, sd.env_map_tex_id)


def _frames(ctx, cam, W, H):
    """Every frame structure the issue names, with counters: {name: (arrays, counters)}."""
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


@pytest.mark.parametrize("scene", ["cornell", "teapots"])
def test_moved_object_renders_like_fresh_upload(scene):
    from radish_pt_amd import api, scenes

    torch = _torch()
    if scene == "cornell":
        sd, cam = scenes.cornell(segments=16, bands=12), scenes.cornell_camera(512, 320)
    else:
        sd, cam = scenes.teapots(segments=24, bands=18), scenes.teapots_camera(512, 320)
    moved = _moved(sd, 0)
    a, b = api.Context(0), api.Context(0)
    try:
        a.upload_scene(sd)
        a.set_camera(cam)
        a.update_geometry(torch.from_numpy(moved.vertices).cuda(), torch.from_numpy(moved.normals).cuda(),
                          (moved.light_sampler, moved.sum_light_power_inv))
        b.upload_scene(moved)
        b.set_camera(cam)
        fa, fb = _frames(a, cam, 512, 320), _frames(b, cam, 512, 320)
        for name in fa:
            for k, (x, y) in enumerate(zip(fa[name][0], fb[name][0])):
                assert_bit_equal(x.view(np.float32), y.view(np.float32), f"{scene} {name} output {k}")
            assert fa[name][1] == fb[name][1], f"{scene} {name}: counters {fa[name][1]} vs {fb[name][1]}"
    finally:
        a.close()
        b.close()


def test_eight_updates_without_synchronisation():
    from radish_pt_amd import api, scenes

    torch = _torch()
    W, H = 256, 192
    sd, cam = scenes.cornell(segments=16, bands=12), scenes.cornell_camera(W, H)
    steps = [_moved(sd, s) for s in range(8)]
    a = api.Context(0)
    try:
        a.upload_scene(sd)
        a.set_camera(cam)
        got = []
        for m in steps:  # no host synchronisation between the updates and frames
            a.update_geometry(torch.from_numpy(m.vertices).cuda(), torch.from_numpy(m.normals).cuda(),
                              (m.light_sampler, m.sum_light_power_inv))
            d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
            a.path_trace(d, i, 0, 2, 4, api.RDH_PT_PERSISTENT)
            got.append((d, i))
        a.synchronize()
        for m, (d, i) in zip(steps, got):
            a.upload_scene(m)
            rd, ri = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
            a.path_trace(rd, ri, 0, 2, 4, api.RDH_PT_PERSISTENT)
            a.synchronize()
            assert_bit_equal(d.cpu().numpy(), rd.cpu().numpy(), f"{m.name} direct")
            assert_bit_equal(i.cpu().numpy(), ri.cpu().numpy(), f"{m.name} indirect")
    finally:
        a.close()


# ---- argument checks: RDH_ERR_ARGS, and the uploaded scene stays usable ----

def test_argument_checks_leave_scene_usable():
    from radish_pt_amd import api, scenes

    torch = _torch()
    W, H = 64, 48
    sd, cam = scenes.cornell(segments=16, bands=12), scenes.cornell_camera(W, H)
    ctx = api.Context(0)
    try:
        lib = api.lib()
        v = torch.from_numpy(sd.vertices).cuda()
        # before any upload
        assert lib.rdh_scene_update_geometry(ctx.h, C.c_void_p(v.data_ptr()), None, None) == -1
        with pytest.raises(api.RadishError):
            ctx.update_geometry(v)
        ctx.upload_scene(sd)
        ctx.set_camera(cam)
        ref = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
        ctx.path_trace(ref[0], ref[1], 0, 0, 4, api.RDH_PT_PERSISTENT)
        # a null pointer
        assert lib.rdh_scene_update_geometry(ctx.h, None, None, None) == -1
        table = np.ascontiguousarray(sd.light_sampler)
        lu = api.LightUpdateC(None, len(table), 1.0)
        assert lib.rdh_scene_update_geometry(ctx.h, C.c_void_p(v.data_ptr()), None, C.byref(lu)) == -1
        # a light table of the wrong length
        lu = api.LightUpdateC(table.ctypes.data, len(table) + 1, 1.0)
        assert lib.rdh_scene_update_geometry(ctx.h, C.c_void_p(v.data_ptr()), None, C.byref(lu)) == -1
        # a wrong triangle count (checked where the count is known: the tensor's size)
        with pytest.raises(api.RadishError):
            ctx.update_geometry(v[:-3])
        assert lib.rdh_build_bvh_device(ctx.h, None, 3, None, None) == -1
        d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
        ctx.path_trace(d, i, 0, 0, 4, api.RDH_PT_PERSISTENT)
        ctx.synchronize()
        assert_bit_equal(d.cpu().numpy(), ref[0].cpu().numpy(), "direct after rejected updates")
        assert_bit_equal(i.cpu().numpy(), ref[1].cpu().numpy(), "indirect after rejected updates")
    finally:
        ctx.close()
