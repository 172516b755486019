"""Every traversal structure against the oracle on the trees the LBVH builder and the refit make (the cases of
test_tree_shapes_cpu.py), bit for bit, work counters included.

The frame tests of test_gpu_bvh_lbvh.py and test_gpu_bvh_refit.py compare an updated context with one that uploaded the same tree:
both run the same kernels, so a walker that goes wrong on a tree shape goes wrong on both sides.  Here the other side is the oracle.
These trees reach what the host's SAH trees barely do: leaves at uneven depths and pair-walk stacks deeper than the LDS ring
(traverse.h pairPush), primary rays past the packet walk's 256-visit budget (refit_scrambled), far children whose provisional
box test the walk's closest distance overtakes.

Each case first checks that the device holds the restated tree (byte-equal to an upload of it), so a failure names its layer."""
import numpy as np
import pytest

from helpers import assert_bit_equal, oracle_path_trace_mt, random_segments
from test_gpu_bvh_refit import _assert_same_state, _cuda, _scene, _tree_state
from test_gpu_configs import teasets_1m  # noqa: F401  (the fixture)
from test_tree_shapes_cpu import CASES, brute_force, case_rays, same_vertex_trees, tree_case

pytestmark = pytest.mark.gpu

COUNTER_KEYS = ("closestRays", "anyRays", "nodeVisits", "triTests", "closestHits")
W, H, DEPTH = 61, 43, 4  # not a multiple of the 8x8 block


def _torch():
    import torch

    return torch


def _apply(ctx, call, m):
    lights = (m.light_sampler, m.sum_light_power_inv)
    if call == "lbvh":
        ctx.update_geometry(_cuda(m.vertices), _cuda(m.normals), lights, builder="lbvh")
    else:
        ctx.refit_geometry(_cuda(m.vertices), _cuda(m.normals), lights)


def _camera(name, w, h, f=0):
    from radish_pt_amd import hostlib

    if "cornell" in name:  # scenes.cornell_camera at f = 0
        return hostlib.make_camera(w, h, eye=(0.04 * f, 1.0, 4.2), rotation=(-90.0, 0.0, 0.0), fovy=20.0)
    return hostlib.make_camera(w, h, eye=(0.3 + 0.05 * f, 1.9, 7.4), rotation=(-91.5, -11.0, 0.0), fovy=19.0)  # scenes.teapots_camera


def _device_with_tree(sd, calls, target, what):
    """A context that uploaded sd and made `calls`, checked to hold `target`'s tree."""
    from radish_pt_amd import api

    ctx, ref = api.Context(0), api.Context(0)
    try:
        ctx.upload_scene(sd)
        for call, m in calls:
            _apply(ctx, call, m)
        ref.upload_scene(target)
        _assert_same_state(_tree_state(ctx), _tree_state(ref), f"{what}: device tree vs an upload of the restated tree")
    except BaseException:
        ctx.close()
        raise
    finally:
        ref.close()
    return ctx


@pytest.fixture(scope="module", params=CASES)
def shaped(request):
    from oracle import pyoracle

    name = request.param
    sd, calls, target = tree_case(name)
    ctx = _device_with_tree(sd, calls, target, name)
    yield name, ctx, target, pyoracle.OracleScene(target)
    ctx.close()


# ---- ray batches ----

WALKERS = ["one_lane_per_ray", "persistent_threaded", "persistent", "sibling_pairs", "workgroup_per_ray"]


def _walker_flags(api, walker):
    return {"one_lane_per_ray": 0, "persistent_threaded": api.RDH_PT_PERSISTENT | api.RDH_PT_NO_PAIRS, "persistent": api.RDH_PT_PERSISTENT,
            "sibling_pairs": api.RDH_PT_PERSISTENT | api.RDH_PT_PAIRS, "workgroup_per_ray": api.RDH_PT_WG_PER_RAY}[walker]


@pytest.mark.parametrize("walker", WALKERS)
def test_ray_batches(shaped, walker):
    """Closest and any hit, with the counters and without them (without, the pair walk stacks only the far children it hit)."""
    from radish_pt_amd import api, layouts as L

    torch = _torch()
    name, ctx, target, o = shaped
    rays = case_rays(target, 4096, 31)
    lo, hi = target.vertices.min(axis=0), target.vertices.max(axis=0)
    seg = random_segments(4096, 37, tuple(lo), tuple(hi))
    o.reset_stats()
    ref_h = o.trace_closest(rays)
    st_h = o.stats()
    o.reset_stats()
    ref_o = o.trace_occluded(seg)
    st_o = o.stats()
    assert (ref_h["primId"] >= 0).mean() > 0.3 and 0.05 < ref_o.mean() < 0.95
    for count in (True, False):
        flags = _walker_flags(api, walker) | (api.RDH_PT_COUNT if count else 0)
        what = f"{name} {walker} count={count}"
        d_hits = torch.full((len(rays), 4), 0x7fffffff, dtype=torch.int32, device="cuda")  # poison: an unwritten record shows
        ctx.counters_reset()
        ctx.trace_closest(_cuda(rays), d_hits, flags)
        got = d_hits.cpu().numpy().view(L.HIT_DTYPE).reshape(-1)
        assert np.array_equal(got["primId"], ref_h["primId"]), f"{what}: {np.count_nonzero(got['primId'] != ref_h['primId'])} primIds differ"
        for f in ("u", "v", "t"):
            assert_bit_equal(got[f], ref_h[f], f"{what}: hit.{f}")
        if count:
            ct = ctx.counters()
            for k in ("closestRays", "nodeVisits", "triTests", "closestHits"):
                assert ct[k] == st_h[k], (what, k, ct[k], st_h[k])
        d_occ = torch.full((len(seg),), -7, dtype=torch.int32, device="cuda")
        ctx.counters_reset()
        ctx.trace_occluded(_cuda(seg), d_occ, flags)
        assert np.array_equal(d_occ.cpu().numpy(), ref_o), f"{what}: occlusion"
        if count:
            ct = ctx.counters()
            for k in ("anyRays", "nodeVisits", "triTests"):
                assert ct[k] == st_o[k], (what, k, ct[k], st_o[k])


# ---- whole frames ----

def _frame_flags(api):
    # (At this size RDH_PT_WF_SUBFRAMES keeps one pipeline: the split starts at 2 048 blocks.  Config 5 below runs it split.)
    return {"megakernel": api.RDH_PT_MEGAKERNEL, "wavefront": api.RDH_PT_WAVEFRONT,
            "wavefront_sort": api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL,
            "wavefront_subframes": api.RDH_PT_WAVEFRONT | api.RDH_PT_WF_SUBFRAMES,
            "wavefront_sort_subframes": api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_WF_SUBFRAMES,
            "wavefront_sort_threaded": api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_NO_PAIRS,
            "wavefront_small_lists": api.RDH_PT_WAVEFRONT | api.RDH_PT_WF_SMALL_LISTS,
            "persistent": api.RDH_PT_PERSISTENT, "persistent_threaded": api.RDH_PT_PERSISTENT | api.RDH_PT_NO_PAIRS,
            "auto": api.RDH_PT_AUTO}


def test_path_trace_frames(shaped):
    """Depth 4, two accumulated iterations, every structure with its counters; the pair walkers once more without them."""
    from radish_pt_amd import api

    torch = _torch()
    name, ctx, target, o = shaped
    cam = _camera(name, W, H)
    ref_d = np.zeros((W * H, 3), np.float32)
    ref_i = np.zeros((W * H, 3), np.float32)
    stats = {k: 0 for k in COUNTER_KEYS}
    for it in range(2):
        _, st = oracle_path_trace_mt(target, cam, ref_d, ref_i, it, 17 + it, DEPTH)
        for k in COUNTER_KEYS:
            stats[k] += st[k]
    assert ref_d.max() > 0 and ref_i.max() > 0
    ctx.set_camera(cam)
    runs = [(s, f | api.RDH_PT_COUNT) for s, f in _frame_flags(api).items()]
    runs += [(s + " (no counters)", _frame_flags(api)[s]) for s in ("persistent", "wavefront_sort")]
    for structure, flags in runs:
        d = torch.zeros(W * H, 3, device="cuda")
        i = torch.zeros(W * H, 3, device="cuda")
        ctx.counters_reset()
        for it in range(2):
            ctx.path_trace(d, i, it, 17 + it, DEPTH, flags)
        assert_bit_equal(d.cpu().numpy(), ref_d, f"{name} {structure}: direct")
        assert_bit_equal(i.cpu().numpy(), ref_i, f"{name} {structure}: indirect")
        if flags & api.RDH_PT_COUNT:
            ct = ctx.counters()
            for k in COUNTER_KEYS:
                assert ct[k] == stats[k], (name, structure, k, ct[k], stats[k])


# ---- G-buffer ----

@pytest.mark.parametrize("kernel", ["packets", "packets_budget_4", "persistent", "one_lane_per_pixel", "no_defer"])
def test_gbuffer(shaped, kernel):
    from oracle import pyoracle
    from radish_pt_amd import api

    name, ctx, target, o = shaped
    flags = api.RDH_PT_COUNT | {"packets": 0, "packets_budget_4": api.RDH_PT_WF_SMALL_LISTS, "persistent": api.RDH_PT_NO_PACKETS,
                                "one_lane_per_pixel": api.RDH_PT_MEGA_GBUFFER, "no_defer": api.RDH_PT_NO_DEFER}[kernel]
    gb_ref = pyoracle.GBufferHost(W, H)
    gb = api.GBuffer()
    gb.create(W, H)
    for f in range(2):
        cam = _camera(name, W, H, f)
        before = o.stats()
        o.gbuffer_render(cam, gb_ref)
        after = o.stats()
        ctx.set_camera(cam)
        ctx.counters_reset()
        ctx.gbuffer_render(gb.c_struct(cam_fallback=cam), flags)
        ctx.synchronize()
        cur = gb.frameIdx
        what = f"{name} {kernel} frame {f}"
        assert np.array_equal(gb.primId[cur].cpu().numpy(), gb_ref.primId[cur]), f"{what}: primId"
        assert np.array_equal(gb.motion.cpu().numpy(), gb_ref.motion), f"{what}: motion"
        assert_bit_equal(gb.albedo.cpu().numpy(), gb_ref.albedo, f"{what}: albedo")
        assert_bit_equal(gb.normal[cur].cpu().numpy(), gb_ref.normal[cur], f"{what}: normal")
        assert_bit_equal(gb.depth[cur].cpu().numpy(), gb_ref.depth[cur], f"{what}: depth")
        ct = ctx.counters()
        for k in ("closestRays", "nodeVisits", "triTests", "closestHits"):
            assert ct[k] == after[k] - before[k], (what, k)
        gb_ref.update(cam)
        gb.update(cam)
    assert (gb_ref.primId[0] >= 0).mean() > 0.3
    gb.destroy()


# ---- ReSTIR DI ----

@pytest.mark.parametrize("structure", ["split", "fused", "no_packets"])
def test_restir(shaped, structure):
    """Two frames with a moving camera, temporal and spatial reuse: images and the reservoirs each frame leaves."""
    from oracle import pyoracle
    from radish_pt_amd import api, layouts as L

    torch = _torch()
    name, ctx, target, o = shaped
    flags = api.RDH_PT_COUNT | {"split": 0, "fused": api.RDH_PT_RESTIR_FUSED, "no_packets": api.RDH_PT_NO_PACKETS}[structure]
    n = W * H
    gb_ref = pyoracle.GBufferHost(W, H)
    gb = api.GBuffer()
    gb.create(W, H)
    res = [np.zeros(n, L.RESERVOIR_DTYPE) for _ in range(3)]
    ref = np.zeros((n, 3), np.float32)
    img = torch.zeros(n, 3, device="cuda")
    ctx.set_camera(_camera(name, W, H))
    ctx.restir_init()
    try:
        for f in range(2):
            cam = _camera(name, W, H, f)
            o.gbuffer_render(cam, gb_ref)
            before = o.stats()
            o.restir_direct(cam, ref, 0, 40 + f, res[0], res[1], res[2], gb_ref, f == 0, 3, 1)
            after = o.stats()
            res[0], res[1] = res[1], res[0]
            ctx.set_camera(cam)
            ctx.gbuffer_render(gb.c_struct(cam_fallback=cam), 0)
            ctx.counters_reset()
            ctx.restir_direct(img, 0, 40 + f, gb.c_struct(cam), 3, flags=flags)
            ctx.synchronize()
            what = f"{name} ReSTIR {structure} frame {f}"
            assert_bit_equal(img.cpu().numpy(), ref, what)
            assert ctx.restir_read(1).tobytes() == res[1].tobytes(), f"{what}: reservoirs"
            ct = ctx.counters()
            for k in COUNTER_KEYS:
                assert ct[k] == after[k] - before[k], (what, k)
            gb_ref.update(cam)
            gb.update(cam)
        assert ref.max() > 0
    finally:
        ctx.restir_free()
        gb.destroy()


# ---- a tree-free invariant ----

def _record_bits(hits):
    return np.ascontiguousarray(hits).view(np.int32).reshape(len(hits), 4)


def test_closest_hits_do_not_depend_on_the_tree():
    """The same vertices under the host's SAH tree, the LBVH tree and a refitted tree: the GPU's closest hits are bitwise equal to each
    other and to brute force, except where the brute-force winner is a tie or far (test_tree_shapes_cpu.brute_force).  Per-triangle
    arithmetic does not depend on the tree, so a walker that misses a hit fails here even where the oracle would share its mistake."""
    from radish_pt_amd import api

    torch = _torch()
    trees = same_vertex_trees()
    sd = _scene("teapots")
    scr = trees["sah"]
    ctxs = {"sah": api.Context(0)}
    try:
        ctxs["sah"].upload_scene(scr)
        ctxs["lbvh"] = _device_with_tree(sd, [("lbvh", scr)], trees["lbvh"], "lbvh of the scrambled teapots")
        ctxs["refit"] = _device_with_tree(sd, [("refit", scr)], trees["refit"], "refit to the scrambled teapots")
        rays = case_rays(scr, 8192, 53)
        b, ok = brute_force(scr, rays)
        assert ok.mean() > 0.99, f"{np.count_nonzero(~ok)} of {len(ok)} rays excluded as ties or far"
        assert (b["primId"][ok] >= 0).mean() > 0.3
        for tree, ctx in ctxs.items():
            for walker in WALKERS:
                d_hits = torch.full((len(rays), 4), 0x7fffffff, dtype=torch.int32, device="cuda")
                ctx.trace_closest(_cuda(rays), d_hits, _walker_flags(api, walker))
                got = d_hits.cpu().numpy()
                bad = np.flatnonzero((got[ok] != _record_bits(b)[ok]).any(axis=1))
                assert len(bad) == 0, f"{tree} {walker}: {len(bad)} of {ok.sum()} hits differ from brute force, first ray {np.flatnonzero(ok)[bad[0]]}"
    finally:
        for c in ctxs.values():
            c.close()


# ---- config 5: the 1 M-triangle teapots at 4K, depth 8 ----

def _frame4k(ctx, flags, looper):
    from radish_pt_amd import api

    torch = _torch()
    n = 3840 * 2160
    d, i = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda")
    ctx.counters_reset()
    ctx.path_trace(d, i, 0, looper, 8, flags | api.RDH_PT_COUNT)
    return d, i, ctx.counters()


def _same_frame(a, b, what):
    for k, plane in enumerate(("direct", "indirect")):
        x, y = a[k].view(_torch().int32), b[k].view(_torch().int32)
        if not _torch().equal(x, y):
            bad = (x != y).any(dim=1).nonzero().flatten()
            raise AssertionError(f"{what} {plane}: {len(bad)} pixels differ bitwise, first {int(bad[0])}")
    assert a[2] == b[2], f"{what}: counters {a[2]} vs {b[2]}"


def _vs_oracle_sample(sd, cam, got, looper, what):
    ref_d = np.zeros((3840 * 2160, 3), np.float32)
    ref_i = np.zeros((3840 * 2160, 3), np.float32)
    idx, _ = oracle_path_trace_mt(sd, cam, ref_d, ref_i, 0, looper, 8, stride=401)
    assert len(idx) >= 20000
    t = _torch().from_numpy(idx).cuda()
    assert_bit_equal(got[0][t].cpu().numpy(), ref_d[idx], f"{what}: direct vs oracle sample")
    assert_bit_equal(got[1][t].cpu().numpy(), ref_i[idx], f"{what}: indirect vs oracle sample")
    assert ref_i[idx].max() > 0


def test_config5_wavefront_subframes(gpu_ctx, teasets_1m):
    """bench.py's wavefront2 (RDH_PT_WAVEFRONT | RDH_PT_WF_SUBFRAMES) and the headline structure (with RDH_PT_SORT_MATERIAL) on the
    uploaded SAH tree: the whole frame equals the persistent kernel's with equal counters, and > 20 000 pixels equal the oracle."""
    from radish_pt_amd import api, scenes

    sd = teasets_1m
    cam = scenes.teapots_camera(3840, 2160)
    gpu_ctx.set_partition(0, 1, 64)
    gpu_ctx.upload_scene(sd)
    gpu_ctx.set_camera(cam)
    persist = _frame4k(gpu_ctx, api.RDH_PT_PERSISTENT, 5)
    assert persist[2]["closestRays"] >= 3840 * 2160
    sort2 = _frame4k(gpu_ctx, api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_WF_SUBFRAMES, 5)
    _same_frame(sort2, persist, "config 5: wavefront + sort, sub-frames vs persistent")
    del sort2
    wave2 = _frame4k(gpu_ctx, api.RDH_PT_WAVEFRONT | api.RDH_PT_WF_SUBFRAMES, 5)
    _same_frame(wave2, persist, "config 5: wavefront, sub-frames vs persistent")
    _vs_oracle_sample(sd, cam, wave2, 5, "config 5: wavefront, sub-frames")


def test_config5_after_lbvh_update(gpu_ctx, teasets_1m):
    """The same scene after update_geometry(builder="lbvh") with its own vertices (the tree behind the LBVH config-3 and config-5
    timings): the headline structure equals the oracle on > 20 000 pixels of the restated LBVH tree and the persistent frame whole."""
    import copy

    import lbvh_model
    from radish_pt_amd import api, scenes

    sd = teasets_1m
    cam = scenes.teapots_camera(3840, 2160)
    target = copy.copy(sd)  # the same arrays, another tree (a SceneData of these vertices would first build the host's)
    target.boxes, target.nodes = lbvh_model.build(sd.vertices)
    ctx = _device_with_tree(sd, [("lbvh", sd)], target, "config 5 LBVH")
    try:
        ctx.set_camera(cam)
        persist = _frame4k(ctx, api.RDH_PT_PERSISTENT, 6)
        sort2 = _frame4k(ctx, api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_WF_SUBFRAMES, 6)
        _same_frame(sort2, persist, "config 5 LBVH: wavefront + sort, sub-frames vs persistent")
        del persist
        _vs_oracle_sample(target, cam, sort2, 6, "config 5 LBVH: wavefront + sort, sub-frames")
    finally:
        ctx.close()
