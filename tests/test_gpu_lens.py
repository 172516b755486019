"""The lens on the GPU (rdh_set_lens).  No oracle knows lens rays, so the new ground is pinned three ways:

  1. rdh_debug_primary_rays — the draw and the cameraSample call of every tracer — against tests/lens_model.py's float32
     restatement, bit for bit, and the mask's device-built alias table against the host's construction, bit for bit;
  2. every kernel structure against the megakernel with the lens on: images and work counters bit-equal;
  3. the megakernel's images against tests/path_model.py's float64 evaluation started from lens_model.lens_rays_f64, on
     tests/path_model_checks.py's frozen scene, size, depth, loopers, tolerance, cap and coverage floor (imported, not re-stated);

and what must not move (the G-buffer, the denoisers, frames after the lens is switched off) is held to what it was."""
import numpy as np
import pytest

import lens_model as LM
import path_model as P
import path_model_checks as C
from helpers import assert_bit_equal, oracle_path_trace_mt
from test_path_model_cpu import COVERED

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

COUNTER_KEYS = ("closestRays", "anyRays", "nodeVisits", "triTests", "closestHits")
W, H, DEPTH, LOOPERS = 64, 48, 4, (7, 8)
N = W * H
# textures of the Cornell stand-in's copy below, in upload order
MASK_NAMES = ("1x1", "1x5", "3x2_one_zero", "16x16_single", "16x16_random", "16x16_black")
RANDOM_MASK = 4
BLACK_MASK = 5


def _torch():
    import torch

    return torch


def _masks():
    rng = np.random.default_rng(31)
    one = np.array([[[0.4, 0.7, 0.2]]], np.float32)                                   # 1 wide, 1 high
    column = (rng.uniform(0.1, 1.0, (5, 1, 3)) ** 2).astype(np.float32)               # 1 wide, 5 high
    m32 = (rng.uniform(0.1, 1.0, (2, 3, 3)) ** 2).astype(np.float32)                  # 3 wide, 2 high
    m32[1, 0] = 0.0
    single = np.zeros((16, 16, 3), np.float32)
    single[5, 11] = (0.3, 0.2, 0.1)
    rand = (rng.uniform(0.0, 1.0, (16, 16, 3)) ** 3).astype(np.float32)
    rand.reshape(-1, 3)[rng.choice(256, 30, replace=False)] = 0.0
    return [one, column, m32, single, rand, np.zeros((16, 16, 3), np.float32)]


@pytest.fixture(scope="module")
def lens_scene(cornell_small):
    """The Cornell stand-in with the masks as its textures (no material uses one)."""
    from radish_pt_amd import scenes

    sd = cornell_small
    return scenes.SceneData("cornell_masks", sd.vertices, sd.normals, sd.texcoords, sd.material_ids, sd.materials, _masks())


def _camera(w, h, radius, focal=4.2):
    from radish_pt_amd import scenes

    cam = scenes.cornell_camera(w, h).copy()
    cam["lensRadius"], cam["focalDist"] = radius, focal
    return cam


def _use(ctx, sd, cam):
    ctx.set_partition(0, 1, 64)
    ctx.upload_scene(sd)
    ctx.set_camera(cam)


def _model_mask(sd, tex_id):
    t = sd.textures[tex_id]
    table, _ = LM.mask_table(t)
    return table, t.shape[1], t.shape[0]


# ---- 1. primary rays by bits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (7, 9), (9, 8), (63, 65), (48, 36)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_primary_rays_equal_the_float32_model(gpu_ctx, lens_scene, shape):
    sd = lens_scene
    _use(gpu_ctx, sd, _camera(*shape, 0.05))
    modes = [(LM.OFF, -1), (LM.DISK, -1)] + [(LM.MASK, t) for t in range(5)]
    for mode, tex in modes:
        gpu_ctx.set_lens(mode, tex)
        mask = _model_mask(sd, tex) if mode == LM.MASK else None
        got_mode, got_tex, gw, gh, table = gpu_ctx.debug_read_lens()
        assert got_mode == mode
        if mode == LM.MASK:
            assert (got_tex, gw, gh) == (tex, mask[1], mask[2])
            assert table.tobytes() == mask[0].tobytes(), f"{MASK_NAMES[tex]}: the device's table is not the host construction's"
        else:
            assert got_tex == -1 and len(table) == 0
        for radius in (0.05, 0.5):
            cam = _camera(*shape, radius)
            gpu_ctx.set_camera(cam)
            for looper in (0, 9999):
                got = gpu_ctx.debug_primary_rays(looper).cpu().numpy().reshape(-1, 6)
                want = LM.lens_rays_f32(cam, sd.sobol, looper, mode, mask)
                assert_bit_equal(got, want, f"{shape} {mode} {MASK_NAMES[tex] if tex >= 0 else ''} radius {radius} looper {looper}")
                if mode == LM.DISK and shape != (1, 1):
                    assert np.ptp(got[:, 0]) > radius  # the origins do move (the camera's right is the x axis)
    gpu_ctx.set_lens("off")


def test_zero_radius_is_the_pinhole(gpu_ctx, lens_scene):
    """A mode other than OFF with lensRadius 0 launches the lens-off kernels: the oracle's frame, bit for bit."""
    from radish_pt_amd import api

    torch = _torch()
    cam = _camera(W, H, 0.0)
    _use(gpu_ctx, lens_scene, cam)
    gpu_ctx.set_lens("disk")
    d, i = torch.zeros(N, 3, device="cuda"), torch.zeros(N, 3, device="cuda")
    gpu_ctx.path_trace(d, i, 0, LOOPERS[0], DEPTH, api.RDH_PT_WAVEFRONT)
    od, oi = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32)
    oracle_path_trace_mt(lens_scene, cam, od, oi, 0, LOOPERS[0], DEPTH)
    assert_bit_equal(d.cpu().numpy(), od, "direct")
    assert_bit_equal(i.cpu().numpy(), oi, "indirect")
    gpu_ctx.set_lens("off")


# ---- 2. structures agree -------------------------------------------------------------------------------------------------------------------
def _frames(ctx, flags, count=False):
    """Iterations 0 and 1 at LOOPERS: [(direct, indirect)] after each, and the counters of both."""
    from radish_pt_amd import api

    torch = _torch()
    d, i = torch.zeros(N, 3, device="cuda"), torch.zeros(N, 3, device="cuda")
    ctx.counters_reset()
    out = []
    for it, looper in enumerate(LOOPERS):
        ctx.path_trace(d, i, it, looper, DEPTH, flags | (api.RDH_PT_COUNT if count else 0))
        out.append((d.cpu().numpy().copy(), i.cpu().numpy().copy()))
    return out, ctx.counters()


@pytest.fixture(scope="module", params=["disk", "mask"])
def lens_ref(request, gpu_ctx, lens_scene):
    """The megakernel's two iterations with the lens on: what every other structure must equal."""
    from radish_pt_amd import api

    mode = request.param
    cam = _camera(W, H, 0.1)

    def use(ctx=gpu_ctx):
        _use(ctx, lens_scene, cam)
        ctx.set_lens(mode, RANDOM_MASK if mode == "mask" else -1)

    use()
    frames, counters = _frames(gpu_ctx, api.RDH_PT_MEGAKERNEL, count=True)
    plain, _ = _frames(gpu_ctx, api.RDH_PT_MEGAKERNEL)
    for (a, b), (c, d) in zip(frames, plain):
        assert_bit_equal(a, c, "counting megakernel, direct")
        assert_bit_equal(b, d, "counting megakernel, indirect")
    gpu_ctx.set_lens("off")
    pin, _ = _frames(gpu_ctx, api.RDH_PT_MEGAKERNEL)
    assert (np.abs(pin[1][1] - frames[1][1]).max(axis=1) > 1e-3).sum() > N // 20, "the lens changes the frame"
    return {"mode": mode, "cam": cam, "use": use, "frames": frames, "counters": counters}


STRUCTURES = ["persistent_threaded", "persistent_pairs", "wavefront", "wavefront_sort", "wavefront_subframes", "wavefront_sort_subframes",
              "wavefront_no_packets", "wavefront_sort_no_packets", "wavefront_subframes_no_packets", "wavefront_sort_subframes_no_packets",
              "wavefront_small_lists", "auto"]


def _structure_flags(api, name):
    if name == "persistent_threaded":
        return api.RDH_PT_PERSISTENT | api.RDH_PT_NO_PAIRS
    if name == "persistent_pairs":
        return api.RDH_PT_PERSISTENT | api.RDH_PT_PAIRS
    if name == "auto":
        return api.RDH_PT_AUTO
    f = api.RDH_PT_WAVEFRONT
    parts = name[len("wavefront"):]
    for part, bit in (("_sort", api.RDH_PT_SORT_MATERIAL), ("_subframes", api.RDH_PT_WF_SUBFRAMES), ("_no_packets", api.RDH_PT_NO_PACKETS),
                      ("_small_lists", api.RDH_PT_WF_SMALL_LISTS)):
        if part in parts:
            f |= bit
            parts = parts.replace(part, "")
    assert parts == "", name
    return f


@pytest.mark.parametrize("structure", STRUCTURES)
def test_structures_equal_the_megakernel(gpu_ctx, lens_ref, structure):
    from radish_pt_amd import api

    lens_ref["use"]()
    flags = _structure_flags(api, structure)
    for count in (True, False):
        frames, counters = _frames(gpu_ctx, flags, count)
        for it, ((d, i), (rd, ri)) in enumerate(zip(frames, lens_ref["frames"])):
            assert_bit_equal(d, rd, f"{structure}, {lens_ref['mode']}, count {count}, iteration {it}: direct")
            assert_bit_equal(i, ri, f"{structure}, {lens_ref['mode']}, count {count}, iteration {it}: indirect")
        if count:
            for k in COUNTER_KEYS:
                assert counters[k] == lens_ref["counters"][k], (structure, k, counters, lens_ref["counters"])
    gpu_ctx.set_lens("off")


def test_three_subframe_pipelines_with_the_lens(gpu_ctx, lens_scene):
    """RDH_PT_WF_SUBFRAMES splits a frame from 2 048 blocks on: 512x256 is exactly that many.  Three pipelines on three streams read
    the mask's table at once; images and counters are the megakernel's."""
    from radish_pt_amd import api

    torch = _torch()
    w, h = 512, 256
    _use(gpu_ctx, lens_scene, _camera(w, h, 0.1))
    gpu_ctx.set_lens("mask", RANDOM_MASK)
    out = []
    for flags in (api.RDH_PT_MEGAKERNEL, api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_WF_SUBFRAMES,
                  api.RDH_PT_WAVEFRONT | api.RDH_PT_WF_SUBFRAMES | api.RDH_PT_NO_PACKETS):
        d, i = torch.zeros(w * h, 3, device="cuda"), torch.zeros(w * h, 3, device="cuda")
        gpu_ctx.counters_reset()
        gpu_ctx.path_trace(d, i, 0, LOOPERS[0], DEPTH, flags | api.RDH_PT_COUNT)
        out.append((d.cpu().numpy(), i.cpu().numpy(), gpu_ctx.counters()))
    gpu_ctx.set_lens("off")
    for d, i, ct in out[1:]:
        assert_bit_equal(d, out[0][0], "sub-frames: direct")
        assert_bit_equal(i, out[0][1], "sub-frames: indirect")
        assert ct == out[0][2]
    assert out[0][1].max() > 0.3


def test_samples_equal_two_frames(gpu_ctx, lens_ref):
    from radish_pt_amd import api

    torch = _torch()
    lens_ref["use"]()
    for flags in (api.RDH_PT_WAVEFRONT, api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL, api.RDH_PT_PERSISTENT):
        d, i = torch.zeros(N, 3, device="cuda"), torch.zeros(N, 3, device="cuda")
        gpu_ctx.path_trace_samples(d, i, 0, LOOPERS[0], 2, DEPTH, flags, samples_per_pass=2 if flags & api.RDH_PT_WAVEFRONT else 0)
        assert_bit_equal(d.cpu().numpy(), lens_ref["frames"][1][0], f"samples, flags {flags}: direct")
        assert_bit_equal(i.cpu().numpy(), lens_ref["frames"][1][1], f"samples, flags {flags}: indirect")
    gpu_ctx.set_lens("off")


def test_adaptive_pass_keeps_its_contract(gpu_ctx, lens_ref):
    """rdh_path_trace_adaptive's contract with the lens on: pixel p with request r over count c holds the images of path_trace at
    iter c + j, looper (looper + c + j) % 10000, j < r — here against the megakernel's lens frames — and a pixel without a request
    is written in no plane.  Requests of 0, 1 and 2 over counts of 0 (all three) and 1 (requests 0 and 1)."""
    from radish_pt_amd import api

    torch = _torch()
    lens_ref["use"]()
    rng = np.random.default_rng(5)
    request = rng.integers(0, 3, N).astype(np.int32)
    count = rng.integers(0, 2, N).astype(np.int32)
    count[request == 2] = 0
    frames = lens_ref["frames"]
    zero = np.zeros((N, 3), np.float32)
    d0, i0 = (np.where((count == 0)[:, None], zero, frames[0][k]) for k in (0, 1))  # the means after 0 or 1 samples
    off = request == 0
    d0[off], i0[off] = -7.25, -7.25
    c0 = count.copy()
    c0[off] = -3
    d, i = torch.from_numpy(d0).cuda(), torch.from_numpy(i0).cuda()
    c, r = torch.from_numpy(c0).cuda(), torch.from_numpy(request).cuda()
    traced = gpu_ctx.path_trace_adaptive(d, i, c, r, LOOPERS[0], DEPTH, api.RDH_PT_WAVEFRONT)
    assert traced == int(request.sum())
    after = count + request
    ed = np.where((after == 1)[:, None], frames[0][0], frames[1][0])
    ei = np.where((after == 1)[:, None], frames[0][1], frames[1][1])
    ed[off], ei[off] = -7.25, -7.25
    ec = after.copy()
    ec[off] = -3
    assert_bit_equal(d.cpu().numpy(), ed, "adaptive: direct")
    assert_bit_equal(i.cpu().numpy(), ei, "adaptive: indirect")
    assert np.array_equal(c.cpu().numpy(), ec)
    gpu_ctx.set_lens("off")


def test_direct_kernel_and_ray_dump_follow_the_lens(gpu_ctx, lens_ref):
    """rdh_path_trace_direct and rdh_dump_rays start from the same primary rays: the dump's first-hit rays are the debug entry's
    (as sets: the dump's order is the atomics'), and the direct image differs from the pinhole's."""
    torch = _torch()
    lens_ref["use"]()
    rays = gpu_ctx.debug_primary_rays(LOOPERS[0]).cpu().numpy().reshape(-1, 6)
    closest, _ = gpu_ctx.dump_rays(LOOPERS[0], 0)
    closest = closest.cpu().numpy().reshape(-1, 6)
    assert len(closest) == N
    key = lambda a: sorted(np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1, 6).tolist())
    assert key(closest) == key(rays)
    d = torch.zeros(N, 3, device="cuda")
    gpu_ctx.path_trace_direct(d, 0, LOOPERS[0])
    gpu_ctx.set_lens("off")
    p = torch.zeros(N, 3, device="cuda")
    gpu_ctx.path_trace_direct(p, 0, LOOPERS[0])
    assert ((d - p).abs().max(dim=1).values > 1e-3).sum().item() > N // 20


def test_two_ranks_of_a_tile_partition_equal_the_whole_frame(gpu_ctx, lens_ref):
    """Two virtual ranks (a context each) of an 8x8-tile partition, untiled, against the whole frame."""
    from radish_pt_amd import api

    torch = _torch()
    packed = []
    ctxs = [api.Context(0) for _ in range(2)]
    try:
        for rank, c in enumerate(ctxs):
            lens_ref["use"](c)
            c.set_partition(rank, 2, 8)
            n = c.tiles_per_rank() * 64
            d, i = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda")
            for it, looper in enumerate(LOOPERS):
                c.path_trace(d, i, it, looper, DEPTH, api.RDH_PT_WAVEFRONT)
            c.synchronize()
            packed.append((d, i))
        for k, what in ((0, "direct"), (1, "indirect")):
            frame = torch.zeros(N, 3, device="cuda")
            ctxs[0].untile(torch.cat([p[k] for p in packed]).contiguous(), frame)
            ctxs[0].synchronize()
            assert_bit_equal(frame.cpu().numpy(), lens_ref["frames"][1][k], f"two ranks, {what}")
    finally:
        for c in ctxs:
            c.close()


# ---- 3. against the float64 model ----------------------------------------------------------------------------------------------------------------
LENS_RADIUS = 0.08


@pytest.fixture(scope="module")
def model_setup():
    """path_model_checks' frozen scene with the 16x16 random mask as one more texture (no material names it), its first camera with
    the lens open and focused on the nearer glass prism."""
    from radish_pt_amd import scenes

    sd, ms, cams = C.setup()
    mask = _masks()[RANDOM_MASK]
    sd2 = scenes.SceneData("path_model_mask", sd.vertices, sd.normals, sd.texcoords, sd.material_ids, sd.materials, list(sd.textures) + [mask],
                           sd.env_map_tex_id)
    cam = cams[0].copy()
    prism = np.array([-0.95, 0.65, -0.27])  # inside the prism of build_scene()'s first _prism call
    cam["lensRadius"] = LENS_RADIUS
    cam["focalDist"] = float((prism - cam["position"].astype(np.float64)) @ cam["view"].astype(np.float64))
    table, _ = LM.mask_table(mask)
    return {"sd": sd2, "ms": ms, "cam": cam, "mask_tex": len(sd.textures), "mask": (table, 16, 16)}


def _model_frames(s, mode, plant=None):
    out, prev = [], None
    for it, looper in enumerate(C.LOOPERS):
        with LM.with_lens(P, s["sd"].sobol, looper, mode, s["mask"], plant):
            out.append(P.single_kernel_pt(s["ms"], s["cam"], looper, C.MAX_DEPTH, it, prev))
        prev = (out[-1]["direct"], out[-1]["indirect"])
    return out


def _gpu_frames(ctx, s, mode):
    from radish_pt_amd import api

    torch = _torch()
    _use(ctx, s["sd"], s["cam"])
    ctx.set_lens(mode, s["mask_tex"] if mode == LM.MASK else -1)
    d, i = torch.zeros(C.N, 3, device="cuda"), torch.zeros(C.N, 3, device="cuda")
    dd = torch.zeros(C.N, 3, device="cuda")
    tested, direct = [], []
    for it, looper in enumerate(C.LOOPERS):
        ctx.path_trace(d, i, it, looper, C.MAX_DEPTH, api.RDH_PT_MEGAKERNEL)
        ctx.path_trace_direct(dd, it, looper)
        tested.append((d.cpu().numpy().copy(), i.cpu().numpy().copy()))
        direct.append(dd.cpu().numpy().copy())
    ctx.set_lens("off")
    return tested, direct


@pytest.mark.parametrize("mode", [LM.DISK, LM.MASK])
def test_megakernel_vs_float64_model_with_lens_rays(gpu_ctx, model_setup, mode):
    """The megakernel's direct and indirect images of both iterations, and the direct kernel's, within path_model_checks' tolerance
    of the model evaluated on lens_rays_f64, outside at most its cap of pixels per image; the model's event masks meet the coverage
    floor with the lens on; the planted mistake (the lens offset on the origin but not on the direction) exceeds the cap tenfold.

    Inputs: radius 0.08, focus on the nearer glass prism (focalDist 4.651); neither was re-chosen.  Pixels left out (measured on an
    MI355X; the cap is 6 per image), the direct images and the direct kernel's none:

        disk   iteration 0: indirect {819}     iteration 1: indirect {1158}
        mask   iteration 0: indirect {}        iteration 1: indirect {23}

    819, no discrete choice, named as what it is: a value below the tolerance's floor.  The pixel's indirect is 3.8e-4, 5.0e-4,
    6.9e-4 after a GGX sample on the normal-mapped metal; the model evaluated on the FLOAT32 lens rays (lens_rays_f32, cast) is
    within 6e-5 relative of the kernel, the model on lens_rays_f64 2.2e-4 to 4.1e-4 away: binary32's rounding of the primary ray
    (1e-7 in origin and direction) carried through the GGX lobe, 2 to 3e-7 absolute against a floor of 2e-4 * 1e-3 = 2e-7.
    1158 and 23, one discrete choice each, the same one: a bounce ray that starts inside binary32's error of its own triangle.
    Pixel 23's first bounce leaves the bowed panel (triangle 25) in a direction whose cosine is 0.100 to the interpolated normal
    but 0.018 to the triangle's plane, so makeOffsetedRay's 1e-5 lifts the origin by 1.8e-7, and the float32 hit position
    (fetchSurface on the kernel's own primary ray, recomputed) lies 1.4e-7 BELOW the plane: the oracle's float32 walker, given that
    ray, hits triangle 25 again at t = 1.4e-6, where the model's ray leaves into the sky.  The path goes on for a bounce (indirect
    5.7e-3 of the map's ground colour instead of 2.2e-2 of its sky).  Pixel 1158's second bounce leaves the normal-mapped metal the
    same way (6.3e-1 instead of 1.6e-2, one closest-hit ray more).  Both are bistable in float32: the oracle's pathTrace on a
    pinhole camera placed at the pixel's lens point and turned onto its lens ray, perturbed by 1e-7, gives the model's value in
    53 of 60 trials and the kernel's, to all digits printed, in 7, for either pixel; the model, perturbed alike, never moves.  Every
    structure's frame is bit-equal to the megakernel's (test_structures_equal_the_megakernel), so these are the pixels of all."""
    s = model_setup
    tested, direct = _gpu_frames(gpu_ctx, s, mode)
    model = _model_frames(s, mode)
    worst = 0
    for it, ((d, i), m) in enumerate(zip(tested, model)):
        for k, g in (("direct", d), ("indirect", i)):
            px = np.flatnonzero(C.far(g, m[k]))
            print(mode, "iteration", it, k, px.tolist())
            C.assert_within_cap(px, f"{mode}, iteration {it}, {k}")
        counts = {k: int(m["events"][k].sum()) for k in COVERED}
        print(mode, it, counts)
        for k, c in counts.items():
            assert c >= C.COVERAGE_FLOOR, (mode, it, k, c)
    assert tested[1][0].max() > 0.3 and tested[1][1].max() > 0.3
    prev = None
    for it, looper in enumerate(C.LOOPERS):
        with LM.with_lens(P, s["sd"].sobol, looper, mode, s["mask"]):
            prev = P.pt_direct(s["ms"], s["cam"], looper, it, prev)
        px = np.flatnonzero(C.far(direct[it], prev))
        print(mode, "path_trace_direct", it, px.tolist())
        C.assert_within_cap(px, f"{mode}, path_trace_direct, iteration {it}")
    planted = _model_frames(s, mode, "dir_pinhole")
    for (d, i), m in zip(tested, planted):
        worst = max(worst, int(C.far(d, m["direct"]).sum()), int(C.far(i, m["indirect"]).sum()))
    print(mode, "planted dir_pinhole: worst image", worst)
    assert worst > 10 * C.CAP


# ---- 4. what must not move -----------------------------------------------------------------------------------------------------------------------
def test_gbuffer_denoisers_and_restir_ignore_or_refuse_the_lens(gpu_ctx, lens_scene):
    from radish_pt_amd import api

    torch = _torch()
    cam = _camera(W, H, 0.3)
    _use(gpu_ctx, lens_scene, cam)

    def planes_and_filter():
        gb = api.GBuffer()
        gb.create(W, H)
        g = gb.c_struct(cam_fallback=cam)
        gpu_ctx.gbuffer_render(g)
        colour = torch.linspace(0.0, 1.0, N * 3, device="cuda").reshape(N, 3).contiguous()
        out = torch.zeros(N, 3, device="cuda")
        gpu_ctx.denoise_eaw(out, colour, g, cam, 64.0, 0.2, 1.0, 1)
        mod = colour.clone()
        gpu_ctx.denoise_modulate(mod, g)
        gpu_ctx.synchronize()
        planes = [gb.albedo, gb.normal[0], gb.motion, gb.depth[0], gb.primId[0], out, mod]
        return gb, g, [p.cpu().numpy().copy() for p in planes]

    _, _, want = planes_and_filter()
    gpu_ctx.set_lens("disk")
    gb, g, got = planes_and_filter()
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    gpu_ctx.restir_init()
    img = torch.full((N, 3), -7.25, device="cuda")
    with pytest.raises(api.RadishError, match=r"error -3:"):
        gpu_ctx.restir_direct(img, 0, 40, g, 3)
    gpu_ctx.synchronize()
    assert (img == -7.25).all().item()
    gpu_ctx.set_lens("off")
    gpu_ctx.restir_direct(img, 0, 40, g, 3)  # and runs again without it
    gpu_ctx.synchronize()
    assert (img != -7.25).any().item()
    gpu_ctx.restir_free()


def test_lens_off_and_a_new_upload_are_the_oracle_again(gpu_ctx, lens_scene):
    from radish_pt_amd import api

    torch = _torch()
    cam = _camera(W, H, 0.3)
    od, oi = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32)
    oracle_path_trace_mt(lens_scene, cam, od, oi, 0, LOOPERS[0], DEPTH)

    def frame(flags):
        d, i = torch.zeros(N, 3, device="cuda"), torch.zeros(N, 3, device="cuda")
        gpu_ctx.path_trace(d, i, 0, LOOPERS[0], DEPTH, flags)
        return d.cpu().numpy(), i.cpu().numpy()

    _use(gpu_ctx, lens_scene, cam)
    for mode, tex in (("disk", -1), ("mask", RANDOM_MASK)):
        for flags in (api.RDH_PT_MEGAKERNEL, api.RDH_PT_PERSISTENT, api.RDH_PT_WAVEFRONT):
            gpu_ctx.set_lens(mode, tex)
            d, _ = frame(flags)
            assert (np.abs(d - od).max(axis=1) > 1e-3).sum() > N // 20
            gpu_ctx.set_lens("off")
            d, i = frame(flags)
            assert_bit_equal(d, od, f"after {mode}, off, flags {flags}: direct")
            assert_bit_equal(i, oi, f"after {mode}, off, flags {flags}: indirect")
    gpu_ctx.set_lens("mask", RANDOM_MASK)
    gpu_ctx.upload_scene(lens_scene)  # resets the mode
    assert gpu_ctx.debug_read_lens()[0] == "off"
    d, i = frame(api.RDH_PT_WAVEFRONT)
    assert_bit_equal(d, od, "after a new upload: direct")
    assert_bit_equal(i, oi, "after a new upload: indirect")


# ---- 5. edits and errors -------------------------------------------------------------------------------------------------------------------------
def test_set_texture_on_the_mask_rebuilds_the_table(gpu_ctx, lens_scene):
    torch = _torch()
    sd = lens_scene
    cam = _camera(48, 36, 0.5)
    _use(gpu_ctx, sd, cam)
    gpu_ctx.set_lens("mask", RANDOM_MASK)
    before = gpu_ctx.debug_primary_rays(11).cpu().numpy().copy()
    rng = np.random.default_rng(77)
    fresh = (rng.uniform(0.0, 1.0, (16, 16, 3)) ** 2).astype(np.float32)
    fresh[:8] = 0.0  # the upper half of the aperture closed
    gpu_ctx.set_texture(RANDOM_MASK, torch.from_numpy(fresh).cuda())
    table, _ = LM.mask_table(fresh)
    assert gpu_ctx.debug_read_lens()[4].tobytes() == table.tobytes()
    got = gpu_ctx.debug_primary_rays(11).cpu().numpy()
    want = LM.lens_rays_f32(cam, sd.sobol, 11, LM.MASK, (table, 16, 16))
    assert_bit_equal(got.reshape(-1, 6), want, "primary rays after the edit")
    assert not np.array_equal(got, before)
    # a texture that is not the mask leaves the table alone
    gpu_ctx.set_texture(3, torch.from_numpy(_masks()[3] * 2).cuda())
    assert gpu_ctx.debug_read_lens()[4].tobytes() == table.tobytes()
    # an edit that would close the aperture is refused, the scene and the table as they were
    from radish_pt_amd import api
    with pytest.raises(api.RadishError, match=r"error -1:"):
        gpu_ctx.set_texture(RANDOM_MASK, torch.zeros(16, 16, 3, device="cuda"))
    assert gpu_ctx.debug_read_lens()[4].tobytes() == table.tobytes()
    assert_bit_equal(gpu_ctx.debug_primary_rays(11).cpu().numpy().reshape(-1, 6), want, "primary rays after the refused edit")
    gpu_ctx.set_lens("off")


def test_bad_arguments_leave_the_previous_mode_in_force(gpu_ctx, lens_scene):
    from radish_pt_amd import api

    sd = lens_scene
    cam = _camera(48, 36, 0.5)
    _use(gpu_ctx, sd, cam)
    set_lens = api.lens_entries()[0]
    for prev_mode, prev_tex in (("disk", -1), ("mask", 2)):
        gpu_ctx.set_lens(prev_mode, prev_tex)
        state = gpu_ctx.debug_read_lens()
        want = gpu_ctx.debug_primary_rays(3).cpu().numpy().copy()
        for mode, tex in ((api.RDH_LENS_MASK, BLACK_MASK), (api.RDH_LENS_MASK, -1), (api.RDH_LENS_MASK, len(sd.textures)), (3, 0), (-1, 0)):
            assert set_lens(gpu_ctx.h, mode, tex) == -1, (mode, tex)  # RDH_ERR_ARGS
            now = gpu_ctx.debug_read_lens()
            assert now[:4] == state[:4] and now[4].tobytes() == state[4].tobytes()
            assert_bit_equal(gpu_ctx.debug_primary_rays(3).cpu().numpy(), want, f"after refused set_lens({mode}, {tex})")
    with pytest.raises(api.RadishError):
        gpu_ctx.set_lens("iris")
    gpu_ctx.set_lens("off")
