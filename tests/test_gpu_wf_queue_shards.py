"""The wavefront queues in packet-indexed shards (kernels_wave.h, WfShardMap; the layout's model: test_wf_queue_shards_model.py).

k_wf_shade appends packet j's rays and shadow rays to shard j % S of the two queues, its waves pull packets from head g % S only, and
k_wf_trace / k_wf_shade find item i of a stage through the shards' counts.  Which lane traces or shades an item changes no image and no
counter, so every case asks that images are bit-equal to the CPU oracle's, that a counting frame's five work counters equal the
oracle's, and that what every stage queued (rdh_debug_wf_counts, summed over the shards) is the same on the full grid and on a share
of it.  Shapes, where the layout can go wrong:
  16x16    256 paths (stage 0 holds the whole 64x64 ownership tile, 16 packets of mostly off-frame slots): every later stage is one
           packet, fewer packets than shards, seven empty shards, nothing behind the static packets
  64x48    3 072 paths: 12 packets of 256 or fewer; on a 64th of the grid (48 waves at most) nothing to pull
  515x403  neither a multiple of 8, 212 160 records in stage 0.  A 64th of the grid bins packets of 1 024 (208 of them: no multiple of
           8) and pulls most of them, so that some heads run dry before others; a 16th bins 768, 512 and 256 (test_gpu_wf_appends.py)
"""
import numpy as np
import pytest

from helpers import assert_bit_equal, oracle_path_trace_mt

pytestmark = pytest.mark.gpu

COUNTER_KEYS = ("closestRays", "anyRays", "nodeVisits", "triTests", "closestHits")
LOOPER = 11
DEPTHS = (0, 1, 3, 8)
SHAPES = {"16x16": ((16, 16), (64,)), "64x48": ((64, 48), (64,)), "515x403": ((515, 403), (64, 16))}  # (w, h), the shares rendered
VARIANTS = ("sorted_pairs", "sorted_threaded", "unsorted_pairs", "unsorted_threaded", "small_lists", "walk_all")


def _torch():
    import torch

    return torch


def _flags(api, variant="sorted_pairs", count=False):
    sort = not variant.startswith("unsorted")
    pairs = not variant.endswith("threaded")
    f = api.RDH_PT_WAVEFRONT | (api.RDH_PT_SORT_MATERIAL if sort else 0) | (api.RDH_PT_PAIRS if pairs else api.RDH_PT_NO_PAIRS)
    f |= api.RDH_PT_WF_SMALL_LISTS if variant == "small_lists" else 0
    f |= api.RDH_PT_WALK_ALL if variant == "walk_all" else 0
    return f | (api.RDH_PT_COUNT if count else 0)


_oracle_cache = {}


def _oracle(sd, cam, depth, samples=1, pix=None):
    """{'d', 'i', 'stats'} of `samples` accumulated oracle samples (iter s, looper LOOPER + s), computed once and read-only."""
    from oracle import pyoracle

    key = (sd.name, cam.tobytes(), depth, samples, pix)
    if key not in _oracle_cache:
        w, h = (int(v) for v in cam["resolution"])
        d, i = np.zeros((w * h, 3), np.float32), np.zeros((w * h, 3), np.float32)
        stats = {k: 0 for k in COUNTER_KEYS}
        for s in range(samples):
            if pix is None:
                _, st = oracle_path_trace_mt(sd, cam, d, i, s, LOOPER + s, depth)
            else:
                o = pyoracle.OracleScene(sd)
                o.path_trace(cam, d, i, s, LOOPER + s, depth, pix=(pix[0], pix[1], 1))
                st = o.stats()
            for k in COUNTER_KEYS:
                stats[k] += st[k]
        d.setflags(write=False)
        i.setflags(write=False)
        _oracle_cache[key] = {"d": d, "i": i, "stats": stats}
    return _oracle_cache[key]


def _use(ctx, sd, cam):
    ctx.set_partition(0, 1, 64)
    ctx.upload_scene(sd)
    ctx.set_camera(cam)


def _render(ctx, depth, flags, share=1, samples=1, elems=None):
    """(direct, indirect, counters, rays per stage, shadow rays per stage) of one pass on a `share`-th of the resident grid."""
    torch = _torch()
    n = elems if elems is not None else ctx.width * ctx.height
    d, i = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda")
    ctx.counters_reset()
    try:
        ctx.set_occupancy_share(share)
        if samples == 1:
            ctx.path_trace(d, i, 0, LOOPER, depth, flags)
        else:
            ctx.path_trace_samples(d, i, 0, LOOPER, samples, depth, flags, samples_per_pass=samples)
        ctx.synchronize()
        rays, shadows = ctx.debug_wf_counts()
    finally:
        ctx.set_occupancy_share(1)
    return d.cpu().numpy(), i.cpu().numpy(), ctx.counters(), np.asarray(rays), np.asarray(shadows)


def _check(got, ref, what, counters, select=None):
    d, i = (got[0], got[1]) if select is None else (got[0][select[1]], got[1][select[1]])
    assert_bit_equal(d, ref["d"] if select is None else ref["d"][select[0]], f"{what}: direct vs oracle")
    assert_bit_equal(i, ref["i"] if select is None else ref["i"][select[0]], f"{what}: indirect vs oracle")
    if counters:
        for k in COUNTER_KEYS:
            assert got[2][k] == ref["stats"][k], (what, k, got[2][k], ref["stats"][k])


def _frames_on_every_share(ctx, depth, variant, shares, ref, what, samples=1, elems=None, select=None, counters=True):
    """A counting and a default frame on the full grid and on every share of it: images (and the counting frames' counters) against
    the oracle, and what each stage queued against the full grid's frame of the same kind."""
    from radish_pt_amd import api

    full = {}
    for share in (1,) + tuple(shares):
        for count in (True, False):
            got = _render(ctx, depth, _flags(api, variant, count), share, samples, elems)
            name = f"{what}, share {share}, {'count' if count else 'no count'}"
            _check(got, ref, name, counters and count, select)
            assert len(got[3]) == depth + 1 and len(got[4]) == depth + 1, name
            if share == 1:
                full[count] = got
            else:
                assert np.array_equal(got[3], full[count][3]) and np.array_equal(got[4], full[count][4]), (name, got[3], got[4], full[count][3:])
    # a default frame queues no more than a counting one, which queues every ray (and exactly as many when it walks them all)
    assert full[False][3][0] == full[True][3][0] and full[False][3].sum() <= full[True][3].sum() and full[False][4].sum() <= full[True][4].sum()
    if variant == "walk_all":
        assert np.array_equal(full[False][3], full[True][3]) and np.array_equal(full[False][4], full[True][4])
    return full


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_frames(gpu_ctx, cornell_small, shape, depth, variant):
    from radish_pt_amd import scenes

    (w, h), shares = SHAPES[shape]
    cam = scenes.cornell_camera(w, h)
    ref = _oracle(cornell_small, cam, depth)
    _use(gpu_ctx, cornell_small, cam)
    full = _frames_on_every_share(gpu_ctx, depth, variant, shares, ref, f"{shape} depth {depth} {variant}")
    rays, shadows = full[True][3], full[True][4]
    assert rays[0] >= ((w + 7) // 8) * ((h + 7) // 8) * 64 and rays[0] % 64 == 0  # (whole ownership tiles)
    if depth >= 1:
        assert 0 < rays[1] <= rays[0] and shadows[0] > 0, (rays, shadows)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_three_samples_in_one_pass(gpu_ctx, cornell_small, shape, depth):
    from radish_pt_amd import scenes

    (w, h), shares = SHAPES[shape]
    cam = scenes.cornell_camera(w, h)
    ref = _oracle(cornell_small, cam, depth, samples=3)
    _use(gpu_ctx, cornell_small, cam)
    full = _frames_on_every_share(gpu_ctx, depth, "sorted_pairs", shares, ref, f"three samples {shape} depth {depth}", samples=3)
    assert full[True][3][0] >= 3 * ((w + 7) // 8) * ((h + 7) // 8) * 64 and full[True][3][0] % 192 == 0


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_no_emitters(gpu_ctx, cornell_small, shape, depth):
    """No light to sample: every shard of the shadow queue stays empty at every stage."""
    from radish_pt_amd import layouts as L, scenes

    mats = cornell_small.materials.copy()
    for m in range(len(mats)):
        if mats[m]["type"] == L.LIGHT:
            mats[m] = L.make_material(L.LAMBERTIAN, (0.73, 0.73, 0.73))
    sd = scenes.SceneData("cornell_unlit", cornell_small.vertices, cornell_small.normals, cornell_small.texcoords,
                          cornell_small.material_ids, mats)
    assert sd.num_lights == 0
    (w, h), shares = SHAPES[shape]
    cam = scenes.cornell_camera(w, h)
    ref = _oracle(sd, cam, depth)
    assert ref["stats"]["anyRays"] == 0
    _use(gpu_ctx, sd, cam)
    for variant in ("sorted_pairs", "unsorted_threaded"):
        full = _frames_on_every_share(gpu_ctx, depth, variant, shares, ref, f"no emitters {shape} depth {depth} {variant}")
        assert not full[True][4].any() and not full[False][4].any()


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("shape", ("64x96", "515x403"))
def test_rank_one_of_two(gpu_ctx, cornell_small, shape, depth):
    """Tiles of 64 dealt to two ranks, rank 1 rendered.  64x96: the rows from 64 on, which the oracle takes as a pixel range, so the
    counters are checked too; 515x403: 28 of the 63 tiles, edge tiles among them, against those pixels of the whole frame's oracle."""
    from radish_pt_amd import partition, scenes

    w, h = (64, 96) if shape == "64x96" else (515, 403)
    cam = scenes.cornell_camera(w, h)
    frame_idx, packed_idx = partition.rank_pixels(w, h, 1, 2, 64)
    if shape == "64x96":
        assert np.array_equal(frame_idx, np.arange(64 * 64, 64 * 96))
        ref = dict(_oracle(cornell_small, cam, depth, pix=(64 * 64, 64 * 96)))
    else:
        ref = _oracle(cornell_small, cam, depth)
    _use(gpu_ctx, cornell_small, cam)
    try:
        gpu_ctx.set_partition(1, 2, 64)
        _frames_on_every_share(gpu_ctx, depth, "sorted_pairs", (64,), ref, f"rank 1 of 2, {shape} depth {depth}",
                               elems=gpu_ctx.tiles_per_rank() * 64 * 64, select=(frame_idx, packed_idx), counters=shape == "64x96")
    finally:
        gpu_ctx.set_partition(0, 1, 64)


def _adaptive(ctx, request, depth, flags, share):
    torch = _torch()
    p = len(request)
    d, i = torch.zeros(p, 3, device="cuda"), torch.zeros(p, 3, device="cuda")
    c, r = torch.zeros(p, dtype=torch.int32, device="cuda"), torch.from_numpy(request).cuda()
    ctx.counters_reset()
    try:
        ctx.set_occupancy_share(share)
        traced = ctx.path_trace_adaptive(d, i, c, r, LOOPER, depth, flags)
        ctx.synchronize()
        rays, shadows = ctx.debug_wf_counts()
    finally:
        ctx.set_occupancy_share(1)
    assert traced == int(request.sum()) and np.array_equal(c.cpu().numpy(), request)
    return d.cpu().numpy(), i.cpu().numpy(), ctx.counters(), np.asarray(rays), np.asarray(shadows)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_adaptive_call(gpu_ctx, cornell_small, shape, depth):
    """One rdh_path_trace_adaptive: k_ad_raygen writes stage 0's slot list as shard 0 alone.  The small frames request 0..3 samples
    per pixel with whole blocks at 0 and blocks of one pixel, counters against the oracle's single (pixel, sample) calls; the large
    one requests two samples of every pixel for the counters (the sum of two whole frames') and 0..2 scattered for the images."""
    import adaptive_oracle as ao
    from radish_pt_amd import api, scenes

    (w, h), shares = SHAPES[shape]
    p = w * h
    num = 3 if p <= 64 * 48 else 2
    cam = scenes.cornell_camera(w, h)
    fr = ao.frames(cornell_small, cam, LOOPER, num, depth)
    rng = np.random.default_rng(5)
    request = rng.integers(0, num + 1, p).astype(np.int32)
    y, x = np.divmod(np.arange(p), w)
    block = (y // 8) * ((w + 7) // 8) + x // 8
    blocks = rng.permutation(block.max() + 1)
    for b in blocks[: len(blocks) // 4]:
        request[block == b] = 0
    keep = rng.choice(np.flatnonzero(block == blocks[-1]))
    request[(block == blocks[-1]) & (np.arange(p) != keep)] = 0
    request[keep] = num
    assert (request > 0).sum() > 100 and (request == 0).sum() > 60
    _use(gpu_ctx, cornell_small, cam)
    cases = [("scattered", request)]
    if p > 64 * 48:
        cases.append(("uniform", np.full(p, num, np.int32)))
    for name, req in cases:
        on = req > 0
        ed, ei = ao.means_at(fr, req)
        if name == "uniform":
            counters = {k: sum(st[k] for st in fr["stats"]) for k in COUNTER_KEYS}
        else:
            counters = ao.pair_counters(cornell_small, cam, LOOPER, np.zeros(p, np.int32), req, depth) if p <= 64 * 48 else None
        full = None
        for share in (1,) + tuple(shares):
            got = _adaptive(gpu_ctx, req, depth, _flags(api, count=True), share)
            what = f"adaptive {name} {shape} depth {depth} share {share}"
            assert_bit_equal(got[0][on], ed[on], f"{what}: direct vs oracle")
            assert_bit_equal(got[1][on], ei[on], f"{what}: indirect vs oracle")
            assert not got[0][~on].any() and not got[1][~on].any(), what
            if counters is not None:
                for k in COUNTER_KEYS:
                    assert got[2][k] == counters[k], (what, k, got[2][k], counters[k])
            if full is None:
                full = got
                assert got[3][0] > 0 and got[3][0] % 64 == 0
            else:
                assert np.array_equal(got[3], full[3]) and np.array_equal(got[4], full[4]), (what, got[3], got[4], full[3], full[4])
