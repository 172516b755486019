"""The ray-batch walkers (kernels_walk.h: walkLanes behind k_walk_persistent and k_walk_pair) with MORE WORK THAN WAVES.

The other ray-batch tests trace 4 096 or 8 192 rays: the launch is then never larger than the work, every wave gets exactly the one
64-ray chunk of its index, and neither the shared chunk head (PersistCounters::blockHead) nor a refill that crosses a chunk
boundary ever runs.  Here the grid is a 64th of the resident one (rdh_set_occupancy_share(64): at most 8 waves x 1 024 SIMDs / 64
= 128 workgroups, at least 8), so from 16 384 rays on every wave takes at least two chunks whatever the occupancy:
  n = 20 000: 312 full chunks and a ragged one of 32 rays,
  n = 16 385: a last chunk of ONE ray.
Every 97th ray is axis-parallel (literal class: traced whole by the wave, met here in the middle of a refill), and two rays have a
NaN origin: on the public entries a ray like any other, which gets a record and is counted
(test_gpu_parity.py, test_nan_origin_ray_gets_a_record_in_every_walker).
Bar: records and occlusion flags bit-equal to the oracle; with RDH_PT_COUNT the five work counters equal the oracle's."""
import numpy as np
import pytest

from helpers import assert_bit_equal, random_rays, random_segments

pytestmark = pytest.mark.gpu

SIZES = (20000, 16385)


@pytest.fixture(scope="module")
def cornell_gpu(gpu_ctx, cornell_small):
    gpu_ctx.set_partition(0, 1, 64)
    gpu_ctx.upload_scene(cornell_small)
    return gpu_ctx


def _batch(n):
    rays, seg = random_rays(n, seed=41 + n), random_segments(n, seed=43 + n)
    k = np.arange(0, n, 97)
    axis = (k // 97) % 3
    sign = np.where((k // 97) % 2 == 0, 1.0, -1.0).astype(np.float32)
    rays[k, 3:] = 0
    rays[k, 3 + axis] = sign
    seg[k, 3:] = seg[k, :3]  # the segment's direction is its end minus its start: they differ along one axis only
    seg[k, 3 + axis] += sign * np.float32(1.5)
    for i in (n // 3, n - 1):  # n - 1: the last chunk's last ray (at 16 385 its only one)
        rays[i, 0] = np.nan
        seg[i, 0] = np.nan
    return rays, seg


@pytest.fixture(scope="module")
def reference(cornell_small):
    """Per n: the rays, the segments, the oracle's records, flags and work counters.  Computed once, read by every case."""
    from oracle import pyoracle

    o = pyoracle.OracleScene(cornell_small)
    ref = {}
    for n in SIZES:
        rays, seg = _batch(n)
        o.reset_stats()
        hits = o.trace_closest(rays)
        st_h = o.stats()
        o.reset_stats()
        occ = o.trace_occluded(seg)
        st_o = o.stats()
        ref[n] = (rays, seg, hits, st_h, occ, st_o)
    return ref


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("count", [False, True], ids=["plain", "count"])
@pytest.mark.parametrize("walker", ["threaded", "sibling_pairs"])
def test_walk_batch_with_several_chunks_per_wave(cornell_gpu, reference, walker, count, n):
    import torch

    from radish_pt_amd import api, layouts as L

    rays, seg, ref_h, st_h, ref_o, st_o = reference[n]
    assert st_h["closestRays"] == n and st_o["anyRays"] == n  # the NaN-origin rays are counted
    assert (ref_h["primId"] >= 0).mean() > 0.25 and 0.05 < ref_o.mean() < 0.95  # the batches hit and miss
    flags = api.RDH_PT_PERSISTENT | (api.RDH_PT_NO_PAIRS if walker == "threaded" else api.RDH_PT_PAIRS) | (api.RDH_PT_COUNT if count else 0)
    d_rays, d_seg = torch.from_numpy(rays).cuda(), torch.from_numpy(seg).cuda()
    d_hits = torch.full((n, 4), 0x7fffffff, dtype=torch.int32, device="cuda")  # poison: an unwritten record shows
    d_occ = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    try:
        cornell_gpu.set_occupancy_share(64)
        cornell_gpu.counters_reset()
        cornell_gpu.trace_closest(d_rays, d_hits, flags)
        ct_h = cornell_gpu.counters()
        cornell_gpu.counters_reset()
        cornell_gpu.trace_occluded(d_seg, d_occ, flags)
        ct_o = cornell_gpu.counters()
    finally:
        cornell_gpu.set_occupancy_share(1)  # the context is shared
    got = d_hits.cpu().numpy().view(L.HIT_DTYPE).reshape(-1)
    assert np.array_equal(got["primId"], ref_h["primId"])
    for f in ("u", "v", "t"):
        assert_bit_equal(got[f], ref_h[f], f"hit.{f}")
    assert np.array_equal(d_occ.cpu().numpy(), ref_o)
    if count:
        assert ct_h == st_h
        assert ct_o == st_o
