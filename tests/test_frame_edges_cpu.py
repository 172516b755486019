"""The inputs of tests/frame_edges.py earn their place: conditions, checked with the CPU oracle alone, that keep
tests/test_gpu_frame_edges.py from passing on frames that exercise nothing.  Figures in the messages are what the committed inputs
give (DESIGN.md §2b quotes the per-bounce ray counts)."""
import copy

import numpy as np
import pytest

import frame_edges as FE

SHAPES = list(FE.SHAPES)
IDS = [FE.SHAPE_IDS[s] for s in SHAPES]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _changed_pixels(a, b):
    return int((_bits(a) != _bits(b)).any(axis=1).sum())


def test_shapes_edge_what_they_claim():
    assert len(FE.SHAPES) == 12 and FE.BASE in FE.SHAPES
    slots = {s: ((s[0] + 7) // 8) * ((s[1] + 7) // 8) * 64 for s in FE.SHAPES}  # 8x8 blocks, one wave each
    assert slots[(16, 8)] == 128 and slots[(16, 16)] == 256 and slots[(32, 32)] == 1024 and slots[(40, 32)] == 1024 + 256
    assert slots[(1, 1)] == slots[(8, 8)] == 64 and slots[(7, 9)] == slots[(9, 8)] == 128
    assert slots[(1, 65)] == slots[(65, 1)] == 9 * 64  # 65 pixels in 576 slots
    assert all(w * h <= 4095 for w, h in FE.SHAPES)
    for shape in FE.SHAPES:
        assert tuple(int(v) for v in FE.closed_camera(shape)["resolution"]) == shape
        assert tuple(int(v) for v in FE.teapots_cameras(shape)[0]["resolution"]) == shape


def test_closed_scene_is_the_measured_one():
    from radish_pt_amd import layouts as L

    for glass in (True, False):
        sd = FE.closed_scene(glass)
        assert sd.num_prims == 1166 and sd.num_lights == 2
        glass_tris = int((sd.materials["type"][sd.material_ids] == L.DIELECTRIC).sum())
        assert glass_tris == (16 * 12 * 2 if glass else 0)


def test_closed_scene_keeps_its_paths_to_bounce_28():
    """16x12, looper 5: 192 primary rays, then 192, 191, ..., 177 extension rays at bounces 1..28."""
    w, h = FE.BASE
    n = w * h
    rays = FE.bounce_rays(FE.BASE)
    assert len(rays) == FE.MAX_DEPTH + 1 and rays[0] == n
    assert rays[FE.MAX_DEPTH] >= n // 2, rays  # measured 177 of 192
    drops = [a - b for a, b in zip(rays, rays[1:])]
    assert all(0 <= d <= 0.05 * n for d in drops), rays
    assert rays == (192, 192, 191, 191, 191, 191, 190, 189, 188, 188, 188, 187, 187, 185, 184, 184, 183, 183, 183, 183, 183, 183, 182,
                    181, 180, 179, 178, 178, 177), rays  # the record DESIGN.md quotes


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_shape_reaches_bounce_28_and_shows_it(shape):
    r27, r28 = FE.closed_ref(shape, 27), FE.closed_ref(shape, 28)
    rays28 = r28["stats"]["closestRays"] - r27["stats"]["closestRays"]
    assert rays28 >= 1, (shape, rays28)
    assert _changed_pixels(r27["i"], r28["i"]) >= 1, shape  # measured: 1 of 1 at 1x1, 29 of 63 at 7x9
    assert r28["d"].max() > 0 and r28["i"].max() > 0 and r28["stats"]["anyRays"] > 0
    if shape == (1, 1):
        assert r28["stats"]["closestRays"] == 29  # the pixel's only path: the primary ray and 28 extension rays


@pytest.mark.parametrize("shape", [FE.BASE, (1, 1)], ids=["16x12", "1x1"])
def test_glass_free_variant_reads_the_last_table_word(shape):
    """looper 9999, no dielectric: a path alive at bounce 28 drew 4 + 7 * 28 values, the last of them table[9999][199].  Shown two
    ways: a ray is traced at bounce 28, and changing that one word changes the depth-28 frame and leaves the depth-27 frame alone
    (depth 27 ends at dimension 192)."""
    r27 = FE.closed_ref(shape, 27, FE.LAST_ROW, 1, False)
    r28 = FE.closed_ref(shape, 28, FE.LAST_ROW, 1, False)
    assert r28["stats"]["closestRays"] - r27["stats"]["closestRays"] >= 1  # measured 179 of 192, 1 of 1
    assert _changed_pixels(r27["i"], r28["i"]) >= 1
    sd = copy.copy(FE.closed_scene(False))
    sd.sobol = sd.sobol.copy()
    assert sd.sobol.shape == (10000, 200)
    sd.sobol[FE.LAST_ROW, 199] ^= np.uint32(0x55555555)
    cam = FE.closed_camera(shape, glass=False)
    p27 = FE.oracle_frames(sd, cam, 27, FE.LAST_ROW)
    p28 = FE.oracle_frames(sd, cam, 28, FE.LAST_ROW)
    assert p27["stats"] == r27["stats"] and _changed_pixels(p27["i"], r27["i"]) == 0 and _changed_pixels(p27["d"], r27["d"]) == 0
    # some path takes its 28th bounce on the half-metallic wall, whose lobe choice is that word: the bounce-28 ray is another
    assert p28["stats"] != r28["stats"], "no path's bounce-28 ray depends on the last word of the table"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_teapots_frames_see_geometry_and_reuse_matters(shape):
    n = shape[0] * shape[1]
    for frame in FE.gbuffer_ref(shape):
        assert (frame["planes"]["primId"] >= 0).sum() * 2 >= n, shape
        assert frame["stats"]["closestRays"] == n and frame["stats"]["anyRays"] == 0
    for faithful in (1, 0):
        plain, reused = FE.restir_ref(shape, 0, faithful), FE.restir_ref(shape, 3, faithful)
        assert len(plain) == len(reused) == 3
        assert all((f["img"] > 0).any() for f in plain) and all((f["img"] > 0).any() for f in reused), shape
        assert sum(_changed_pixels(a["img"], b["img"]) for a, b in zip(plain, reused)) >= 1, shape
        assert any(a["reservoirs"] != b["reservoirs"] for a, b in zip(plain, reused))
        assert all((f["primId"] >= 0).sum() * 2 >= n for f in reused)


def test_partitions_cover_each_frame_once_and_leave_ranks_empty():
    """(7, 9) tile 8 world 3 -> 56 / 7 / 0 pixels, (1, 1) world 2 -> 1 / 0, (63, 65) tile 64 world 3 -> 4032 / 63 / 0: world exceeds
    the tile count and the last rank's tile lies wholly past numTiles.  (65, 1) tile 8 world 4 -> 17 / 16 / 16 / 16 has no empty rank
    (9 tiles): there ranks 1..3 hold a third tile whose index is past numTiles beside two real ones; world 10 on the same frame adds
    the empty rank."""
    from radish_pt_amd import partition

    assert set(FE.PARTITIONS) >= {((7, 9), 8, 3), ((1, 1), 8, 2), ((63, 65), 64, 3), ((65, 1), 8, 4)}
    with_empty = 0
    for (w, h), tile, world in FE.PARTITIONS:
        num_tiles = ((w + tile - 1) // tile) * ((h + tile - 1) // tile)
        tpr = partition.tiles_per_rank(w, h, world, tile)
        assert tpr >= 1 and tpr * world > num_tiles  # some rank's share reaches past the frame's tiles
        seen = np.zeros(w * h, np.int32)
        counts = []
        for rank in range(world):
            frame_idx, packed_idx = partition.rank_pixels(w, h, rank, world, tile)
            seen[frame_idx] += 1
            counts.append(len(frame_idx))
            assert len(set(packed_idx.tolist())) == len(packed_idx) and (len(packed_idx) == 0 or packed_idx.max() < tpr * tile * tile)
        assert (seen == 1).all(), ((w, h), tile, world)
        assert (0 in counts) == (world > num_tiles), counts
        with_empty += 0 in counts
        if ((w, h), tile, world) == ((7, 9), 8, 3):
            assert counts == [56, 7, 0]
        if ((w, h), tile, world) == ((1, 1), 8, 2):
            assert counts == [1, 0]
    assert with_empty == len(FE.PARTITIONS) - 1
