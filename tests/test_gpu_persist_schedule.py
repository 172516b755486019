"""The persistent path tracer's block scheduler and the launch sequence rdh_path_trace keeps around it.

k_persist_schedule alone (rdh_debug_persist_schedule) against the integer model of tests/persist_schedule_model.py, and launch
sequences against the CPU oracle, launch by launch: image bits and the five work counters, with the sequence's state
(rdh_debug_persist_read) held to the model after every launch.  rdh_debug_persist_set_order feeds the persistent kernel orders the
renderer never makes for itself (reversed, cheapest first, shuffled).  Every comparison is exact.

Contexts are the tests' own, so the sequence state is known.  Scene: cornell_small (conftest.py), depth 4 unless a case says
otherwise."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import material_edit
import persist_schedule_model as M
from helpers import assert_bit_equal, oracle_path_trace_mt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTER_KEYS = ("closestRays", "anyRays", "nodeVisits", "triTests", "closestHits")
DEPTH = 4
RDH_ERR_ARGS = -1


def _torch():
    import torch

    return torch


@functools.lru_cache(maxsize=None)
def _sd():
    from radish_pt_amd import scenes

    return scenes.cornell(segments=16, bands=12)  # conftest's cornell_small


def _cam(w, h):
    from radish_pt_amd import scenes

    return scenes.cornell_camera(w, h)


def _oracle_frame(sd, cam, looper, depth=DEPTH):
    w, h = (int(v) for v in cam["resolution"])
    d, i = np.zeros((w * h, 3), np.float32), np.zeros((w * h, 3), np.float32)
    _, st = oracle_path_trace_mt(sd, cam, d, i, 0, looper, depth)
    d.setflags(write=False)
    i.setflags(write=False)
    return {"d": d, "i": i, "stats": {k: st[k] for k in COUNTER_KEYS}}


@functools.lru_cache(maxsize=None)
def _ref(w, h, looper, depth=DEPTH):
    """The oracle's frame of cornell_small at iter 0 and its counters: computed once per process, read-only."""
    return _oracle_frame(_sd(), _cam(w, h), looper, depth)


@functools.lru_cache(maxsize=None)
def _rank_ref(w, h, rank, world, tile, looper, depth=DEPTH):
    """The oracle over the pixels of one rank of a tile partition, in the rank's packed layout, with the counters of those pixels."""
    from oracle import pyoracle
    from radish_pt_amd import partition

    frame_idx, packed_idx = partition.rank_pixels(w, h, rank, world, tile)
    o = pyoracle.OracleScene(_sd())
    d, i = np.zeros((w * h, 3), np.float32), np.zeros((w * h, 3), np.float32)
    idx = np.sort(frame_idx)
    cuts = np.flatnonzero(np.diff(idx) != 1) + 1
    for run in np.split(idx, cuts):  # a tile's rows: runs of consecutive pixels
        o.path_trace(_cam(w, h), d, i, 0, looper, depth, pix=(int(run[0]), int(run[-1]) + 1, 1))
    st = o.stats()
    return {"frame_idx": frame_idx, "packed_idx": packed_idx, "d": d[frame_idx], "i": i[frame_idx],
            "stats": {k: st[k] for k in COUNTER_KEYS}}


def block_pixels(w, h, rank=0, world=1, tile=64):
    """Pixels of the frame in each 8x8 block of a rank's launch (the host's restatement of mapPixel's block layout: tiles dealt
    round robin, a 64-pixel tile's blocks along the Morton curve, smaller tiles' row by row)."""
    bpe = tile // 8
    tiles_x, tiles_y = (w + tile - 1) // tile, (h + tile - 1) // tile
    tpr = (tiles_x * tiles_y + world - 1) // world
    out = np.zeros(tpr * bpe * bpe, np.int64)
    for block in range(len(out)):
        local, b = divmod(block, bpe * bpe)
        if bpe == 8:
            bx = (b & 1) | ((b >> 1) & 2) | ((b >> 2) & 4)
            by = ((b >> 1) & 1) | ((b >> 2) & 2) | ((b >> 3) & 4)
        else:
            bx, by = b % bpe, b // bpe
        tid = local * world + rank
        if tid >= tiles_x * tiles_y:
            continue
        x0, y0 = (tid % tiles_x) * tile + bx * 8, (tid // tiles_x) * tile + by * 8
        out[block] = max(0, min(8, w - x0)) * max(0, min(8, h - y0))
    return out


@pytest.fixture
def make_ctx():
    """Contexts of a test's own with cornell_small uploaded, closed when it ends."""
    from radish_pt_amd import api

    made = []

    def make(sd=None):
        c = api.Context(0)
        made.append(c)
        c.upload_scene(_sd() if sd is None else sd)
        return c

    yield make
    for c in made:
        c.close()


def _launch(ctx, elems, looper, flags, depth=DEPTH, fill=0.0):
    """One counted launch into images of its own at iter 0 -> (direct, indirect, counters)."""
    from radish_pt_amd import api

    torch = _torch()
    d, i = torch.full((elems, 3), fill, device="cuda"), torch.full((elems, 3), fill, device="cuda")
    ctx.counters_reset()
    ctx.path_trace(d, i, 0, looper, depth, flags | api.RDH_PT_COUNT)
    ct = ctx.counters()
    return d.cpu().numpy(), i.cpu().numpy(), ct


def _same(got, ref, what):
    d, i, ct = got
    assert_bit_equal(d, ref["d"], f"{what}: direct vs oracle")
    assert_bit_equal(i, ref["i"], f"{what}: indirect vs oracle")
    for k in COUNTER_KEYS:
        assert ct[k] == ref["stats"][k], (what, k, ct[k], ref["stats"][k])


def _same_rank(got, ref, what):
    d, i, ct = got
    assert_bit_equal(d[ref["packed_idx"]], ref["d"], f"{what}: direct vs oracle")
    assert_bit_equal(i[ref["packed_idx"]], ref["i"], f"{what}: indirect vs oracle")
    for k in COUNTER_KEYS:
        assert ct[k] == ref["stats"][k], (what, k, ct[k], ref["stats"][k])


def _check_state(ctx, frame, blocks, pixels=None, what=""):
    """What rdh_debug_persist_read must show after launch number `frame` (1-based) of a sequence."""
    st = ctx.debug_persist_read()
    assert (st["frame"], st["valid"], st["blocks"], st["pending"]) == (frame, True, blocks, 0), (what, st["frame"], st["valid"], st["blocks"])
    assert not st["costs"].any(), f"{what}: a cost buffer is not zero after launch {frame}"
    new = (frame - 1) & 1  # launch n (0-based) has its schedule write order buffer n & 1
    M.check_order(st["orders"][new], st["ema"], blocks, f"{what}: newest order after launch {frame}")
    if frame >= 2:  # sorted by means that have moved since: a permutation is all that is left to assert
        M.check_order(st["orders"][1 - new], np.zeros(blocks, np.uint32), blocks, f"{what}: older order after launch {frame}")
    assert st["ema"].max() > 0, f"{what}: no block has a positive mean"
    if pixels is not None:
        empty = pixels == 0
        assert not st["ema"][empty].any(), f"{what}: a block without a pixel has a cost"
        zero_means = int((st["ema"] == 0).sum())
        where = np.empty(blocks, np.int64)
        where[st["orders"][new]] = np.arange(blocks)
        assert np.all(where[empty] >= blocks - zero_means), f"{what}: a block without a pixel is not at the end of the order"
    return st


# ---------------------------------------------------------------------------------------------------------------------------------
# a. the kernel alone against the model
# ---------------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 32400, 129600)
TAIL = 64
POISON = {"cost": 0xDEADBEEF, "ema": 0xA5A5A5A5, "order": 0x80000007}
# one cost per bucket number in use, most expensive first: 49152 (bucket 0), the first cost of each quarter octave, 2, 1 and 0
REPRESENTATIVES = np.array([49152] + [(1 << k) * m // 4 for k in range(15, 1, -1) for m in (7, 6, 5, 4) if (1 << k) * m // 4 < 49152]
                           + [2, 1, 0], np.uint32)


def _patterns(n):
    """name -> (cost, ema), uint32 [n] each.  A wave of the kernel holds 64 consecutive blocks."""
    i = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(1000 + n)
    zero = np.zeros(n, np.uint32)
    reps = REPRESENTATIVES
    edges = np.array(sorted({int(c) for t in reps if t > 0 for c in (int(t) - 1, int(t), int(t) + 1)}), np.uint32)
    smooth = 400.0 + 300.0 * np.sin(i / 37.0) * np.cos(i / 411.0)
    out = {
        "all zero": (zero, zero),
        "all equal": (np.full(n, 1000, np.uint32), np.full(n, 900, np.uint32)),
        # every wave holds all 58 bucket numbers there are, each wave in another rotation: the longest per-wave atomic loop
        "58 buckets per wave": (reps[(i + i // 64) % len(reps)], zero),
        "one bucket per wave": (reps[(i // 64) % len(reps)], zero),
        "bucket boundaries": (edges[i % len(edges)], zero),
        "boundaries as means": (edges[(i * 7) % len(edges)], np.maximum(edges[(i * 7) % len(edges)], 1).astype(np.uint32)),
        "sign bit": (np.array([0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 3], np.uint32)[i % 4], zero),
        "smooth field": ((smooth * rng.uniform(0.9, 1.1, n)).astype(np.uint32), (smooth * rng.uniform(0.8, 1.2, n)).astype(np.uint32)),
        "full range": (rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)),
    }
    return out


class _Arrays:
    """cost / ema / order on the device, n + 64 words each, poisoned beyond n."""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, n
        self.t = {}
        for name in ("cost", "ema", "order"):
            host = np.full(n + TAIL, POISON[name], np.uint32)
            self.t[name] = _torch().from_numpy(host.view(np.int32)).cuda()

    def put(self, name, values):
        self.t[name][:self.n] = _torch().from_numpy(np.ascontiguousarray(values, np.uint32).view(np.int32)).cuda()

    def run(self):
        self.ctx.debug_persist_schedule(self.t["cost"], self.t["ema"], self.t["order"], self.n)

    def get(self, name):
        """The first n words; asserts that the 64 beyond them still hold the poison."""
        host = self.t[name].cpu().numpy().view(np.uint32)
        assert np.all(host[self.n:] == POISON[name]), f"n = {self.n}: the kernel wrote beyond {name}[n - 1]"
        return host[:self.n].view(np.int32) if name == "order" else host[:self.n]


@pytest.fixture(scope="module")
def bare_ctx(gpu_ctx):
    """No scene, no camera: rdh_debug_persist_schedule needs neither."""
    from radish_pt_amd import api

    ctx = api.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("n", SIZES)
def test_schedule_kernel_against_the_model(bare_ctx, n):
    """1 / 2 / 63..65 blocks: below, at and over a wave; 1 023..1 025: the workgroup; 4 095..4 097: one round of four blocks per
    thread and the start of the second; 8 193: the third; 32 400 and 129 600: the block counts of 1080p and 4K frames."""
    for name, (cost, ema) in _patterns(n).items():
        a = _Arrays(bare_ctx, n)
        a.put("cost", cost)
        a.put("ema", ema)
        a.run()
        M.check(cost, ema, a.get("cost"), a.get("ema"), a.get("order"), n, f"n = {n}, {name}")


@pytest.mark.parametrize("n", (65, 4097, 32400))
def test_three_schedules_in_a_row_follow_the_recurrence(bare_ctx, n):
    rng = np.random.default_rng(n)
    a = _Arrays(bare_ctx, n)
    ema = np.zeros(n, np.uint32)
    a.put("ema", ema)
    base = 50.0 + 2000.0 * rng.random(n) ** 4
    for k in range(3):
        cost = (base * rng.uniform(0.5, 1.5, n)).astype(np.uint32)
        cost[rng.random(n) < 0.1] = 0  # a block whose paths all missed the scene this launch
        a.put("cost", cost)  # into the buffer the last call zeroed, as the launch after next does
        a.run()
        after = a.get("ema")
        M.check(cost, ema, a.get("cost"), after, a.get("order"), n, f"n = {n}, call {k}")
        ema = after.copy()
    assert ema.max() > 0


@pytest.mark.parametrize("n", (64, 8193))
def test_equal_inputs_give_equal_means_and_bucket_sets(bare_ctx, n):
    """The order inside a bucket may differ from run to run; nothing else may."""
    cost, ema = _patterns(n)["smooth field"]
    runs = []
    for _ in range(2):
        a = _Arrays(bare_ctx, n)
        a.put("cost", cost)
        a.put("ema", ema)
        a.run()
        runs.append((a.get("ema").copy(), a.get("order").copy()))
    assert np.array_equal(runs[0][0], runs[1][0])
    for b, first, end in M.spans(M.buckets_of(runs[0][0])):
        assert np.array_equal(np.sort(runs[0][1][first:end]), np.sort(runs[1][1][first:end])), f"bucket {b}"


def test_schedule_entry_refuses_bad_arguments(bare_ctx):
    from radish_pt_amd import api

    sched = api.persist_entries()[0]
    t = _torch().zeros(8, dtype=_torch().int32, device="cuda")
    p = t.data_ptr()
    assert sched(bare_ctx.h, p, p, p, 0) == RDH_ERR_ARGS
    assert sched(bare_ctx.h, p, p, p, -3) == RDH_ERR_ARGS
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert sched(bare_ctx.h, *args, 8) == RDH_ERR_ARGS
    bare_ctx.synchronize()
    assert not t.any().item()


# ---------------------------------------------------------------------------------------------------------------------------------
# b. launch sequences equal the oracle, launch by launch
# ---------------------------------------------------------------------------------------------------------------------------------
# (width, height, tile, blocks)
FRAMES = ((8, 8, 8, 1), (24, 8, 8, 3), (40, 8, 8, 5), (37, 29, 8, 20), (64, 48, 64, 64))
LOOPERS = tuple(range(30, 36))


def _sequence(ctx, w, h, tile, blocks, flags_of, what):
    """Six launches, each into its own images; flags_of(k) gives launch k's flags."""
    pixels = block_pixels(w, h, 0, 1, tile)
    assert len(pixels) == blocks
    ctx.set_partition(0, 1, tile)
    ctx.set_camera(_cam(w, h))
    states = []
    for k, looper in enumerate(LOOPERS):
        _same(_launch(ctx, w * h, looper, flags_of(k)), _ref(w, h, looper), f"{what} launch {k}")
        states.append(_check_state(ctx, k + 1, blocks, pixels, what))
    return states


@pytest.mark.parametrize("walk", ["pairs", "no_pairs"])
@pytest.mark.parametrize("frame", FRAMES, ids=[f"{w}x{h}-tile{t}" for w, h, t, _ in FRAMES])
def test_six_launches_equal_the_oracle(make_ctx, frame, walk):
    from radish_pt_amd import api

    w, h, tile, blocks = frame
    flags = api.RDH_PT_PERSISTENT | (api.RDH_PT_NO_PAIRS if walk == "no_pairs" else 0)
    states = _sequence(make_ctx(), w, h, tile, blocks, lambda k: flags, f"{w}x{h} {walk}")
    if (w, h) == (64, 48):
        assert int((block_pixels(w, h) == 0).sum()) == 16
        assert states[0]["ema"].max() > states[0]["ema"][states[0]["ema"] > 0].min()  # the frame's blocks differ in cost


# ---------------------------------------------------------------------------------------------------------------------------------
# c. RDH_PT_NO_SCHEDULE
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("when", ["every launch", "launches 2 and 4"])
def test_no_schedule_changes_no_frame_and_no_state(make_ctx, when):
    """The flag keeps a launch from READING an order; the costs, the means, the schedule kernel and the launch count go on, so a
    later launch without it has a current order to read.  Frames and counters are the oracle's either way."""
    from radish_pt_amd import api

    on = (lambda k: True) if when == "every launch" else (lambda k: k in (2, 4))
    _sequence(make_ctx(), 64, 48, 64, 64, lambda k: api.RDH_PT_PERSISTENT | (api.RDH_PT_NO_SCHEDULE if on(k) else 0), f"no schedule on {when}")


# ---------------------------------------------------------------------------------------------------------------------------------
# d. any permutation gives the frame
# ---------------------------------------------------------------------------------------------------------------------------------
# (width, height, rank, world, tile, blocks): the last is a rank whose tenth tile lies beyond the frame's 28
ORDER_FRAMES = ((37, 29, 0, 1, 8, 20), (64, 48, 0, 1, 64, 64), (100, 60, 1, 3, 16, 40))
ORDER_LOOPER = 37


def _order_ref(frame):
    """(reference, comparison): one rank's packed share of the frame on a partition, the frame itself without one."""
    w, h, rank, world, tile, _ = frame
    if world == 1:
        return _ref(w, h, ORDER_LOOPER), _same
    return _rank_ref(w, h, rank, world, tile, ORDER_LOOPER), _same_rank


def _orders(blocks, means):
    """identity, reversed, cheapest first (the opposite of what the scheduler makes; ties by block number) and three shuffles."""
    ident = np.arange(blocks, dtype=np.int32)
    out = [("identity", ident), ("reversed", ident[::-1].copy()),
           ("cheapest first", np.argsort(means.astype(np.int64), kind="stable").astype(np.int32))]
    for seed in (1, 2, 3):
        out.append((f"shuffle {seed}", np.random.default_rng(seed).permutation(blocks).astype(np.int32)))
    return out


@pytest.mark.parametrize("no_schedule", [False, True], ids=["scheduled", "no_schedule"])
@pytest.mark.parametrize("inject_at", [0, 3])
@pytest.mark.parametrize("frame", ORDER_FRAMES, ids=[f"{w}x{h}-rank{r}of{n}-tile{t}" for w, h, r, n, t, _ in ORDER_FRAMES])
def test_any_injected_permutation_gives_the_frame(make_ctx, frame, inject_at, no_schedule):
    """Every order on one context; a new upload of the scene restarts the sequence between them.  A restart zeroes the means, so
    the last round's 'cheapest first' is taken from the means read before it: the same frame's, from the round before."""
    from radish_pt_amd import api

    w, h, rank, world, tile, blocks = frame
    flags = api.RDH_PT_PERSISTENT | (api.RDH_PT_NO_SCHEDULE if no_schedule else 0)
    ctx = make_ctx()
    ctx.set_partition(rank, world, tile)
    ctx.set_camera(_cam(w, h))
    elems = ctx.tiles_per_rank() * tile * tile if world > 1 else w * h
    ref, same = _order_ref(frame)

    def launch(what):
        same(_launch(ctx, elems, ORDER_LOOPER, flags), ref, what)

    means = np.zeros(blocks, np.uint32)
    for name, order in _orders(blocks, means) + [("cheapest first, by the means so far", None)]:
        if order is None:
            means = ctx.debug_persist_read()["ema"]
            assert means.max() > 0
            order = _orders(blocks, means)[2][1]
            assert means[order[0]] == means.min() and means[order[-1]] == means.max()
        ctx.upload_scene(_sd())
        assert not ctx.debug_persist_read()["valid"]
        for k in range(inject_at):
            launch(f"{name}: launch {k} before the injection")
        ctx.debug_persist_set_order(order)
        assert ctx.debug_persist_read()["pending"] == blocks
        launch(f"{name}: the injected launch {inject_at}")
        st = _check_state(ctx, inject_at + 1, blocks, None, name)  # costs, means, schedule and count went on
        launch(f"{name}: launch {inject_at + 1}, the library's own order again")
        _check_state(ctx, inject_at + 2, blocks, None, name)
        assert st["pending"] == 0


@pytest.mark.parametrize("frame", ORDER_FRAMES[1:], ids=["64x48", "100x60-rank1of3"])
def test_refused_orders_leave_the_next_launch_alone(make_ctx, frame):
    from radish_pt_amd import api

    w, h, rank, world, tile, blocks = frame
    set_order = api.persist_entries()[2]
    ctx = make_ctx()
    ctx.set_partition(rank, world, tile)
    ctx.set_camera(_cam(w, h))
    elems = ctx.tiles_per_rank() * tile * tile if world > 1 else w * h
    ref, same = _order_ref(frame)
    ident = np.arange(blocks, dtype=np.int32)
    dup, neg, big = ident.copy(), ident.copy(), ident.copy()
    dup[5] = dup[6]
    neg[0] = -1
    big[blocks - 1] = blocks
    bad = (("one entry short", ident[:-1]), ("one entry long", np.arange(blocks + 1, dtype=np.int32)), ("a duplicate", dup),
           ("a negative entry", neg), ("an entry equal to n", big))
    for k in range(4):  # before launches 0..3: plain-order launches and ordered ones
        for name, order in bad:
            assert set_order(ctx.h, order.ctypes.data, len(order)) == RDH_ERR_ARGS, name
            assert ctx.debug_persist_read()["pending"] == 0, name
        assert set_order(ctx.h, None, blocks) == RDH_ERR_ARGS
        same(_launch(ctx, elems, ORDER_LOOPER, api.RDH_PT_PERSISTENT), ref, f"launch {k} after refused orders")
        _check_state(ctx, k + 1, blocks, None, "refused orders")


def test_whatever_restarts_the_sequence_drops_a_pending_order(make_ctx):
    ctx = make_ctx()
    ctx.set_camera(_cam(64, 48))
    ident = np.arange(64, dtype=np.int32)
    events = (lambda: ctx.upload_scene(_sd()), lambda: ctx.set_camera(_cam(48, 64)), lambda: ctx.set_partition(0, 1, 32),
              lambda: ctx.set_occupancy_share(2))
    for event in events:
        ctx.debug_persist_set_order(ident)
        assert ctx.debug_persist_read()["pending"] == 64
        event()
        assert ctx.debug_persist_read()["pending"] == 0
    ctx.set_occupancy_share(1)
    ctx.set_partition(0, 1, 64)
    ctx.set_camera(_cam(64, 48))
    ctx.debug_persist_set_order(ident)
    ctx.set_camera(_cam(64, 48))  # the same resolution: no restart, the order stays
    assert ctx.debug_persist_read()["pending"] == 64


# ---------------------------------------------------------------------------------------------------------------------------------
# e. an ordered launch with fewer workgroups than blocks
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ordered_launches_with_fewer_workgroups_than_blocks(make_ctx):
    """128x96 at share 64 (the frame test_occupancy_share_changes_no_result derives): 48 workgroups against 256 blocks, so most
    blocks are taken through the shared head, in the scheduled order from launch 2 on."""
    from radish_pt_amd import api

    w, h = 128, 96
    ctx = make_ctx()
    ctx.set_camera(_cam(w, h))
    pixels = block_pixels(w, h)
    assert len(pixels) == 256 and int((pixels > 0).sum()) == 192
    ctx.set_occupancy_share(64)
    try:
        for k, looper in enumerate((42, 43, 42, 43)):
            got = _launch(ctx, w * h, looper, api.RDH_PT_PERSISTENT)
            _same(got, _ref(w, h, looper), f"share 64, launch {k}")
            _check_state(ctx, k + 1, 256, pixels, "share 64")
        ctx.debug_persist_set_order(np.arange(256, dtype=np.int32)[::-1].copy())
        _same(_launch(ctx, w * h, 43, api.RDH_PT_PERSISTENT), _ref(w, h, 43), "share 64, launch 3 again under a reversed order")
        _check_state(ctx, 5, 256, pixels, "share 64")
    finally:
        ctx.set_occupancy_share(1)


# ---------------------------------------------------------------------------------------------------------------------------------
# f. more than 4 096 blocks at a small pixel count
# ---------------------------------------------------------------------------------------------------------------------------------
def test_second_scheduler_round_in_a_render(make_ctx):
    """9x4097 at tile 64: one column of 65 tiles, 4 160 blocks (the schedule kernel's second round of four blocks per thread) for
    36 873 pixels; 3 134 of the blocks hold no pixel.  Depth 1.  All three launches are compared with the oracle (its three frames
    take well under a second)."""
    from radish_pt_amd import api

    w, h, depth = 9, 4097, 1
    ctx = make_ctx()
    ctx.set_camera(_cam(w, h))
    pixels = block_pixels(w, h)
    assert len(pixels) == 4160 and int((pixels == 0).sum()) == 3134
    for k, looper in enumerate((50, 51, 52)):
        ref = _ref(w, h, looper, depth)
        _same(_launch(ctx, w * h, looper, api.RDH_PT_PERSISTENT, depth), ref, f"9x4097 launch {k}")
        _check_state(ctx, k + 1, 4160, pixels, "9x4097")
    lit = (ref["d"] > 0).any(axis=1) & (ref["d"] != 1.0).any(axis=1)  # (a primary ray that leaves the scene writes direct = 1)
    assert ref["stats"]["closestHits"] > 1000 and lit.sum() > 100 and ref["i"].max() > 0, "the oracle's frame shows nothing"


# ---------------------------------------------------------------------------------------------------------------------------------
# g. ordered launches on a tile partition
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ordered_launches_on_every_rank_of_a_partition(make_ctx):
    from radish_pt_amd import api, partition

    w, h, world, tile, looper = 100, 60, 3, 16, 44
    ctx = make_ctx()
    ctx.set_camera(_cam(w, h))
    whole = _ref(w, h, looper)
    shards, total = [], {k: 0 for k in COUNTER_KEYS}
    for rank in range(world):
        ctx.set_partition(rank, world, tile)
        elems = ctx.tiles_per_rank() * tile * tile
        assert elems == partition.shard_elems(w, h, world, tile)
        pixels = block_pixels(w, h, rank, world, tile)
        assert len(pixels) == 40
        for k in range(3):
            got = _launch(ctx, elems, looper, api.RDH_PT_PERSISTENT, fill=-3.0)
            _check_state(ctx, k + 1, 40, pixels, f"rank {rank}")  # a change of rank restarted the sequence: 1, 2, 3
        shards.append(got)
        for key in COUNTER_KEYS:
            total[key] += got[2][key]
    assert int((block_pixels(w, h, 1, world, tile) == 0).sum()) > 4  # rank 1's tenth tile is a phantom: tile 28 of 28
    src = partition.untile_indices(w, h, world, tile)
    for plane, name in ((0, "d"), (1, "i")):
        gathered = np.concatenate([s[plane] for s in shards])
        assert_bit_equal(gathered[src], whole[name], f"the three ranks' third launches, un-tiled: {name}")
    assert total == whole["stats"]


# ---------------------------------------------------------------------------------------------------------------------------------
# h. what restarts the sequence and what does not
# ---------------------------------------------------------------------------------------------------------------------------------
def _dev(a, dtype=np.float32):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=dtype).reshape(-1)).cuda()


def _three_launches(ctx):
    from radish_pt_amd import api

    ctx.set_camera(_cam(64, 48))
    for k in range(3):
        _same(_launch(ctx, 64 * 48, 60 + k, api.RDH_PT_PERSISTENT), _ref(64, 48, 60 + k), f"launch {k}")
    assert ctx.debug_persist_read()["frame"] == 3


RESTARTS = ("camera 48x64", "camera 72x48", "partition", "occupancy share", "stream", "upload_scene", "refit_geometry", "update_geometry",
            "set_geometry")


@pytest.mark.parametrize("event", RESTARTS)
def test_events_that_restart_the_sequence(make_ctx, event):
    """After the event the next launch is launch 0 again (plain order, cost buffers and means zeroed) and equals the oracle.  The
    geometry entries are given the uploaded scene's own arrays: the tree they leave is the uploaded one (a refit's boxes are the
    same minima and maxima), so the oracle's frame and counters of the scene stand."""
    from radish_pt_amd import api

    torch = _torch()
    sd = _sd()
    ctx = make_ctx()
    _three_launches(ctx)
    w, h, blocks, elems, stream = 64, 48, 64, 64 * 48, None
    if event == "camera 48x64":
        w, h = 48, 64
        ctx.set_camera(_cam(w, h))
        elems = w * h
    elif event == "camera 72x48":
        w, h, blocks = 72, 48, 128
        ctx.set_camera(_cam(w, h))
        elems = w * h
    elif event == "partition":
        ctx.set_partition(0, 1, 32)  # four tiles of 16 blocks: the same count in another layout
    elif event == "occupancy share":
        ctx.set_occupancy_share(2)
    elif event == "stream":
        stream = torch.cuda.Stream()
        ctx.check(api.lib().rdh_set_stream(ctx.h, C.c_void_p(stream.cuda_stream)))
    elif event == "upload_scene":
        ctx.upload_scene(sd)
    elif event == "refit_geometry":
        ctx.keep = _dev(sd.vertices)
        ctx.refit_geometry(ctx.keep)
    elif event == "update_geometry":
        ctx.keep = _dev(sd.vertices)
        ctx.update_geometry(ctx.keep)
    elif event == "set_geometry":
        ctx.keep = (_dev(sd.vertices), _dev(sd.normals), _dev(sd.texcoords), _dev(sd.material_ids, np.int32))
        ctx.set_geometry(*ctx.keep)
    assert not ctx.debug_persist_read()["valid"], event
    ref = _ref(w, h, 63)
    if stream is None:
        got = _launch(ctx, elems, 63, api.RDH_PT_PERSISTENT)
    else:
        with torch.cuda.stream(stream):  # the images are made, written and read on the context's new stream
            got = _launch(ctx, elems, 63, api.RDH_PT_PERSISTENT)
    _same(got, ref, f"the launch after {event}")
    # ... with nothing left of the old layout's means: blocks that hold no pixel NOW have mean 0 (48x64 after 64x48: other blocks)
    _check_state(ctx, 1, blocks, block_pixels(w, h, 0, 1, 32 if event == "partition" else 64), event)


CONTINUES = ("camera eye", "set_materials", "track_motion")


@pytest.mark.parametrize("event", CONTINUES)
def test_events_that_leave_the_sequence_running(make_ctx, event):
    """The block layout and the tree are what they were: the order in flight still fits, and launch 3 reads it."""
    from radish_pt_amd import api, hostlib, layouts as L

    sd = _sd()
    ctx = make_ctx()
    _three_launches(ctx)
    cam = _cam(64, 48)
    if event == "camera eye":
        cam = hostlib.make_camera(64, 48, eye=(0.3, 1.1, 4.0), rotation=(-90.0, 0.0, 0.0), fovy=20.0)
        ctx.set_camera(cam)
    elif event == "set_materials":
        lambert = int(np.flatnonzero(sd.materials["type"] == L.LAMBERTIAN)[0])
        mats = sd.materials[[lambert]].copy()
        mats["baseColor"] = (0.2, 0.3, 0.9)
        ids = np.array([lambert], np.int32)
        ctx.set_materials(ids, mats)
        sd = material_edit.edited(sd, ids, mats)
    elif event == "track_motion":
        ctx.track_motion(True)
    st = ctx.debug_persist_read()
    assert (st["frame"], st["valid"]) == (3, True), event
    ref = _oracle_frame(sd, cam, 63)
    if event != "track_motion":
        assert not np.array_equal(ref["d"], _ref(64, 48, 63)["d"]) or not np.array_equal(ref["i"], _ref(64, 48, 63)["i"]), f"{event} changed nothing"
    _same(_launch(ctx, 64 * 48, 63, api.RDH_PT_PERSISTENT), ref, f"the launch after {event}")
    _check_state(ctx, 4, 64, block_pixels(64, 48), event)


def test_set_texture_leaves_the_sequence_running(make_ctx):
    """cornell_small has no texture to replace: this case runs on cornell_textured, texture 0 replaced (tests/texture_edit.py)."""
    import texture_edit
    from radish_pt_amd import api

    sd = texture_edit.cornell()
    tex_id, texels = sorted(texture_edit.plain_edits().items())[0]
    edited = texture_edit.with_textures(sd, {tex_id: texels})
    ctx = make_ctx(sd)
    cam = _cam(64, 48)
    ctx.set_camera(cam)
    for k in range(3):
        _launch(ctx, 64 * 48, 60 + k, api.RDH_PT_PERSISTENT)
    ctx.keep = _torch().from_numpy(np.ascontiguousarray(texels, np.float32)).cuda()
    ctx.set_texture(tex_id, ctx.keep)
    st = ctx.debug_persist_read()
    assert (st["frame"], st["valid"]) == (3, True)
    ref, before = _oracle_frame(edited, cam, 63), _oracle_frame(sd, cam, 63)
    assert not (np.array_equal(ref["d"], before["d"]) and np.array_equal(ref["i"], before["i"])), "the texture edit changed nothing"
    _same(_launch(ctx, 64 * 48, 63, api.RDH_PT_PERSISTENT), ref, "the launch after set_texture")
    _check_state(ctx, 4, 64, block_pixels(64, 48), "set_texture")


# ---------------------------------------------------------------------------------------------------------------------------------
# i. the side stream shared with the wavefront pipelines
# ---------------------------------------------------------------------------------------------------------------------------------
CHILD_TIMEOUT = 300  # seconds; the child takes a few
# The pipeline count (RADISH_WF_PARTS) is read once per process, hence a child process: two pipelines, the second on the side stream
# the schedule kernel runs on.  Sub-frames engage from 2 048 blocks: 9x2049 at tile 64 is a column of 33 tiles, 2 112 blocks for
# 18 441 pixels.  Seven launches without a host synchronisation between them, then everything is compared with the oracle.
CHILD = r"""
import numpy as np
import torch
from helpers import assert_bit_equal, oracle_path_trace_mt
from radish_pt_amd import api, scenes

W, H, depth = 9, 2049, 4
sd = scenes.cornell(segments=16, bands=12)
cam = scenes.cornell_camera(W, H)
P = api.RDH_PT_PERSISTENT
WF = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_WF_SUBFRAMES
ctx = api.Context(0)
ctx.upload_scene(sd)
ctx.set_camera(cam)
images = []
for k, flags in enumerate((P, P, WF, P, WF, P, P)):
    d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
    ctx.path_trace(d, i, 0, 70 + k, depth, flags)
    images.append((d, i))
ctx.synchronize()
st = ctx.debug_persist_read()
assert (st["frame"], st["valid"], st["blocks"]) == (5, True, 2112), (st["frame"], st["blocks"])
assert not st["costs"].any() and st["ema"].max() > 0
for k, (d, i) in enumerate(images):
    rd, ri = np.zeros((W * H, 3), np.float32), np.zeros((W * H, 3), np.float32)
    oracle_path_trace_mt(sd, cam, rd, ri, 0, 70 + k, depth)
    assert ri.max() > 0
    assert_bit_equal(d.cpu().numpy(), rd, f"launch {k}: direct vs oracle")
    assert_bit_equal(i.cpu().numpy(), ri, f"launch {k}: indirect vs oracle")
    print(f"launch {k} equals the oracle", flush=True)
ctx.close()
"""


def test_schedule_beside_wavefront_subframe_pipelines():
    env = dict(os.environ, RADISH_WF_PARTS="2")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    print(r.stdout)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert r.stdout.count("equals the oracle") == 7
