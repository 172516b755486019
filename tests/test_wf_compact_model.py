"""A numpy model of the wavefront slot renumbering (kernels_wave.h, WaveWorkspace / k_wf_shade).

shade(k) walks stage k's ray queue in packets; a record that goes on (an extension ray, a shadow ray or both) gets the slot
q = its position in the stage's processing order — the queue index, or with the material sort the packet's base plus its place in
class order — in set (k + 1) & 1, and home (its bounce-0 slot) is copied along.  The model keeps, beside what the kernels keep,
the truth: which path every queue entry belongs to.  Checked per stage: the new slots are unique and below the stage's record count,
the set being read is not written, and home read from any live slot is the path's bounce-0 slot.
"""
import numpy as np
import pytest

FREE = -1


def _packets(n, packet):
    return [(b, min(packet, n - b)) for b in range(0, n, packet)]


def _run(seed, n0, depth, packet, sorted_mode, survive, off_frame):
    rng = np.random.default_rng(seed)
    # the state that rides, two sets: home per slot (FREE: never written); `truth` is the model's own knowledge, not the kernels'
    home = [np.full(n0, FREE, np.int64), np.full(n0, FREE, np.int64)]
    valid = rng.random(n0) >= off_frame
    queue = np.where(valid, np.arange(n0), -1)  # bounce 0: the identity, -1 off the frame
    truth = np.where(valid, np.arange(n0), -1)  # path (= its bounce-0 slot) of every queue entry
    home[0][valid] = np.arange(n0)[valid]       # k = 0: home is the slot itself (never stored by raygen, asked for by nobody)
    counts = []
    for k in range(depth + 1):
        n = len(queue)
        counts.append(n)
        rs, ws = k & 1, (k + 1) & 1
        before = home[rs].copy()
        cls = rng.integers(0, 4, n)
        cls[queue < 0] = 0  # off-frame entries sort with the terminal class
        goes_on = (rng.random(n) < survive) & (queue >= 0)
        has_ray = goes_on & (rng.random(n) < 0.8)  # the others end on their shadow ray
        new_slots, out_q, out_truth = [], [], []
        order = _packets(n, packet)
        order = [order[j] for j in rng.permutation(len(order))]  # the waves append in any order
        for base, cnt in order:
            idx = np.arange(base, base + cnt)
            if sorted_mode:
                idx = idx[np.argsort(cls[idx], kind="stable")]  # the counting sort by class
            q = base + np.arange(cnt)  # position in processing order
            live = goes_on[idx]
            p = queue[idx]
            # a live record reads its slot p of set rs: home must be there and be the path it belongs to
            assert (home[rs][p[live]] == truth[idx][live]).all()
            assert (q[live] < n).all()
            home[ws][q[live]] = home[rs][p[live]]
            new_slots.append(q[live])
            ray = has_ray[idx]
            out_q.append(q[ray])
            out_truth.append(truth[idx][ray])
        new_slots = np.concatenate(new_slots) if new_slots else np.zeros(0, np.int64)
        assert len(np.unique(new_slots)) == len(new_slots), "two records of a stage share a slot"
        assert (new_slots >= 0).all() and (new_slots < n).all()
        assert np.array_equal(home[rs], before), "the set being read was written"
        queue = np.concatenate(out_q) if out_q else np.zeros(0, np.int64)
        truth = np.concatenate(out_truth) if out_truth else np.zeros(0, np.int64)
        # every entry of the next stage's queue leads home
        assert np.array_equal(home[ws][queue], truth)
        assert len(queue) <= n
        if len(queue) == 0:
            break
    return counts


@pytest.mark.parametrize("sorted_mode", [False, True])
@pytest.mark.parametrize("packet", [256, 512, 1024])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_renumbered_slots_are_unique_dense_and_lead_home(seed, packet, sorted_mode):
    counts = _run(seed, n0=52 * 36 + 37, depth=8, packet=packet, sorted_mode=sorted_mode, survive=0.85, off_frame=0.1)
    assert len(counts) == 9 and all(a >= b for a, b in zip(counts, counts[1:])) and counts[-1] > 0


@pytest.mark.parametrize("survive", [0.0, 0.05, 0.5, 1.0])
def test_survival_extremes(survive):
    counts = _run(7, n0=3000, depth=6, packet=256, sorted_mode=True, survive=survive, off_frame=0.0)
    if survive == 0.0:
        assert counts == [3000]
    if survive == 1.0:
        assert len(counts) == 7


def test_the_nee_tag_holds_home_and_kind():
    """nee.w = home << 2 | kind as 32 bits (kind 0 direct, 1 indirect, 2 nothing): every slot below 2^30 comes back with its kind."""
    homes = np.array([0, 1, 63, 64, 2_073_599, (1 << 30) - 1], np.uint32)
    for kind in (0, 1, 2):
        tag = (homes << np.uint32(2)) | np.uint32(kind)
        assert np.array_equal(tag >> np.uint32(2), homes) and ((tag & np.uint32(3)) == kind).all()
        # the tag travels as a float's bits: a bit-for-bit view, no arithmetic
        assert np.array_equal(tag.view(np.float32).view(np.uint32), tag)
