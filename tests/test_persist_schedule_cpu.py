"""The scheduler model (tests/persist_schedule_model.py) held to its own conditions, without a GPU: the bucket function against an
independent derivation, the running mean on the domain the renderer can reach, and check() against hand-made wrong results.
tests/test_gpu_persist_schedule.py compares k_persist_schedule with this model."""
import numpy as np
import pytest

import persist_schedule_model as M


# ---------------------------------------------------------------------------------------------------------------------------------
# bucket_of
# ---------------------------------------------------------------------------------------------------------------------------------
def _thresholds():
    """The costs at which a new bucket begins, ascending: 1, 2, then 2^k * {4, 5, 6, 7} / 4 for k = 2.. (a quarter octave each),
    with the rank b that bucket_of's formula gives the first of them (1 -> 1, 2 -> 5, 4 -> 9, 5 -> 10, ...)."""
    out = [(1, 1), (2, 5)]
    b = 9
    for k in range(2, 32):
        for m in (4, 5, 6, 7):
            out.append(((1 << k) * m // 4, b))
            b += 1
    return out


THRESHOLDS = _thresholds()


def _bucket_by_thresholds(c):
    """Exact integer comparison: the rank of the last threshold that c reaches, saturated at 63, counted down from 63."""
    b = 0
    for t, rank in THRESHOLDS:
        if c >= t:
            b = rank
    return 63 - min(63, b)


def test_thresholds_are_exact_integers_and_ascending():
    ts = [t for t, _ in THRESHOLDS]
    assert ts == sorted(set(ts))
    assert all((1 << k) * m % 4 == 0 for k in range(2, 32) for m in (4, 5, 6, 7))
    assert ts[:8] == [1, 2, 4, 5, 6, 7, 8, 10] and ts[-1] == 7 << 29


def test_bucket_of_over_every_small_cost():
    n = (1 << 17) + 1
    want = np.empty(n, np.int64)
    edge = 0
    b = 0
    for c in range(n):  # one pass over the thresholds: the same comparison as _bucket_by_thresholds, incrementally
        while edge < len(THRESHOLDS) and c >= THRESHOLDS[edge][0]:
            b = THRESHOLDS[edge][1]
            edge += 1
        want[c] = 63 - min(63, b)
    assert [M.bucket_of(c) for c in range(n)] == want.tolist()
    assert np.array_equal(M.buckets_of(np.arange(n, dtype=np.uint32)), want)
    assert want[0] == 63 and want[1] == 62 and want[2] == want[3] == 58 and want[4] == 54


def test_bucket_of_around_every_power_of_two():
    cs = sorted({c for k in range(0, 33) for c in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 0 <= c <= M.MASK})
    assert cs[-1] == M.MASK
    for c in cs:
        assert M.bucket_of(c) == _bucket_by_thresholds(c), c
    assert np.array_equal(M.buckets_of(np.array(cs, np.uint64).astype(np.uint32)), [_bucket_by_thresholds(c) for c in cs])
    for c in (0x7fffffff, 0x80000000, 0xffffffff):  # a signed count-leading-zeros must read these as 31 bits, not as negative
        assert M.bucket_of(c) == 0


def test_bucket_of_is_monotone_and_saturates():
    b = M.buckets_of(np.arange(1 << 17, dtype=np.uint32))
    assert np.all(np.diff(b) <= 0)
    assert M.bucket_of(M.SATURATE - 1) == 1 and M.bucket_of(M.SATURATE) == 0
    assert np.all(b[M.SATURATE:] == 0) and np.all(b[:M.SATURATE] > 0)


def test_which_buckets_are_never_used():
    used = set(M.buckets_of(np.arange(1 << 17, dtype=np.uint32)).tolist())
    assert sorted(set(range(64)) - used) == list(M.UNUSED_BUCKETS)
    assert len(used) == 58


# ---------------------------------------------------------------------------------------------------------------------------------
# ema_next
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ema_starts_at_the_first_cost():
    for c in (0, 1, 7, 12345, M.MASK):
        assert M.ema_next(0, c) == c
    assert np.array_equal(M.emas_next([0, 0, 5], [9, 0, 5]), [9, 0, 5])


@pytest.mark.parametrize("c", [0, 1, 5, 100, 2800, 49152, (1 << 29) - 1])
@pytest.mark.parametrize("start", [1, 3, 100, 65536, (1 << 29) - 1])
def test_ema_converges_to_a_constant_cost(start, c):
    """mean' - mean = floor((c - mean + 3) / 8): the mean moves towards c while it is more than 4 below or 3 above it, and rests
    inside [c - 4, c + 3] (integer division: the last eighth is not taken).  A mean that has reached 0 restarts at the next cost."""
    e = start
    for _ in range(400):  # the distance shrinks by an eighth per step: 8 * ln(2^29) < 170 steps from anywhere in the domain
        nxt = M.ema_next(e, c)
        assert abs(nxt - c) <= abs(e - c)
        e = nxt
    assert c - 4 <= e <= c + 3 or (e == 0 and c <= 4)
    assert M.ema_next(e, c) == e or e == 0


def test_ema_never_wraps_on_the_reachable_domain():
    """old, c < 2^29: 7 * old + c + 3 < 2^32, so the 32-bit sum is the true sum and the new mean is again below 2^29.  The
    renderer stays inside: a block's cost is pathSteps, the box-loop iterations ONE path was in flight for, at most 57 rays of a
    28-bounce path; the longest walks measured are a few thousand iterations, and 2^29 iterations of one wave would last minutes."""
    top = (1 << 29) - 1
    rng = np.random.default_rng(5)
    old = np.concatenate([[top, top, 1, 1], rng.integers(1, top + 1, 4096)]).astype(np.uint64)
    c = np.concatenate([[top, 0, top, 0], rng.integers(0, top + 1, 4096)]).astype(np.uint64)
    true = (7 * old.astype(object) + c.astype(object) + 3) // 8  # Python integers: no modulus
    assert np.array_equal(M.emas_next(old, c).astype(object), true)
    assert max(true) <= top
    assert [M.ema_next(int(o), int(k)) for o, k in zip(old[:64], c[:64])] == list(true[:64])
    lo, hi = np.minimum(old, c).astype(object), np.maximum(old, c).astype(object)
    assert all(l <= t <= h for l, t, h in zip(lo, true, hi))  # a mean lies between what it averages


def test_ema_outside_the_domain_is_the_wrapped_sum():
    assert M.ema_next(M.MASK, M.MASK) == ((8 * M.MASK + 3) % (1 << 32)) // 8
    assert M.ema_next(1 << 31, 0) == ((7 << 31) % (1 << 32)) // 8
    assert np.array_equal(M.emas_next([M.MASK, 1 << 31], [M.MASK, 0]), [M.ema_next(M.MASK, M.MASK), M.ema_next(1 << 31, 0)])


# ---------------------------------------------------------------------------------------------------------------------------------
# check() rejects what it must
# ---------------------------------------------------------------------------------------------------------------------------------
def _good():
    """Ten blocks in four buckets and what a correct launch leaves."""
    cost = np.array([0, 1, 5, 5, 300, 70000, 2, 0, 299, 6], np.uint32)
    ema = np.array([0, 0, 5, 40, 0, 0, 9, 0, 310, 0], np.uint32)
    after = M.emas_next(ema, cost)
    bk = M.buckets_of(after)
    order = np.argsort(bk, kind="stable").astype(np.int32)
    return cost, ema, np.zeros(10, np.uint32), after, order


def test_check_accepts_a_correct_result_in_any_order_inside_a_bucket():
    cost, ema, zero, after, order = _good()
    M.check(cost, ema, zero, after, order, 10)
    bk = M.buckets_of(after)[order]
    k = int(np.flatnonzero(bk[1:] == bk[:-1])[0])  # two neighbours of one bucket, swapped: still right
    swapped = order.copy()
    swapped[[k, k + 1]] = swapped[[k + 1, k]]
    M.check(cost, ema, zero, after, swapped, 10)
    M.check(cost, ema, zero, after, np.concatenate([order, [-7, 99]]), 10)  # what lies beyond n is not the order's business


def _rejected(match, **changed):
    cost, ema, zero, after, order = _good()
    args = {"cost_after": zero, "ema_after": after, "order": order}
    args.update(changed)
    with pytest.raises(AssertionError, match=match):
        M.check(cost, ema, args["cost_after"], args["ema_after"], args["order"], 10)


def test_check_rejects_a_duplicated_entry():
    order = _good()[4].copy()
    order[3] = order[4]
    _rejected("listed 2 times", order=order)


def test_check_rejects_a_missing_entry():
    """In n entries a block can only be missing because another is listed twice or an entry is out of range: the last block of the
    order (the cheapest: 64 stale pixels nobody would look for) gives way to a second copy of the first, and to nothing at all."""
    order = _good()[4].copy()
    gone = int(order[9])
    order[9] = order[0]
    assert gone not in order
    _rejected("listed 2 times", order=order)
    with pytest.raises(AssertionError, match="shorter than n"):
        M.check_order(_good()[4][:9], _good()[3], 10)


@pytest.mark.parametrize("bad", [10, -1, 1 << 30])
def test_check_rejects_an_entry_outside_the_range(bad):
    order = _good()[4].copy()
    order[5] = bad
    _rejected("outside 0..9", order=order)


def test_check_rejects_a_pair_swapped_across_buckets():
    cost, ema, zero, after, order = _good()
    bk = M.buckets_of(after)[order]
    k = int(np.flatnonzero(bk[1:] != bk[:-1])[0])
    swapped = order.copy()
    swapped[[k, k + 1]] = swapped[[k + 1, k]]
    _rejected("is followed by bucket", order=swapped)


def test_check_rejects_a_stale_cost():
    cost_after = np.zeros(10, np.uint32)
    cost_after[4] = 300
    _rejected("not zeroed", cost_after=cost_after)


def test_check_rejects_a_wrong_mean():
    after = _good()[3].copy()
    after[3] += 1  # (7 * 40 + 5 + 3) // 8 = 36, not 37: a mean rounded up instead of to nearest
    _rejected("the model says 36", ema_after=after)
    after = _good()[3].copy()
    after[8] = 299  # the cost taken over where a mean existed
    _rejected("the model says", ema_after=after)


def test_check_rejects_a_sorted_order_of_the_old_means():
    """An order that is a permutation and bucket-sorted, but by the means BEFORE the fold."""
    cost, ema, zero, after, _ = _good()
    stale = np.argsort(M.buckets_of(ema), kind="stable").astype(np.int32)
    with pytest.raises(AssertionError):
        M.check(cost, ema, zero, after, stale, 10)
