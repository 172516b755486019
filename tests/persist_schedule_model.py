"""A CPU model of the persistent path tracer's block scheduler (k_persist_schedule, radish_pt_amd/csrc/device/kernels_persist.h),
written from the comment above the kernel: what one schedule launch must leave in its three arrays, in plain integers.

The contract.  Each persistent launch records, per 8x8 block, the largest number of box-loop iterations one of its paths was in
flight for (`cost`).  One schedule launch over n blocks
  * folds every block's cost into its running mean: mean' = cost when the mean was 0, else (7 * mean + cost + 3) // 8, in 32-bit
    unsigned arithmetic (ema_next);
  * zeroes the costs (the launch after next accumulates into the same buffer with atomicMax);
  * writes `order`, a permutation of range(n) in which the quarter-octave bucket (bucket_of) of the NEW mean never decreases:
    bucket 0 holds the most expensive blocks and comes first, bucket 63 holds the blocks whose mean is 0 (among them the blocks
    without a pixel) and comes last.
Nothing beyond entry n - 1 of any array is touched.

What is deliberately not pinned.  The order INSIDE a bucket: the kernel hands out a bucket's slots with one LDS atomic per wave
and bucket, so which wave's blocks come first is decided by which atomic lands first; ties are equally expensive and any order
of them is right.  check() therefore compares each bucket's span as a SET.  The cost values a render produces are not modelled
either (they depend on which lanes share a wave), nor is any meaning of means beyond 2^29: ema_next is computed modulo 2^32 so
that the model says what the kernel does there too, but such a mean is no longer a mean.
"""
import numpy as np

BUCKETS = 64
KEEP = 7                 # RD_EMA_KEEP: mean' = (KEEP * mean + cost + KEEP // 2) // (KEEP + 1)
SATURATE = 49152         # 2^15 * 6 / 4: every cost from here on is in bucket 0
# bucket numbers no cost maps to: below 4 there are no fractional bits, so 1, 2..3 and 4 are 4 bucket numbers apart
UNUSED_BUCKETS = (55, 56, 57, 59, 60, 61)
MASK = (1 << 32) - 1


def bucket_of(c):
    """Quarter-octave bucket of a cost or mean, descending: 63 for 0, otherwise 63 - min(63, 4 * floor(log2 c) + f + 1) with f the
    two bits below the leading one (0 while c < 4: there are none)."""
    c = int(c)
    assert 0 <= c <= MASK
    if c == 0:
        return BUCKETS - 1
    lg = c.bit_length() - 1
    f = (c >> (lg - 2)) & 3 if lg >= 2 else 0
    return BUCKETS - 1 - min(BUCKETS - 1, 4 * lg + f + 1)


def buckets_of(values):
    """bucket_of over an array (uint32 values), vectorised with exact integer operations only."""
    v = np.asarray(values).astype(np.uint64)
    lg = np.zeros(v.shape, np.int64)
    for shift in (16, 8, 4, 2, 1):  # floor(log2 v) by halving: no floating point
        big = (v >> np.uint64(lg + shift)) > 0
        lg = np.where(big, lg + shift, lg)
    f = np.where(lg >= 2, (v >> np.maximum(lg - 2, 0).astype(np.uint64)) & np.uint64(3), np.uint64(0)).astype(np.int64)
    b = np.minimum(BUCKETS - 1, 4 * lg + f + 1)
    return np.where(v == 0, BUCKETS - 1, BUCKETS - 1 - b).astype(np.int64)


def ema_next(old, c):
    """The running mean after one more cost, modulo 2^32 as the kernel's unsigned arithmetic computes it."""
    old, c = int(old), int(c)
    assert 0 <= old <= MASK and 0 <= c <= MASK
    if old == 0:
        return c
    return ((KEEP * old + c + KEEP // 2) & MASK) // (KEEP + 1)


def emas_next(old, cost):
    """ema_next over arrays -> uint32."""
    old = np.asarray(old).astype(np.uint64)
    cost = np.asarray(cost).astype(np.uint64)
    folded = ((np.uint64(KEEP) * old + cost + np.uint64(KEEP // 2)) & np.uint64(MASK)) // np.uint64(KEEP + 1)
    return np.where(old == 0, cost, folded).astype(np.uint32)


def spans(buckets):
    """[(bucket, first, end)] of the non-empty buckets in the order the permutation lists them."""
    hist = np.bincount(np.asarray(buckets, np.int64), minlength=BUCKETS)
    out, first = [], 0
    for b in range(BUCKETS):
        if hist[b]:
            out.append((b, first, first + int(hist[b])))
            first += int(hist[b])
    return out


def check_order(order, means, n, what=""):
    """order[:n] is a permutation of range(n), bucket-sorted by `means`, with each bucket's span holding exactly its blocks."""
    order = np.asarray(order)[:n].astype(np.int64)
    means = np.asarray(means)[:n]
    assert len(order) == n and len(means) == n, f"{what}: arrays shorter than n = {n}"
    outside = np.flatnonzero((order < 0) | (order >= n))
    assert len(outside) == 0, f"{what}: order[{outside[0]}] = {order[outside[0]]} is outside 0..{n - 1}"
    seen = np.bincount(order, minlength=n)
    assert seen.max(initial=0) <= 1, f"{what}: block {int(np.argmax(seen))} is listed {int(seen.max())} times"
    assert seen.min(initial=1) >= 1, f"{what}: block {int(np.argmin(seen))} is missing"
    bk = buckets_of(means)
    along = bk[order]
    down = np.flatnonzero(np.diff(along) < 0)
    assert len(down) == 0, f"{what}: bucket {along[down[0]]} at position {down[0]} is followed by bucket {along[down[0] + 1]}"
    for b, first, end in spans(bk):
        want = np.flatnonzero(bk == b)
        got = np.sort(order[first:end])
        assert np.array_equal(got, want), f"{what}: bucket {b}'s span [{first}, {end}) does not hold the bucket's blocks"


def check(cost_before, ema_before, cost_after, ema_after, order, n, what=""):
    """One schedule launch over n blocks did what the contract says (the module's docstring).  The order inside a bucket is not
    pinned."""
    cost_before, ema_before = np.asarray(cost_before)[:n], np.asarray(ema_before)[:n]
    cost_after, ema_after = np.asarray(cost_after)[:n], np.asarray(ema_after)[:n]
    assert min(len(cost_before), len(ema_before), len(cost_after), len(ema_after)) == n, f"{what}: arrays shorter than n = {n}"
    want = emas_next(ema_before, cost_before)
    bad = np.flatnonzero(ema_after.astype(np.uint32) != want)
    assert len(bad) == 0, (f"{what}: mean of block {bad[0]} is {int(ema_after[bad[0]])}, the model says {int(want[bad[0]])} "
                           f"(old {int(ema_before[bad[0]])}, cost {int(cost_before[bad[0]])}); {len(bad)} differ")
    stale = np.flatnonzero(cost_after != 0)
    assert len(stale) == 0, f"{what}: cost of block {stale[0]} was left at {int(cost_after[stale[0]])}; {len(stale)} not zeroed"
    check_order(order, want, n, what)
