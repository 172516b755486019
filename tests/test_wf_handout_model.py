"""The hand-out of k_wf_trace (kernels_wave.h: fixed first packets, tracePull) as a plain Python model, run under random
interleavings.

G workgroups of four waves, a literal-class list of nLit entries, `total` items, packets of 128.  Tickets below L = min(nLit, G)
have list duty: their waves own no first packet and start at the shared head once the list is done.  The waves of ticket t >= L
own packets 4 (t - L) .. 4 (t - L) + 3; the head hands out what lies behind 4 (G - L) packets.  A wave whose first reservation
starts at or beyond `total` declares itself exhausted at once and never pulls.

Every wave is a generator that yields after each access to the head and while it 'walks', and a seeded scheduler picks which
wave goes next, so pulls interleave arbitrarily and duty workgroups come to the head early, late or after it is dry.  Asserted:
every item of [0, total) is handed out exactly once; a wave is exhausted only after a reservation of its own landed at or beyond
`total`; the head is pulled at most once per packet behind the fixed ones plus once per wave."""
import random

import pytest

WAVES, PACKET = 4, 128


def wave(state, rnd, G, L, total, wg, w):
    duty = wg < L
    head_base = (G - L) * WAVES * PACKET
    res_next = head_base if duty else ((wg - L) * WAVES + w) * PACKET
    res_end = res_next if duty else res_next + PACKET
    exhausted = res_next >= total
    res_end = min(res_end, total)
    if duty:
        for _ in range(rnd.randrange(0, 40)):  # the workgroup's list ray, short or very long
            yield
    while not exhausted:
        n_idle = rnd.randrange(16, 65)  # RD_REFILL_MIN .. 64 idle lanes
        taken = 0
        while taken < n_idle and not exhausted:
            if res_next == res_end:
                res_next = state["head"] + head_base  # tracePull: one atomic
                state["head"] += PACKET
                state["pulls"] += 1
                yield
                res_end = res_next + PACKET
                if res_next >= total:
                    exhausted = True
                    break
                res_end = min(res_end, total)
            give = min(n_idle - taken, res_end - res_next)
            for item in range(res_next, res_next + give):
                state["handed"][item] += 1
            res_next += give
            taken += give
        for _ in range(rnd.randrange(0, 4)):  # the lanes walk
            yield


def run(seed):
    rnd = random.Random(seed)
    G = rnd.choice((1, 2, 3, 5, 8))
    n_lit = max(rnd.choice((0, 0, 1, G - 1, G, G + 3, rnd.randrange(0, 2 * G + 1))), 0)
    fixed = G * WAVES * PACKET
    total = rnd.choice((0, 1, PACKET - 1, PACKET, PACKET + 1, fixed - 1, fixed, fixed + 1, rnd.randrange(0, 6 * fixed)))
    L = min(n_lit, G)
    state = {"head": 0, "pulls": 0, "handed": [0] * total}
    live = [wave(state, rnd, G, L, total, wg, w) for wg in range(G) for w in range(WAVES)]
    burst = rnd.choice((1, 1, 4, 32))  # some schedules let one wave run for long stretches while the others stand still
    while live:
        g = rnd.choice(live)
        for _ in range(rnd.randrange(1, burst + 1)):
            try:
                next(g)
            except StopIteration:
                live.remove(g)
                break
    bad = [i for i, h in enumerate(state["handed"]) if h != 1]
    assert not bad, (seed, G, L, total, bad[:8])
    behind = max(0, total - (G - L) * WAVES * PACKET)
    assert state["pulls"] <= (behind + PACKET - 1) // PACKET + G * WAVES, (seed, G, L, total, state["pulls"])
    return G, L, total


@pytest.mark.parametrize("block", range(4))
def test_every_item_is_handed_out_exactly_once(block):
    seen = {"all_duty": 0, "some_duty": 0, "no_duty": 0, "head_dry_for_duty": 0}
    for seed in range(block * 100, block * 100 + 100):
        G, L, total = run(seed)
        seen["all_duty" if L == G else ("some_duty" if L else "no_duty")] += 1
        if 0 < L and total <= (G - L) * WAVES * PACKET:
            seen["head_dry_for_duty"] += 1  # the fixed packets cover the stage: duty workgroups leave without a pull
    assert all(v > 0 for v in seen.values()), seen  # the schedules must have reached the cases this is about
