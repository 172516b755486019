"""The sharded layout of the wavefront queues, modelled in numpy (kernels_wave.h: WfShardMap, wfQueueStride, wavePull).

Producer: a stage of n records is shaded in packets of `packet` records; packet j appends its entries, at most one of a kind per
record, to shard j % S at s * R + (what the shard holds so far), R = ceil(ceil(n / packet) / S) * packet, in whatever order the
packets' appends arrive.  Consumer: item i of the queue lives at s * R + (i - prefix[s]), prefix[s] <= i < prefix[s + 1], resolved
as the kernel resolves it: i + step[0] + the steps of the shards whose first item is not beyond i.  Pulls: behind the G static
packets wave g pulls from head g % Se only, Se = min(S, G), and its head's t-th pull is packet G + Se * t + g % Se.
"""
import numpy as np
import pytest

PACKETS = (256, 512, 768, 1024)
SHARDS = (1, 2, 8)


def stride(n, packet, S):
    packets = -(-n // packet)
    return -(-packets // S) * packet


def produce(rng, n, packet, S):
    """(R, counts [S], written {address: (packet, entry)}) after every packet's append, in random order."""
    R = stride(n, packet, S)
    P = -(-n // packet)
    records = np.minimum(packet, n - np.arange(P) * packet)
    mode = rng.integers(0, 3)  # every record an entry / none for most packets / anything
    entries = records.copy() if mode == 0 else rng.integers(0, records + 1)
    if mode == 1:
        entries[rng.random(P) < 0.7] = 0
    counts = np.zeros(S, np.int64)
    written = {}
    for j in rng.permutation(P):
        s = int(j) % S
        at = counts[s]  # the returning atomic
        counts[s] += entries[j]
        for t in range(int(entries[j])):
            a = s * R + int(at) + t
            assert a not in written, "two entries at one address"
            assert s * R <= a < (s + 1) * R, "an entry outside its shard's region"
            written[a] = (int(j), t)
    return R, counts, written


def shard_map(counts, R, item_base=0):
    """first[], step[] as WfShardMap::load makes them."""
    S = len(counts)
    first, step = np.zeros(S, np.int64), np.zeros(S, np.int64)
    at = shift = 0
    for j in range(S):
        first[j] = item_base + at
        step[j] = j * R - first[j] - shift
        shift += step[j]
        at += counts[j]
    return first, step, at


def address(i, first, step):
    """WfShardMap::at for an array of items."""
    a = i + step[0]
    for j in range(1, len(first)):
        a = a + np.where(i >= first[j], step[j], 0)
    return a


@pytest.mark.parametrize("S", SHARDS)
@pytest.mark.parametrize("seed", range(40))
def test_layout(seed, S):
    rng = np.random.default_rng(1000 * S + seed)
    packet = int(rng.choice(PACKETS))
    n = int(rng.choice([1, packet - 1, packet, packet + 1, S * packet, S * packet + 1, int(rng.integers(1, 40 * packet))]))
    R, counts, written = produce(rng, n, packet, S)
    assert (counts <= R).all(), "a shard outgrew its region"
    assert S * R <= n + S * packet
    assert S * R <= n + S * 1024  # what the host adds to the queues
    if S == 1:
        assert R >= n and sorted(written) == list(range(len(written)))  # one region from 0: the unsharded queue
    # the consumers' map, with the queue anywhere in the stage's item space (the shadow rays lie behind the extension rays)
    for item_base in (0, int(rng.integers(1, 5000))):
        first, step, total = shard_map(counts, R, item_base)
        assert total == len(written)
        items = item_base + np.arange(total)
        a = address(items, first, step)
        assert len(set(a.tolist())) == total, "two items at one address"
        assert set(a.tolist()) == set(written), "the items are not the written entries"
        s = np.searchsorted(np.cumsum(counts), items - item_base, side="right")  # the definition: prefix[s] <= i < prefix[s + 1]
        prefix = np.concatenate([[0], np.cumsum(counts)])
        assert np.array_equal(a, s * R + (items - item_base - prefix[s]))


def test_layout_of_an_empty_queue():
    for S in SHARDS:
        first, step, total = shard_map(np.zeros(S, np.int64), 0)
        assert total == 0 and not first.any() and not step.any()  # stage 0 before anything ran: the identity
        first, step, total = shard_map(np.array([640] + [0] * (S - 1)), 0)  # raygen: shard 0 alone, whatever the stride
        assert np.array_equal(address(np.arange(640), first, step), np.arange(640))


def pulls(rng, n, packet, S, G):
    """The packets the waves shade, static ones included, and the atomics made, under a random interleaving of the waves."""
    taken, atomics = list(range(min(G, -(-n // packet)))), 0
    if n <= G * packet:
        return taken, atomics
    Se = min(S, G)
    heads = [0] * Se
    live = list(range(G))  # n > G * packet: every wave has a whole static packet, and pulls when it is done with it
    while live:
        g = live[int(rng.integers(len(live)))]
        x = g % Se
        t = heads[x]
        heads[x] += 1
        atomics += 1
        pkt = G + Se * t + x
        if pkt * packet >= n:
            live.remove(g)
        else:
            taken.append(pkt)
    return taken, atomics


@pytest.mark.parametrize("S", SHARDS)
@pytest.mark.parametrize("seed", range(40))
def test_pulls(seed, S):
    rng = np.random.default_rng(7000 * S + seed)
    packet = int(rng.choice(PACKETS))
    G = int(rng.choice([1, 2, 3, S - 1 if S > 1 else 1, S, S + 1, 12, 48, int(rng.integers(1, 200))]))
    n = int(rng.choice([1, G * packet, G * packet + 1, (G + S) * packet - 1, int(rng.integers(1, 4 * (G + S) * packet))]))
    taken, atomics = pulls(rng, n, packet, S, G)
    P = -(-n // packet)
    assert sorted(taken) == list(range(P)), "a packet shaded twice or not at all"
    if n <= G * packet:
        assert atomics == 0
    else:
        assert atomics == (P - G) + G  # one per pulled packet and one failing pull per wave
