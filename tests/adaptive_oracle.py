"""What the adaptive-sampling tests expect, from the CPU oracle alone: the finished samples of every pixel and the running means after
k of them, whole frames; the moments those samples give through the numpy model; the work counters of single (pixel, sample) pairs."""
import numpy as np

import adaptive_model as am
from helpers import oracle_path_trace_mt

COUNTER_KEYS = ("closestRays", "anyRays", "nodeVisits", "triTests", "closestHits")


def frames(sd, cam, looper0, num, depth):
    """{"sd", "si": [num, P, 3] finished samples (a call at iter 0 into zeroed images returns the sample itself), "ad", "ai":
    [num + 1, P, 3] the oracle's own running means after k samples, "stats": [num] the whole frame's counters per sample}.
    Sample k of every pixel draws Sobol row (looper0 + k) % 10000."""
    w, h = (int(v) for v in cam["resolution"])
    p = w * h
    out = {"sd": np.zeros((num, p, 3), np.float32), "si": np.zeros((num, p, 3), np.float32),
           "ad": np.zeros((num + 1, p, 3), np.float32), "ai": np.zeros((num + 1, p, 3), np.float32), "stats": []}
    d, i = np.zeros((p, 3), np.float32), np.zeros((p, 3), np.float32)
    for k in range(num):
        row = (looper0 + k) % 10000
        _, st = oracle_path_trace_mt(sd, cam, out["sd"][k], out["si"][k], 0, row, depth)
        out["stats"].append({key: st[key] for key in COUNTER_KEYS})
        oracle_path_trace_mt(sd, cam, d, i, k, row, depth)
        out["ad"][k + 1], out["ai"][k + 1] = d, i
    for key in ("sd", "si", "ad", "ai"):
        out[key].setflags(write=False)
    return out


def moments_after(fr, counts):
    """[P, 2]: the model's running means of L and L * L over samples 0 .. counts[p] - 1 of every pixel."""
    p = fr["sd"].shape[1]
    m = np.zeros((p, 2), np.float32)
    zero = np.zeros(p, np.int32)
    am.fold(np.zeros((p, 3), np.float32), np.zeros((p, 3), np.float32), zero.copy(), m, fr["sd"], fr["si"], np.asarray(counts, np.int32))
    return m


def means_at(fr, counts):
    """([P, 3], [P, 3]): the oracle's running means of every pixel after its own counts[p] samples."""
    idx = np.arange(fr["sd"].shape[1])
    return fr["ad"][counts, idx].copy(), fr["ai"][counts, idx].copy()


def pair_counters(sd, cam, looper0, counts, requests, depth):
    """The oracle's work counters of exactly the requested (pixel, sample) pairs: one single-pixel call each."""
    from oracle import pyoracle

    orc = pyoracle.OracleScene(sd)
    p = len(counts)
    d, i = np.zeros((p, 3), np.float32), np.zeros((p, 3), np.float32)
    orc.reset_stats()
    for px in np.flatnonzero(requests > 0):
        for j in range(int(requests[px])):
            n = int(counts[px]) + j
            orc.path_trace(cam, d, i, n, (looper0 + n) % 10000, depth, pix=(int(px), int(px) + 1, 1))
    st = orc.stats()
    return {key: st[key] for key in COUNTER_KEYS}
