"""numpy restatement of the LBVH tree contract (rdh_build_bvh_device_ex with RDH_BVH_LBVH), shared by
test_bvh_lbvh_cpu.py and test_gpu_bvh_lbvh.py.

Every float operation is one float32 IEEE operation, as on the device.  The hierarchy is Karras' radix tree over the sorted
Morton codes; slots are the depth-first pre-order with the lower sorted range first; boxes follow the refit contract
(refit_model.py), so a refit with unchanged vertices leaves an LBVH tree as built.  build(v) returns what hostlib.build_bvh
returns: (boxes float32 [2N-1, 6] per slot, six MTBVH_NODE_DTYPE arrays)."""
import numpy as np

import refit_model

FLT_MAX = refit_model.FLT_MAX
MTBVH_NODE_DTYPE = np.dtype([("primitiveId", "<i4"), ("boundingBoxId", "<i4"), ("nextNodeIfMiss", "<i4")])


def leaf_boxes(vertices):
    """Per primitive: bvhLo / bvhHi folded over its three vertices in order from the empty box: float32 [N, 6]."""
    t = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3, 3)
    lo = np.where(t[:, 0] < FLT_MAX, t[:, 0], FLT_MAX)
    hi = np.where(-FLT_MAX < t[:, 0], t[:, 0], -FLT_MAX)
    for j in (1, 2):
        lo = refit_model._comb_lo(lo, t[:, j])
        hi = refit_model._comb_hi(hi, t[:, j])
    return np.concatenate([lo, hi], axis=1).astype(np.float32)


def _spread(q):
    """10-bit cells -> every third bit (bit i at 3i)."""
    q = q.astype(np.uint32)
    q = (q | (q << 16)) & np.uint32(0x030000FF)
    q = (q | (q << 8)) & np.uint32(0x0300F00F)
    q = (q | (q << 4)) & np.uint32(0x030C30C3)
    q = (q | (q << 2)) & np.uint32(0x09249249)
    return q


def morton_codes(vertices):
    """Steps 1-4: the 30-bit code of every primitive's centre, uint32 [N]."""
    b = leaf_boxes(vertices)
    c = (b[:, :3] + b[:, 3:]) * np.float32(0.5)
    with np.errstate(invalid="ignore"):
        ok = ~np.isnan(c)
    c_lo = np.where(ok, c, FLT_MAX).min(axis=0).astype(np.float32)  # values only: the fold order does not matter
    c_hi = np.where(ok, c, -FLT_MAX).max(axis=0).astype(np.float32)
    e = (c_hi - c_lo).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = np.where(e > 0, (c - c_lo) / np.where(e > 0, e, np.float32(1)), np.float32(0)).astype(np.float32)
        s = (t * np.float32(1024)).astype(np.float32)
        q = np.where(s > 0, np.where(s < np.float32(1023), np.floor(np.where(s > 0, s, 0)), 1023), 0).astype(np.uint32)
    return (_spread(q[:, 0]) << 2) | (_spread(q[:, 1]) << 1) | _spread(q[:, 2])


def _clz32(x):
    """Leading zeros of uint32 values (x > 0)."""
    _, e = np.frexp(x.astype(np.float64))
    return 32 - e.astype(np.int64)


def _delta(keys, i, j):
    """Karras' delta over the sorted keys, -1 where j is out of range."""
    n = len(keys)
    ok = (j >= 0) & (j < n)
    jj = np.where(ok, j, 0)
    x = keys[i] ^ keys[jj]
    same = x == 0
    d = np.where(same, 32 + _clz32(np.where(same, (i ^ jj).astype(np.uint32), 1)), _clz32(np.where(same, 1, x)))
    return np.where(ok, d, -1)


def karras(keys):
    """Step 6: for inner node i in [0, N-2] of the sorted keys, (first, last, split) with children [first, split] and
    [split + 1, last]."""
    n = len(keys)
    i = np.arange(n - 1, dtype=np.int64)
    d = np.where(_delta(keys, i, i + 1) - _delta(keys, i, i - 1) > 0, 1, -1)
    dmin = _delta(keys, i, i - d)
    lmax = np.full(n - 1, 2, np.int64)
    grow = _delta(keys, i, i + lmax * d) > dmin
    while grow.any():
        lmax = np.where(grow, lmax * 2, lmax)
        grow = grow & (_delta(keys, i, i + lmax * d) > dmin)
    l = np.zeros(n - 1, np.int64)
    t = lmax // 2
    while (t >= 1).any():
        step = (t >= 1) & (_delta(keys, i, i + (l + t) * d) > dmin)
        l = np.where(step, l + t, l)
        t = t // 2
    j = i + l * d
    dnode = _delta(keys, i, j)
    s = np.zeros(n - 1, np.int64)
    t = l.copy()
    active = np.ones(n - 1, bool)
    while active.any():
        t = np.where(active, (t + 1) >> 1, t)
        step = active & (_delta(keys, i, i + (s + t) * d) > dnode)
        s = np.where(step, s + t, s)
        active = active & (t > 1)
    split = i + s * d + np.minimum(d, 0)
    return np.minimum(i, j), np.maximum(i, j), split


def build(vertices):
    """(boxes float32 [2N-1, 6] per slot, nodes: six MTBVH_NODE_DTYPE arrays), as the LBVH builder must emit them."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    N = v.shape[0] // 3
    S = 2 * N - 1
    lb = leaf_boxes(v)
    codes = morton_codes(v)
    order = np.argsort(codes, kind="stable")  # step 5
    keys = codes[order]
    # node ids: inner i -> i, leaf at sorted position j -> N - 1 + j; root = 0 either way
    first = np.empty(S, np.int64)
    last = np.empty(S, np.int64)
    first[N - 1:] = last[N - 1:] = np.arange(N)
    left = np.full(S, -1, np.int64)
    right = np.full(S, -1, np.int64)
    parent = np.full(S, -1, np.int64)
    if N > 1:
        f, l, g = karras(keys)
        inner = np.arange(N - 1)
        first[:N - 1], last[:N - 1] = f, l
        left[:N - 1] = np.where(f == g, N - 1 + g, g)
        right[:N - 1] = np.where(l == g + 1, N - 1 + g + 1, g + 1)
        parent[left[:N - 1]] = inner
        parent[right[:N - 1]] = inner
    is_leaf = np.arange(S) >= N - 1
    count = last - first + 1
    # levels, top-down
    levels = []
    frontier = np.array([0], np.int64)
    while len(frontier):
        levels.append(frontier)
        fi = frontier[~is_leaf[frontier]]
        frontier = np.concatenate([left[fi], right[fi]])
    assert len(levels) <= 60, "deeper than the contract allows"
    # step 8 and the orderings' choices, bottom-up: bits k = ordering k visits the right (upper range) child first
    box = np.zeros((S, 6), np.float32)
    box[N - 1:] = lb[order]
    bits = np.zeros(S, np.int64)
    for lvl in reversed(levels):
        p = lvl[~is_leaf[lvl]]
        if len(p) == 0:
            continue
        A, B = box[left[p]], box[right[p]]
        ca = (A[:, :3] + A[:, 3:]) * np.float32(0.5)
        cb = (B[:, :3] + B[:, 3:]) * np.float32(0.5)
        for k in range(6):
            rf = (ca[:, k // 2] < cb[:, k // 2]) != bool(k & 1)
            bits[p] |= rf.astype(np.int64) << k
        a_first = (bits[p] & 1) == 0
        a = np.where(a_first[:, None], A, B)
        b = np.where(a_first[:, None], B, A)
        box[p, :3] = refit_model._comb_lo(a[:, :3], b[:, :3])
        box[p, 3:] = refit_model._comb_hi(a[:, 3:], b[:, 3:])
    # step 7 and the orderings' positions, top-down
    slot = np.zeros(S, np.int64)
    pos = np.zeros((6, S), np.int64)
    size = 2 * count - 1
    for lvl in levels:
        p = lvl[~is_leaf[lvl]]
        if len(p) == 0:
            continue
        L, R = left[p], right[p]
        slot[L] = slot[p] + 1
        slot[R] = slot[p] + 1 + size[L]
        for k in range(6):
            rf = ((bits[p] >> k) & 1) == 1
            fst, snd = np.where(rf, R, L), np.where(rf, L, R)
            pos[k, fst] = pos[k, p] + 1
            pos[k, snd] = pos[k, p] + 1 + size[fst]
    prim = np.where(is_leaf, np.concatenate([np.full(N - 1, -1), order]), -1)
    boxes = np.empty((S, 6), np.float32)
    boxes[slot] = box
    nodes = []
    for k in range(6):
        a = np.empty(S, MTBVH_NODE_DTYPE)
        a["primitiveId"][pos[k]] = prim
        a["boundingBoxId"][pos[k]] = slot
        a["nextNodeIfMiss"][pos[k]] = pos[k] + size
        nodes.append(a)
    return boxes, nodes


def depth(nodes0):
    """Levels of the tree in ordering 0 (the root alone: 1)."""
    _, _, _, levels = refit_model._structure(nodes0)
    return len(levels)
