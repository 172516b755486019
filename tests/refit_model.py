"""numpy restatement of the refit contract (rdh_scene_refit_geometry) and of rdh_scene_tree_cost, shared by
test_bvh_refit_cpu.py and test_gpu_bvh_refit.py.

Nodes are walked in ordering 0: an inner node at position p has child a at p + 1 and child b at the miss link of p + 1.
A leaf's box folds its three vertices in order from the empty box; an inner node's box is comb(box a, box b), a first."""
import numpy as np

FLT_MAX = np.float32(3.402823466e38)


def _comb_lo(a, b):
    return np.where(b < a, b, a)


def _comb_hi(a, b):
    return np.where(a < b, b, a)


def _structure(nodes0):
    prim = np.asarray(nodes0["primitiveId"], np.int64)
    nxt = np.asarray(nodes0["nextNodeIfMiss"], np.int64)
    S = len(prim)
    inner = np.flatnonzero(prim < 0)
    ca = np.full(S, -1, np.int64)
    cb = np.full(S, -1, np.int64)
    ca[inner] = inner + 1
    cb[inner] = nxt[inner + 1]
    # levels, top-down (a child's position is larger than its parent's)
    levels = []
    frontier = np.array([0], np.int64)
    while len(frontier):
        levels.append(frontier)
        f = frontier[prim[frontier] < 0]
        frontier = np.concatenate([ca[f], cb[f]])
    return prim, ca, cb, levels


def refit_positions(vertices, nodes0):
    """Boxes per ordering-0 position: float32 [S, 6] (lo.xyz, hi.xyz)."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3, 3)
    prim, ca, cb, levels = _structure(nodes0)
    S = len(prim)
    box = np.zeros((S, 6), np.float32)
    leaves = np.flatnonzero(prim >= 0)
    t = v[prim[leaves]]
    lo = np.where(t[:, 0] < FLT_MAX, t[:, 0], FLT_MAX)
    hi = np.where(-FLT_MAX < t[:, 0], t[:, 0], -FLT_MAX)
    for j in (1, 2):
        lo = _comb_lo(lo, t[:, j])
        hi = _comb_hi(hi, t[:, j])
    box[leaves, :3] = lo
    box[leaves, 3:] = hi
    for lvl in reversed(levels):
        p = lvl[prim[lvl] < 0]
        if len(p) == 0:
            continue
        a, b = box[ca[p]], box[cb[p]]
        box[p, :3] = _comb_lo(a[:, :3], b[:, :3])
        box[p, 3:] = _comb_hi(a[:, 3:], b[:, 3:])
    return box


def refit_boxes(vertices, nodes):
    """Boxes per slot (the layout of hostlib.build_bvh's `boxes`) for the topology `nodes` (six MTBVH_NODE_DTYPE arrays)."""
    pos = refit_positions(vertices, nodes[0])
    out = np.empty_like(pos)
    out[np.asarray(nodes[0]["boundingBoxId"], np.int64)] = pos
    return out


def tree_cost(boxes):
    """sum over every node of surfaceArea(box) / surfaceArea(root box), float64 (boxes per slot, root at slot 0).  A root box of
    zero surface area makes every node count 1: the node count."""
    b = np.asarray(boxes, np.float32).astype(np.float64)
    s = b[:, 3:] - b[:, :3]
    area = 2.0 * (s[:, 0] * s[:, 1] + s[:, 1] * s[:, 2] + s[:, 2] * s[:, 0])
    if not area[0] > 0.0:
        return float(len(area))
    return float(np.sum(area / area[0]))


# ---- triangle soups the refit tests share ----

def soup(n, seed, scale=1.0):
    """n random small triangles in [-scale, scale]^3: float32 [3n, 3]."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 1, 3)) * scale
    return (c + rng.normal(0, 0.05 * scale, (n, 3, 3))).astype(np.float32).reshape(-1, 3)


SIGNED_ZERO_VALUES = np.array([0.0, -0.0, 1.0, -1.0, 0.5], np.float32)


def signed_zeros_soup(rng, n=3000):
    """n triangles whose coordinates are drawn from {+0, -0, 1, -1, 0.5}: float32 [3n, 3]."""
    return rng.choice(SIGNED_ZERO_VALUES, size=(3 * n, 3)).astype(np.float32)
