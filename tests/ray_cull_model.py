"""The emitter-box test of the wavefront path (radish_pt_amd/csrc/device/ray_cull.h: k_emitter_bounds, mayReachEmitters) restated in
numpy binary32, operation by operation: every array below is float32 and numpy rounds each float32 operation once, as the device
does (the library is built without contraction)."""
import numpy as np

F = np.float32
PAD = F(2.0 ** -10)          # kEmitPad
FAR_MARGIN = F(1.0 + 2.0 ** -19)
HINT2 = F(1.21e-12)          # (1.1e-6)^2, on the squared length
AXIS2 = F(0.999997)          # (1 - 1.5e-6)^2: a direction this close to an axis is kept


def padded_box(emissive_vertices, root_lo, root_hi):
    """k_emitter_bounds: (lo, hi) float32[3] of the box over the emissive triangles' vertices, padded by 2^-10 of the largest extent
    of the root box (or of the emitters' own box, if larger); None without emissive triangles."""
    v = np.asarray(emissive_vertices, F).reshape(-1, 3)
    if v.shape[0] == 0:
        return None
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = np.max(hi - lo)
    ext = max(ext, np.max(np.asarray(root_hi, F) - np.asarray(root_lo, F)))
    pad = F(ext) * PAD
    return (lo - pad).astype(F), (hi + pad).astype(F)


def may_reach(box, o, d):
    """mayReachEmitters for rays o, d (float32 [n, 3]): bool [n], False = the ray is not queued."""
    o, d = np.asarray(o, F), np.asarray(d, F)
    assert o.dtype == F and d.dtype == F
    if box is None:
        return np.zeros(len(o), bool)
    lo, hi = box
    len2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    l2 = len2 * HINT2
    hinted = ~((d[:, 0] * d[:, 0] >= l2) & (d[:, 1] * d[:, 1] >= l2) & (d[:, 2] * d[:, 2] >= l2))
    hinted |= ~(np.fmax(np.fmax(d[:, 0] * d[:, 0], d[:, 1] * d[:, 1]), d[:, 2] * d[:, 2]) <= len2 * AXIS2)
    inside = np.all((o >= lo) & (o <= hi), axis=1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = F(1.0) / d
        a, b = (lo - o) * inv, (hi - o) * inv
        t_near = np.fmax(np.fmax(np.fmin(a[:, 0], b[:, 0]), np.fmin(a[:, 1], b[:, 1])), np.fmin(a[:, 2], b[:, 2]))
        t_far = np.fmin(np.fmin(np.fmax(a[:, 0], b[:, 0]), np.fmax(a[:, 1], b[:, 1])), np.fmax(a[:, 2], b[:, 2]))
        miss = (t_far < F(0.0)) | (t_near > t_far * FAR_MARGIN)
    return hinted | inside | ~miss
