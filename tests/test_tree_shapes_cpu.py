"""The tree shapes that the LBVH builder and the refit make, as inputs of the traversal tests (the device checks are in
test_gpu_tree_shapes.py), and the CPU checks of the oracle on them.

Each case is a scene as the device holds it after upload_scene, update_geometry(builder="lbvh") and refit_geometry calls, and the
same vertices carrying the restated tree (lbvh_model.build, refit_model.refit_boxes) as the SceneData the oracle walks:
  * lbvh_*: Karras radix trees (duplicate Morton codes split by index: leaves at uneven depths, one box on several levels);
  * refit_scrambled: a host SAH tree refitted to vertices where every teapot of the grid stands at another teapot's place and every
    triangle is jittered by a few percent of the room: large, overlapping boxes and orderings that no longer follow the geometry;
  * lbvh_refit: an LBVH tree refitted the same way.

The oracle must walk every one of them like brute force, and its hits on different trees of the same vertices must agree, except
where the brute-force winner is a tie (another triangle at the same distance: the walk order decides) or lies so far away that the
box test's own rounding decides.  Both exceptions are counted and must stay rare."""
import ctypes as C

import numpy as np
import pytest

import lbvh_model
import refit_model
from helpers import random_rays
from test_gpu_bvh_build import _moved
from test_gpu_bvh_refit import _scene, _target, _with_vertices

CASES = ["lbvh_cornell", "lbvh_cornell_moved", "lbvh_teapots", "lbvh_teapots_moved", "refit_scrambled", "lbvh_refit"]
REFIT_CASES = ["refit_scrambled", "lbvh_refit"]


def scrambled_vertices(sd, seed=5, jitter=0.05):
    """The teapots scene with its 16 teapots dealt to each other's places (a fixed derangement) and every teapot triangle moved
    rigidly by up to `jitter` of the room's extent per axis; room and lights stay."""
    from radish_pt_amd import layouts as L

    rng = np.random.default_rng(seed)
    v = sd.vertices.reshape(-1, 3, 3).astype(np.float64)
    light = [i for i in range(len(sd.materials)) if sd.materials[i]["type"] == L.LIGHT]
    pots = [m for m in np.unique(sd.material_ids) if m not in light and np.count_nonzero(sd.material_ids == m) > 100]
    assert len(pots) == 16, len(pots)
    centre = {m: v[sd.material_ids == m].reshape(-1, 3).mean(axis=0) * np.array([1.0, 0.0, 1.0]) for m in pots}
    perm = np.roll(rng.permutation(len(pots)), 1)
    out = v.copy()
    extent = v.reshape(-1, 3).max(axis=0) - v.reshape(-1, 3).min(axis=0)
    for k, m in enumerate(pots):
        sel = sd.material_ids == m
        shift = centre[pots[perm[k]]] - centre[m]
        out[sel] += shift + rng.uniform(-jitter, jitter, (int(sel.sum()), 1, 3)) * extent
    return out.astype(np.float32).reshape(-1, 3)


def _lbvh_target(sd, verts):
    m = _with_vertices(sd, verts)
    m.boxes, m.nodes = lbvh_model.build(m.vertices)
    return m


def tree_case(name):
    """(scene to upload, [(call, SceneData whose vertices, normals and lights the call takes)], the oracle's SceneData: the vertices
    after the calls carrying the tree the device must then hold).  call is "lbvh" (update_geometry with builder="lbvh") or "refit"
    (refit_geometry)."""
    if name.startswith("lbvh_") and name != "lbvh_refit":
        sd = _scene(name.split("_")[1])
        m = _moved(sd, 1) if name.endswith("_moved") else _with_vertices(sd, sd.vertices)
        return sd, [("lbvh", m)], _lbvh_target(m, m.vertices)
    sd = _scene("teapots")
    scr = _with_vertices(sd, scrambled_vertices(sd))
    if name == "refit_scrambled":
        return sd, [("refit", scr)], _target(sd, scr)
    if name == "lbvh_refit":
        own = _lbvh_target(sd, sd.vertices)
        return sd, [("lbvh", own), ("refit", scr)], _target(own, scr)
    raise ValueError(name)


def same_vertex_trees():
    """Three trees over the scrambled teapots' vertices: the host SAH build, the LBVH restatement and the SAH tree of the unmoved
    scene refitted to them.  {name: SceneData}."""
    sd = _scene("teapots")
    v = scrambled_vertices(sd)
    sah = _with_vertices(sd, v)
    return {"sah": sah, "lbvh": _lbvh_target(sd, v), "refit": _target(sd, _with_vertices(sd, v))}


def case_rays(sd, n, seed):
    v = sd.vertices
    lo, hi = v.min(axis=0), v.max(axis=0)
    pad = 0.2 * (hi - lo) + 1e-3
    return random_rays(n, seed, tuple(lo - pad), tuple(hi + pad))


def brute_force(sd, rays):
    """(brute-force hits, mask of the rays whose winner is trustworthy: not a tie, not far).  A tie shows as a different winner when
    the triangles are tested in the reverse order (the strict < keeps the first of equal distances)."""
    from oracle import pyoracle

    b = pyoracle.OracleScene(sd).trace_closest(rays, naive=True)
    rev = _with_vertices(sd, sd.vertices.reshape(-1, 3, 3)[::-1].reshape(-1, 3))
    r = pyoracle.OracleScene(rev).trace_closest(rays, naive=True)
    n = sd.num_prims
    last = np.where(r["primId"] >= 0, n - 1 - r["primId"], -1)
    tie = last != b["primId"]
    v = sd.vertices
    far = (b["primId"] >= 0) & ~(b["t"] < 1e3 * float(np.linalg.norm(v.max(axis=0) - v.min(axis=0))))
    return b, ~(tie | far)


def primary_visit_histogram(sd, cam):
    """The oracle's per-ray visit counts of the G-buffer's primary rays as log2 buckets: counts[b] rays made [2^(b-1), 2^b) visits."""
    from oracle import pyoracle

    o = pyoracle.OracleScene(sd)
    lib = pyoracle.lib()
    lib.orc_debug_visit_hist.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.orc_debug_visit_hist.restype = None
    hist = np.zeros(6 * sd.bvh_size, np.uint32)
    rl = np.zeros(128, np.uint64)
    w, h = (int(x) for x in cam["resolution"])
    lib.orc_debug_visit_hist(o.h, hist.ctypes.data, rl.ctypes.data)
    try:
        o.gbuffer_render(cam, pyoracle.GBufferHost(w, h))
    finally:
        lib.orc_debug_visit_hist(o.h, None, None)
    assert rl[32:64].sum() == 0 and rl[0:32].sum() == w * h, "a G-buffer frame is one closest-hit ray per pixel"
    return rl[0:32]


# ---- the cases are what they claim ----

@pytest.mark.parametrize("name", CASES)
def test_case_tree_is_valid(name):
    from test_bvh_lbvh_cpu import check_tree

    sd, calls, target = tree_case(name)
    assert check_tree(target.boxes, target.nodes, target.num_prims) <= 59
    again = refit_model.refit_boxes(target.vertices, target.nodes)
    assert np.array_equal(again.view(np.uint32), target.boxes.view(np.uint32)), "the boxes are not the refit contract's"
    if name.startswith("lbvh") and name != "lbvh_refit":
        b, n = lbvh_model.build(calls[-1][1].vertices)
        assert np.array_equal(b.view(np.uint32), target.boxes.view(np.uint32))
    else:
        assert not np.array_equal(target.vertices, sd.vertices)


def test_scrambled_refit_makes_long_primary_walks():
    """The refitted tree of refit_scrambled sends some primary rays of the 61x43 test frame through more than 256 visits (the packet
    walk's budget, traverse.h kPacketBudget): the hand-over to per-lane walks happens without the test flag."""
    from radish_pt_amd import scenes

    _, _, target = tree_case("refit_scrambled")
    counts = primary_visit_histogram(target, scenes.teapots_camera(61, 43))
    assert counts[10:].sum() > 0, f"no primary ray made 512 visits or more: {counts.tolist()}"
    own = primary_visit_histogram(_scene("teapots"), scenes.teapots_camera(61, 43))
    assert np.flatnonzero(counts)[-1] > np.flatnonzero(own)[-1], "the scrambled refit should walk longer than the SAH build"


# ---- the oracle walks refitted trees like brute force ----

@pytest.mark.parametrize("name", REFIT_CASES)
def test_oracle_walks_refitted_trees_like_brute_force(name):
    from oracle import pyoracle

    _, _, target = tree_case(name)
    rays = case_rays(target, 3000, 7)
    a = pyoracle.OracleScene(target).trace_closest(rays)
    b, ok = brute_force(target, rays)
    assert (b["primId"][ok] >= 0).sum() >= 300, "too few hits to show anything"
    assert ok.mean() > 0.99, f"{name}: {np.count_nonzero(~ok)} of {len(ok)} rays excluded as ties or far"
    assert a[ok].tobytes() == b[ok].tobytes(), f"{name}: {np.count_nonzero(a[ok] != b[ok])} of {ok.sum()} hits differ"


# ---- a tree-free invariant: different trees of the same vertices give the same hits ----

def test_oracle_hits_agree_across_trees():
    from oracle import pyoracle

    trees = same_vertex_trees()
    ref = trees["sah"]
    for t in trees.values():
        assert np.array_equal(t.vertices, ref.vertices)
    assert not np.array_equal(trees["lbvh"].boxes, ref.boxes) and not np.array_equal(trees["refit"].boxes, ref.boxes)
    rays = case_rays(ref, 3000, 9)
    b, ok = brute_force(ref, rays)
    assert ok.mean() > 0.99, f"{np.count_nonzero(~ok)} of {len(ok)} rays excluded as ties or far"
    hits = {k: pyoracle.OracleScene(t).trace_closest(rays) for k, t in trees.items()}
    for k, h in hits.items():
        assert h[ok].tobytes() == hits["sah"][ok].tobytes(), f"{k} vs sah: {np.count_nonzero(h[ok] != hits['sah'][ok])} hits differ"
        assert h[ok].tobytes() == b[ok].tobytes(), f"{k} vs brute force"
    assert (b["primId"][ok] >= 0).mean() > 0.3
