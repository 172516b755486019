"""CPU checks of the LBVH builder (kernels_lbvh.h, RDH_BVH_LBVH): the entries and constants are declared and bound, the kernels
cross-compile for gfx950 within their budgets, the bottom-up hand-off keeps k_refit's lowering, and the numpy restatement of the
tree contract (lbvh_model.py) gives a valid tree that the oracle walks like brute force.  The device checks are in
test_gpu_bvh_lbvh.py."""
import os
import re
import shutil

import numpy as np
import pytest

import lbvh_model
import refit_model
from helpers import random_rays
from test_kernel_resources import HIPCC, _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_HIPCC = shutil.which(HIPCC) is not None or os.path.exists(HIPCC)


def test_entries_declared_and_bound():
    from radish_pt_amd import api

    header = open(os.path.join(ROOT, "include", "radish_hip.h")).read()
    for name in ("rdh_build_bvh_device_ex", "rdh_scene_update_geometry_ex"):
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in api.EXPORTS, name
    assert re.search(r"#define RDH_BVH_SAH 0\b", header) and re.search(r"#define RDH_BVH_LBVH 1\b", header)
    assert (api.RDH_BVH_SAH, api.RDH_BVH_LBVH) == (0, 1)
    import inspect

    for meth in ("build_bvh_device", "update_geometry"):
        assert inspect.signature(getattr(api.Context, meth)).parameters["builder"].default == "sah", meth


def test_library_exports_entries():
    from radish_pt_amd import api

    lib = api.lib()
    for name in ("rdh_build_bvh_device_ex", "rdh_scene_update_geometry_ex"):
        assert hasattr(lib, name), name
    assert lib.rdh_build_bvh_device_ex(None, None, 3, api.RDH_BVH_LBVH, None, None) == -1  # RDH_ERR_ARGS
    assert lib.rdh_scene_update_geometry_ex(None, None, None, None, api.RDH_BVH_LBVH) == -1


def test_unknown_builder_name_is_refused():
    from radish_pt_amd import api

    with pytest.raises(api.RadishError, match="builder"):
        api._builder("update_geometry", "ploc")


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_lbvh_kernels_budgets():
    res = _resources()
    # (mangled-name prefix, VGPR bound, waves per SIMD, scratch bytes per lane, LDS bytes)
    budgets = [
        ("_ZN2rd13k_lbvh_leaves", 32, 8, 0, 6144),
        ("_ZN2rd13k_lbvh_bounds", 32, 8, 0, 6144),
        ("_ZN2rd12k_lbvh_codes", 32, 8, 0, 0),
        ("_ZN2rd11k_lbvh_hist", 16, 8, 0, 1024),
        ("_ZN2rd11k_lbvh_scan", 32, 8, 0, 4096),
        ("_ZN2rd14k_lbvh_scatter", 32, 8, 0, 5120),
        ("_ZN2rd13k_lbvh_karras", 32, 8, 0, 0),
        ("_ZN2rd9k_lbvh_up", 40, 8, 0, 0),
        ("_ZN2rd12k_lbvh_place", 48, 8, 0, 0),
    ]
    for prefix, vgprs, waves, scratch, lds in budgets:
        hits = {k: v for k, v in res.items() if k.startswith(prefix)}
        assert hits, f"no kernel matches {prefix}"
        for name, r in hits.items():
            assert r["vgpr"] <= vgprs and r["occupancy"] >= waves, (name, r)
            assert r["scratch"] <= scratch and r["lds"] <= lds, (name, r)


def _kernel_isa(header, mangled):
    """gfx950 assembly of one kernel, from `header` compiled on its own with the library's flags."""
    import subprocess
    import tempfile

    from radish_pt_amd import _build

    flags = [f for f in _build.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "isa.hip")
        with open(src, "w") as f:
            f.write(f'#include <hip/hip_runtime.h>\n#include "device/{header}"\n')
        out = os.path.join(tmp, "isa.s")
        cmd = [HIPCC] + flags + ["--cuda-device-only", "-S", "-I", os.path.join(ROOT, "radish_pt_amd", "csrc"), src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(out).read()
    start = re.search(r"^" + re.escape(mangled) + r"\S*:", asm, re.M)
    assert start, f"{mangled} not found in the assembly"
    return asm[start.end():asm.index("s_endpgm", start.end())]


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_lbvh_up_handoff_lowering():
    """k_lbvh_up hands boxes from lane to lane exactly as k_refit does: sc1 stores of the box, a drain before
    every counter add, sc1 loads of the children's boxes, and no cache maintenance."""
    isa = _kernel_isa("kernels_lbvh.h", "_ZN2rd9k_lbvh_upE")
    lines = [ln.strip() for ln in isa.splitlines() if ln.strip() and not ln.strip().startswith(";")]
    stores_sc1 = [ln for ln in lines if re.match(r"global_store_dword\s", ln) and ln.endswith("sc1")]
    loads_sc1 = [ln for ln in lines if re.match(r"global_load_dword\s", ln) and ln.endswith("sc1")]
    assert len(stores_sc1) >= 12, f"the node's box must be stored write-through (sc1), leaf and climb: {stores_sc1}"
    assert len(loads_sc1) >= 12, f"the children's boxes must be loaded with sc1: {loads_sc1}"
    assert not any(ln.startswith(("buffer_wbl2", "buffer_inv")) for ln in lines), "k_lbvh_up should need no cache maintenance"
    atomics = [i for i, ln in enumerate(lines) if ln.startswith("global_atomic_add")]
    assert atomics, "no arrival counter add"
    for i in atomics:
        drains = [j for j in range(i) if lines[j].startswith("s_waitcnt") and "vmcnt(0)" in lines[j]]
        assert drains, "no vmcnt(0) before the counter add"
        between = lines[drains[-1] + 1:i]
        assert not any(ln.startswith(("global_store", "buffer_store", "flat_store")) or ln.startswith("s_cbranch") or ln.endswith(":")
                       for ln in between), f"a store or a branch target between the drain and the add: {between}"


# ---- the restatement ----

def _coincident():
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    return np.tile(tri, (4096, 1))


def _zero_width():
    v = refit_model.soup(5000, 7)
    v[:, 1] = 0.25
    return v


def _magnitudes():
    rng = np.random.default_rng(11)
    scale = np.repeat(10.0 ** rng.uniform(-3, 3, (20000, 1, 1)), 3, axis=1).reshape(-1, 1)
    return (refit_model.soup(20000, 12) * scale).astype(np.float32)


def case_vertices(name):
    """The inputs the LBVH tests share (CPU and GPU)."""
    from radish_pt_amd import scenes

    if name == "cornell":
        return scenes.cornell().vertices
    if name == "teapots":
        return scenes.teapots().vertices
    if name == "coincident4096":
        return _coincident()
    if name == "zero_width":
        return _zero_width()
    if name == "signed_zeros":
        return refit_model.signed_zeros_soup(np.random.default_rng(3))
    if name == "magnitudes":
        return _magnitudes()
    if name.startswith("soup"):
        n = int(name[4:])
        return refit_model.soup(n, n)
    raise ValueError(name)


CASES = ["cornell", "teapots", "soup1", "soup2", "soup3", "soup17", "soup100003", "coincident4096", "zero_width", "signed_zeros",
         "magnitudes"]


def check_tree(boxes, nodes, n):
    """Every primitive in exactly one leaf; the six orderings are pre-orders of one binary tree (same nodes, same children, same
    leaves; only the order of the two children differs); returns the deepest leaf's depth in edges."""
    S = 2 * n - 1
    assert boxes.shape == (S, 6)
    kids = None
    for k in range(6):
        a = nodes[k]
        prim = a["primitiveId"].astype(np.int64)
        slot = a["boundingBoxId"].astype(np.int64)
        nxt = a["nextNodeIfMiss"].astype(np.int64)
        assert len(a) == S
        assert np.array_equal(np.sort(slot), np.arange(S)), f"ordering {k}: slots are not a permutation"
        assert slot[0] == 0 and nxt[0] == S, f"ordering {k}: the root"
        leaf = prim >= 0
        assert np.array_equal(np.sort(prim[leaf]), np.arange(n)), f"ordering {k}: a primitive not in exactly one leaf"
        p = np.arange(S)
        assert np.all(nxt[leaf] == p[leaf] + 1), f"ordering {k}: leaf miss links"
        inner = np.flatnonzero(~leaf)
        assert np.all(inner + 1 < S)
        second = nxt[inner + 1]
        assert np.all((second > inner + 1) & (second < S)) and np.all(nxt[second] == nxt[inner]), f"ordering {k}: inner miss links"
        by_slot = np.full((S, 4), -1, np.int64)  # prim, subtree size, the smaller and larger child slot
        by_slot[slot, 0] = prim
        by_slot[slot, 1] = nxt - p
        c1, c2 = slot[inner + 1], slot[second]
        by_slot[slot[inner], 2] = np.minimum(c1, c2)
        by_slot[slot[inner], 3] = np.maximum(c1, c2)
        if kids is None:
            kids = by_slot
        else:
            assert np.array_equal(by_slot, kids), f"ordering {k} is not an ordering of ordering 0's tree"
    return lbvh_model.depth(nodes[0]) - 1


@pytest.mark.parametrize("name", CASES)
def test_restatement_gives_a_valid_tree(name):
    v = case_vertices(name)
    n = len(v) // 3
    boxes, nodes = lbvh_model.build(v)
    assert check_tree(boxes, nodes, n) <= 59
    # step 8: each inner box is the union of its children's boxes (the refit contract), so a refit leaves the tree as built
    again = refit_model.refit_boxes(v, nodes)
    assert np.array_equal(again.view(np.uint32), boxes.view(np.uint32)), "the boxes are not the refit contract's"


def test_coincident_triangles_make_a_balanced_tree():
    boxes, nodes = lbvh_model.build(_coincident())
    assert lbvh_model.depth(nodes[0]) - 1 == 12, "4 096 equal codes: a tree of 12 levels (index bits break the ties)"


def test_one_triangle_is_a_leaf_root():
    v = refit_model.soup(1, 1)
    boxes, nodes = lbvh_model.build(v)
    for k in range(6):
        assert nodes[k].tolist() == [(0, 0, 1)]
    assert np.array_equal(boxes[0], lbvh_model.leaf_boxes(v)[0])


def test_codes_follow_the_contract():
    """Step 3's corner cases: the centroid bound's low corner is cell 0, the high corner cell 1023, a zero-width axis cell 0."""
    v = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [2, 5, 0], [2, 5, 0], [2, 5, 0], [1, 2.5, 0], [1, 2.5, 0], [1, 2.5, 0]], np.float32)
    c = lbvh_model.morton_codes(v)
    assert c[0] == 0
    assert c[1] == (lbvh_model._spread(np.array([1023]))[0] << 2) | (lbvh_model._spread(np.array([1023]))[0] << 1)
    assert c[2] == (lbvh_model._spread(np.array([512]))[0] << 2) | (lbvh_model._spread(np.array([512]))[0] << 1)


def _scene_with_tree(v, boxes, nodes):
    from radish_pt_amd import scenes

    base = scenes.tiny()
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    n = v.shape[0] // 3
    sd = scenes.SceneData("lbvh", v, np.tile(base.normals[:3], (n, 1)), np.tile(base.texcoords[:3], (n, 1)),
                          np.full(n, base.material_ids[0], np.int32), base.materials)
    sd.boxes, sd.nodes = boxes, nodes
    return sd


# Not the zero-width and signed-zeros soups: their triangles overlap in one plane, so most closest hits are ties that any walk
# order settles its own way (the host builder's tree disagrees with brute force there as often).  check_tree covers them.
@pytest.mark.parametrize("name", ["cornell", "teapots", "soup300", "soup3000", "magnitudes"])
def test_oracle_walks_the_restated_tree_like_brute_force(name):
    from oracle import pyoracle

    v = case_vertices(name)
    boxes, nodes = lbvh_model.build(v)
    sd = _scene_with_tree(v, boxes, nodes)
    o = pyoracle.OracleScene(sd)
    lo, hi = v.min(axis=0), v.max(axis=0)
    pad = 0.2 * (hi - lo) + 1e-3
    rays = random_rays(3000, 5, tuple(lo - pad), tuple(hi + pad))
    a = o.trace_closest(rays)
    b = o.trace_closest(rays, naive=True)
    assert (b["primId"] >= 0).sum() >= 20, "too few hits to show anything"
    # A ray with a 1e-7 direction component can hit a triangle millions of units away, where the box test's own rounding decides
    # (the host builder's tree misses the same hits on Cornell): compare the rays whose brute-force hit, if any, is near.
    near = (b["primId"] < 0) | (b["t"] < 1e3 * float(np.linalg.norm(hi - lo)))
    assert near.mean() > 0.99
    assert a[near].tobytes() == b[near].tobytes(), f"{name}: {np.count_nonzero(a[near] != b[near])} of {near.sum()} hits differ"
