"""CPU checks of the refit (kernels_refit.h, rdh_scene_refit_geometry / rdh_scene_tree_cost): the entries are declared and bound,
the kernels cross-compile for gfx950 within their budgets, and the numpy restatement of the refit contract (refit_model.py)
gives the host builder's boxes from the unmoved vertices.  The device checks are in test_gpu_bvh_refit.py."""
import os
import re
import shutil

import numpy as np
import pytest

import refit_model
from test_kernel_resources import HIPCC, _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_declared_and_bound():
    from radish_pt_amd import api

    header = open(os.path.join(ROOT, "include", "radish_hip.h")).read()
    for name in ("rdh_scene_refit_geometry", "rdh_scene_tree_cost"):
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in api.EXPORTS, name
    for meth in ("refit_geometry", "tree_cost"):
        assert callable(getattr(api.Context, meth)), meth


def test_library_exports_entries():
    from radish_pt_amd import api

    lib = api.lib()
    for name in ("rdh_scene_refit_geometry", "rdh_scene_tree_cost"):
        assert hasattr(lib, name), name
    assert lib.rdh_scene_refit_geometry(None, None, None, None) == -1  # RDH_ERR_ARGS
    assert lib.rdh_scene_tree_cost(None, None, None) == -1  # RDH_ERR_ARGS


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_refit_kernels_budgets():
    res = _resources()
    # (mangled-name prefix, VGPR bound, waves per SIMD, scratch bytes per lane, LDS bytes)
    budgets = [
        ("_ZN2rd7k_refitE", 48, 8, 0, 0),
        ("_ZN2rd13k_refit_links", 32, 8, 0, 0),
        ("_ZN2rd13k_refit_count", 16, 8, 0, 64),
        ("_ZN2rd12k_refit_scan", 32, 8, 0, 1088),
        ("_ZN2rd14k_refit_number", 32, 8, 0, 64),
        ("_ZN2rd18k_refit_plan_climb", 32, 8, 0, 0),
        ("_ZN2rd13k_refit_check", 40, 8, 0, 0),
        ("_ZN2rd19k_tree_cost_partial", 32, 8, 0, 2048),
        ("_ZN2rd17k_tree_cost_final", 32, 8, 0, 2048),
    ]
    for prefix, vgprs, waves, scratch, lds in budgets:
        hits = {k: v for k, v in res.items() if k.startswith(prefix)}
        assert hits, f"no kernel matches {prefix}"
        for name, r in hits.items():
            assert r["vgpr"] <= vgprs and r["occupancy"] >= waves, (name, r)
            assert r["scratch"] <= scratch and r["lds"] <= lds, (name, r)


def _signed_zeros():
    return refit_model.signed_zeros_soup(np.random.default_rng(3))


def _zero_width():
    v = refit_model.soup(5000, 7)
    v[:, 1] = 0.25
    return v


def _case(name):
    from radish_pt_amd import scenes

    if name == "cornell":
        return scenes.cornell().vertices
    if name == "teapots":
        return scenes.teapots().vertices
    if name == "zero_width":
        return _zero_width()
    if name == "signed_zeros":
        return _signed_zeros()
    n = int(name.split("_")[1])
    return refit_model.soup(n, n)


@pytest.mark.parametrize("name", ["cornell", "teapots", "soup_1", "soup_2", "soup_17", "soup_20000", "zero_width"])
def test_restatement_reproduces_builder_boxes(name):
    from radish_pt_amd import hostlib

    v = _case(name)
    boxes, nodes = hostlib.build_bvh(v)
    got = refit_model.refit_boxes(v, nodes)
    assert np.array_equal(got.view(np.uint32), boxes.view(np.uint32)), f"{name}: {np.argwhere(got.view(np.uint32) != boxes.view(np.uint32))[:3]}"


def test_restatement_signed_zeros_equal_in_value():
    """The builder folds each node over its primitives in the order they held BEFORE that node's partition, which interleaves
    the two children's primitives; with keep-first-on-tie folds the sign of a zero follows that order, which no bottom-up
    combination of the children's boxes can see.  Values agree; only signs of zero may differ."""
    from radish_pt_amd import hostlib

    v = _signed_zeros()
    boxes, nodes = hostlib.build_bvh(v)
    got = refit_model.refit_boxes(v, nodes)
    assert np.array_equal(got, boxes)
    differ = got.view(np.uint32) != boxes.view(np.uint32)
    assert np.all((got[differ] == 0) & (boxes[differ] == 0))


def test_restatement_follows_moved_vertices():
    """Moving one triangle changes exactly the boxes on its path to the root, and each is the union of its children's."""
    from radish_pt_amd import hostlib

    v = refit_model.soup(500, 5)
    boxes, nodes = hostlib.build_bvh(v)
    moved = v.copy()
    moved[3 * 17:3 * 18] += np.float32(3.0)
    got = refit_model.refit_boxes(moved, nodes)
    changed = np.flatnonzero(np.any(got != boxes, axis=1))
    n0 = nodes[0]
    leaf_pos = int(np.flatnonzero(n0["primitiveId"] == 17)[0])
    path = {int(n0["boundingBoxId"][p]) for p in range(len(n0)) if p <= leaf_pos < n0["nextNodeIfMiss"][p]}
    assert set(changed.tolist()) <= path and 0 in changed
    assert refit_model.tree_cost(got) != refit_model.tree_cost(boxes)


def test_cost_of_a_degenerate_root_is_the_node_count():
    from radish_pt_amd import hostlib

    v = np.zeros((3 * 50, 3), np.float32)
    v[:, 0] = np.arange(3 * 50, dtype=np.float32) * np.float32(0.01)  # every triangle on the x axis: zero-area boxes throughout
    boxes, _ = hostlib.build_bvh(v)
    assert refit_model.tree_cost(boxes) == float(len(boxes))


def _refit_isa():
    """gfx950 assembly of k_refit, from kernels_refit.h compiled on its own with the library's flags."""
    import subprocess
    import tempfile

    from radish_pt_amd import _build

    flags = [f for f in _build.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "refit_isa.hip")
        with open(src, "w") as f:
            f.write('#include <hip/hip_runtime.h>\n#include "device/kernels_refit.h"\n')
        out = os.path.join(tmp, "refit_isa.s")
        cmd = [HIPCC] + flags + ["--cuda-device-only", "-S", "-I", os.path.join(ROOT, "radish_pt_amd", "csrc"), src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(out).read()
    start = re.search(r"^_ZN2rd7k_refitE\S*:", asm, re.M)
    assert start, "k_refit not found in the assembly"
    return asm[start.end():asm.index("s_endpgm", start.end())]


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_refit_handoff_lowering():
    """k_refit's hand-off rests on how the compiler lowers relaxed agent-scope atomics for gfx950 (the AMDGPU memory
    model's GFX942 code sequences): stores and loads with sc1, no cache maintenance.  Pin that lowering, so that a compiler that
    changes it fails here instead of in a frame."""
    isa = _refit_isa()
    lines = [ln.strip() for ln in isa.splitlines() if ln.strip() and not ln.strip().startswith(";")]
    stores_sc1 = [ln for ln in lines if re.match(r"global_store_dword\s", ln) and ln.endswith("sc1")]
    loads_sc1 = [ln for ln in lines if re.match(r"global_load_dword\s", ln) and ln.endswith("sc1")]
    assert len(stores_sc1) >= 12, f"ordering 0's box must be stored write-through (sc1), leaf and climb: {stores_sc1}"
    assert len(loads_sc1) >= 12, f"the children's boxes must be loaded with sc1: {loads_sc1}"
    assert not any(ln.startswith(("buffer_wbl2", "buffer_inv")) for ln in lines), "k_refit should need no cache maintenance"
    atomics = [i for i, ln in enumerate(lines) if ln.startswith("global_atomic_add")]
    assert atomics, "no arrival counter add"
    for i in atomics:  # every counter add sits behind a drain with no store after it (the climb loops back above the drain)
        drains = [j for j in range(i) if lines[j].startswith("s_waitcnt") and "vmcnt(0)" in lines[j]]
        assert drains, "no vmcnt(0) before the counter add"
        between = lines[drains[-1] + 1:i]
        assert not any(ln.startswith(("global_store", "buffer_store", "flat_store")) or ln.startswith("s_cbranch") or ln.endswith(":")
                       for ln in between), f"a store or a branch target between the drain and the add: {between}"
