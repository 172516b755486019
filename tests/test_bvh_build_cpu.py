"""CPU checks of the device BVH builder (kernels_bvh.h): its kernels cross-compile for gfx950 within their register / LDS
budgets, and the new entries are declared and bound.  The bit-exactness tests are in test_gpu_bvh_build.py."""
import os
import re
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_declared_and_bound():
    from radish_pt_amd import api

    header = open(os.path.join(ROOT, "include", "radish_hip.h")).read()
    for name in ("rdh_build_bvh_device", "rdh_scene_update_geometry", "rdh_debug_read_tree"):
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in api.EXPORTS, name
    assert "typedef struct rdh_light_update" in header
    assert [f[0] for f in api.LightUpdateC._fields_] == ["lightSampler", "lightSamplerLength", "sumLightPowerInv"]
    for meth in ("build_bvh_device", "update_geometry", "debug_read_tree"):
        assert callable(getattr(api.Context, meth)), meth


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_builder_kernels_budgets():
    res = _resources()
    # (mangled-name prefix, VGPR bound, waves per SIMD, scratch bytes per lane, LDS bytes).  k_bvh_build: thread 0's child jobs
    # (indexed by which child goes first) live in scratch; one lane per workgroup touches it.
    budgets = [
        ("_ZN2rd11k_bvh_build", 168, 3, 256, 4096),
        ("_ZN2rd10k_bvh_init", 32, 8, 0, 0),
        ("_ZN2rd14k_bvh_noderecs", 32, 8, 0, 0),
        ("_ZN2rd11k_bvh_pairs", 32, 8, 0, 0),
        ("_ZN2rd13k_geom_update", 32, 8, 0, 0),
    ]
    for prefix, vgprs, waves, scratch, lds in budgets:
        hits = {k: v for k, v in res.items() if k.startswith(prefix)}
        assert hits, f"no kernel matches {prefix}"
        for name, r in hits.items():
            assert r["vgpr"] <= vgprs and r["occupancy"] >= waves, (name, r)
            assert r["scratch"] <= scratch and r["lds"] <= lds, (name, r)
