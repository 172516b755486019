"""Resources of k_wf_trace_primary (kernels_wave.h; CPU test: hipcc cross-compiles gfx950 and reports them), in the manner of
test_kernel_resources.py, and what adding it must not move: the k_wf_trace instantiations' budgets stated there.

The packet walk is a chain of dependent scalar loads, one node at a time per wave, that many resident waves hide; k_walk_packet runs at
eight waves per SIMD (64 VGPRs).  With the workgroup trace of the literal-class list in the same kernel the compiler takes 68: seven
waves, no scratch.  Held to eight waves it spills 28 bytes per lane and stage 0 of the teapots 1080p frame measures the same (275-299 us
against 280-298: profiles/wf_primary_packets/), so the kernel is pinned where it is: at most 72 VGPRs, seven waves, no scratch, and
the 8 KB of LDS of one WgTraceSharedT<256>, which leaves room for more workgroups per CU than seven waves per SIMD fill."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_primary_packet_kernel_and_the_trace_kernels_it_stands_beside():
    res = _resources()

    def one(prefix):
        hits = {k: v for k, v in res.items() if k.startswith(prefix)}
        assert hits, f"no kernel matches {prefix}"
        return hits

    for name, r in one("_ZN2rd18k_wf_trace_primaryILb0E").items():
        print(name, r)
        assert r["vgpr"] <= 72 and r["occupancy"] >= 7, (name, r, "budget 72 VGPRs / 7 waves per SIMD")
        assert r["scratch"] == 0, (name, r, "spills to scratch")
        assert r["lds"] <= 8448, (name, r, "one WgTraceSharedT<256> and nothing else")
    for name, r in one("_ZN2rd18k_wf_trace_primaryILb1E").items():  # the counting variant (tests only): no scratch either
        assert r["scratch"] == 0, (name, r)
    # the budgets of tests/test_kernel_resources.py for the kernel this one is launched instead of at k = 0
    for prefix, vgprs, waves in (("_ZN2rd10k_wf_traceILb0ELb0E", 72, 7), ("_ZN2rd10k_wf_traceILb0ELb1E", 80, 6)):
        for name, r in one(prefix).items():
            assert r["vgpr"] <= vgprs and r["occupancy"] >= waves and r["scratch"] == 0, (name, r, f"budget {vgprs} VGPRs / {waves} waves per SIMD")
    for name, r in one("_ZN2rd10k_wf_shadeE").items():
        assert r["vgpr"] <= 168 and r["occupancy"] >= 3 and r["scratch"] == 0, (name, r)
