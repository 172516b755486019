"""Adaptive sampling without a GPU (rdh_path_trace_adaptive, rdh_adaptive_plan): the exports, declarations and Python
entries, the resources of the new kernels, and the numpy model (tests/adaptive_model.py) that tests/test_gpu_adaptive.py holds the
kernels to — the finish fold with its moments, the plan rule, the slot layout."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import adaptive_model as am
from helpers import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# The threshold of the GPU plan test (tests/test_gpu_adaptive.py) is am.PLAN_THRESHOLD = 0.15, fixed on the oracle alone: the model
# marks 19 of the 35 blocks of the 52x36 Cornell frame active (54 %) on the oracle's own moments after 8 samples, 292 of 1 872 pixels
# wanting (test_plan_threshold_splits_the_oracle_frame).
PLAN_THRESHOLD = am.PLAN_THRESHOLD
PLAN_W, PLAN_H, PLAN_DEPTH, PLAN_LOOPER, PLAN_SAMPLES = 52, 36, 4, 9998, 8


def test_library_exports_the_entries():
    from radish_pt_amd import api

    lib = ctypes.CDLL(api.HIP_LIB_PATH)  # loads without a GPU; no compute call is made
    for name in ("rdh_path_trace_adaptive", "rdh_adaptive_plan"):
        assert name in api.EXPORTS
        assert hasattr(lib, name)


def test_header_declares_the_entries():
    with open(os.path.join(ROOT, "include", "radish_hip.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    assert ("int rdh_path_trace_adaptive(rdh_ctx *ctx, float *d_directIllum, float *d_indirectIllum, int32_t *d_sampleCount, "
            "const int32_t *d_request, float *d_moments, int looper, int maxDepth, uint32_t flags, int64_t *samplesTraced);") in text
    assert ("typedef struct rdh_adaptive_stats { int64_t samplesRequested; int32_t activeBlocks; int32_t wantingPixels; } "
            "rdh_adaptive_stats;") in text
    assert ("int rdh_adaptive_plan(rdh_ctx *ctx, const int32_t *d_sampleCount, const float *d_moments, int32_t *d_request, "
            "int minSamples, int maxSamples, int step, float threshold, rdh_adaptive_stats *out);") in text
    assert "#define RDH_ADAPTIVE_MAX_REQUEST 16" in text


def test_python_entries_exist():
    from radish_pt_amd import api

    sig = inspect.signature(api.Context.path_trace_adaptive)
    assert list(sig.parameters) == ["self", "direct", "indirect", "counts", "requests", "looper", "max_depth", "flags", "moments"]
    assert sig.parameters["moments"].default is None
    assert list(inspect.signature(api.Context.adaptive_plan).parameters) == [
        "self", "counts", "moments", "requests", "min_samples", "max_samples", "step", "threshold"]
    assert list(inspect.signature(api.Context.converge).parameters) == [
        "self", "direct", "indirect", "counts", "moments", "looper", "max_depth", "flags", "min_samples", "max_samples", "step",
        "threshold", "max_passes"]
    assert ctypes.sizeof(api.AdaptiveStatsC) == 16 and api.RDH_ADAPTIVE_MAX_REQUEST == am.MAX_REQUEST == 16


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_new_kernels_use_no_scratch():
    """kernels_adaptive.h compiled from a one-line translation unit with the library's flags, in the manner of test_samples_cpu.py.
    The list raygen, the finish (its sample loop carries running means, not an array) and the plan kernel may not spill; the two
    kernels of the wavefront pipeline that know a pixel stay one symbol each (the new ones have names of their own)."""
    from radish_pt_amd import _build

    flags = [f for f in _build.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "adaptive_only.hip")
        with open(src, "w") as f:
            f.write('#include "device/kernels_adaptive.h"\n')
        cmd = [HIPCC] + flags + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "radish_pt_amd", "csrc"), "-c", src,
                                 "-o", os.path.join(tmp, "x.o"), "-Rpass-analysis=kernel-resource-usage"]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split("\n")[0].split(" ")[0].strip()
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        res[name] = {"vgpr": get("VGPRs"), "scratch": get(r"ScratchSize \[bytes/lane\]"), "lds": get(r"LDS Size \[bytes/block\]")}
    for prefix in ("_ZN2rd11k_ad_raygenE", "_ZN2rd11k_ad_finishE", "_ZN2rd9k_ad_planE", "_ZN2rd10k_ad_countE", "_ZN2rd12k_ad_scatterE",
                   "_ZN2rd9k_ad_scanE"):
        hits = {k: v for k, v in res.items() if k.startswith(prefix)}
        assert len(hits) == 1, (prefix, sorted(res))
        for name, r in hits.items():
            print(name, r)
            assert r["scratch"] == 0, (name, r)
    for prefix in ("_ZN2rd11k_wf_raygenE", "_ZN2rd11k_wf_finishE"):
        assert len([k for k in res if k.startswith(prefix)]) == 1, (prefix, sorted(res))


# ---- the finish fold ---------------------------------------------------------------------------------------------------------
def test_fold_equals_successive_single_sample_updates():
    """Uneven requests over uneven counts: the fold of a pixel's r samples is r updates of that pixel alone, each at its own iter;
    pixels without a request keep every plane."""
    rng = np.random.default_rng(7)
    P, K = 500, 24
    sd = (rng.uniform(0, 1, (K, P, 3)) ** 3).astype(np.float32)
    si = (rng.uniform(0, 1, (K, P, 3)) ** 3).astype(np.float32)
    count = rng.integers(0, 8, P).astype(np.int32)
    request = rng.integers(0, 17, P).astype(np.int32)
    request[rng.choice(P, 100, replace=False)] = 0
    d0, i0 = rng.uniform(0, 1, (P, 3)).astype(np.float32), rng.uniform(0, 1, (P, 3)).astype(np.float32)
    m0 = rng.uniform(0, 1, (P, 2)).astype(np.float32)
    d, i, c, m = am.fold(d0.copy(), i0.copy(), count.copy(), m0.copy(), sd, si, request)
    for p in range(P):
        ed, ei, em = d0[p].copy(), i0[p].copy(), m0[p].copy()
        for j in range(request[p]):
            n = int(count[p]) + j
            ed = (ed * np.float32(n) + sd[n, p]) / np.float32(n + 1)
            ei = (ei * np.float32(n) + si[n, p]) / np.float32(n + 1)
            s = sd[n, p] + si[n, p]
            L = np.float32(np.float32(np.float32(0.2126) * s[0] + np.float32(0.7152) * s[1]) + np.float32(0.0722) * s[2])
            em = np.array([(em[0] * np.float32(n) + L) / np.float32(n + 1), (em[1] * np.float32(n) + L * L) / np.float32(n + 1)], np.float32)
        assert_bit_equal(d[p], ed, f"direct of pixel {p}")
        assert_bit_equal(i[p], ei, f"indirect of pixel {p}")
        assert_bit_equal(m[p], em, f"moments of pixel {p}")
    assert np.array_equal(c, count + request)
    assert d.dtype == i.dtype == m.dtype == np.float32


# ---- the slot layout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(52, 36), (1, 1), (130, 70)])
def test_slot_layout(W, H):
    rng = np.random.default_rng(W * 1000 + H)
    request = rng.integers(0, 17, W * H).astype(np.int32)
    request[rng.choice(W * H, W * H // 3, replace=False)] = 0
    order = am.work_order(W, H)
    assert sorted(order[order >= 0]) == list(range(W * H))  # every pixel once
    assert len(order) % 64 == 0
    base, owner, total = am.slot_layout(request, W, H)
    assert total == int(request.sum()) == len(owner)
    work, j = owner >> am.OWNER_SHIFT, owner & (am.MAX_REQUEST - 1)
    assert (np.diff(work) >= 0).all()  # pixel-major inside work (block) order
    assert (order[work] >= 0).all()
    for w_ in np.unique(work):  # a pixel's slots are neighbours, j = 0 .. r - 1 in order, starting at its slotBase
        at = np.flatnonzero(work == w_)
        assert at[0] == base[w_] and list(j[at]) == list(range(request[order[w_]])) and list(at) == list(range(at[0], at[0] + len(at)))
    # a block's pixels follow each other: the slots of one 8x8 block are one interval
    blocks = work >> 6
    assert (np.diff(blocks) >= 0).all()


# ---- the plan ----------------------------------------------------------------------------------------------------------------
def test_plan_on_hand_made_planes():
    W, H = am.HAND_W, am.HAND_H
    count, m = am.hand_made_planes()
    request, stats = am.plan(count, m, W, H, **am.HAND_PARAMS)
    r = request.reshape(H, W)
    w = am.wants(count, m, am.HAND_PARAMS["min_samples"], am.HAND_PARAMS["threshold"]).reshape(H, W)
    assert w[0:8, 0:8].all() and (r[0:8, 0:8] == 4).all()                      # n below the minimum
    assert w[0:8, 8:16].all()                                                  # n at and above the maximum: wanting, but nothing given
    assert (r[0:7, 8:16] == 0).all() and (r[7, 8:16] == 2).all()               # ... and min(step, max - n) below it
    assert not w[0:8, 16:24].any() and (r[0:8, 16:24] == 0).all()              # zero mean, no variance
    assert w[0:8, 24:32].sum() == 1 and w[3, 27] and (r[0:8, 24:32] == 2).all()  # zero mean: one wanting pixel carries its block
    assert not w[0:8, 32:40].any() and (r[0:8, 32:40] == 0).all()              # negative var
    assert not w[0:8, 40:48].any() and (r[0:8, 40:48] == 0).all()              # NaN moments
    assert w[0:8, 48:52].sum() == 1 and (r[0:8, 48:52] == 3).all()             # ragged column: 4 x 8 pixels
    assert w[32:36, 48:52].sum() == 1 and (r[32:36, 48:52] == 3).all()         # ragged corner: 4 x 4 pixels
    assert (r[8:32] == 0).all() and (r[32:36, 0:48] == 0).all()
    assert stats == {"samplesRequested": 64 * 4 + 8 * 2 + 64 * 2 + 32 * 3 + 16 * 3, "activeBlocks": 5, "wantingPixels": 64 + 64 + 1 + 1 + 1}


def test_plan_threshold_splits_the_oracle_frame(cornell_small):
    """A plan that selects everything or nothing pins nothing: on the oracle's own 8-sample moments of the GPU test's frame the
    model must call between 20 % and 80 % of the blocks active at PLAN_THRESHOLD (measured: 19 of 35, 54 %)."""
    import adaptive_oracle as ao
    from radish_pt_amd import scenes

    cam = scenes.cornell_camera(PLAN_W, PLAN_H)
    fr = ao.frames(cornell_small, cam, PLAN_LOOPER, PLAN_SAMPLES, PLAN_DEPTH)
    counts = np.full(PLAN_W * PLAN_H, PLAN_SAMPLES, np.int32)
    m = ao.moments_after(fr, counts)
    _, stats = am.plan(counts, m, PLAN_W, PLAN_H, 4, 64, 4, PLAN_THRESHOLD)
    share = stats["activeBlocks"] / 35
    print(stats, share)
    assert 0.2 <= share <= 0.8, stats
    assert stats == {"samplesRequested": 4608, "activeBlocks": 19, "wantingPixels": 292}  # the measured share, pinned
