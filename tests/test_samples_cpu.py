"""rdh_path_trace_samples without a GPU: the export, the declaration, the Python entry, the resources of the two kernels that
know what a slot's pixel is (k_wf_raygen, k_wf_finish), and the arithmetic of the finish fold."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from helpers import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_library_exports_the_entry():
    from radish_pt_amd import api

    assert "rdh_path_trace_samples" in api.EXPORTS
    lib = ctypes.CDLL(api.HIP_LIB_PATH)  # loads without a GPU; no compute call is made
    assert hasattr(lib, "rdh_path_trace_samples")


def test_header_declares_the_entry():
    with open(os.path.join(ROOT, "include", "radish_hip.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    assert ("int rdh_path_trace_samples(rdh_ctx *ctx, float *d_directIllum, float *d_indirectIllum, int iter, int looper, "
            "int numSamples, int samplesPerPass, int maxDepth, uint32_t flags);") in text


def test_python_entries_exist():
    import inspect

    from radish_pt_amd import api

    params = list(inspect.signature(api.Context.path_trace_samples).parameters)
    assert params == ["self", "direct", "indirect", "iter", "looper", "samples", "max_depth", "flags", "samples_per_pass"]
    assert inspect.signature(api.Context.path_trace_samples).parameters["samples_per_pass"].default == 0
    assert list(inspect.signature(api.pathTraceSamples).parameters) == ["directIllum", "indirectIllum", "iter", "samples"]


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_raygen_and_finish_use_no_scratch():
    """kernels_wave.h compiled from a one-line translation unit with the library's flags, in the manner of
    test_pose_kernel_resources.py: the same header and flags, hence the same code for these kernels.  Neither may spill (the
    sample loop of k_wf_finish carries two running means, not an array), and neither needs LDS."""
    from radish_pt_amd import _build

    flags = [f for f in _build.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "wave_only.hip")
        with open(src, "w") as f:
            f.write('#include "device/kernels_wave.h"\n')
        cmd = [HIPCC] + flags + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "radish_pt_amd", "csrc"), "-c", src,
                                 "-o", os.path.join(tmp, "x.o"), "-Rpass-analysis=kernel-resource-usage"]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split("\n")[0].split(" ")[0].strip()
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        res[name] = {"vgpr": get("VGPRs"), "scratch": get(r"ScratchSize \[bytes/lane\]"), "occupancy": get(r"Occupancy \[waves/SIMD\]"),
                     "lds": get(r"LDS Size \[bytes/block\]")}
    for prefix in ("_ZN2rd11k_wf_raygenE", "_ZN2rd11k_wf_finishE"):
        hits = {k: v for k, v in res.items() if k.startswith(prefix)}
        assert len(hits) == 1, (prefix, sorted(res))
        for name, r in hits.items():
            print(name, r)
            assert r["scratch"] == 0 and r["lds"] == 0, (name, r)


# ---- the finish fold (k_wf_finish, foldRunningMean) restated in numpy float32 ----------------------------------------------
def _scrub_ldr(v):
    """hasNanOrInf -> 0 for the whole pixel, then HDRToLDR: c / (c + 1) * 1 (pathtrace.cu:279-286)."""
    v = np.where(np.isfinite(v).all(axis=1, keepdims=True), v, np.float32(0)).astype(np.float32)
    return v / (v + np.float32(1)) * np.float32(1)


def _update(img, v, it):
    """storeRunningMean: (img * float(iter) + v) / float(iter + 1)"""
    return (img * np.float32(it) + v) / np.float32(it + 1)


def _fold(img, samples, it0):
    """One thread per pixel: load once, B updates in sample order, store once."""
    mean = img.copy()  # the load
    for b, v in enumerate(samples):
        mean = _update(mean, _scrub_ldr(v), it0 + b)
    img[...] = mean  # the store
    return img


@pytest.mark.parametrize("it0", [0, 1, 3, 4095])
@pytest.mark.parametrize("B", [1, 2, 3, 5, 16])
def test_finish_fold_equals_successive_updates(B, it0):
    rng = np.random.default_rng(1000 * B + it0)
    n = 4096
    img0 = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    img0[rng.choice(n, 16, replace=False), rng.integers(0, 3, 16)] = np.nan  # what an earlier frame may have left
    samples = (rng.uniform(0, 1, (B, n, 3)) ** 4 * 50).astype(np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        samples[rng.integers(0, B, 64), rng.choice(n, 64, replace=False), rng.integers(0, 3, 64)] = bad
    samples[rng.integers(0, B, 64), rng.choice(n, 64, replace=False)] = 0
    with np.errstate(all="ignore"):
        folded = _fold(img0.copy(), samples, it0)
        looped = img0.copy()
        for b in range(B):  # B single-sample launches: each loads the image and stores it
            looped[...] = _update(looped.copy(), _scrub_ldr(samples[b]), it0 + b)
    assert folded.dtype == np.float32 and looped.dtype == np.float32
    assert_bit_equal(folded, looped, f"B={B} iter={it0}")
    scrubbed = ~np.isfinite(samples).all(axis=2)
    assert scrubbed.any() and np.isfinite(_scrub_ldr(samples.reshape(-1, 3))).all()
    if it0 == 0:  # iter 0 multiplies the stored image by 0: a NaN left there survives, in the loop as in the fold
        assert np.isnan(folded).any()
