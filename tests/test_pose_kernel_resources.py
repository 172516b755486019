"""Resources of k_pose_objects (kernels_pose.h; CPU test: hipcc cross-compiles gfx950 and reports them), in the manner of
test_kernel_resources.py.

kernels_pose.h includes only layouts.h, so the kernel is compiled here from a one-line translation unit with the library's flags
(seconds, where the whole library takes a minute): the same header, the same flags, hence the same code object for this kernel.
It must use no scratch and no LDS, and keep the eight waves per SIMD the build reported when it was written (22 VGPRs)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_pose_kernel_resources():
    from radish_pt_amd import _build

    flags = [f for f in _build.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "pose_only.hip")
        with open(src, "w") as f:
            f.write('#include "device/kernels_pose.h"\n')
        cmd = [HIPCC] + flags + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "radish_pt_amd", "csrc"), "-c", src,
                                 "-o", os.path.join(tmp, "x.o"), "-Rpass-analysis=kernel-resource-usage"]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split("\n")[0].split(" ")[0].strip()
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        res[name] = {"vgpr": get("VGPRs"), "scratch": get(r"ScratchSize \[bytes/lane\]"), "occupancy": get(r"Occupancy \[waves/SIMD\]"),
                     "lds": get(r"LDS Size \[bytes/block\]")}
    hits = {k: v for k, v in res.items() if k.startswith("_ZN2rd14k_pose_objects")}
    assert len(hits) == 1, sorted(res)
    for name, r in hits.items():
        print(name, r)
        assert r["scratch"] == 0 and r["lds"] == 0, (name, r)
        assert r["occupancy"] >= 8, (name, r)
    seed = {k: v for k, v in res.items() if k.startswith("_ZN2rd11k_pose_seed")}
    assert len(seed) == 1 and all(r["scratch"] == 0 and r["lds"] == 0 for r in seed.values()), seed
