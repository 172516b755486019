"""The reference-signature side of the boundary, radish_pt_amd/csrc/radish_shim.hpp, must at least compile: -fsyntax-only,
-Wall -Werror, against the minimal declarations of the reference types it touches in tests/shim/ref_decls.h (glm and the
reference's own headers are not in the build image; the header carries the layout asserts), included by
tests/shim/shim_syntax_check.cpp, in its single-GPU, its RADISH_SHIM_MULTI_GPU (one process per GPU) and its
RADISH_SHIM_ONE_PROCESS_GPUS (one process, n GPUs) form.  The same pair is linked into tests/shim/shim_runner and run on the GPU
by tests/test_gpu_shim_runs.py; the last test here checks the binaries build() makes for that."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.parametrize("multi_gpu", [False, True, "one_process"])
def test_shim_compiles(multi_gpu):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not found")
    cmd = [HIPCC, "-fsyntax-only", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-x", "c++",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "radish_pt_amd", "csrc"), "-I", "/opt/rocm/include",
           "-D__HIP_PLATFORM_AMD__=1"]
    if multi_gpu == "one_process":
        cmd.append("-DSHIM_CHECK_ONE_PROCESS")
    elif multi_gpu:
        cmd.append("-DSHIM_CHECK_MULTI_GPU")
    cmd.append(os.path.join(ROOT, "tests", "shim", "shim_syntax_check.cpp"))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


def test_build_makes_three_runner_binaries_that_need_the_library(monkeypatch):
    """tests/shim/shim_runner.cpp (the program tests/test_gpu_shim_runs.py starts) is built by build() in the shim's three forms;
    each binary's dynamic section names libradish_hip.so and the HIP runtime, found through a RUNPATH that starts at the binary."""
    from radish_pt_amd import _build

    called = []
    for name in ("build_host", "build_hip", "build_probe", "build_shim_runner"):
        monkeypatch.setattr(_build, name, lambda force=False, _n=name: called.append(_n))
    _build.build_all()
    assert called == ["build_host", "build_hip", "build_probe", "build_shim_runner"]
    monkeypatch.undo()
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")) or not shutil.which("readelf"):
        pytest.skip("hipcc or readelf not found")
    paths = _build.build_shim_runner()  # a no-op after build()
    assert [os.path.basename(p) for p in paths] == ["shim_runner", "shim_runner_multi_gpu", "shim_runner_one_process"]
    for p in paths:
        assert os.path.dirname(p) == os.path.join(ROOT, "tests", "shim") and os.access(p, os.X_OK), p
        dyn = subprocess.run(["readelf", "-d", p], capture_output=True, text=True, timeout=60, check=True).stdout
        needed = [line.split("[")[1].rstrip("]") for line in dyn.splitlines() if "(NEEDED)" in line]
        assert "libradish_hip.so" in needed and any(n.startswith("libamdhip64.so") for n in needed), (p, needed)
        runpath = [line.split("[")[1].rstrip("]") for line in dyn.splitlines() if "(RUNPATH)" in line]
        assert runpath and runpath[0].startswith("$ORIGIN/../../radish_pt_amd/csrc"), (p, runpath)
