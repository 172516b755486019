"""In-tree builds of the product libraries: libradish_host.so (g++) and libradish_hip.so (hipcc, gfx950).

Everything lands next to its sources so the `.so` files travel with the gpurun snapshot; nothing is installed.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radish_pt_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

HOST_SOURCES = [os.path.join(CSRC, "host", "scene_build.cpp"), os.path.join(CSRC, "host", "scene_load.cpp")]
HIP_SOURCES = [os.path.join(CSRC, "radish_hip.hip")]
HIP_DEPS = [
    os.path.join(CSRC, "device", f)
    for f in ("rmath.h", "layouts.h", "traverse.h", "bsdf.h", "lights.h", "path_step.h", "kernels_pt.h", "kernels_restir.h", "kernels_wave.h", "ray_cull.h", "kernels_persist.h", "kernels_walk.h", "kernels_gbuffer.h", "wg_trace.h", "kernels_display.h", "kernels_denoise.h", "kernels_bvh.h", "kernels_refit.h", "kernels_lbvh.h", "kernels_lights.h", "kernels_pose.h", "kernels_materials.h", "kernels_textures.h", "display_math.h", "denoise_math.h", "reservoir.h", "kernels_adaptive.h")
] + [os.path.join(ROOT, "include", "radish_hip.h")]

# -ffp-contract=off: the HIP path must execute the same IEEE-754 operation sequence as the CPU checker
# (DESIGN.md "Numerics contract"); no fast-math anywhere.
HIP_FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
    "-fno-gpu-rdc", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result",
]


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    print("[build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def build_host(force=False):
    out = os.path.join(CSRC, "libradish_host.so")
    deps = HOST_SOURCES + [os.path.join(ROOT, "include", "radish_host.h")]
    if force or _newer(out, deps):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-o", out]
             + HOST_SOURCES + ["-lz"])
    return out


def build_hip(force=False):
    out = os.path.join(CSRC, "libradish_hip.so")
    if force or _newer(out, HIP_SOURCES + HIP_DEPS):
        _run([HIPCC] + HIP_FLAGS + ["-I", os.path.join(ROOT, "include"), "-o", out] + HIP_SOURCES
             + ["-Wl,-rpath,/opt/rocm/lib"])
    return out


def build_variant(name, defines):
    """Tuning builds: csrc/variants/libradish_hip_<name>.so compiled with extra -D flags (select with RADISH_HIP_LIB)."""
    d = os.path.join(CSRC, "variants")
    os.makedirs(d, exist_ok=True)
    out = os.path.join(d, f"libradish_hip_{name}.so")
    _run([HIPCC] + HIP_FLAGS + [f"-D{x}" for x in defines] + ["-I", os.path.join(ROOT, "include"), "-o", out]
         + HIP_SOURCES + ["-Wl,-rpath,/opt/rocm/lib"])
    return out


PROBE_SOURCE = os.path.join(ROOT, "tests", "probe", "device_probe.hip")


def build_probe(force=False, extra_flags=(), out=None):
    """Test-only: tests/probe/libradish_probe.so, one tiny kernel around each __device__ function of the kernel-free headers,
    compiled with exactly the product's HIP_FLAGS (plus hidden visibility: only the probe_* entries are exported).  The product
    never loads it.  `extra_flags` / `out` are for scratch builds that show the tests can fail (select with RADISH_PROBE_LIB)."""
    out = out or os.path.join(ROOT, "tests", "probe", "libradish_probe.so")
    vmap = os.path.join(os.path.dirname(PROBE_SOURCE), "probe.map")  # linker script: hides the compiler's own __hip_cuid_* symbol too
    if force or _newer(out, [PROBE_SOURCE, vmap] + HIP_DEPS):
        _run([HIPCC] + HIP_FLAGS + ["-fvisibility=hidden"] + list(extra_flags) + ["-I", os.path.join(CSRC, "device"), "-o", out,
              PROBE_SOURCE, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--version-script=" + vmap])
    return out


SHIM_HEADER = os.path.join(CSRC, "radish_shim.hpp")
SHIM_RUNNER_SOURCE = os.path.join(ROOT, "tests", "shim", "shim_runner.cpp")
SHIM_RUNNER_FORMS = {  # binary name -> the shim's form
    "shim_runner": [],
    "shim_runner_multi_gpu": ["-DRADISH_SHIM_MULTI_GPU"],
    "shim_runner_one_process": ["-DRADISH_SHIM_ONE_PROCESS_GPUS"],
}


def build_shim_runner(force=False, out_dir=None, shim=None):
    """Test-only: tests/shim/shim_runner{,_multi_gpu,_one_process}, host-only programs (hipcc as C++, no device code) that run
    radish_shim.hpp in its three forms against tests/shim/ref_decls.h, linked against libradish_hip.so (found through an
    $ORIGIN-relative run path) and the HIP runtime.  The product never starts them.  `out_dir` / `shim` are for scratch builds
    against a changed copy of the header (a file named radish_shim.hpp in another directory) that show the tests can fail
    (select with RADISH_SHIM_RUNNER_DIR).  Returns the three paths."""
    out_dir = os.path.abspath(out_dir or os.path.dirname(SHIM_RUNNER_SOURCE))
    shim = os.path.abspath(shim or SHIM_HEADER)
    if os.path.basename(shim) != "radish_shim.hpp":
        raise ValueError("the runner includes \"radish_shim.hpp\": a changed copy keeps that name, in a directory of its own")
    os.makedirs(out_dir, exist_ok=True)
    deps = [SHIM_RUNNER_SOURCE, os.path.join(os.path.dirname(SHIM_RUNNER_SOURCE), "ref_decls.h"), shim,
            os.path.join(ROOT, "include", "radish_hip.h")]
    outs = []
    for name, defines in SHIM_RUNNER_FORMS.items():
        out = os.path.join(out_dir, name)
        outs.append(out)
        if force or _newer(out, deps):
            if not os.path.exists(os.path.join(CSRC, "libradish_hip.so")):
                build_hip()  # the link needs the library to exist, not to be current: its exports are fixed by include/radish_hip.h
            _run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__=1"]
                 + defines + ["-I", os.path.dirname(shim), "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                              SHIM_RUNNER_SOURCE, "-o", out, "-L", CSRC, "-lradish_hip", "-L", "/opt/rocm/lib", "-lamdhip64", "-ldl",
                              "-Wl,-rpath,$ORIGIN/" + os.path.relpath(CSRC, out_dir), "-Wl,-rpath,/opt/rocm/lib"])
    return outs


def build_all(force=False):
    build_host(force)
    build_hip(force)
    build_probe(force)
    build_shim_runner(force)


if __name__ == "__main__":
    build_all(force="--force" in sys.argv)
