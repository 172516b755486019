"""Textures and the environment map edited on the device (rdh_scene_set_texture, rdh_scene_env_power, kernels_textures.h; DESIGN
11h): what can be checked without a GPU.

The entries exist in the header, the library and the Python layer; the numpy float32 model of an environment edit
(texture_edit.weights, then alias_model.sweep) equals the host's build_envmap_sampler bit for bit on every map size and content
the GPU tests use; the tables encode the distribution of their weights within test_light_rebuild_cpu.py's bound; and the new
kernels compile for gfx950 without scratch."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import alias_model
import texture_edit
from helpers import assert_bit_equal
from test_light_rebuild_cpu import _margin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRIES = ("rdh_scene_set_texture", "rdh_scene_env_power", "rdh_debug_read_textures")
CASES = [(size, content) for size in texture_edit.SIZES for content in texture_edit.CONTENTS]


def test_library_exports_the_entries():
    from radish_pt_amd import api

    lib = ctypes.CDLL(api.HIP_LIB_PATH)  # loads without a GPU; no compute call is made
    for name in ENTRIES:
        assert name in api.EXPORTS
        assert hasattr(lib, name), name


def test_header_declares_the_entries():
    with open(os.path.join(ROOT, "include", "radish_hip.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    assert "int rdh_scene_set_texture(rdh_ctx *ctx, int32_t texId, const float *d_texels, int32_t width, int32_t height);" in text
    assert "int rdh_scene_env_power(rdh_ctx *ctx, float *out);" in text
    assert "long long rdh_debug_read_textures(rdh_ctx *ctx, int which, void *hostOut, long long maxBytes);" in text


def test_python_entries_exist():
    import inspect

    from radish_pt_amd import api

    assert list(inspect.signature(api.Context.set_texture).parameters) == ["self", "tex_id", "texels"]
    assert list(inspect.signature(api.Context.env_power).parameters) == ["self"]
    assert list(inspect.signature(api.Context.debug_read_textures).parameters) == ["self", "which"]


@pytest.mark.parametrize("size,content", CASES, ids=[f"{s[0]}x{s[1]}-{c}" for s, c in CASES])
def test_model_equals_host_sampler(size, content):
    from radish_pt_amd import hostlib

    env = texture_edit.env_map(size, content)
    w, h = size
    pdf = np.empty(w * h, np.float32)
    assert hostlib.lib().rdh_build_envmap_pdf(np.ascontiguousarray(env).ctypes.data, w, h, pdf.ctypes.data) == 0
    weights = texture_edit.weights(env)
    assert_bit_equal(weights, pdf, "pixel weights")
    ht, hs = hostlib.build_envmap_sampler(env, w, h)
    mt, ms = texture_edit.sampler(env)
    assert_bit_equal(np.array([ms], np.float32), np.array([hs], np.float32), "sum")
    assert np.array_equal(mt["failId"], ht["failId"]), f"failId differs at {np.flatnonzero(mt['failId'] != ht['failId'])[:5]}"
    nan = np.isnan(ht["prob"])
    assert np.array_equal(np.isnan(mt["prob"]), nan)  # NaN payloads are left aside
    assert_bit_equal(mt["prob"][~nan], ht["prob"][~nan], "prob")
    scaled = weights * (np.float32(w * h) / np.float32(hs)) if hs > 0 else weights
    if content == "constant":  # every scaled value is exactly 1: nothing is above the mean
        assert (scaled == np.float32(1)).all() and (mt["prob"] == np.float32(1)).all()
        assert np.array_equal(mt["failId"], np.arange(w * h))
    if content == "one_pixel":
        assert np.count_nonzero(weights) == 1 and hs > 0
    if content == "black":
        assert hs == 0 and nan.all() and np.array_equal(mt["failId"], np.arange(w * h))


@pytest.mark.parametrize("size,content", [c for c in CASES if c[1] != "black"], ids=lambda v: str(v).replace(" ", ""))
def test_table_encodes_its_distribution(size, content):
    """float64: sampling the table returns pixel i with probability pdf_i / sum, within the bound test_light_rebuild_cpu.py derives
    for a table built in binary32 from n non-negative values, 4 (n + 1) 2^-24.  (An all-black map has no distribution.)"""
    from radish_pt_amd import hostlib

    env = texture_edit.env_map(size, content)
    values = texture_edit.weights(env).astype(np.float64)
    n = len(values)
    for what, table in (("host", hostlib.build_envmap_sampler(env, size[0], size[1])[0]), ("model", texture_edit.sampler(env)[0])):
        dev = np.abs(alias_model.encoded_distribution(table) - values / values.sum()).max()
        print(f"{size[0]}x{size[1]} {content} ({what}): deviation {dev:.3e}, bound {_margin(n):.3e}")
        assert dev <= _margin(n), f"{what}: {dev:.3e} > {_margin(n):.3e}"


def test_edits_change_the_sampler():
    """The maps the GPU tests edit to differ from the uploaded one in table or power wherever the size leaves room for it, so that
    `edited equals fresh upload` cannot be met by a call that does nothing."""
    for size in texture_edit.SIZES:
        base = texture_edit.sampler(texture_edit.env_map(size, "sky"))
        for content in texture_edit.EDITS:
            if np.array_equal(texture_edit.env_map(size, content), texture_edit.env_map(size, "sky")):
                assert size == (1, 1) and content == "moved_sun", (size, content)  # one pixel sees neither sun
                continue
            t, s = texture_edit.sampler(texture_edit.env_map(size, content))
            same_table = np.array_equal(t["failId"], base[0]["failId"]) and np.array_equal(np.isnan(t["prob"]), np.isnan(base[0]["prob"])) \
                and np.array_equal(t["prob"][~np.isnan(t["prob"])].view(np.uint32), base[0]["prob"][~np.isnan(t["prob"])].view(np.uint32))
            assert not same_table or np.float32(s).tobytes() != np.float32(base[1]).tobytes(), (size, content)


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_texture_kernels_use_no_scratch():
    """kernels_textures.h compiled from a one-line translation unit with the library's flags (as test_pose_kernel_resources.py does):
    the same header, the same flags, hence the same code objects.  Neither new kernel may spill or use LDS."""
    from radish_pt_amd import _build

    flags = [f for f in _build.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "textures_only.hip")
        with open(src, "w") as f:
            f.write('#include "device/kernels_textures.h"\n')
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
    for prefix in ("_ZN2rd13k_env_weights", "_ZN2rd17k_light_power_dev"):
        hits = {k: v for k, v in res.items() if k.startswith(prefix)}
        assert len(hits) == 1, (prefix, sorted(res))
        for name, r in hits.items():
            print(name, r)
            assert r["scratch"] == 0 and r["lds"] == 0, (name, r)
            assert r["occupancy"] >= 8, (name, r)
    for name, r in res.items():  # the alias kernels the edit reuses come with the header
        assert r["scratch"] == 0, (name, r)
