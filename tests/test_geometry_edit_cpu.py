"""The triangle set replaced on the device, without a GPU (rdh_scene_set_geometry, kernels_geometry.h): the exports and
declarations, the conditions that make the GPU test scenes worth running, and the resources of the two new kernels."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import geometry_edit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRIES = ("rdh_scene_set_geometry", "rdh_debug_read_geometry")


def test_library_exports_the_entries():
    from radish_pt_amd import api

    lib = ctypes.CDLL(api.HIP_LIB_PATH)  # loads without a GPU; no compute call is made
    for name in ENTRIES:
        assert name in api.EXPORTS
        assert hasattr(lib, name), name


def test_header_declares_the_entries():
    with open(os.path.join(ROOT, "include", "radish_hip.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    assert ("int rdh_scene_set_geometry(rdh_ctx *ctx, const float *d_vertices, const float *d_normals, const float *d_texcoords, "
            "const int32_t *d_materialIds, int32_t numPrims, int builder, float envPower);") in text
    assert "long long rdh_debug_read_geometry(rdh_ctx *ctx, int which, void *hostOut, long long maxBytes);" in text
    assert "still takes rdh_scene_upload" not in text
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "still take an upload" not in re.sub(r"\s+", " ", f.read())


def test_python_entries_exist():
    from radish_pt_amd import api

    sig = inspect.signature(api.Context.set_geometry)
    assert list(sig.parameters) == ["self", "vertices", "normals", "texcoords", "material_ids", "builder", "env_power"]
    assert sig.parameters["builder"].default == "sah" and sig.parameters["env_power"].default == 0.0
    assert list(inspect.signature(api.Context.debug_read_geometry).parameters) == ["self", "which"]


# ---- the GPU test scenes ----------------------------------------------------------------------------------------------------------
def test_every_edit_changes_the_count_or_the_ids():
    for scene, make in geometry_edit.SCENES.items():
        sd = make()
        for edit in geometry_edit.EDITS:
            ed = geometry_edit.result(scene, edit)
            same = ed.num_prims == sd.num_prims and np.array_equal(ed.material_ids, sd.material_ids)
            assert same == (edit == "back"), (scene, edit)
            assert ed.materials.tobytes() == sd.materials.tobytes() and ed.env_map_tex_id == sd.env_map_tex_id
        env = 1 if sd.env_map_tex_id >= 0 else 0
        for edit, lights in (("one_light", 1), ("one_dark", 0)):
            ed = geometry_edit.result(scene, edit)
            assert (ed.num_prims, ed.bvh_size, ed.num_lights, len(ed.light_sampler)) == (1, 1, lights, lights + env), (scene, edit)
        assert geometry_edit.result(scene, "remove").num_prims < sd.num_prims < geometry_edit.result(scene, "add").num_prims
    assert geometry_edit.SCENES["teapots"]().num_prims == 14092


@pytest.mark.parametrize("edit", ["remove", "add", "reassign"])
def test_teapots_edits_exercise_the_compaction(edit):
    """Emitters in at least three 256-triangle blocks, across a 64-triangle boundary, with an empty block between two that have
    some: otherwise the scatter's block offsets are never told apart from ranks in a block."""
    sd, ed = geometry_edit.SCENES["teapots"](), geometry_edit.result("teapots", edit)
    ids = np.asarray(ed.light_prim_ids)
    blocks = np.unique(ids // 256)
    assert len(blocks) >= 3, blocks
    lit = np.zeros(ed.num_prims + 1, bool)
    lit[ids] = True
    last = np.arange(63, ed.num_prims - 1, 64)
    assert (lit[last] & lit[last + 1]).any(), "no emitter pair across a 64-triangle boundary"
    assert (np.diff(blocks) > 1).any(), "no empty block between two blocks with emitters"
    assert len(ids) != sd.num_lights
    if edit == "add":  # past both uploaded capacities: triangles, and emitters by more than a stand-in's worth
        assert ed.num_prims > sd.num_prims and ed.num_lights >= sd.num_lights + 864


# ---- kernel resources -------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_geometry_kernels_use_no_scratch():
    """kernels_geometry.h compiled from a small translation unit with the library's flags (as test_material_edit_cpu.py does): neither
    kernel may spill; k_geom_check keeps 1 024 integer bins in LDS in one instantiation and none in the other."""
    from radish_pt_amd import _build

    flags = [f for f in _build.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "geometry_only.hip")
        with open(src, "w") as f:
            f.write('#include "device/kernels_geometry.h"\n'
                    "template __global__ void rd::k_geom_check<true>(const float *, const float *, const int *, int, int, int *);\n"
                    "template __global__ void rd::k_geom_check<false>(const float *, const float *, const int *, int, int, int *);\n")
        cmd = [HIPCC] + flags + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "radish_pt_amd", "csrc"), "-c", src,
                                 "-o", os.path.join(tmp, "x.o"), "-Rpass-analysis=kernel-resource-usage"]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split("\n")[0].split(" ")[0].strip()
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        res[name] = {"vgpr": get("VGPRs"), "scratch": get(r"ScratchSize \[bytes/lane\]"), "lds": get(r"LDS Size \[bytes/block\]")}
    want = {r"_ZN2rd\d+k_geom_checkILb1EE.*": 4096, r"_ZN2rd\d+k_geom_checkILb0EE.*": 0, r"_ZN2rd\d+k_geom_packE.*": 0}
    for pattern, lds in want.items():
        hits = {k: v for k, v in res.items() if re.fullmatch(pattern, k)}
        assert len(hits) == 1, (pattern, sorted(res))
        for name, r in hits.items():
            print(name, r)
            assert r["scratch"] == 0 and r["lds"] == lds, (name, r)
