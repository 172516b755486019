"""Material edits without a GPU (rdh_scene_set_materials, rdh_build_light_list_device): the exports and declarations,
the conditions that make the GPU test scenes worth running, the three compaction passes restated in numpy against the host's
build_light_list, and the resources of the new kernels."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import material_edit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRIES = ("rdh_scene_set_materials", "rdh_build_light_list_device")


def test_library_exports_the_entries():
    from radish_pt_amd import api

    lib = ctypes.CDLL(api.HIP_LIB_PATH)  # loads without a GPU; no compute call is made
    for name in ENTRIES:
        assert name in api.EXPORTS
        assert hasattr(lib, name), name


def test_header_declares_the_entries():
    with open(os.path.join(ROOT, "include", "radish_hip.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    assert ("int rdh_scene_set_materials(rdh_ctx *ctx, const int32_t *materialIds, const void *materials, int32_t count, "
            "float envPower);") in text
    assert ("int rdh_build_light_list_device(rdh_ctx *ctx, const float *d_vertices, const int32_t *d_materialIds, int32_t numPrims, "
            "const void *d_materials, int32_t numMaterials, int32_t *d_lightPrimIds, float *d_lightUnitRadiance, "
            "float *d_lightPower, int32_t *d_count);") in text


def test_python_entries_exist():
    import inspect

    from radish_pt_amd import api

    assert list(inspect.signature(api.Context.set_materials).parameters) == ["self", "ids", "materials", "env_power"]
    assert inspect.signature(api.Context.set_materials).parameters["env_power"].default == 0.0
    assert list(inspect.signature(api.Context.build_light_list_device).parameters) == ["self", "vertices", "material_ids", "materials"]


# ---- the GPU test scenes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edit", material_edit.LIST_EDITS)
def test_teapots_edits_exercise_the_compaction(edit):
    """The edits that change the list must spread emitters over blocks and wave boundaries, or the scatter's offsets are never
    told apart from ranks."""
    sd, ed = material_edit.teapots(), material_edit.result("teapots", edit)
    ids = np.asarray(ed.light_prim_ids)
    blocks = np.unique(ids // 256)
    assert len(blocks) >= 3, blocks
    lit = np.zeros(sd.num_prims + 1, bool)
    lit[ids] = True
    last = np.arange(63, sd.num_prims - 1, 64)
    assert (lit[last] & lit[last + 1]).any(), "no emitter pair across a 64-triangle boundary"
    assert (np.diff(blocks) > 1).any(), "no empty block between two blocks with emitters"
    assert len(ids) != sd.num_lights
    if edit == "grow":
        assert len(ids) > sd.num_lights  # past the uploaded capacity


def test_every_edit_changes_the_description():
    from radish_pt_amd import layouts as L

    for scene in material_edit.SCENES:
        sd = material_edit.SCENES[scene]()
        for edit in material_edit.EDITS:
            ed = material_edit.result(scene, edit)
            same = ed.materials.tobytes() == sd.materials.tobytes()
            assert same == (edit == "back_on"), (scene, edit)
        assert len(material_edit.result(scene, "no_lights").light_sampler) == (1 if sd.env_map_tex_id >= 0 else 0)
        assert np.any(sd.materials["type"][material_edit.PICKS[scene]["lambert"]] == L.LAMBERTIAN)
        assert sd.materials["type"][material_edit.PICKS[scene]["many"]] != L.LIGHT
    assert material_edit.teapots().env_map_tex_id < 0 and material_edit.cornell().env_map_tex_id >= 0


# ---- the three passes against the host ----------------------------------------------------------------------------------------------
def _random_case(n, seed, share=None):
    from radish_pt_amd import layouts as L

    rng = np.random.default_rng(seed)
    mats = np.zeros(11, L.MATERIAL_DTYPE)
    mats["type"] = rng.integers(0, 4, 11)
    if share is None:
        mats["type"][rng.choice(11, 3, replace=False)] = L.LIGHT
    elif share == 1:
        mats["type"] = L.LIGHT
    mats["baseColor"] = rng.uniform(0.1, 9, (11, 3))
    return rng.uniform(-1, 1, (3 * n, 3)).astype(np.float32), rng.integers(0, 11, n).astype(np.int32), mats


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 5000])
@pytest.mark.parametrize("share", [None, 0, 1])
def test_compaction_model_equals_host_light_list(n, share):
    from radish_pt_amd import hostlib, layouts as L

    v, ids, mats = _random_case(n, 100 + n, share)
    prims, _, _ = hostlib.build_light_list(v, ids, mats)
    emits = mats["type"][ids] == L.LIGHT
    got, total = material_edit.compaction_model(emits)
    assert total == len(prims) == {None: total, 0: 0, 1: n}[share]
    assert np.array_equal(got, prims)


# ---- kernel resources -------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_material_kernels_use_no_scratch():
    """kernels_materials.h compiled from a one-line translation unit with the library's flags (as test_samples_cpu.py does for the
    wavefront kernels): no kernel may spill, and the count / scatter kernels need only their four wave totals in LDS."""
    from radish_pt_amd import _build

    flags = [f for f in _build.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "materials_only.hip")
        with open(src, "w") as f:
            f.write('#include "device/kernels_materials.h"\n')
        cmd = [HIPCC] + flags + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "radish_pt_amd", "csrc"), "-c", src,
                                 "-o", os.path.join(tmp, "x.o"), "-Rpass-analysis=kernel-resource-usage"]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split("\n")[0].split(" ")[0].strip()
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        res[name] = {"vgpr": get("VGPRs"), "scratch": get(r"ScratchSize \[bytes/lane\]"), "lds": get(r"LDS Size \[bytes/block\]")}
    want = {"k_emit_count_scene": 16, "k_emit_count_ref": 16, "k_emit_scatter_scene": 16, "k_emit_scatter_ref": 16,
            "k_emit_scan": 1028, "k_mat_write": 0}
    for kernel, lds in want.items():
        hits = {k: v for k, v in res.items() if re.fullmatch(rf"_ZN2rd\d+{kernel}E.*", k)}
        assert len(hits) == 1, (kernel, sorted(res))
        for name, r in hits.items():
            print(name, r)
            assert r["scratch"] == 0 and r["lds"] == lds, (name, r)
