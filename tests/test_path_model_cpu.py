"""The oracle's textured, environment-lit path against tests/path_model.py, a float64 statement of the same rules written from the
reference text in another form: general triangles with interpolated normals and texcoords, the four maps and the procedural
colour, the environment map as a light and as what a miss sees, glass and mapped metal inside the bounce loop with a draw cursor
per pixel.  The oracle and the device code are one author's two restatements and agree bit for bit
(tests/test_gpu_parity.py::test_textures_and_envmap_bit_exact); what this closes is a misreading the two share.
tests/test_gpu_path_model.py holds the HIP kernels to the same model; tests/path_model_checks.py holds the frozen scene, cameras,
loopers, tolerance and cap, and its docstring the measured figures."""
import numpy as np
import pytest

import path_model as P
import path_model_checks as C
import restir_model_checks as RC

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")  # rejected light draws divide by zero on purpose


@pytest.fixture(scope="module")
def setup():
    return C.setup()


# ---------------------------------------------------------------------------------------------------------------------
# coverage: a branch that fewer pixels depend on than the cap leaves out could be wrong everywhere and still pass
# ---------------------------------------------------------------------------------------------------------------------
COVERED = ("env_nee_direct", "env_nee_indirect", "env_nee_occluded", "miss_into_map_mis", "miss_into_map_after_specular",
           "primary_miss", "emitter_seen_directly", "emitter_collected", "emitter_refused_single_sided", "refract_enter",
           "refract_leave", "tir_reflects", "metal_diffuse_lobe", "metal_ggx_lobe", "metal_below_horizon", "normal_map_flip_differs",
           "base_colour_wrapped_uv", "procedural_at_depth_2_or_more", "cursor_behind_at_depth_3")


def test_every_branch_decides_at_least_thirty_pixels(setup):
    """From the MODEL's event masks, per image (each iteration has its own cap): every rule of COVERED decides at
    least 30 pixels, five times the cap.  Total internal reflection is counted where the reference puts it: `fresnel()` returns 1
    for it (material.h:55-57) and `r.z < 1` then REFLECTS (:165-168); the `Invalid` of :170-174 needs the draw 1.0f itself and
    ends no path here, which is asserted so."""
    sd, ms, _ = setup
    for it, r in enumerate(C.model_path_trace()):
        counts = {k: int(r["events"][k].sum()) for k in COVERED}
        print(it, counts)
        for k, c in counts.items():
            assert c >= C.COVERAGE_FLOOR, (it, k, c)
        assert int(r["events"]["tir_invalid"].sum()) == 0
        assert (r["cursor"] <= 4 + 7 * C.MAX_DEPTH).all()
    # the scene: few triangles, wrapped uvs on the mapped ground, the procedural panel inside [0, 1), no two equal vertex normals
    assert sd.num_prims <= 300 and sd.num_lights >= 3
    t = sd.texcoords[np.repeat(sd.materials["baseColorMapId"][sd.material_ids] == 0, 3)]
    assert t.min() < 0 and t.max() > 1
    t = sd.texcoords[np.repeat(sd.materials["baseColorMapId"][sd.material_ids] == -2, 3)]
    assert 0 <= t.min() and t.max() < 1
    n = sd.normals.reshape(-1, 3, 3)[sd.materials["type"][sd.material_ids] != P.DIELECTRIC]
    smooth = sd.materials["type"][sd.material_ids][sd.materials["type"][sd.material_ids] != P.DIELECTRIC] != P.LIGHT
    assert (np.abs(n[smooth, 0] - n[smooth, 1]).max(1) > 1e-3).all() and (np.abs(n[smooth, 0] - n[smooth, 2]).max(1) > 1e-3).all()
    # the alias tables: real demotions in the map's, and the map's entry picked neither always nor never
    assert (sd.env_map_sampler["prob"] < 1).sum() > 100
    ls = sd.light_sampler
    mass = ls["prob"].astype(np.float64) / len(ls)
    np.add.at(mass, ls["failId"], (1.0 - ls["prob"].astype(np.float64)) / len(ls))
    assert 0.25 < mass[-1] < 0.75, mass


# ---------------------------------------------------------------------------------------------------------------------
# the three kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_path_trace_vs_model(setup):
    """singleKernelPT, depth 3, iterations 0 and 1 on two loopers: direct and indirect within 2e-4 relative (floor 1e-3) on all but
    at most 6 of 1728 pixels per image."""
    ex = C.oracle_excluded()["path_trace"]
    for it, e in enumerate(ex):
        print(it, {k: v.tolist() for k, v in e.items()})
        for k, px in e.items():
            C.assert_within_cap(px, f"oracle path_trace, iteration {it}, {k}")
    m = C.model_path_trace()
    assert m[1]["indirect"].max() > 0.3 and m[1]["direct"].max() > 0.3


def test_oracle_pt_direct_vs_model(setup):
    ex = C.oracle_excluded()["pt_direct"]
    for it, px in enumerate(ex):
        print(it, px.tolist())
        C.assert_within_cap(px, f"oracle path_trace_direct, iteration {it}")
    assert C.model_pt_direct()[1].max() > 1.0  # no tone map: an emitter's colour


def test_oracle_gbuffer_vs_model(setup):
    """Three cameras: primId and motion exactly, normal, depth and albedo within the tolerance."""
    ex = C.oracle_excluded()["gbuffer"]
    for f, px in enumerate(ex):
        print(f, px.tolist())
        C.assert_within_cap(px, f"oracle gbuffer_render, camera {f}")
    gb = C.model_gbuffer()
    assert (gb[0]["primId"] == -1).sum() > 100 and (gb[0]["albedo"][gb[0]["primId"] == -1] > 0).all()  # the sky as albedo
    assert (gb[0]["primId"] == -2).sum() > 30 and (gb[1]["motion"] != np.arange(C.N)).sum() > 500


@pytest.mark.parametrize("reuse,faithful", C.RESTIR_CASES)
def test_oracle_restir_vs_model(setup, reuse, faithful):
    """restir_model's three steps on this scene through PathScene, by restir_model_checks' sequence with its step-wise hand-over:
    frames 0-2 under a moving camera.  The candidates read the mapped metallic and roughness and the normal after the normal
    map, the environment entry comes with dist = 1e10 and is shadow-tested to pos + wi * dist, and a pixel that sees the sky is
    the map's colour times the G-buffer albedo, which is the same colour."""
    _, ms, cams = setup
    for f, (ex, p1, p2) in enumerate(C.oracle_restir_excluded(reuse, faithful)):
        what = f"oracle, reuse {reuse}, faithful {faithful}, frame {f}"
        print(what, {k: v.tolist() for k, v in ex.items()})
        RC.assert_within_cap(ex, what)
        sky = p1["status"] == 1
        env_kept = p1["stored"] & (p1["out"]["dist"] == 1e10)
        assert p1["stored"].sum() > 1000 and sky.sum() > 100 and (p2["image"][sky] > 0).all()
        assert env_kept.sum() >= C.COVERAGE_FLOOR and (env_kept & (p1["out"]["weight"] == 0)).sum() >= C.COVERAGE_FLOOR, f  # shadowed too
        assert (env_kept & (p1["out"]["weight"] > 0)).sum() >= C.COVERAGE_FLOOR
        assert (p1["stored"] & (ms.mat_type[p1["mat"]] == P.METALLIC_WORKFLOW)).sum() > 100


# ---------------------------------------------------------------------------------------------------------------------
# light sampling with the environment entry
# ---------------------------------------------------------------------------------------------------------------------
def test_sample_direct_light_environment_branch_vs_float64(setup):
    """orc_sample_direct_light, both visibility forms, against PathScene.sample_light on 3000 positions above the ground and
    draws of which about half pick the environment entry: pdf, radiance, wi, dist."""
    from oracle import pyoracle

    sd, ms, _ = setup
    o = pyoracle.OracleScene(sd)
    rng = np.random.default_rng(2)
    n = 3000
    pos = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(0.15, 1.6, n), rng.uniform(-2.3, 1.6, n)], 1)
    r4 = rng.random((n, 4))
    r4[:40, 0] = 1.0  # Sampler::sample can return exactly 1.0f: the index clamp picks the LAST entry, the map
    r4[40:80, 2] = 1.0
    pos, r4 = pos.astype(np.float32).astype(np.float64), r4.astype(np.float32).astype(np.float64)
    pdf0, rad0, wi0, dist0, is_env, _ = ms.sample_light(pos, r4, False)
    pdf1, rad1, wi1, _, _, occ = ms.sample_light(pos, r4, True)
    assert 0.3 < is_env.mean() < 0.7 and is_env[:40].all() and 0.1 < occ[is_env].mean() < 0.9
    assert (dist0[is_env] == 1e10).all() and (pdf0[is_env] > 0).all()
    bad = 0
    for i in range(n):
        p, rad, wi, d = o.sample_direct_light(pos[i], r4[i], visibility=False)
        if pdf0[i] < 0:
            assert p == -1.0, i
        else:
            assert p == pytest.approx(pdf0[i], rel=5e-5), i
            assert np.allclose(rad, rad0[i], rtol=1e-6) and np.allclose(wi, wi0[i], atol=2e-6) and d == pytest.approx(dist0[i], rel=2e-6), i
        p1, rad_v, wi_v, _ = o.sample_direct_light(pos[i], r4[i], visibility=True)
        if (p1 == -1.0) != (pdf1[i] < 0):
            bad += 1  # a shadow ray that grazes a triangle's edge
        elif p1 != -1.0:
            assert p1 == p and np.array_equal(rad_v, rad) and np.array_equal(wi_v, wi), i
    print("shadow rays classified differently:", bad)
    assert bad <= 0.004 * n, bad


# ---------------------------------------------------------------------------------------------------------------------
# planted mistakes: each changes the MODEL in one place; the oracle must then fall outside the cap
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", P.PLANTS)
def test_planted_mistake_is_caught(setup, plant):
    """(`metallicMapId` tested with `!=` is left out: both loaders refuse -2 in that field, so no scene can tell `>` from `!=`.)"""
    sd, _, cams = setup
    worst = {}
    for it, e in enumerate(C.path_trace_excluded(C.oracle_path_trace(sd, cams[0]), plant)):
        for k, px in e.items():
            worst[f"path_trace {it} {k}"] = len(px)
    for it, px in enumerate(C.images_excluded(C.oracle_pt_direct(sd, cams[0]), C.model_pt_direct(plant))):
        worst[f"pt_direct {it}"] = len(px)
    for f, px in enumerate(C.gbuffer_excluded(C.oracle_gbuffer(sd, cams), plant)):
        worst[f"gbuffer {f}"] = len(px)
    print(plant, worst)
    assert max(worst.values()) > C.CAP, f"the oracle passes the comparison with {plant} planted in the model: {worst}"


def test_normal_map_decode_times_two_minus_one_is_the_same_rule(setup):
    """The reference decodes a normal map as `normalize(mapped * 1.f - 0.5f)` (scene.h:107-108).  That is half of the usual
    `mapped * 2 - 1` and the normalisation removes the factor, so the two are ONE rule and no input can tell them apart: planted,
    it leaves every output of the model where it was.  What the inputs do see is the offset (`normal_map_decode_no_offset`
    above)."""
    for a, b in zip(C.model_path_trace(), C.model_path_trace("normal_map_decode_2x_minus_1")):
        assert np.allclose(a["direct"], b["direct"], rtol=1e-12, atol=0) and np.allclose(a["indirect"], b["indirect"], rtol=1e-9, atol=1e-15)
    for a, b in zip(C.model_gbuffer(), C.model_gbuffer("normal_map_decode_2x_minus_1")):
        assert np.allclose(a["normal"], b["normal"], rtol=0, atol=1e-14)


def test_vectorised_helpers_equal_the_scalar_statements(setup):
    """path_model's array forms against the scalar float64 statements the known-answer tests already use: linearSample
    (float64_models.linear_sample_py) at uvs from -2 to 3, texel centres and borders included; the procedural colour as
    tests/test_oracle_kat.py::test_procedural_texture_matches_python_minstd computes it; toPlane as toSphere's inverse."""
    import math

    from float64_models import linear_sample_py

    sd, ms, _ = setup
    rng = np.random.default_rng(9)
    uv = rng.uniform(-2.0, 3.0, (400, 2))
    uv[:40] = np.round(uv[:40] * 16) / 16  # texel borders of the 16-wide maps
    uv[40:80] = (np.round(uv[40:80] * 16) + 0.5) / 16  # and centres, where `fract > 0.5` decides
    for tex in ms.textures:
        got = P.linear_sample(tex, uv)
        want = np.array([linear_sample_py(tex, u, v) for u, v in uv])
        assert np.allclose(got, want, rtol=1e-13, atol=1e-15)
    uv = rng.uniform(0.0, 0.999, (200, 2))
    got = P.procedural_texture(uv)
    for (u, v), g in zip(uv, got):
        x = (int(u * 1024) * 1024 + int(v * 1024)) % 2147483647 or 1
        rs = []
        for _ in range(2):
            x = (x * 48271) % 2147483647
            rs.append((x - 1) / 2147483648.0)
        f = (math.sin(u * 10 * 2 * math.pi + rs[0] * 2 * math.pi) + 1) * 0.5
        h = (math.sin(v * 10 * 2 * math.pi + rs[1] * 2 * math.pi) + 1) * 0.5
        assert np.allclose(g, f * h, rtol=1e-12, atol=1e-15)
    pq = np.stack([rng.uniform(0.0, 1.0, 300), rng.uniform(0.02, 0.98, 300)], 1)
    assert np.allclose(P.to_plane(P.to_sphere(pq)), pq, atol=1e-12)
    # localRefMatrix: orthonormal, third column n, and the helper axis switches at |n.y| = 0.9999
    n = P.normalize(rng.normal(size=(300, 3)))
    n[:3] = P.normalize(np.array([[0.01, 0.99995, 0.0], [0.0141, 0.9999, 0.0], [0.0, -1.0, 0.0]]))
    t, b, n3 = P.local_ref(n)
    m = np.stack([t, b, n3], 2)
    assert np.allclose(np.einsum("kij,kil->kjl", m, m), np.eye(3), atol=1e-12) and np.array_equal(n3, n)
    assert abs(b[0, 2]) < 1e-12 and abs(b[2, 2]) < 1e-12  # cross(n, +z) has no z; cross(n, +y) has no y
    assert abs(P.local_ref(np.array([[0.6, 0.8, 0.0]]))[1][0, 1]) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# the model stands alone
# ---------------------------------------------------------------------------------------------------------------------
def test_model_reads_no_device_code_and_calls_no_oracle_entry():
    import ast
    import inspect

    tree = ast.parse(inspect.getsource(P))
    names = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name)} | {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute)}
    mods = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names} | \
           {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert mods == {"numpy", "restir_model", "float64_models", "test_oracle_float64"}, mods
    assert not {n for n in names if n.startswith("orc_")} and "pyoracle" not in names and "lib" not in names
    strings = {n.value for n in ast.walk(tree) if isinstance(n, ast.Constant) and isinstance(n.value, str) and "\n" not in n.value}
    assert not {s for s in strings if "csrc" in s or s.endswith((".cpp", ".h", ".hip", ".so"))}, strings
    assert "open" not in names and "fromfile" not in names and "load" not in names
