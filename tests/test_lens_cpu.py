"""The lens without a GPU (rdh_set_lens): the exports, the numpy restatements of tests/lens_model.py against the
oracle's pinhole, against geometry (every lens ray of a pixel passes its point on the focal plane) and against the distributions
the two samplers are meant to have, planted mistakes that each check must catch, and the resources of the new kernels.

Statistical level: p > 1e-4, as tests/test_oracle_statistics.py (_chi2_ok) uses."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
from scipy import stats

import frame_edges as FE
import lens_model as LM
from helpers import assert_bit_equal
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
P_LEVEL = 1e-4


def _sobol():
    from radish_pt_amd import scenes

    return scenes.sobol_table()


def _camera(shape, lens_radius=0.05, focal_dist=2.5):
    from radish_pt_amd import hostlib

    w, h = shape
    return hostlib.make_camera(w, h, eye=(0.3, 1.1, 3.2), rotation=(-97.0, -8.0, 0.0), fovy=19.0, lens_radius=lens_radius, focal_dist=focal_dist)


def _random_mask(w, h, seed, zeros=0):
    rng = np.random.default_rng(seed)
    m = (rng.uniform(0.05, 1.0, (h, w, 3)) ** 2).astype(np.float32)
    if zeros:
        flat = m.reshape(-1, 3)
        flat[rng.choice(w * h, zeros, replace=False)] = 0.0
    return m


def _mask(texels):
    table, _ = LM.mask_table(texels)
    return table, texels.shape[1], texels.shape[0]


def _chi2_p(obs, exp):
    chi2 = ((obs - exp) ** 2 / exp).sum()
    return float(stats.chi2.sf(chi2, len(exp) - 1))


# ---- the entries -----------------------------------------------------------------------------------------------------------------
def test_library_exports_and_declares_the_entries():
    from radish_pt_amd import api

    lib = ctypes.CDLL(api.HIP_LIB_PATH)  # loads without a GPU; no compute call is made
    for name in ("rdh_set_lens", "rdh_debug_primary_rays", "rdh_debug_read_lens"):
        assert name in api.EXPORTS and hasattr(lib, name)
    with open(os.path.join(ROOT, "include", "radish_hip.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    assert "int rdh_set_lens(rdh_ctx *ctx, int mode, int32_t maskTexId);" in text
    assert "int rdh_debug_primary_rays(rdh_ctx *ctx, int looper, float *d_rays6);" in text
    assert "long long rdh_debug_read_lens(rdh_ctx *ctx, int which, void *hostOut, long long maxBytes);" in text
    for k, v in (("OFF", 0), ("DISK", 1), ("MASK", 2)):
        assert f"#define RDH_LENS_{k} {v}" in text and getattr(api, f"RDH_LENS_{k}") == v
    sig = inspect.signature(api.Context.set_lens)
    assert list(sig.parameters) == ["self", "mode", "mask_tex_id"] and sig.parameters["mask_tex_id"].default == -1
    assert list(inspect.signature(api.Context.debug_primary_rays).parameters) == ["self", "looper"]
    assert list(inspect.signature(api.Context.debug_read_lens).parameters) == ["self"]


def test_scene_file_hands_over_the_mask_and_switches_nothing_on(tmp_path):
    """A scene file with LensRadius > 0 and an ApertureMask loads as before: the camera carries the two numbers, the mask is one of
    the scene's textures, and SceneData names it for Context.set_lens."""
    from radish_pt_amd import scenes
    from test_scene_loader import _png

    (tmp_path / "a.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    (tmp_path / "iris.png").write_bytes(_png(2, 2, 1, 0, [[0b10000000], [0b01000000]]))
    (tmp_path / "s.txt").write_text(
        "Material m\nType Lambertian\nBaseColor 0.5 0.5 0.5\nMetallic 0\nRoughness 1\nIor 1\nNormalMap Null\n\n"
        "Object 0\na.obj\nMaterial m\n\nCamera\nResolution 8 8\nFovY 20\nLensRadius 0.25\nFocalDist 3\nApertureMask iris.png\n"
        "Sample 1\nDepth 2\nFile x\nEye 0 0 3\nRotation -90 0 0\nUp 0 1 0\n\n")
    sd, cam, _ = scenes.load_scene_file(str(tmp_path / "s.txt"))
    assert sd.aperture_mask_tex_id == 0 and sd.textures[0].shape == (2, 2, 3)
    assert float(cam["lensRadius"]) == 0.25 and float(cam["focalDist"]) == 3.0
    assert scenes.tiny().aperture_mask_tex_id == -1
    table, _ = LM.mask_table(sd.textures[0])
    assert sorted(np.flatnonzero(LM.mask_weights(sd.textures[0]) > 0).tolist()) == sorted(set(table["failId"].tolist()))


# ---- the float32 model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(FE.SHAPES), ids=[FE.SHAPE_IDS[s] for s in FE.SHAPES])
def test_lens_off_is_the_oracles_camera_sample(shape):
    """Mode OFF, a lens radius set all the same: orc_camera_sample's ray of every pixel, bit for bit, at two rows of the table."""
    sobol = _sobol()
    cam = _camera(shape, lens_radius=0.3)
    buf = np.frombuffer(cam.tobytes(), np.uint8).copy()
    w, h = shape
    for looper in (0, 9999):
        got = LM.lens_rays_f32(cam, sobol, looper, LM.OFF)
        r = LM.draws_f32(sobol, looper, np.arange(w * h))
        want = np.zeros((w * h, 6), np.float32)
        for i in range(w * h):
            pyoracle.lib().orc_camera_sample(buf.ctypes.data, i % w, i // w, r[i].ctypes.data, want[i].ctypes.data)
        assert_bit_equal(got, want, f"{shape}, looper {looper}")


@pytest.mark.parametrize("mode", [LM.OFF, LM.DISK, LM.MASK])
@pytest.mark.parametrize("radius", [0.05, 0.5])
def test_every_ray_passes_its_focus_point(mode, radius):
    """The distance of the pixel's focus point position + M * pFocus from the float32 ray's line, in float64, relative to the
    focus point's distance from the origin."""
    sobol = _sobol()
    cam = _camera((63, 65), lens_radius=radius)
    mask = _mask(_random_mask(16, 16, 4)) if mode == LM.MASK else None
    for looper in (0, 9999):
        rays = LM.lens_rays_f32(cam, sobol, looper, mode, mask).astype(np.float64)
        focus = LM.focus_points_f64(cam, sobol, looper)
        o, d = rays[:, :3], rays[:, 3:]
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        to = focus - o
        off = np.linalg.norm(to - (to * d).sum(1, keepdims=True) * d, axis=1)
        rel = off / np.linalg.norm(to, axis=1)
        print(mode, radius, looper, rel.max())
        assert rel.max() < 1e-5
        if mode != LM.OFF:  # and the origins do leave the pinhole, inside the aperture's square
            lens = o - cam["position"].astype(np.float64)
            assert np.abs(lens @ cam["view"].astype(np.float64)).max() < 1e-6
            assert 0.1 * radius < np.linalg.norm(lens, axis=1).max() <= radius * (1.0 if mode == LM.DISK else 2 ** 0.5) * (1 + 1e-6)


def test_lens_rays_f64_agrees_with_the_pinhole_and_with_f32():
    from test_oracle_float64 import _camera_rays_f64, sobol_draws

    sobol = _sobol()
    W, H = 48, 36
    cam = _camera((W, H), lens_radius=0.08)
    u = sobol_draws(sobol, 77, np.arange(W * H), 4)
    o0, d0 = _camera_rays_f64(cam, W, H, u[:, 0:2])
    o1, d1 = LM.lens_rays_f64(cam, W, H, u[:, 0:2], u[:, 2:4], LM.OFF)
    assert np.abs(o0 - o1).max() == 0 and np.abs(d0 - d1).max() < 1e-15
    mask = _mask(_random_mask(16, 16, 4))
    for mode in (LM.DISK, LM.MASK):
        o, d = LM.lens_rays_f64(cam, W, H, u[:, 0:2], u[:, 2:4], mode, mask)
        r32 = LM.lens_rays_f32(cam, sobol, 77, mode, mask).astype(np.float64)
        assert np.abs(o - r32[:, :3]).max() < 2e-6 and np.abs(d - r32[:, 3:]).max() < 2e-6, mode
        assert np.abs(o - o0).max() > 0.02


def test_bokeh_orientation():
    """A mask with texel (row 0, col 0) alone lit, a point on the optical axis: behind the focal plane the pixels that see it lie up
    and to the left of the centre (the mask upright, as the texture looks as a picture), in front of it down and to the right."""
    from radish_pt_amd import hostlib

    W = H = 32
    cam = hostlib.make_camera(W, H, eye=(0, 0, 0), rotation=(-90.0, 0.0, 0.0), fovy=10.0, lens_radius=0.2, focal_dist=4.0)
    tex = np.zeros((4, 4, 3), np.float32)
    tex[0, 0] = 1.0
    mask = _mask(tex)
    view = cam["view"].astype(np.float64)
    rng = np.random.default_rng(0)
    for depth, upper_left in ((8.0, True), (2.0, False)):
        seen = np.zeros(W * H, bool)
        for _ in range(60):
            o, d = LM.lens_rays_f64(cam, W, H, rng.random((W * H, 2)), rng.random((W * H, 2)), LM.MASK, mask)
            p = o + d * (((depth * view - o) @ view) / (d @ view))[:, None]
            seen |= np.linalg.norm(p - depth * view, axis=1) < 0.01 * depth
        ys, xs = np.divmod(np.flatnonzero(seen), W)
        assert len(xs) > 4
        assert (xs.max() < W / 2 and ys.max() < H / 2) if upper_left else (xs.min() >= W / 2 and ys.min() >= H / 2), (depth, xs, ys)


# ---- DISK ----------------------------------------------------------------------------------------------------------------------------
def test_disk_points_are_uniform_on_the_disk():
    rng = np.random.default_rng(12)
    n = 256 * 1024
    rz, rw = rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)
    ax, ay, _ = LM.aperture_f32(LM.DISK, rz, rw)
    ax, ay = ax.astype(np.float64), ay.astype(np.float64)
    r2 = ax * ax + ay * ay
    assert r2.max() <= 1.0 + 1e-6
    assert np.abs(np.sqrt(r2) - np.sqrt(rz.astype(np.float64))).max() < 1e-6  # the radius is sqrt(r.z) ...
    ang = np.arctan2(ay, ax) % (2 * np.pi)
    want = (2 * np.pi * rw.astype(np.float64)) % (2 * np.pi)
    dang = np.abs(ang - want)
    assert np.minimum(dang, 2 * np.pi - dang)[r2 > 1e-6].max() < 1e-5       # ... and the angle 2 pi r.w
    ring = np.minimum((np.minimum(r2, 1.0) * 8).astype(int), 7)               # 8 rings of equal area x 8 sectors
    sector = np.minimum((ang / (2 * np.pi) * 8).astype(int), 7)
    obs = np.bincount(ring * 8 + sector, minlength=64).astype(np.float64)
    p = _chi2_p(obs, np.full(64, n / 64.0))
    print("disk chi2 p", p)
    assert p > P_LEVEL


# ---- MASK ----------------------------------------------------------------------------------------------------------------------------
def _mask_sample(texels, n, seed, plant=None):
    rng = np.random.default_rng(seed)
    rz, rw = rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)
    table, w, h = _mask(texels)
    ax, ay, (k, jx, jy) = LM.aperture_f32(LM.MASK, rz, rw, (table, w, h), plant)
    return ax.astype(np.float64), ay.astype(np.float64), k, jx.astype(np.float64), jy.astype(np.float64)


def _check_texel_frequencies(texels, plant=None):
    """Texels are chosen in proportion to their luminance; zero-weight texels never."""
    n = 400_000
    _, _, k, _, _ = _mask_sample(texels, n, 21, plant)
    wts = LM.mask_weights(texels).astype(np.float64)
    obs = np.bincount(k, minlength=len(wts)).astype(np.float64)
    assert obs[wts == 0].sum() == 0
    lit = wts > 0
    p = _chi2_p(obs[lit], n * wts[lit] / wts.sum())
    print("texel chi2 p", p)
    assert p > P_LEVEL


def _check_points_lie_in_their_texel(texels, plant=None):
    """The aperture point, mapped back through pAperture = (1 - 2u, 1 - 2v), lies in the square of the chosen texel: the mask is
    oriented like the screen, columns along u and rows along v."""
    h, w = texels.shape[:2]
    ax, ay, k, jx, jy = _mask_sample(texels, 100_000, 22, plant)
    u, v = (1.0 - ax) / 2.0, (1.0 - ay) / 2.0
    col, row = k % w, k // w
    eps = 1e-6
    assert ((u * w >= col - eps) & (u * w <= col + 1 + eps)).all(), "u is not in the chosen texel's column"
    assert ((v * h >= row - eps) & (v * h <= row + 1 + eps)).all(), "v is not in the chosen texel's row"
    assert np.abs(u * w - (col + jx)).max() < 1e-5 and np.abs(v * h - (row + jy)).max() < 1e-5


def _check_uniform_inside_a_texel(texels, plant=None):
    """jx and jy are uniform on [0, 1) within a chosen texel — over all texels, and within the texels chosen most often, where a
    texel's own `prob` and the shares it receives from others are both in play."""
    _, _, k, jx, jy = _mask_sample(texels, 400_000, 23, plant)
    assert jx.min() >= 0 and jx.max() < 1 and jy.min() >= 0 and jy.max() < 1
    busiest = np.argsort(np.bincount(k))[-3:]
    for name, j in (("jx", jx), ("jy", jy)):
        for sel, what in [(np.ones(len(k), bool), "all")] + [(k == t, f"texel {t}") for t in busiest]:
            obs = np.bincount(np.minimum((j[sel] * 16).astype(int), 15), minlength=16).astype(np.float64)
            p = _chi2_p(obs, np.full(16, sel.sum() / 16.0))
            print(name, what, int(sel.sum()), p)
            assert p > P_LEVEL, (name, what, p)


MASK_3x2 = np.array([[[0.9, 0.8, 0.1], [0.0, 0.0, 0.0], [0.2, 0.3, 0.9]], [[0.05, 0.1, 0.0], [1.0, 1.0, 1.0], [0.4, 0.1, 0.6]]], np.float32)


def test_mask_texel_frequencies_follow_the_luminance():
    _check_texel_frequencies(MASK_3x2)
    _check_texel_frequencies(_random_mask(16, 16, 4, zeros=40))
    lit = np.zeros((16, 16, 3), np.float32)
    lit[5, 11] = (0.3, 0.2, 0.1)
    _, _, k, _, _ = _mask_sample(lit, 10_000, 5)
    assert (k == 5 * 16 + 11).all()


def test_mask_points_lie_in_their_texel():
    _check_points_lie_in_their_texel(MASK_3x2)
    _check_points_lie_in_their_texel(_random_mask(5, 1, 6))   # 1x5 and 5x1: rows and columns cannot be confused
    _check_points_lie_in_their_texel(_random_mask(1, 5, 7))
    _check_points_lie_in_their_texel(_random_mask(16, 16, 4))


def test_mask_points_are_uniform_inside_a_texel():
    _check_uniform_inside_a_texel(MASK_3x2)
    _check_uniform_inside_a_texel(_random_mask(16, 16, 4))


@pytest.mark.parametrize("plant,check,texels", [
    ("swap_uv", _check_points_lie_in_their_texel, MASK_3x2),
    ("no_flip", _check_points_lie_in_their_texel, MASK_3x2),
    ("jy_raw", _check_uniform_inside_a_texel, MASK_3x2),
])
def test_planted_mistakes_are_caught(plant, check, texels):
    check(texels)
    with pytest.raises(AssertionError):
        check(texels, plant)


def test_mask_table_is_a_distribution():
    """The host's table over the luminances: every entry's own share plus what it receives is its weight's share."""
    for texels in (MASK_3x2, _random_mask(16, 16, 4, zeros=40)):
        table, s = LM.mask_table(texels)
        wts = LM.mask_weights(texels).astype(np.float64)
        n = len(wts)
        got = np.minimum(table["prob"].astype(np.float64), 1.0)
        np.add.at(got, table["failId"], 1.0 - np.minimum(table["prob"].astype(np.float64), 1.0))
        assert np.abs(got / n - wts / wts.sum()).max() < 1e-6
        assert s == pytest.approx(wts.sum(), rel=1e-5)


# ---- kernel resources ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_lens_kernels_stay_within_their_registers():
    """The weight kernel and every lens instantiation that tests/test_kernel_resources.py does not bind already (k_pt_persistent's
    match its prefixes and budgets), compiled from a small translation unit with the library's flags, in the manner of
    test_adaptive_cpu.py.  Bounds: the build's figure (in brackets) rounded up to the 8-register allocation step plus one step,
    where that keeps the occupancy the build reports; no scratch anywhere.  The pinhole kernels keep one symbol each."""
    from radish_pt_amd import _build

    flags = [f for f in _build.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "lens_only.hip")
        with open(src, "w") as f:
            f.write('#include "device/kernels_adaptive.h"\n#include "device/kernels_textures.h"\nnamespace rd {\n'
                    "template __global__ void k_path_trace_mega<false, false, true>(DScene, DCamera, PixelMap, int, int, int, float *, float *, RayDump, DLens);\n"
                    "template __global__ void k_path_trace_direct<false, true>(DScene, DCamera, PixelMap, int, int, float *, DLens);\n"
                    "template __global__ void k_primary_rays<true>(DScene, DCamera, PixelMap, int, float *, DLens);\n}\n")
        cmd = [HIPCC] + flags + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "radish_pt_amd", "csrc"), "-c", src,
                                 "-o", os.path.join(tmp, "x.o"), "-Rpass-analysis=kernel-resource-usage"]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split("\n")[0].split(" ")[0].strip()
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        res[name] = {"vgpr": get("VGPRs"), "scratch": get(r"ScratchSize \[bytes/lane\]"), "occupancy": get(r"Occupancy \[waves/SIMD\]")}
    budgets = [  # (prefix, VGPR bound, waves per SIMD)
        ("_ZN2rd14k_lens_weightsE", 16, 8),                    # [8]
        ("_ZN2rd16k_wf_raygen_lensE", 40, 8),                  # [26]
        ("_ZN2rd16k_ad_raygen_lensE", 40, 8),                  # [26]
        ("_ZN2rd14k_primary_raysILb1EE", 32, 8),               # [18]
        ("_ZN2rd17k_path_trace_megaILb0ELb0ELb1EE", 128, 4),   # [115]; the pinhole's 115
        ("_ZN2rd19k_path_trace_directILb0ELb1EE", 80, 6),      # [80]; the pinhole's 80, at the line of six waves
    ]
    for prefix, vgprs, waves in budgets:
        hits = {k: v for k, v in res.items() if k.startswith(prefix)}
        assert len(hits) == 1, (prefix, sorted(res))
        for name, r in hits.items():
            print(name, r)
            assert r["vgpr"] <= vgprs and r["occupancy"] >= waves and r["scratch"] == 0, (name, r)
    for prefix in ("_ZN2rd11k_wf_raygenE", "_ZN2rd11k_ad_raygenE"):
        assert len([k for k in res if k.startswith(prefix)]) == 1, (prefix, sorted(res))
