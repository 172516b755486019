"""Narrowing the unpinned oracle further.  CPU only; numpy + the oracle, nothing from the device code.

The reference ships no vectors and cannot be compiled here, so parity stays "unpinned": the oracle and the device code are one
author's two restatements.  tests/test_oracle_float64.py re-derived light sampling, reservoirs and a depth-1 path in float64; what
it left open is checked here, each against a statement written from the reference TEXT in a different form (float64, vectorised):

  1. multi-bounce transport: a complete depth-3 `singleKernelPT` (src/pathtrace.cu:149-291) on an analytic scene of horizontal
     quads — bounce loop order, throughput products, normal flipping, NEE of bounce >= 2 going to `indirect`, occlusion BEFORE the
     single-sided test (scene.h:435-448), both MIS weights with their mutually inconsistent pdfs, early termination — per pixel,
     on the same Sobol draws;
  2. the DISTRIBUTIONS the samplers produce: chi-square of `cosineSampleHemisphere` (mathUtil.h:161-166) against cos/pi, of
     `ggxSample` + reflection (material.h:106-126,215-233) against the visible-normal density its construction defines
     (D * G1_Smith * max(0, wo.h) / (n.wo) / (4 wo.h), mixed with the diffuse lobe by 1/(2 - metallic)), and of
     `dielectricSample`'s reflect / refract choice (material.h:159-183) against the exact Fresnel reflectance (:44-64);
  3. `Camera::sample` (sceneStructs.h:72-91) against a float64 pinhole for a rotated camera, random pixels and jitters.

Why not an analytic "white furnace" value: the reference applies HDRToLDR (c / (c + 1)) to EVERY sample before averaging
(pathtrace.cu:285-286) and its NEE / emitter-hit pdfs are mutually inconsistent, so no closed form exists for the
mean of its estimator even in a uniform enclosure; (1) checks the same thing — that energy is carried over several bounces as
the reference text says — sample by sample, which is stronger than a 3-sigma statement about a mean.
"""
import ctypes as C
import math

import numpy as np
import pytest
from scipy import stats

from oracle import pyoracle
from radish_pt_amd import hostlib, layouts as L, scenes

from test_oracle_float64 import _camera_rays_f64, _hit_quads, build_scene, light_pdf_f64, luminance, normalize, sobol_draws

PI = math.pi


# ---------------------------------------------------------------------------------------------------------------------
# 1. depth-3 singleKernelPT in float64
# ---------------------------------------------------------------------------------------------------------------------
def _cosine_dir(n_sign, rx, ry):
    """cosineSampleHemisphere(n = (0, s, 0), rx, ry): concentricSampleDisk is the polar map (sqrt(x), 2 pi y) (mathUtil.h:132-136);
    localRefMatrix(n) for |n.y| > 0.9999 is t = (0,0,1), b = normalize(cross(n, (0,0,1))) = (s,0,0) (mathUtil.h:149-155), so
    mat3(t, b, n) * (dx, dy, dz) = (s dy, s dz, dx)."""
    r, th = np.sqrt(rx), 2.0 * PI * ry
    dx, dy = r * np.cos(th), r * np.sin(th)
    dz = np.sqrt(np.maximum(1.0 - (dx * dx + dy * dy), 0.0))
    return normalize(np.stack([n_sign * dy, n_sign * dz, dx], 1))


def _slab_scene():
    """Horizontal quads only (so the float64 side needs no general triangle code): a floor, a Lambertian ceiling above the lights —
    paths bounce between the two for several bounces instead of leaving the scene — a hovering occluder, and three emissive quads
    wound to face the floor (NEE accepts them) whose authored vertex normals point up (so a BSDF-sampled ray that reaches one
    passes the emitter-hit branch's single-sided test on the INTERPOLATED normal, pathtrace.cu:252-256)."""
    mats = [L.make_material(L.LAMBERTIAN, (0.75, 0.6, 0.5)), L.make_material(L.LAMBERTIAN, (0.3, 0.5, 0.7)),
            L.make_material(L.LAMBERTIAN, (0.8, 0.8, 0.65))]
    verts, norms, ids = [], [], []

    def quad(p0, p1, p2, p3, n, mat):
        verts.extend([p0, p1, p2, p0, p2, p3])
        norms.extend([n] * 6)
        ids.extend([mat, mat])

    quad((-2.5, 0, -2.5), (-2.5, 0, 2.5), (2.5, 0, 2.5), (2.5, 0, -2.5), (0, 1, 0), 0)
    quad((-0.5, 0.6, -0.4), (-0.5, 0.6, 0.4), (0.3, 0.6, 0.4), (0.3, 0.6, -0.4), (0, 1, 0), 1)
    quad((-2.5, 2.4, -2.5), (-2.5, 2.4, 2.5), (2.5, 2.4, 2.5), (2.5, 2.4, -2.5), (0, 1, 0), 2)
    rng = np.random.default_rng(15)
    for q in range(3):
        cx, cz = rng.uniform(-1.2, 1.2, 2)
        hx, hz = rng.uniform(0.35, 0.6, 2)
        mats.append(L.make_material(L.LIGHT, tuple(rng.uniform(2.0, 9.0, 3))))
        y = 2.0 - 0.03 * q
        quad((cx - hx, y, cz - hz), (cx + hx, y, cz - hz), (cx + hx, y, cz + hz), (cx - hx, y, cz + hz), (0, 1, 0), len(mats) - 1)
    v, n = np.array(verts, np.float32), np.array(norms, np.float32)
    return scenes.SceneData("slabs", v, n, np.zeros((len(v), 2), np.float32), np.array(ids, np.int32), np.array(mats, dtype=L.MATERIAL_DTYPE))


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_depth3_path_tracer_vs_float64():
    sd = _slab_scene()
    W, H, looper, D = 72, 44, 11, 3
    cam = hostlib.make_camera(W, H, eye=(0.3, 1.1, 3.6), rotation=(-94.0, -20.0, 0.0), fovy=26.0)
    o = pyoracle.OracleScene(sd)
    ref_d, ref_i = np.zeros((W * H, 3), np.float32), np.zeros((W * H, 3), np.float32)
    o.path_trace(cam, ref_d, ref_i, 0, looper, D)

    n_px = W * H
    u = sobol_draws(sd.sobol, looper, np.arange(n_px), 4 + 7 * D)
    org, dirs = _camera_rays_f64(cam, W, H, u[:, 0:2])
    V = sd.vertices.astype(np.float64).reshape(-1, 3, 3)
    mat_of_tri = sd.material_ids
    # quads: tag = index of the quad's first triangle // 2; floor 0, occluder 1, lights 2..
    quads, albedo, is_light, light_col, tri_area = [], {}, {}, {}, {}
    for q in range(len(V) // 2):
        a, b = V[2 * q], V[2 * q + 1]
        lo, hi = np.minimum(a.min(0), b.min(0)), np.maximum(a.max(0), b.max(0))
        quads.append((lo[1], lo[0], hi[0], lo[2], hi[2], q))
        m = sd.materials[mat_of_tri[2 * q]]
        is_light[q] = int(m["type"]) == L.LIGHT
        albedo[q] = m["baseColor"].astype(np.float64)
        light_col[q] = m["baseColor"].astype(np.float64)
        tri_area[q] = np.linalg.norm(np.cross(a[1] - a[0], a[2] - a[0])) * 0.5
    lightq = np.array([is_light[q] for q in range(len(quads))])

    t, tag = _hit_quads(org, dirs, quads)
    direct, indirect = np.zeros((n_px, 3)), np.zeros((n_px, 3))
    hit_light0 = (tag >= 0) & lightq[np.maximum(tag, 0)]
    direct[(tag < 0) | hit_light0] = 1.0  # miss or an emitter seen directly (pathtrace.cu:169-182)
    alive = (tag >= 0) & ~hit_light0
    pos = org + dirs * t[:, None]
    wo = -dirs
    thr = np.ones((n_px, 3))
    base = np.ones((n_px, 3))  # first hit: material.baseColor = 1 (DENOISER_DEMODULATE, :175-178)
    n_nee = n_bounce_light = 0
    for depth in range(1, D + 1):
        c0 = 4 + 7 * (depth - 1)
        ns = np.where(wo[:, 1] < 0.0, -1.0, 1.0)  # the geometric normal is +y for every quad; flipped to face wo (:190-193)
        nrm = np.stack([np.zeros(n_px), ns, np.zeros(n_px)], 1)
        # ---- NEE (:195-208): occlusion first, then the single-sided test (scene.h:435-448) ----
        lpdf, rad, wi, dist, sampled, valid = light_pdf_f64(sd, pos, u[:, c0:c0 + 4])
        sdir = normalize(sampled - pos)
        so = pos + sdir * 1e-5  # makeOffsetedRay (intersections.h:16-18)
        st, _ = _hit_quads(so, sdir, quads)
        occluded = st < (np.linalg.norm(sampled - pos, axis=1) - 1e-4)
        cos_x = np.maximum(np.einsum("ij,ij->i", nrm, wi), 0.0)
        bsdf_pdf = cos_x / PI
        mis = lpdf ** 2 / (lpdf ** 2 + bsdf_pdf ** 2)
        contrib = thr * (base / PI) * rad * (cos_x / lpdf * mis)[:, None]
        use = alive & ~occluded & valid & (lpdf > 0)
        (direct if depth == 1 else indirect)[use] += contrib[use]
        n_nee += int(use.sum())
        # ---- BSDF sample (material.h:141-147), throughput (:220-223) ----
        sd_dir = _cosine_dir(ns, u[:, c0 + 4], u[:, c0 + 5])
        spdf = np.maximum(np.einsum("ij,ij->i", nrm, sd_dir), 0.0) / PI
        alive = alive & ~(spdf < 1e-8)
        thr = thr * (base / PI) / spdf[:, None] * np.abs(np.einsum("ij,ij->i", nrm, sd_dir))[:, None]
        cur = pos
        o2 = pos + sd_dir * 1e-5
        t2, tag2 = _hit_quads(o2, sd_dir, quads)
        alive = alive & (tag2 >= 0)  # a miss ends the path (no env map; tests/path_model.py has the miss branch with one)
        hp = o2 + sd_dir * t2[:, None]
        hl = alive & lightq[np.maximum(tag2, 0)]
        # emitter hit (:251-271): single-sided test on the INTERPOLATED normal (authored +y here): break if dot(norm, dir) < 0
        collect = hl & ~(sd_dir[:, 1] < 0.0)
        for q in np.unique(tag2[collect]):
            sel = collect & (tag2 == q)
            col = light_col[q]
            pdf_area = luminance(col) * float(sd.sum_light_power_inv) * tri_area[q]  # sic: times the area
            yx = cur - hp
            lp = pdf_area * np.einsum("ij,ij->i", yx, yx) / np.abs(normalize(yx)[:, 1])
            w = spdf ** 2 / (spdf ** 2 + lp ** 2)
            indirect[sel] += (col * thr * w[:, None])[sel]
            n_bounce_light += int(sel.sum())
        alive = alive & ~hl
        pos, wo = hp, -sd_dir
        base = np.stack([albedo[q] for q in np.maximum(tag2, 0)], 0)
    deep = (np.abs(indirect).sum(1) > 0).sum()
    assert n_nee > 1500 and n_bounce_light > 60 and deep > 300, (n_nee, n_bounce_light, deep)  # bounces >= 2 really contribute
    want_d, want_i = direct / (direct + 1.0), indirect / (indirect + 1.0)  # HDRToLDR (mathUtil.h:49-51), iter = 0
    bad = (np.abs(ref_d - want_d) > 2e-4 * np.maximum(np.abs(want_d), 1e-3)).any(1) | (np.abs(ref_i - want_i) > 2e-4 * np.maximum(np.abs(want_i), 1e-3)).any(1)
    # float32 vs float64 can classify a ray differently exactly at a quad's border or a triangle diagonal, and then the whole
    # path differs: a fraction of a percent of the pixels at most
    assert bad.sum() <= 0.004 * n_px, f"{bad.sum()} of {n_px} pixels differ from the float64 depth-{D} re-derivation; first {np.argwhere(bad)[:6].ravel()}"


# ---------------------------------------------------------------------------------------------------------------------
# 2. sampling distributions
# ---------------------------------------------------------------------------------------------------------------------
def _lib():
    return pyoracle.lib()


def _sample_many(mat, n, wo, r):
    """Material::sample for every row of r (N x 3) -> (dir [N,3], pdf [N], type [N])."""
    buf = np.frombuffer(mat.tobytes(), np.uint8).copy()
    n32, wo32 = np.ascontiguousarray(n, np.float32), np.ascontiguousarray(wo, np.float32)
    r32 = np.ascontiguousarray(r, np.float32)
    out = np.zeros((len(r32), 8), np.float32)
    fn = _lib().orc_material_eval
    bp, np_, wp = buf.ctypes.data, n32.ctypes.data, wo32.ctypes.data
    rb, ob = r32.ctypes.data, out.ctypes.data
    for k in range(len(r32)):
        fn(bp, 2, np_, wp, rb + 12 * k, ob + 32 * k)
    return out[:, :3].astype(np.float64), out[:, 6].astype(np.float64), out[:, 7].copy().view(np.uint32)


def _frame(n):
    n = normalize(np.asarray(n, np.float64))
    a = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    t = normalize(np.cross(n, a))
    return t, np.cross(n, t), n


NC, NP = 6, 12  # bins in cos(theta) x phi of the hemisphere around n


def _bin(dirs, n):
    t, b, nn = _frame(n)
    c = dirs @ nn
    ph = np.arctan2(dirs @ b, dirs @ t) % (2 * PI)
    ci = np.minimum((np.clip(c, 0, 1) * NC).astype(int), NC - 1)
    pi_ = np.minimum((ph / (2 * PI) * NP).astype(int), NP - 1)
    return ci * NP + pi_


def _expected(density, n, sub=40):
    """Integral of density(wi) d omega over every bin (d omega = d cos(theta) d phi), midpoint rule sub x sub per bin."""
    t, b, nn = _frame(n)
    out = np.zeros(NC * NP)
    ks = (np.arange(sub) + 0.5) / sub
    for ci in range(NC):
        c = (ci + ks) / NC
        s = np.sqrt(1 - c * c)
        for pi_ in range(NP):
            ph = (pi_ + ks) / NP * 2 * PI
            cc, pp = np.meshgrid(c, ph, indexing="ij")
            ss = np.sqrt(1 - cc * cc)
            w = (ss * np.cos(pp))[..., None] * t + (ss * np.sin(pp))[..., None] * b + cc[..., None] * nn
            out[ci * NP + pi_] = density(w.reshape(-1, 3)).mean() * (1.0 / NC) * (2 * PI / NP)
    return out


def _chi2_ok(counts, probs, n_total, what):
    # merge bins with a small expectation, add the "everything else" bin (directions under the horizon / invalid samples)
    rest_p = max(1.0 - probs.sum(), 0.0)
    rest_c = n_total - counts.sum()
    exp = np.append(probs, rest_p) * n_total
    obs = np.append(counts, rest_c).astype(np.float64)
    keep = exp >= 8
    obs_m = np.append(obs[keep], obs[~keep].sum())
    exp_m = np.append(exp[keep], exp[~keep].sum())
    if exp_m[-1] < 1e-9:
        obs_m, exp_m = obs_m[:-1], exp_m[:-1]
    chi2 = ((obs_m - exp_m) ** 2 / np.maximum(exp_m, 1e-12)).sum()
    p = stats.chi2.sf(chi2, len(exp_m) - 1)
    assert p > 1e-4, f"{what}: chi2 = {chi2:.1f} over {len(exp_m)} bins, p = {p:.2e}"
    return p


def _ggx_vndf_density(alpha, n, wo):
    """Density over wi of `-reflect(wo, h)` with h drawn from the distribution of visible normals of GGX(alpha) — what ggxSample's
    construction (Heitz 2018: stretch, orthonormal basis, disk sample warped by s = (1 + vh.z)/2, unstretch) produces:
    D_v(h) = D(h) G1(wo) max(0, wo.h) / (n.wo) with the SMITH G1 of GGX, and d omega_h = d omega_i / (4 wo.h)."""
    t, b, nn = _frame(n)

    def dens(wi):
        h = normalize(wi + wo)
        ch = h @ nn
        a2 = alpha * alpha
        D = a2 / (PI * (ch * ch * (a2 - 1) + 1) ** 2)
        co = wo @ nn
        tan2 = (1 - co * co) / (co * co)
        G1 = 2.0 / (1.0 + math.sqrt(1.0 + a2 * tan2))
        woh = h @ wo
        return np.where((woh > 0) & (ch > 0), D * G1 * np.maximum(woh, 0) / co / (4 * np.maximum(woh, 1e-12)), 0.0)

    return dens


@pytest.mark.parametrize("case", ["lambertian", "metal_rough", "metal_mixture"])
def test_bsdf_sampling_distributions_chi_square(case):
    rng = np.random.default_rng({"lambertian": 1, "metal_rough": 2, "metal_mixture": 3}[case])
    n = normalize(np.array([0.2, 1.0, -0.3]))
    wo = normalize(np.array([0.5, 0.7, 0.2]))
    N = 60000
    r = rng.uniform(0, 1, (N, 3))
    if case == "lambertian":
        mat = L.make_material(L.LAMBERTIAN, (0.5, 0.6, 0.7))
        dens = lambda wi: np.maximum(wi @ n, 0) / PI
    else:
        metallic, rough = (1.0, 0.6) if case == "metal_rough" else (0.4, 0.5)
        mat = L.make_material(L.METALLIC_WORKFLOW, (0.8, 0.7, 0.6), metallic=metallic, roughness=rough)
        a = 1.0 / (2.0 - metallic)  # probability of the specular lobe: r.z <= 1/(2 - metallic) (material.h:219)
        spec = _ggx_vndf_density(rough * rough, n, wo)
        dens = lambda wi: (1 - a) * np.maximum(wi @ n, 0) / PI + a * spec(wi)
    d, pdf, typ = _sample_many(mat, n, wo, r)
    valid = typ != (1 << 15)  # BSDFSampleType::Invalid
    assert valid.mean() > 0.8
    assert np.allclose(np.linalg.norm(d[valid], axis=1), 1.0, atol=1e-5)
    assert (d[valid] @ n >= -1e-6).all()
    counts = np.bincount(_bin(d[valid], n), minlength=NC * NP)
    probs = _expected(dens, n)
    _chi2_ok(counts, probs, N, case)
    # the pdf returned with a sample is Material::pdf at that direction
    buf = np.frombuffer(mat.tobytes(), np.uint8).copy()
    out = np.zeros(8, np.float32)
    n32, wo32 = np.ascontiguousarray(n, np.float32), np.ascontiguousarray(wo, np.float32)
    for k in np.flatnonzero(valid)[:200]:
        w32 = np.ascontiguousarray(d[k], np.float32)
        _lib().orc_material_eval(buf.ctypes.data, 1, n32.ctypes.data, wo32.ctypes.data, w32.ctypes.data, out.ctypes.data)
        assert out[0] == pytest.approx(pdf[k], rel=2e-4, abs=1e-7)


def _fresnel_exact(cos_in, ior):  # material.h:44-64 (MATERIAL_DIELECTRIC_USE_SCHLICK_APPROX undefined -> exact), written from Snell
    if cos_in < 0:
        ior, cos_in = 1.0 / ior, -cos_in
    sin_tr = math.sqrt(max(0.0, 1 - cos_in * cos_in)) / ior
    if sin_tr >= 1.0:
        return 1.0
    cos_tr = math.sqrt(1 - sin_tr * sin_tr)
    rpa = (cos_in - ior * cos_tr) / (cos_in + ior * cos_tr)
    rpe = (ior * cos_in - cos_tr) / (ior * cos_in + cos_tr)
    return 0.5 * (rpa * rpa + rpe * rpe)


@pytest.mark.parametrize("cos_o", [0.95, 0.5, 0.15, -0.9, -0.8])
def test_dielectric_reflect_refract_frequencies(cos_o):
    ior = 1.5
    n = np.array([0.0, 1.0, 0.0])
    wo = np.array([math.sqrt(1 - cos_o * cos_o), cos_o, 0.0])
    mat = L.make_material(L.DIELECTRIC, (1, 1, 1), ior=ior)
    N = 20000
    r = np.random.default_rng(7).uniform(0, 1, (N, 3))
    d, pdf, typ = _sample_many(mat, n, wo, r)
    F = _fresnel_exact(cos_o, ior)
    refl = (typ & 16) != 0  # Reflection
    trans = (typ & 32) != 0  # Transmission
    invalid = typ == (1 << 15)
    assert (refl | trans | invalid).all()
    k = int(refl.sum())
    # two-sided binomial test against the exact reflectance
    assert stats.binomtest(k, N, min(max(F, 0.0), 1.0)).pvalue > 1e-4 if 0 < F < 1 else k == N, (k / N, F)
    # geometry: reflected rays are the mirror direction, refracted ones obey Snell's law
    mirror = 2 * (n @ wo) * n - wo
    assert np.allclose(d[refl], mirror, atol=2e-6)
    if trans.any():
        eta = ior if cos_o > 0 else 1.0 / ior
        sin_t = math.sqrt(1 - cos_o * cos_o) / eta
        assert np.allclose(np.abs(d[trans][:, 0]), sin_t, atol=2e-6) and (np.sign(d[trans][:, 1]) == -np.sign(cos_o)).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. Camera::sample against a float64 pinhole
# ---------------------------------------------------------------------------------------------------------------------
def test_camera_sample_vs_float64_pinhole():
    W, H = 320, 180
    cam = hostlib.make_camera(W, H, eye=(1.5, 0.7, -2.0), rotation=(37.0, -18.0, 0.0), fovy=21.0)
    buf = np.frombuffer(cam.tobytes(), np.uint8).copy()
    rng = np.random.default_rng(3)
    # float64 pinhole from the camera's OWN basis vectors (Camera::update's output is checked in tests/test_scene_loader.py)
    right, up, view = (cam[k].astype(np.float64) for k in ("right", "up", "view"))
    tan_fov = math.tan(math.radians(float(cam["fov"][1])))  # sic: the full fov.y as the half angle
    out = np.zeros(6, np.float32)
    worst = 0.0
    for _ in range(500):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        r4 = rng.uniform(0, 1, 4).astype(np.float32)
        _lib().orc_camera_sample(buf.ctypes.data, x, y, r4.ctypes.data, out.ctypes.data)
        ru = 1.0 - 2.0 * (x + float(r4[0])) / W  # NDC mirrored (:79)
        rv = 1.0 - 2.0 * (y + float(r4[1])) / H
        p = np.array([ru * (W / H) * tan_fov, rv * tan_fov, 1.0]) * float(cam["focalDist"])
        d = normalize(p[0] * right + p[1] * up + p[2] * view)
        assert np.array_equal(out[:3], cam["position"])  # pAperture = 0 (:81): the lens sample r.zw is unused
        worst = max(worst, float(np.abs(out[3:] - d).max()))
    assert worst < 3e-7
