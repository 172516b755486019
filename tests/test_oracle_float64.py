"""Independent float64 re-derivations of the parts of the path where the round-1 KATs were thin.

The oracle (oracle/oracle.cpp) and the device code are one author's two restatements of the reference, so a shared misreading
would pass every bit-exact parity test.  The reference holds no fixtures (parity stays "unpinned"); what narrows the gap is a
THIRD, differently structured statement of the same formulas — numpy, float64, vectorised, written from the reference text —
checked against the oracle:

  * `sampleDirectLight` / `sampleDirectLightNoVisibility` pdfs, radiance, wi, dist      (src/scene.h:419-492)
  * `Reservoir::merge / preClampedMerge / update / checkValidity / W`                   (src/restir.h:10-92)
  * a complete depth-1 `singleKernelPT` on an analytic scene: camera, NEE with the power-heuristic MIS weight, Lambertian
    sampling, the emitter-hit MIS weight, HDRToLDR                                       (src/pathtrace.cu:149-291)
  * statistics: the mean of 256 frames of two-pass ReSTIR (corrected RIS) against a brute-force quadrature over all lights of
    the integral the reference's estimator defines                                       (src/restir.cu:97-203)
These use horizontal Lambertian quads with one authored normal each, zero texcoords, no textures and no environment map; what a
general triangle, a texture, the environment map, glass or metal adds to the path is stated in tests/path_model.py and checked by
tests/test_path_model_cpu.py and tests/test_gpu_path_model.py.
All CPU (`-m "not gpu"`); the GPU is bit-equal to the oracle by the parity tests, so what holds for the oracle holds for it.
"""
import numpy as np
import pytest

from oracle import pyoracle
from radish_pt_amd import hostlib, layouts as L, scenes

PI = np.pi


# ---------------------------------------------------------------------------------------------------------------------
# float64 helpers, written from the reference text
# ---------------------------------------------------------------------------------------------------------------------
def utilhash(a):  # src/mathUtil.h:199-207 on uint32 arrays
    a = np.asarray(a, np.uint64)
    M = np.uint64(0xFFFFFFFF)
    a = ((a + np.uint64(0x7ED55D16)) + (a << np.uint64(12))) & M
    a = ((a ^ np.uint64(0xC761C23C)) ^ (a >> np.uint64(19))) & M
    a = ((a + np.uint64(0x165667B1)) + (a << np.uint64(5))) & M
    a = ((a + np.uint64(0xD3A2646C)) ^ (a << np.uint64(9))) & M
    a = ((a + np.uint64(0xFD7046C5)) + (a << np.uint64(3))) & M
    a = ((a ^ np.uint64(0xB55A4F09)) ^ (a >> np.uint64(16))) & M
    return a


def sobol_draws(sobol, looper, pixel_index, count):
    """The first `count` draws of every pixel's Sampler (src/sampler.h:15-37): value k = (table[looper*200 + k] XOR h_k) * 2^-32,
    h_0 = utilhash(index), h_{k+1} = utilhash(h_k).  float32 conversion as `r * 0x1p-32f` does (round to nearest)."""
    h = utilhash(np.asarray(pixel_index, np.uint64))
    out = np.zeros((len(h), count))
    row = sobol[looper].astype(np.uint64)
    for k in range(count):
        r = (row[k] ^ h).astype(np.uint32)
        out[:, k] = (r.astype(np.float32) * np.float32(2.0 ** -32)).astype(np.float64)
        h = utilhash(h)
    return out


def normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def luminance(c):  # src/mathUtil.h:128-130
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def sample_triangle_uniform(v0, v1, v2, ru, rv):  # src/mathUtil.h:100-108
    r = np.sqrt(rv)
    u = 1.0 - r
    v = ru * r
    return v1 * u[..., None] + v2 * v[..., None] + v0 * (1.0 - u - v)[..., None]


def alias_pick(table, r1, r2):  # DevDiscreteSampler1D::sample, src/sampler.h:204-208
    n = len(table)
    pass_id = np.minimum((np.float32(n) * r1.astype(np.float32)).astype(np.int64), n - 1)
    prob = table["prob"][pass_id].astype(np.float64)
    return np.where(r2 < prob, pass_id, table["failId"][pass_id])


def light_pdf_f64(sd, pos, r4):
    """sampleDirectLightNoVisibility (src/scene.h:458-492) for arrays of positions and draws: (pdf, radiance, wi, dist, sampled)."""
    lid = alias_pick(sd.light_sampler, r4[:, 0], r4[:, 1])
    prim = sd.light_prim_ids[lid]
    V = sd.vertices.astype(np.float64).reshape(-1, 3, 3)
    v0, v1, v2 = V[prim, 0], V[prim, 1], V[prim, 2]
    sampled = sample_triangle_uniform(v0, v1, v2, r4[:, 2], r4[:, 3])
    cr = np.cross(v1 - v0, v2 - v0)
    normal = normalize(cr)
    to = sampled - pos
    valid = ~(np.einsum("ij,ij->i", normal, to) > -1e-6)  # SCENE_LIGHT_SINGLE_SIDED: reject unless the light faces pos
    area = np.linalg.norm(cr, axis=1) * 0.5
    radiance = sd.light_unit_radiance.astype(np.float64)[lid]
    dist = np.linalg.norm(to, axis=1)
    wi = to / dist[:, None]
    power = luminance(radiance) / (area * 2.0 * PI)  # sic: the reference divides where its selection weight multiplies
    yx = pos - sampled
    pdf = power * float(sd.sum_light_power_inv) * np.einsum("ij,ij->i", yx, yx) / np.abs(np.einsum("ij,ij->i", normal, normalize(yx)))
    return np.where(valid, pdf, -1.0), radiance, wi, dist, sampled, valid


def build_scene(light_normals_up=False, occluder=True, n_light_quads=6, light_half=(0.08, 0.3)):
    """Floor quad, an optional hovering occluder, and `n_light_quads` small emissive quads (2 triangles each) at y = 2 whose
    WINDING faces the floor (so NEE accepts them).  light_normals_up authors their vertex normals pointing away from the floor:
    the emitter-hit branch of singleKernelPT tests `dot(intersec.norm, ray.direction) < 0` with the INTERPOLATED normal
    (pathtrace.cu:252-256), so this is what lets a BSDF-sampled ray collect emission and exercises that MIS weight."""
    floor = L.make_material(L.LAMBERTIAN, (0.75, 0.6, 0.5))
    block = L.make_material(L.LAMBERTIAN, (0.3, 0.5, 0.7))
    mats = [floor, block]
    verts, norms, ids = [], [], []

    def quad(p0, p1, p2, p3, n, mat):
        verts.extend([p0, p1, p2, p0, p2, p3])
        norms.extend([n] * 6)
        ids.extend([mat, mat])

    quad((-2, 0, -2), (-2, 0, 2), (2, 0, 2), (2, 0, -2), (0, 1, 0), 0)  # winding normal +y
    if occluder:
        quad((-0.5, 0.6, -0.4), (-0.5, 0.6, 0.4), (0.3, 0.6, 0.4), (0.3, 0.6, -0.4), (0, 1, 0), 1)
    rng = np.random.default_rng(5)
    for q in range(n_light_quads):
        cx, cz = rng.uniform(-1.4, 1.4, 2)
        hx, hz = rng.uniform(light_half[0], light_half[1], 2)
        col = tuple(rng.uniform(2.0, 9.0, 3))
        mats.append(L.make_material(L.LIGHT, col))
        m = len(mats) - 1
        y = 2.0 - 0.01 * q
        # winding normal -y (faces the floor)
        quad((cx - hx, y, cz - hz), (cx + hx, y, cz - hz), (cx + hx, y, cz + hz), (cx - hx, y, cz + hz),
             (0, 1, 0) if light_normals_up else (0, -1, 0), m)
    v = np.array(verts, np.float32)
    n = np.array(norms, np.float32)
    t = np.zeros((len(v), 2), np.float32)
    return scenes.SceneData("kat", v, n, t, np.array(ids, np.int32), np.array(mats, dtype=L.MATERIAL_DTYPE))


# ---------------------------------------------------------------------------------------------------------------------
# 1. light sampler
# ---------------------------------------------------------------------------------------------------------------------
def test_sample_direct_light_pdfs_vs_float64():
    sd = build_scene()
    assert sd.num_lights == 12
    o = pyoracle.OracleScene(sd)
    rng = np.random.default_rng(1)
    n = 4000
    # heights away from the lights' plane (y ~ 2), where float32's cos(light) cancels catastrophically; some points ABOVE the lights
    ys = np.where(rng.random(n) < 0.85, rng.uniform(0.0, 1.6, n), rng.uniform(2.15, 2.4, n))
    pos = np.stack([rng.uniform(-1.9, 1.9, n), ys, rng.uniform(-1.9, 1.9, n)], 1)
    r4 = rng.random((n, 4))
    r4[:50, 0] = 1.0  # Sampler::sample can return exactly 1.0f: the index clamp
    pos, r4 = pos.astype(np.float32).astype(np.float64), r4.astype(np.float32).astype(np.float64)  # the inputs the oracle sees
    pdf, rad, wi, dist, sampled, valid = light_pdf_f64(sd, pos, r4)
    assert 0.3 < valid.mean() < 0.98
    occluded = o.trace_occluded(np.concatenate([pos, sampled], 1).astype(np.float32)).astype(bool)
    assert 0.02 < occluded[valid].mean() < 0.9
    for i in range(n):
        p0, rad0, wi0, d0 = o.sample_direct_light(pos[i], r4[i], visibility=False)
        if not valid[i]:
            assert p0 == -1.0
            continue
        assert p0 == pytest.approx(pdf[i], rel=5e-5), i
        assert np.allclose(rad0, rad[i], rtol=1e-6) and np.allclose(wi0, wi[i], atol=2e-6) and d0 == pytest.approx(dist[i], rel=2e-6)
        # with visibility: the shadow ray is traced BEFORE the single-sided test (Q6) and an occluded sample is rejected
        p1, rad1, wi1, _ = o.sample_direct_light(pos[i], r4[i], visibility=True)
        if occluded[i]:
            assert p1 == -1.0
        else:
            assert p1 == p0 and np.array_equal(rad1, rad0) and np.array_equal(wi1, wi0)


def test_light_selection_matches_power_distribution():
    """The alias table (scene.cpp:145-169, sampler.h:81-125) must select light l with probability power_l / sum, power_l =
    luminance * 2 pi * area (scene.cpp:211-216): exact, by summing the table's mass per light in float64."""
    sd = build_scene()
    t = sd.light_sampler
    n = len(t)
    mass = np.zeros(n)
    for i in range(n):
        mass[i] += float(t["prob"][i]) / n
        mass[int(t["failId"][i])] += (1.0 - float(t["prob"][i])) / n
    V = sd.vertices.astype(np.float64).reshape(-1, 3, 3)[sd.light_prim_ids]
    area = np.linalg.norm(np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]), axis=1) * 0.5
    power = luminance(sd.light_unit_radiance.astype(np.float64)) * 2.0 * PI * area
    assert np.allclose(mass, power / power.sum(), rtol=2e-5)
    assert float(sd.sum_light_power_inv) == pytest.approx(1.0 / power.sum(), rel=1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# 2. reservoir arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def _smp(r):  # the `sample` member of a reservoir record, as bytes
    return r["Li"].tobytes() + r["wi"].tobytes() + r["dist"].tobytes()


def _resv(rng, weight=None, num=None):
    r = np.zeros(1, L.RESERVOIR_DTYPE)
    r["Li"] = rng.uniform(0, 5, 3)
    r["wi"] = normalize(rng.normal(size=3))
    r["dist"] = rng.uniform(0.5, 4)
    r["numSamples"] = rng.integers(0, 700) if num is None else num
    r["weight"] = rng.uniform(0, 50) if weight is None else weight
    return r


def test_reservoir_arithmetic_vs_restir_h():
    rng = np.random.default_rng(3)
    f32 = np.float32
    for trial in range(3000):
        a, b = _resv(rng), _resv(rng)
        if trial % 7 == 0:
            b["weight"] = 0.0
        if trial % 11 == 0:
            a["numSamples"] = 0
        rnd = f32(rng.random())
        # merge (restir.h:51-58): weights and counts add; rhs's sample wins iff rnd * (new weight) < rhs.weight
        m = pyoracle.reservoir_op(0, a, b, rnd)
        w = f32(a["weight"][0]) + f32(b["weight"][0])
        assert m["weight"][0] == w and m["numSamples"][0] == a["numSamples"][0] + b["numSamples"][0]
        take = f32(rnd * w) < f32(b["weight"][0])
        assert _smp(m) == _smp(b if take else a)
        # preClampedMerge<20> (restir.h:69-77): rhs is scaled down to (M-1) * own count when it has more
        M = 20
        c = pyoracle.reservoir_op(1, a, b, rnd, M)
        na, nb = int(a["numSamples"][0]), int(b["numSamples"][0])
        bw, bn = f32(b["weight"][0]), nb
        if nb > 0 and nb > (M - 1) * na and na > 0:
            bw = f32(bw * f32(f32(f32(M - 1) * f32(na)) / f32(nb)))
            bn = (M - 1) * na
        w2 = f32(a["weight"][0]) + bw
        assert c["weight"][0] == w2 and c["numSamples"][0] == na + bn
        take = f32(rnd * w2) < bw
        assert _smp(c) == _smp(b if take else a)
        # update (restir.h:17-24): as written the NEW candidate always wins unless rnd * weight / newWeight is exactly 0
        # (NaN and inf are truthy); the corrected form is weighted reservoir sampling
        for new_w in (f32(b["weight"][0]), f32(0.0)):
            cand = b.copy()
            cand["weight"] = new_w
            u = pyoracle.reservoir_op(2, a, cand, rnd)
            w3 = f32(a["weight"][0]) + new_w
            assert u["weight"][0] == w3 and u["numSamples"][0] == na + 1
            with np.errstate(divide="ignore", invalid="ignore"):
                expr = f32(rnd * w3) / new_w
            truthy = bool(expr != 0) or bool(np.isnan(expr))
            assert _smp(u) == _smp(cand if truthy else a)
            k = pyoracle.reservoir_op(3, a, cand, rnd)
            assert _smp(k) == _smp(cand if f32(rnd * w3) < new_w else a)
    # checkValidity (restir.h:42-49): NaN / inf / negative weight clears weight and count but keeps the stale sample (Q3)
    for bad in (np.nan, np.inf, -1.0):
        a = _resv(rng, weight=bad, num=17)
        c = pyoracle.reservoir_op(4, a, a, 0.5)
        assert c["weight"][0] == 0 and c["numSamples"][0] == 0 and _smp(c) == _smp(a)
    a = _resv(rng, weight=3.0, num=5)
    assert pyoracle.reservoir_op(4, a, a, 0.5).tobytes() == a.tobytes()


def test_reservoir_W_vs_float64():
    """W = weight / (|Li * BSDF * satDot(n, wi)| * numSamples) (restir.h:31-40) with the Lambertian BSDF c / pi."""
    rng = np.random.default_rng(4)
    for _ in range(500):
        r = _resv(rng, num=int(rng.integers(1, 200)))
        col = rng.uniform(0.1, 1.0, 3)
        mat = L.make_material(L.LAMBERTIAN, tuple(col))
        n = normalize(rng.normal(size=3)).astype(np.float32).astype(np.float64)  # what the oracle sees
        if np.dot(n, r["wi"][0]) < 0:
            n = -n
        if np.dot(n, r["wi"][0]) < 0.2:  # away from grazing, where float32's cosine loses digits
            continue
        wo = normalize(rng.normal(size=3))
        p_hat = r["Li"][0].astype(np.float64) * (mat["baseColor"].astype(np.float64) / PI) * max(float(np.dot(n, r["wi"][0].astype(np.float64))), 0.0)
        want = float(r["weight"][0]) / (np.linalg.norm(p_hat) * int(r["numSamples"][0]))
        got = pyoracle.reservoir_W(r, mat, n, wo)
        if np.linalg.norm(p_hat) < 1e-6:
            continue
        assert got == pytest.approx(want, rel=5e-5)
    assert pyoracle.power_heuristic(3.0, 4.0) == pytest.approx(9.0 / 25.0, rel=1e-6)  # mathUtil.h:81-84


# ---------------------------------------------------------------------------------------------------------------------
# 3. depth-1 singleKernelPT in float64 on an analytic scene: both MIS weights
# ---------------------------------------------------------------------------------------------------------------------
def _camera_rays_f64(cam, W, H, jitter):
    """Camera::sample (src/sceneStructs.h:72-91): pinhole, NDC mirrored, tanFovY = tan(radians(fov.y)) of the FULL fov.y."""
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.reshape(-1).astype(np.float64), y.reshape(-1).astype(np.float64)
    aspect = W / H
    tan_fov = np.tan(np.radians(float(cam["fov"][1])))
    ruv = np.stack([(x + jitter[:, 0]) / W, (y + jitter[:, 1]) / H], 1)
    ruv = 1.0 - ruv * 2.0
    d = np.stack([ruv[:, 0] * aspect * tan_fov, ruv[:, 1] * tan_fov, np.ones_like(x)], 1) * float(cam["focalDist"])
    right, up, view = (cam[k].astype(np.float64) for k in ("right", "up", "view"))
    dirs = normalize(d[:, :1] * right + d[:, 1:2] * up + d[:, 2:3] * view)
    return np.broadcast_to(cam["position"].astype(np.float64), dirs.shape), dirs


def _hit_quads(o, d, quads):
    """Closest hit of rays with axis-aligned horizontal quads [(y, x0, x1, z0, z1, tag)]: (t, tag) with tag -1 for a miss."""
    best_t = np.full(len(o), np.inf)
    best = np.full(len(o), -1)
    for (qy, x0, x1, z0, z1, tag) in quads:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (qy - o[:, 1]) / d[:, 1]
        p = o + d * t[:, None]
        ok = (t > 0) & (p[:, 0] >= x0) & (p[:, 0] <= x1) & (p[:, 2] >= z0) & (p[:, 2] <= z1) & (t < best_t)
        best_t = np.where(ok, t, best_t)
        best = np.where(ok, tag, best)
    return best_t, best


@pytest.mark.filterwarnings("ignore::RuntimeWarning")  # rays that miss every quad divide by zero on purpose
def test_depth1_path_tracer_vs_float64_mis():
    sd = build_scene(light_normals_up=True, occluder=False, n_light_quads=2, light_half=(0.5, 0.8))
    W, H, looper = 64, 40, 7
    cam = hostlib.make_camera(W, H, eye=(0.2, 1.2, 3.4), rotation=(-92.0, -24.0, 0.0), fovy=24.0)
    o = pyoracle.OracleScene(sd)
    ref_d, ref_i = np.zeros((W * H, 3), np.float32), np.zeros((W * H, 3), np.float32)
    o.path_trace(cam, ref_d, ref_i, 0, looper, 1)

    idx = np.arange(W * H)
    u = sobol_draws(sd.sobol, looper, idx, 11)  # 4 camera + 4 NEE + 3 BSDF (pathtrace.cu: sample4D, sample4D, sample3D)
    org, dirs = _camera_rays_f64(cam, W, H, u[:, 0:2])
    V = sd.vertices.astype(np.float64).reshape(-1, 3, 3)
    quads = [(0.0, -2, 2, -2, 2, 0)]
    light_col = {}
    for q in range(2):
        tri = V[2 + 2 * q]
        lo, hi = np.minimum(tri.min(0), V[3 + 2 * q].min(0)), np.maximum(tri.max(0), V[3 + 2 * q].max(0))
        quads.append((lo[1], lo[0], hi[0], lo[2], hi[2], 1 + q))
        light_col[1 + q] = sd.materials["baseColor"][sd.material_ids[2 + 2 * q]].astype(np.float64)
    t, tag = _hit_quads(org, dirs, quads)
    direct = np.zeros((W * H, 3))
    indirect = np.zeros((W * H, 3))
    direct[tag != 0] = 1.0  # miss, or a light seen directly (pathtrace.cu:169-182)
    fl = tag == 0
    pos = org + dirs * t[:, None]
    n = np.tile(np.array([0.0, 1.0, 0.0]), (W * H, 1))  # floor normal faces wo = -dir (dir.y < 0)
    # ---- NEE with the power heuristic (pathtrace.cu:195-208); material.baseColor = 1 (DENOISER_DEMODULATE) ----
    lpdf, rad, wi, dist, sampled, valid = light_pdf_f64(sd, pos, u[:, 4:8])
    cos_x = np.maximum(np.einsum("ij,ij->i", n, wi), 0.0)
    bsdf_pdf = cos_x / PI
    mis = lpdf ** 2 / (lpdf ** 2 + bsdf_pdf ** 2)
    nee = (1.0 / PI) * rad * (cos_x / lpdf * mis)[:, None]
    use = fl & valid & (lpdf > 0)
    direct[use] += nee[use]
    # ---- Lambertian sample (material.h:141-147) -> extension ray -> emitter hit with MIS (pathtrace.cu:251-271) ----
    r, theta = np.sqrt(u[:, 8]), 2.0 * PI * u[:, 9]
    dx, dy = r * np.cos(theta), r * np.sin(theta)
    dz = np.sqrt(np.maximum(1.0 - (dx * dx + dy * dy), 0.0))
    # localRefMatrix(n = +y): t0 = (0,0,1) because |n.y| > 0.9999; b = normalize(cross(n, t0)) = (1,0,0); t = cross(b, n) = (0,0,1)
    sdir = normalize(dx[:, None] * np.array([0.0, 0.0, 1.0]) + dy[:, None] * np.array([1.0, 0.0, 0.0]) + dz[:, None] * n)
    spdf = np.maximum(np.einsum("ij,ij->i", n, sdir), 0.0) / PI
    alive = fl & ~(spdf < 1e-8)
    thr = (1.0 / PI) / spdf * np.abs(np.einsum("ij,ij->i", n, sdir))
    o2 = pos + sdir * 1e-5
    t2, tag2 = _hit_quads(o2, sdir, quads[1:])
    hitl = alive & (tag2 > 0)
    # single-sided test with the INTERPOLATED normal (authored +y): dot(norm, dir) < 0 would break; here dir.y > 0 -> passes
    for q in (1, 2):
        sel = hitl & (tag2 == q)
        if not sel.any():
            continue
        col = light_col[q]
        hp = o2 + sdir * t2[:, None]
        tri_area = np.linalg.norm(np.cross(V[2 * q, 1] - V[2 * q, 0], V[2 * q, 2] - V[2 * q, 0])) * 0.5  # getPrimitiveArea of ONE triangle
        pdf_area = luminance(col) * float(sd.sum_light_power_inv) * tri_area  # sic: multiplies by the area
        yx = pos - hp
        lp = pdf_area * np.einsum("ij,ij->i", yx, yx) / np.abs(normalize(yx)[:, 1])  # |dot((0,1,0), normalize(yx))|
        wgt = spdf ** 2 / (spdf ** 2 + lp ** 2)
        indirect[sel] += (col * (thr * wgt)[:, None])[sel]
    assert hitl.sum() > 30 and use.sum() > 500
    want_d, want_i = direct / (direct + 1.0), indirect / (indirect + 1.0)  # HDRToLDR (mathUtil.h:49-51), iter = 0
    # the two triangles of a light quad have equal areas here, so tri_area above is right for either
    bad = (np.abs(ref_d - want_d) > 1e-4 * np.maximum(np.abs(want_d), 1e-3)).any(1) | (np.abs(ref_i - want_i) > 1e-4 * np.maximum(np.abs(want_i), 1e-3)).any(1)
    # float32 vs float64 may classify a ray differently exactly at a quad's border: a handful of pixels at most
    assert bad.sum() <= 3, f"{bad.sum()} pixels differ from the float64 re-derivation; first {np.argwhere(bad)[:5].ravel()}"
    assert (ref_i.sum(1) > 0).sum() == pytest.approx(hitl.sum(), abs=3)


# ---------------------------------------------------------------------------------------------------------------------
# 4. statistics: two-pass ReSTIR's mean against a brute-force quadrature of the estimator's expectation
# ---------------------------------------------------------------------------------------------------------------------
def _restir_frames(o, sd, cam, W, H, frames, reuse, faithful):
    n = W * H
    gb = pyoracle.GBufferHost(W, H)
    res = [np.zeros(n, L.RESERVOIR_DTYPE) for _ in range(3)]
    out = np.zeros((frames, n, 3), np.float32)
    img = np.zeros((n, 3), np.float32)
    for f in range(frames):
        o.gbuffer_render(cam, gb)
        o.restir_direct(cam, img, 0, f, res[0], res[1], res[2], gb, f == 0, reuse, faithful)
        res[0], res[1] = res[1], res[0]
        out[f] = img
        gb.update(cam)
    return out, gb


def test_restir_mean_vs_brute_force_all_lights():
    """E[Li f cos W] of RIS with candidate weights p_hat / pdf_ref equals  sum_l (2 pi)^2 area_l  INT_{A_l} Li f cos(x) cos(l) / r^2 V dA
    — the reference's pdf_ref divides by (area 2 pi) where its selection probability multiplies, hence the factor —
    times the G-buffer albedo.  Brute force: 4x4 jitter positions per pixel x 12 lights x 8x8 stratified points per light,
    visibility from the oracle's any-hit walk.  256 frames of the two-pass ReSTIR with the corrected `update` must agree
    within 3 standard errors (+1 %) where it is unbiased (no reuse), and within a few percent with temporal + spatial reuse
    (the reference's merge without re-normalisation is the biased ReSTIR)."""
    sd = build_scene()
    W, H, frames = 16, 12, 256
    cam = hostlib.make_camera(W, H, eye=(0.1, 2.6, 2.4), rotation=(-90.0, -48.0, 0.0), fovy=17.0)
    o = pyoracle.OracleScene(sd)
    n = W * H
    # ---- brute force ----
    J, S = 4, 8
    V = sd.vertices.astype(np.float64).reshape(-1, 3, 3)
    lv = V[sd.light_prim_ids]
    lrad = sd.light_unit_radiance.astype(np.float64)
    jit = (np.stack(np.meshgrid(np.arange(J), np.arange(J)), -1).reshape(-1, 2) + 0.5) / J
    uu = (np.stack(np.meshgrid(np.arange(S), np.arange(S)), -1).reshape(-1, 2) + 0.5) / S
    expect = np.zeros((n, 3))
    same_surface = np.ones(n, bool)
    gb0 = pyoracle.GBufferHost(W, H)
    o.gbuffer_render(cam, gb0)
    centre_id = gb0.primId[0].copy()
    for j in range(len(jit)):
        org, dirs = _camera_rays_f64(cam, W, H, np.tile(jit[j], (n, 1)))
        hits = o.trace_closest(np.concatenate([org, dirs], 1).astype(np.float32))
        hit = hits["primId"] >= 0
        mat = np.where(hit, sd.material_ids[np.maximum(hits["primId"], 0)], -1)
        same_surface &= (mat == centre_id) & (mat >= 0) & (sd.materials["type"][np.maximum(mat, 0)] == L.LAMBERTIAN)
        pos = org + dirs * hits["t"].astype(np.float64)[:, None]
        nrm = np.tile(np.array([0.0, 1.0, 0.0]), (n, 1))  # floor and occluder both face +y; wo has positive y
        for l in range(sd.num_lights):
            v0, v1, v2 = lv[l]
            y = sample_triangle_uniform(v0, v1, v2, np.tile(uu[:, 0], n), np.tile(uu[:, 1], n)).reshape(n, S * S, 3)
            nl = normalize(np.cross(v1 - v0, v2 - v0))
            area = np.linalg.norm(np.cross(v1 - v0, v2 - v0)) * 0.5
            to = y - pos[:, None, :]
            r2 = np.einsum("ijk,ijk->ij", to, to)
            wi = to / np.sqrt(r2)[..., None]
            cos_x = np.maximum(np.einsum("ik,ijk->ij", nrm, wi), 0.0)
            facing = np.einsum("k,ijk->ij", nl, to) <= -1e-6
            cos_l = np.abs(np.einsum("k,ijk->ij", nl, wi))
            seg = np.concatenate([np.repeat(pos[:, None, :], S * S, 1), y], 2).reshape(-1, 6).astype(np.float32)
            vis = 1.0 - o.trace_occluded(seg).reshape(n, S * S)
            g = np.where(facing & hit[:, None], cos_x * cos_l / r2 * vis, 0.0).mean(1)  # mean over the light's area
            expect += (2.0 * PI) ** 2 * area * area * g[:, None] * (lrad[l] / PI)[None, :]
    expect /= len(jit)
    expect *= gb0.albedo.astype(np.float64)
    interior = same_surface & (expect.sum(1) > 0)
    assert interior.sum() > 0.6 * n
    # ---- unbiased: RIS only, corrected update ----
    fr, _ = _restir_frames(o, sd, cam, W, H, frames, reuse=0, faithful=0)
    mean, sem = fr.mean(0, dtype=np.float64), fr.std(0, dtype=np.float64) / np.sqrt(frames)
    err = np.abs(mean - expect)[interior]
    tol = (3.0 * sem + 0.01 * expect)[interior]
    assert (err <= tol).mean() > 0.98, f"{(err > tol).sum()} of {err.size} pixel-channels outside 3 sigma + 1 %"
    assert mean[interior].sum() == pytest.approx(expect[interior].sum(), rel=0.01)
    # shadowed pixels exist and are darker: the visibility term matters
    assert (expect[interior].sum(1).min() < 0.5 * np.median(expect[interior].sum(1)))
    # ---- the reference's update (truthiness test, F7) keeps candidate #32 with weight = sum w.  That estimator is NOT unbiased:
    # the kept candidate is not drawn in proportion to its weight, and a rejected last candidate (back-facing light: weight 0,
    # zero-initialised sample, Q19) still replaces the sample, so the pixel gets W = x/0 -> scrubbed to 0.  It must come out
    # darker than the integral by a modest amount, and noisier than weighted reservoir sampling. ----
    ff, _ = _restir_frames(o, sd, cam, W, H, frames, reuse=0, faithful=1)
    fmean = ff.mean(0, dtype=np.float64)
    ratio = fmean[interior].sum() / expect[interior].sum()
    assert 0.85 < ratio < 1.0, ratio
    assert ff.std(0, dtype=np.float64)[interior].mean() > 1.1 * fr.std(0, dtype=np.float64)[interior].mean()
    # ---- temporal + spatial reuse: lower variance, small bias ----
    fb, _ = _restir_frames(o, sd, cam, W, H, frames, reuse=3, faithful=0)
    bmean = fb.mean(0, dtype=np.float64)
    assert bmean[interior].sum() == pytest.approx(expect[interior].sum(), rel=0.05)
    assert fb[frames // 2:].std(0, dtype=np.float64)[interior].mean() < fr.std(0, dtype=np.float64)[interior].mean()
