"""Input sets for the per-function comparisons (tests/test_probe_inputs_cpu.py on the CPU, tests/test_gpu_device_functions.py on
the GPU).  Pure numpy, seeded, about 2^20 records per set, laid out as the records of tests/probe/device_probe.hip.

Bit-pinned domains that are narrower than "every binary32 value", each with its reason (DESIGN.md §2 lists them too):
  * linearSample, proceduralTexture: FINITE uv only.  linearSample indexes its texel array with int(NaN) otherwise, which on
    the host is INT_MIN (out of bounds) and on gfx950 is 0.
  * proceduralTexture: |uv| * 1024 < 2^31 (PROC_TEX_UV_MAX).  `int(uv.x * 1024)` beyond that is an out-of-range float -> int
    conversion: x86 gives INT_MIN, gfx950 saturates.  The path cannot send one: rdh_scene_upload and rdh_scene_set_geometry,
    the two entries that take texture coordinates, refuse |uv| >= 2^21, and the uv of a hit is a convex combination of three.
  * sincos_det: finite |x| < 2^31 (SINCOS_X_MAX), plus inf and NaN.  Its quadrant is `(int)rint(x * 2/pi)`, out of range from
    x = 2^31 * pi/2 = 3.37e9 on: x86 gives INT_MIN (quadrant 0), gfx950 saturates (quadrant 3), and the two outputs differ —
    measured: first differing record of the full-exponent set x = 3.6651466e9, 610 103 differing words.  The path cannot get
    there: its arguments are 2 pi u with u in [0, 1) (concentricSampleDisk, toSphere on pixel centres) and, in
    proceduralTexture, 2 pi (10 uv + r) with |uv| < 2^21 by the bound above, i.e. |x| < 1.4e8.  (Non-finite x stays in: the
    reduced argument is NaN whatever the quadrant.)
  * toSphere: |uv| < 2^28 (TO_SPHERE_UV_MAX) or non-finite, so that uv * {2 pi, pi} stays inside sincos_det's domain; the
    path calls it on pixel centres in [0, 1].
"""
import numpy as np

N = 1 << 20
F32 = np.float32
ONE_BELOW = np.nextafter(F32(1), F32(0))  # the largest float below 1
PROC_TEX_UV_MAX = 2.0 ** 21  # * 1024 = 2^31: the first value whose conversion to int is out of range
SINCOS_X_MAX = 2.0 ** 31  # rint(x * 2/pi) converts to int in range below 2^31 * pi/2; 2^31 is the round bound inside that
TO_SPHERE_UV_MAX = 2.0 ** 28  # * 2 pi < SINCOS_X_MAX


def _f32(a):
    with np.errstate(over="ignore", under="ignore"):  # subnormal and overflowing casts are meant
        return np.ascontiguousarray(a, dtype=np.float32)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def ulp_up(x):
    return np.nextafter(F32(x), F32(np.inf))


def ulp_down(x):
    return np.nextafter(F32(x), F32(-np.inf))


# ---------------------------------------------------------------------------------------------------------------------------------
# Ray classes of makeRaySlab (traverse.h) restated in float32 numpy, and the branch of AABB::intersect a record takes
# ---------------------------------------------------------------------------------------------------------------------------------
EPS = F32(1e-6)
ONE_MINUS_EPS = F32(1) - EPS
FAR = F32(1e30)


def ray_class(o, d):
    """cls of makeRaySlab for float32 origins / directions [n, 3]."""
    o, d = _f32(o), _f32(d)
    a = np.abs(d)
    with np.errstate(invalid="ignore"):
        cls = np.where(a[:, 0] > ONE_MINUS_EPS, 1,
              np.where(a[:, 1] > ONE_MINUS_EPS, 2,
              np.where(a[:, 2] > ONE_MINUS_EPS, 3,
              np.where((a < EPS).any(axis=1), 4, 0))))
        literal = ~(np.abs(o) < FAR).all(axis=1) | ~(a <= F32(1)).all(axis=1)
    return np.where((cls == 0) & literal, 5, cls).astype(np.int32)


AABB_RETURNS = ("x-parallel: slab", "x-parallel: outside", "y-parallel: slab", "y-parallel: outside", "z-parallel: slab",
                "z-parallel: outside", "tiny x", "tiny y", "tiny z", "general: overlap", "general: no overlap")


def aabb_return_taken(records):
    """Which return statement of aabbIntersect (traverse.h; bvh.h:91-155) each record reaches: an index into AABB_RETURNS.
    Restates the branch SELECTION only, in float32; the values the branches return are the oracle's business."""
    r = _f32(records)
    lo, hi, o, d = r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9:12]
    cls = ray_class(o, d)
    out = np.full(len(r), -1, np.int32)
    with np.errstate(all="ignore"):
        inside = (o >= lo) & (o <= hi)
        for k, (a, b) in enumerate(((1, 2), (2, 0), (0, 1))):
            m = cls == k + 1
            out[m] = 2 * k + np.where(inside[m][:, a] & inside[m][:, b], 0, 1)
        inv = F32(1) / d
        t1, t2 = (lo - o) * inv, (hi - o) * inv
        tn = np.where(t2 < t1, t2, t1)  # glm::min(x, y) = (y < x) ? y : x
        tf = np.where(t1 < t2, t2, t1)
        td = tf - tn
        yz, zx, xy = tf[:, 2] - tn[:, 1], tf[:, 0] - tn[:, 2], tf[:, 1] - tn[:, 0]
        cy, cz, cx = td[:, 1] + td[:, 2] > yz, td[:, 2] + td[:, 0] > zx, td[:, 0] + td[:, 1] > xy
        a = np.abs(d)
        rest = out < 0
        c4 = cls == 4
        pick = np.where(c4 & (a[:, 0] < EPS) & cy, 6,
               np.where(c4 & (a[:, 1] < EPS) & cz, 7,
               np.where(c4 & (a[:, 2] < EPS) & cx, 8,
               np.where(cy & cz & cx, 9, 10))))
    out[rest] = pick[rest]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Boxes x rays: float32 [N, 12] = pMin, pMax, origin, direction
# ---------------------------------------------------------------------------------------------------------------------------------
def boxes_rays(n=N, seed=101):
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-2, 0, (n, 3))
    size = rng.uniform(0.2, 2, (n, 3))
    bk = rng.integers(0, 10, n)  # 6, 7, 8: zero thickness on x / y / z; 9: a point box
    for a in range(3):
        size[bk == 6 + a, a] = 0
    size[bk == 9] = 0
    sk = rng.integers(0, 12, n)  # 0: coordinates around 1e-30; 1: up to 9.9e29; else around 1
    scale = np.where(sk == 0, 1e-30, np.where(sk == 1, 9.9e29 / 2, 1.0))[:, None]
    lo32 = _f32(lo * scale)
    hi32 = _f32((lo + size) * scale)
    hi32 = np.where(size == 0, lo32, hi32)
    lo64, hi64 = lo32.astype(np.float64), hi32.astype(np.float64)
    centre, ext = (lo64 + hi64) / 2, np.maximum(hi64 - lo64, scale * 0.2)

    # origins: 0-1 inside, 2-4 outside, 5 on a face, 6 on an edge, 7 at a corner (the other coordinates inside)
    ok = rng.integers(0, 8, n)
    inside = lo64 + rng.uniform(0, 1, (n, 3)) * (hi64 - lo64)
    outside = centre + _unit(rng.normal(size=(n, 3))) * ext * rng.uniform(1.5, 4, (n, 1))
    o = np.where((ok >= 2)[:, None] & (ok <= 4)[:, None], outside, inside)
    o32 = _f32(o)
    pinned = rng.permuted(np.tile(np.arange(3), (n, 1)), axis=1)  # which axes sit exactly on a box plane
    side = rng.integers(0, 2, (n, 3)).astype(bool)
    for j in range(3):
        m = ok >= 5 + j  # face: 1 axis, edge: 2, corner: 3
        ax = pinned[m, j]
        o32[m, ax] = np.where(side[m, j], hi32[m, ax], lo32[m, ax])

    # directions
    target = lo64 + rng.uniform(0, 1, (n, 3)) * (hi64 - lo64)
    aimed = target - o32.astype(np.float64)
    aimed = np.where((np.abs(aimed).sum(axis=1) == 0)[:, None], rng.normal(size=(n, 3)), aimed)
    with np.errstate(all="ignore"):
        aimed = _unit(aimed / np.abs(aimed).max(axis=1, keepdims=True))
    rnd = _unit(rng.normal(size=(n, 3)))
    dk = rng.integers(0, 20, n)
    d = np.where((dk % 3 == 0)[:, None], rnd, np.where((dk % 3 == 1)[:, None], aimed, -aimed))  # -aimed: the box is behind the ray
    d32 = _f32(d)
    axis = rng.integers(0, 3, n)
    sign = rng.choice(_f32([-1, 1]), n)
    rows = np.arange(n)
    # 10-11: exactly axis-parallel, the other components +0 / -0
    m = (dk == 10) | (dk == 11)
    d32[m] = _f32(rng.choice([0.0, -0.0], (m.sum(), 3)))
    d32[rows[m], axis[m]] = sign[m]
    # 12-13: one component at 1 - 1e-6 and its neighbours, or 1; the others small but above 1e-6 (classes 0 and 1-3)
    m = (dk == 12) | (dk == 13)
    near1 = _f32([ONE_MINUS_EPS, ulp_up(ONE_MINUS_EPS), ulp_down(ONE_MINUS_EPS), 1.0])
    d32[m] = _f32(rng.uniform(2e-6, 1e-3, (m.sum(), 3)) * rng.choice([-1, 1], (m.sum(), 3)))
    d32[rows[m], axis[m]] = rng.choice(near1, m.sum()) * sign[m]
    # 14-16: one component zero, tiny, or at 1e-6 and its neighbours (classes 4 and 0); the rest aimed or random
    m = (dk >= 14) & (dk <= 16)
    tiny = _f32([0.0, -0.0, 1e-7, -1e-7, EPS, ulp_up(EPS), ulp_down(EPS), -EPS, -ulp_down(EPS), 1e-30, 1e-45])
    d32[rows[m], axis[m]] = rng.choice(tiny, m.sum())
    # 17: two tiny components, the third well below 1 - 1e-6
    m = dk == 17
    d32[m] = _f32(rng.choice(tiny, (m.sum(), 3)))
    d32[rows[m], axis[m]] = F32(0.9) * sign[m]
    # 18: what makeRaySlab sends down the literal path for safety: NaN / inf / |d| > 1 / an origin at or beyond 1e30
    m = dk == 18
    bad = _f32([np.nan, np.inf, -np.inf, 1.5, -2.0, 1e30, -3e38])
    which = rng.integers(0, 4, n)
    mo, md = m & (which <= 1), m & (which >= 1)
    o32[rows[mo], axis[mo]] = rng.choice(bad, mo.sum())
    d32[rows[md], rng.integers(0, 3, n)[md]] = rng.choice(bad[:5], md.sum())
    return np.concatenate([lo32, hi32, o32, d32], axis=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# Triangles x rays: float32 [N, 15] = origin, direction, v0, v1, v2
# ---------------------------------------------------------------------------------------------------------------------------------
FLT_EPSILON = F32(1.1920928955078125e-7)


def triangles_rays(n=N, seed=202):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (n, 3, 3))
    o = rng.uniform(-2, 2, (n, 3))
    bu = rng.uniform(0.02, 0.96, n)
    bv = rng.uniform(0.02, 0.96, n) * (0.98 - bu)
    target = v[:, 0] + bu[:, None] * (v[:, 1] - v[:, 0]) + bv[:, None] * (v[:, 2] - v[:, 0])
    d = _unit(target - o)
    k = rng.integers(0, 16, n)  # 0-5 and 11-13 aimed at the interior (both faces), 6-7 random direction
    m = (k == 6) | (k == 7)
    d[m] = _unit(rng.normal(size=(m.sum(), 3)))
    # 8: zero-area (two equal vertices, or three collinear ones) and slivers
    m = k == 8
    sub = rng.integers(0, 3, n)
    v[m & (sub == 0), 1] = v[m & (sub == 0), 0]
    mm = m & (sub >= 1)
    v[mm, 2] = v[mm, 0] + (v[mm, 1] - v[mm, 0]) * rng.uniform(0.1, 2, (mm.sum(), 1))
    mm = m & (sub == 2)
    v[mm, 2] += rng.normal(size=(mm.sum(), 3)) * 1e-6
    rec = _f32(np.concatenate([o, d, v.reshape(n, 9)], axis=1))
    # 9: coordinates up to 9.9e29; 10: subnormal edge vectors
    m = k == 9
    rec[m, 0:3] = _f32(rec[m, 0:3].astype(np.float64) * 4.9e29)
    rec[m, 6:15] = _f32(rec[m, 6:15].astype(np.float64) * 9.9e29)
    m = k == 10
    rec[m, 6:15] = _f32(rec[m, 6:15].astype(np.float64) * 1e-39)
    rec[m, 0:3] = _f32(rec[m, 0:3].astype(np.float64) * 1e-39)
    # 14: exact cases on the triangle (0,0,0) (s,0,0) (0,s,0) + integer offset, ray along +-z at dyadic (x, y):
    # bary.x == 0, bary.y == 0, u + v == det (x + y == s), vertices, outside by one step, t == 0 exactly, behind the ray.
    m = (k == 14) & (rng.integers(0, 2, n) == 0)  # (the other half of 14 stays aimed at the interior)
    c = int(m.sum())
    s = rng.choice([0.5, 1.0, 4.0], c)
    off = rng.integers(-3, 4, (c, 3)).astype(np.float64)
    gx, gy = rng.integers(-2, 11, c) / 8.0, rng.integers(-2, 11, c) / 8.0
    gy = np.where(rng.integers(0, 3, c) == 0, 1.0 - gx, gy)  # on the hypotenuse
    h = rng.choice([2.0, 0.0, -1.0, 0.375], c)
    dz = rng.choice([-1.0, 1.0], c)
    ex = np.zeros((c, 15))
    ex[:, 0], ex[:, 1], ex[:, 2] = gx * s, gy * s, h
    ex[:, 5] = dz
    ex[:, 9], ex[:, 13] = s, s
    for j in range(3):
        ex[:, [j, 6 + j, 9 + j, 12 + j]] += off[:, [j]]
    rec[m] = _f32(ex)
    # 15: |det| at FLT_EPSILON and its neighbours: e01 = (a, 0, 0), e02 = (0, 1, 0), d = (0, 0, -1) gives det = a exactly
    m = k == 15
    c = int(m.sum())
    a = rng.choice(_f32([FLT_EPSILON, ulp_up(FLT_EPSILON), ulp_down(FLT_EPSILON)]), c) * rng.choice(_f32([-1, 1]), c)
    ex = np.zeros((c, 15), np.float32)
    ex[:, 0] = a * _f32(rng.uniform(0, 0.5, c))
    ex[:, 1] = _f32(rng.uniform(0, 0.5, c))
    ex[:, 2], ex[:, 5], ex[:, 9], ex[:, 13] = 1, -1, a, 1
    rec[m] = ex
    return rec


# ---------------------------------------------------------------------------------------------------------------------------------
# BSDF: float32 [N, 20] = type (int bits), baseColor, metallic, roughness, ior, n, wo, wi, r, unused
# ---------------------------------------------------------------------------------------------------------------------------------
LAMBERTIAN, METALLIC_WORKFLOW, DIELECTRIC, DISNEY, LIGHT = range(5)
ROUGHNESS = (0.0, 1e-3, 0.05, 0.3, 1.0)
METALLIC = (0.0, 0.5, 1.0)
IOR = (0.67, 1.0, 1.0001, 1.5, 2.4)
GRAZING_COS = (0.0, 1e-7, 1e-4)


def _frame(nrm):
    t = np.where((np.abs(nrm[:, 1]) > 0.9)[:, None], [[0.0, 0.0, 1.0]], [[0.0, 1.0, 0.0]])
    b = _unit(np.cross(nrm, t))
    return np.cross(b, nrm), b


def _hemisphere(nrm, cos_t, phi):
    t, b = _frame(nrm)
    sin_t = np.sqrt(np.maximum(0, 1 - cos_t * cos_t))
    return t * (sin_t * np.cos(phi))[:, None] + b * (sin_t * np.sin(phi))[:, None] + nrm * cos_t[:, None]


def _reflect32(i, nrm):  # rmath.h reflect(I, N) = I - N * dot(N, I) * 2, in float32 as written
    i, nrm = _f32(i), _f32(nrm)
    dt = (nrm[:, 0] * i[:, 0] + nrm[:, 1] * i[:, 1]) + nrm[:, 2] * i[:, 2]
    return i - nrm * dt[:, None] * F32(2)


def bsdf_records(n=N, seed=303):
    rng = np.random.default_rng(seed)
    typ = rng.choice([LAMBERTIAN, METALLIC_WORKFLOW, METALLIC_WORKFLOW, METALLIC_WORKFLOW, DIELECTRIC, DIELECTRIC, DISNEY, LIGHT], n)
    base = rng.uniform(0.05, 1, (n, 3))
    nk = rng.integers(0, 4, n)  # (0,1,0); within localRefMatrix's |n.y| > 0.9999 branch; random
    nrm = _unit(rng.normal(size=(n, 3)))
    nrm[nk == 0] = [0, 1, 0]
    m = nk == 1
    nrm[m] = _unit(np.stack([rng.uniform(-5e-3, 5e-3, m.sum()), np.ones(m.sum()), rng.uniform(-5e-3, 5e-3, m.sum())], axis=1))
    grid_cos = (np.arange(16) + 0.5) / 16
    grid_phi = np.arange(32) * (2 * np.pi / 32)

    def directions():
        kind = rng.integers(0, 8, n)  # 0-4 hemisphere grid, 5 grazing, 6 below the surface, 7 random on the sphere
        cos_t = rng.choice(grid_cos, n)
        cos_t = np.where(kind == 5, rng.choice(GRAZING_COS, n), cos_t)
        cos_t = np.where(kind == 6, -cos_t, cos_t)
        cos_t = np.where(kind == 7, rng.uniform(-1, 1, n), cos_t)
        return _hemisphere(nrm, cos_t, rng.choice(grid_phi, n))

    n32 = _f32(nrm)
    wo32 = _f32(directions())
    wi32 = _f32(directions())
    wk = rng.integers(0, 10, n)
    m = wk == 0  # the mirror direction of the float32 wo about the float32 n, exactly as reflect() rounds it
    wi32[m] = _reflect32(-wo32[m], n32[m])
    m = wk == 1
    wi32[m] = wo32[m]
    r = rng.uniform(0, 1, (n, 3))
    r32 = _f32(r)
    edge = rng.integers(0, 8, (n, 3))
    r32[edge == 0] = 0
    r32[edge == 1] = ONE_BELOW
    rec = np.zeros((n, 20), np.float32)
    rec[:, 0] = typ.astype(np.int32).view(np.float32)
    rec[:, 1:4] = _f32(base)
    rec[:, 4] = _f32(rng.choice(METALLIC, n))
    rec[:, 5] = _f32(rng.choice(ROUGHNESS, n))
    rec[:, 6] = _f32(rng.choice(IOR, n))
    rec[:, 7:10], rec[:, 10:13], rec[:, 13:16], rec[:, 16:19] = n32, wo32, wi32, r32
    return rec


# ---------------------------------------------------------------------------------------------------------------------------------
# One-argument functions: every binary32 exponent, both signs, 2^12 random mantissas plus mantissa 0 and all-ones
# ---------------------------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000,
                     0xFFC00000, 0x7F800001], np.uint32).view(np.float32)  # +-0, smallest / largest subnormal, +-inf, NaNs


def all_exponents(seed=404, mantissas=1 << 12, exponents=range(256)):
    """float32 [len(exponents) * 2 * (mantissas + 2) + specials].  Exponent 0 is the subnormals, 255 is inf and the NaNs."""
    rng = np.random.default_rng(seed)
    ex = np.asarray(list(exponents), np.uint32)
    man = rng.integers(0, 1 << 23, (len(ex), 2, mantissas), dtype=np.uint32)
    man = np.concatenate([man, np.zeros((len(ex), 2, 1), np.uint32), np.full((len(ex), 2, 1), 0x7FFFFF, np.uint32)], axis=2)
    bits = man | (ex[:, None, None] << np.uint32(23)) | (np.array([0, 1], np.uint32)[None, :, None] << np.uint32(31))
    return np.concatenate([bits.reshape(-1).view(np.float32), SPECIALS])


def _within(a, limit):
    """Rows of `a` whose components are all below `limit` in magnitude or non-finite (the stated domain bound, module docstring)."""
    a = np.asarray(a)
    with np.errstate(invalid="ignore"):
        keep = (np.abs(a) < limit) | ~np.isfinite(a)
    return a[keep if a.ndim == 1 else keep.all(axis=1)]


def sincos_arguments():
    return _within(all_exponents(), SINCOS_X_MAX)


def to_sphere_uv(seed=31):
    return _within(pairs(seed, N + N // 4), TO_SPHERE_UV_MAX)


def pairs(seed, n=N):
    """float32 [n, 2] for the two-argument functions: both components from all_exponents, independently shuffled, plus every
    pair of SPECIALS."""
    rng = np.random.default_rng(seed)
    a = all_exponents(seed)
    x, y = rng.choice(a, n), rng.choice(a, n)
    sx, sy = np.meshgrid(SPECIALS, SPECIALS)
    return np.concatenate([np.stack([x, y], axis=1), np.stack([sx.reshape(-1), sy.reshape(-1)], axis=1)])


def moderate_pairs(seed, n=N):
    """float32 [n, 2]: normal-distributed pairs scaled over 10^-3 .. 10^3 (tests/test_oracle_kat.py's atan2 set, enlarged)."""
    rng = np.random.default_rng(seed)
    return _f32(rng.normal(size=(n, 2)) * 10 ** rng.uniform(-3, 3, (n, 1)))


def triples(seed, n=N):
    rng = np.random.default_rng(seed)
    a = all_exponents(seed)
    return np.stack([rng.choice(a, n), rng.choice(a, n), rng.choice(a, n)], axis=1)


def hash_words(seed=505, n=N):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), np.array([0, 0xFFFFFFFF], np.uint32)])


def colours(seed=606, n=N):
    """float32 [n, 3] for the display functions: half from every exponent, half in the image range [0, 16)."""
    rng = np.random.default_rng(seed)
    t = triples(seed, n // 2)
    return np.concatenate([t, _f32(rng.uniform(0, 1, (n // 2, 3)) ** 2 * 16)])


# ---------------------------------------------------------------------------------------------------------------------------------
# Textures.  Finite uv only (module docstring).
# ---------------------------------------------------------------------------------------------------------------------------------
TEXTURE_SIZES = ((1, 1), (1, 7), (7, 1), (64, 32))  # (width, height)


def texture(width, height, seed=707):
    rng = np.random.default_rng(seed + 64 * width + height)
    return _f32(rng.uniform(0, 4, (height, width, 3)))


def _uv_axis(rng, n, size, limit):
    u = rng.uniform(-3, 3, n)
    k = rng.integers(0, 12, n)
    u = np.where(k == 0, rng.integers(-4, 5, n), u)  # exact integers
    u32 = _f32(u)
    texel = rng.integers(-size, 2 * size + 1, n)
    centre = _f32((texel + 0.5) / size)  # texel centres and boundaries, +-1 ulp
    bound = _f32(texel / float(size))
    for kk, base in ((1, centre), (2, bound)):
        step = rng.integers(-1, 2, n)
        val = np.where(step < 0, np.nextafter(base, F32(-np.inf)), np.where(step > 0, np.nextafter(base, F32(np.inf)), base))
        u32 = np.where(k == kk, val, u32)
    edge = _f32([ONE_BELOW, -ONE_BELOW, 1e-45, -1e-45, 1e-38, -1e-38, 0.0, -0.0, limit, -limit, np.nextafter(F32(limit), F32(0))])
    u32 = np.where(k == 3, rng.choice(edge, n), u32)
    return _f32(u32)


def uv_records(width, height, n, seed=808, limit=1e30):
    """Finite float32 uv [n, 2]: negatives, exact integers, the largest float below 1, +-`limit`, subnormals, texel centres and
    boundaries +-1 ulp of a width x height texture."""
    rng = np.random.default_rng(seed + 64 * width + height)
    uv = np.stack([_uv_axis(rng, n, width, limit), _uv_axis(rng, n, height, limit)], axis=1)
    assert np.isfinite(uv).all()
    return uv


def procedural_uv(n=N, seed=909):
    """uv for proceduralTexture: |uv| * 1024 stays inside int's range (PROC_TEX_UV_MAX, module docstring)."""
    lim = float(np.nextafter(F32(PROC_TEX_UV_MAX), F32(0)))
    uv = uv_records(64, 32, n, seed, limit=lim)
    assert (np.abs(uv) < PROC_TEX_UV_MAX).all()
    return uv


# ---------------------------------------------------------------------------------------------------------------------------------
# Reservoirs: float32 [N, 20] = r (Li, wi, dist, numSamples as int bits, weight), rhs (the same), rnd, M as int bits
# ---------------------------------------------------------------------------------------------------------------------------------
RESERVOIR_M = 20  # the temporal clamp the product uses


def reservoir_records(n=N, seed=1010):
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 20), np.float32)
    weights = _f32([0.0, -0.0, 1e-45, 1e-39, 3e38, np.inf, -np.inf, np.nan, -1.0, -1e-45])
    counts = np.array([0, 1, 2, RESERVOIR_M - 1, RESERVOIR_M, RESERVOIR_M + 1, 19 * 20, 19 * 20 + 1, 1 << 20, -1], np.int32)
    for base in (0, 9):
        rec[:, base:base + 7] = _f32(rng.uniform(0, 2, (n, 7)))
        cnt = np.where(rng.integers(0, 2, n) == 0, rng.choice(counts, n), rng.integers(0, 64, n)).astype(np.int32)
        rec[:, base + 7] = cnt.view(np.float32)
        w = _f32(rng.uniform(0, 1, n) * 10 ** rng.uniform(-3, 3, n))
        rec[:, base + 8] = np.where(rng.integers(0, 3, n) == 0, rng.choice(weights, n), w)
    rnd = _f32(rng.uniform(0, 1, n))
    e = rng.integers(0, 8, n)
    rnd[e == 0] = 0
    rnd[e == 1] = ONE_BELOW
    rec[:, 18] = rnd
    rec[:, 19] = np.full(n, RESERVOIR_M, np.int32).view(np.float32)
    return rec


def reservoir_w_records(n=N, seed=1111):
    """float32 [n, 24] = reservoir, material (type .. ior), n, wo, 2 unused: the reservoirs of reservoir_records with the BSDF
    set's materials and directions (sample.wi = that set's wi), for Reservoir::W."""
    rng = np.random.default_rng(seed)
    r, b = reservoir_records(n, seed), bsdf_records(n, seed + 1)
    rec = np.zeros((n, 24), np.float32)
    rec[:, 0:9] = r[:, 0:9]
    rec[:, 0:3] = _f32(rng.uniform(0, 20, (n, 3)) * (rng.integers(0, 8, (n, 3)) > 0))  # radiance, some components zero
    rec[:, 3:6] = b[:, 13:16]
    rec[:, 9:16] = b[:, 0:7]
    rec[:, 16:19], rec[:, 19:22] = b[:, 7:10], b[:, 10:13]
    return rec
