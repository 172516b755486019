"""Plain float64 models of the small functions the oracle and the device restate in binary32, written from the reference's
text and independent of both.  The scalar ones came out of tests/test_oracle_kat.py (which imports them back); the `_n` ones are
the same formulas over numpy arrays, for the million-record sets of tests/probe_inputs.py."""
import math

import numpy as np


def utilhash_py(a):
    M = 0xFFFFFFFF
    a = ((a + 0x7ED55D16) + (a << 12)) & M
    a = ((a ^ 0xC761C23C) ^ (a >> 19)) & M
    a = ((a + 0x165667B1) + (a << 5)) & M
    a = ((a + 0xD3A2646C) ^ (a << 9)) & M
    a = ((a + 0xFD7046C5) + (a << 3)) & M
    a = ((a ^ 0xB55A4F09) ^ (a >> 16)) & M
    return a


def norm(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def metallic_ref(base, metallic, rough, n, wo, wi):
    alpha = rough * rough
    h = norm(wo + wi)
    cosO, cosI = n @ wo, n @ wi
    if cosI * cosO < 1e-7:
        return np.zeros(3), None
    f0 = 0.08 * (1 - metallic) + base * metallic
    f = f0 + (1 - f0) * (1 - h @ wo) ** 5
    def ggxD(c):
        if c < 1e-6:
            return 0.0
        a2 = alpha * alpha
        return a2 / (math.pi * ((c * c) * (a2 - 1) + 1) ** 2)
    def schlickG(c):
        a = alpha * 0.5
        return c / (c * (1 - a) + a)
    d = ggxD(n @ h)
    g = schlickG(abs(cosO)) * schlickG(abs(cosI))
    diffuse = base / math.pi * (1 - metallic)
    bsdf = diffuse * (1 - f) + (g * d / (4 * cosI * cosO)) * f
    pdf_spec = ggxD(n @ h) * schlickG(n @ wo) * abs(h @ wo) / abs(n @ wo) / (4 * abs(h @ wo))
    pdf_diff = max(n @ wi, 0) / math.pi
    a = 1 / (2 - metallic)
    return bsdf, pdf_diff * (1 - a) + pdf_spec * a


def linear_sample_py(t, u, v):
    """float64 re-derivation of linearSample from the reference text (src/image.h:42-87)."""
    h, w, _ = t.shape
    fr = lambda x: x - math.floor(x)
    u, v = fr(u), fr(v)
    fx, fy = u * w + 0.5, v * h + 0.5
    ix = int(fx if fr(fx) > 0.5 else fx - 1)
    iy = int(fy if fr(fy) > 0.5 else fy - 1)
    ix += w if ix < 0 else 0
    iy += h if iy < 0 else 0
    ux, uy = (ix + 1) % w, (iy + 1) % h
    lx, ly = fr(fx + 0.5), fr(fy + 0.5)
    c1 = t[iy, ix] * (1 - lx) + t[iy, ux] * lx
    c2 = t[uy, ix] * (1 - lx) + t[uy, ux] * lx
    return c1 * (1 - ly) + c2 * ly


# ---- the same formulas over arrays -------------------------------------------------------------------------------------------
def utilhash_n(a):
    a = np.asarray(a, np.uint64)
    M = np.uint64(0xFFFFFFFF)
    a = ((a + np.uint64(0x7ED55D16)) + (a << np.uint64(12))) & M
    a = ((a ^ np.uint64(0xC761C23C)) ^ (a >> np.uint64(19))) & M
    a = ((a + np.uint64(0x165667B1)) + (a << np.uint64(5))) & M
    a = ((a + np.uint64(0xD3A2646C)) ^ (a << np.uint64(9))) & M
    a = ((a + np.uint64(0xFD7046C5)) + (a << np.uint64(3))) & M
    a = ((a ^ np.uint64(0xB55A4F09)) ^ (a >> np.uint64(16))) & M
    return a.astype(np.uint32)


def slab_n(records):
    """The plain slab test (tests/test_oracle_kat.py:test_aabb_random_vs_slab_float64) on float32 [n, 12] = box6, ray6.
    Returns (expect hit, tNear, tFar) in float64."""
    r = np.asarray(records, np.float64)
    lo, hi, o, d = r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9:12]
    with np.errstate(all="ignore"):
        t1, t2 = (lo - o) / d, (hi - o) / d
        tn, tf = np.minimum(t1, t2).max(axis=1), np.maximum(t1, t2).min(axis=1)
    return (tf >= 0) & (tf >= tn), tn, tf


def triangle_solve_n(records):
    """float64 solve of o + t d = v0 + u e1 + v e2 (Cramer's rule) on float32 [n, 15] = ray6, v9.  Returns u, v, t, det."""
    r = np.asarray(records, np.float64)
    o, d, v0, v1, v2 = r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9:12], r[:, 12:15]
    e1, e2, s = v1 - v0, v2 - v0, o - v0
    with np.errstate(all="ignore"):
        p = np.cross(d, e2)
        det = np.einsum("ij,ij->i", e1, p)
        q = np.cross(s, e1)
        u = np.einsum("ij,ij->i", s, p) / det
        v = np.einsum("ij,ij->i", d, q) / det
        t = np.einsum("ij,ij->i", e2, q) / det
    return u, v, t, det


def metallic_n(base, metallic, rough, n, wo, wi):
    """metallic_ref over arrays ([k, 3] vectors, [k] scalars).  Returns (bsdf [k, 3], pdf [k], cosI * cosO [k])."""
    dot = lambda a, b: np.einsum("ij,ij->i", a, b)
    with np.errstate(all="ignore"):
        alpha = rough * rough
        h = wo + wi
        h = h / np.linalg.norm(h, axis=1, keepdims=True)
        cosO, cosI = dot(n, wo), dot(n, wi)
        f0 = 0.08 * (1 - metallic)[:, None] + base * metallic[:, None]
        f = f0 + (1 - f0) * ((1 - dot(h, wo)) ** 5)[:, None]
        a2 = alpha * alpha

        def ggxD(c):
            return np.where(c < 1e-6, 0.0, a2 / (math.pi * ((c * c) * (a2 - 1) + 1) ** 2))

        def schlickG(c):
            a = alpha * 0.5
            return c / (c * (1 - a) + a)

        d = ggxD(dot(n, h))
        g = schlickG(np.abs(cosO)) * schlickG(np.abs(cosI))
        diffuse = base / math.pi * (1 - metallic)[:, None]
        bsdf = diffuse * (1 - f) + (g * d / (4 * cosI * cosO))[:, None] * f
        bsdf = np.where((cosI * cosO < 1e-7)[:, None], 0.0, bsdf)
        pdf_spec = d * schlickG(cosO) * np.abs(dot(h, wo)) / np.abs(cosO) / (4 * np.abs(dot(h, wo)))
        pdf_diff = np.maximum(cosI, 0) / math.pi
        a = 1 / (2 - metallic)
        pdf = pdf_diff * (1 - a) + pdf_spec * a
    return bsdf, pdf, cosI * cosO


def fresnel_exact_n(cos_in, eta):
    """Unpolarised Fresnel reflectance for |cos_in| on the incident side and relative index eta (already inverted for a ray that
    leaves the medium), written from Snell's law as tests/test_oracle_statistics.py:_fresnel_exact; 1 under total internal
    reflection.  Returns (F, sin^2 of the transmitted angle)."""
    c = np.abs(cos_in)
    with np.errstate(all="ignore"):
        sin2_tr = np.maximum(0.0, 1 - c * c) / (eta * eta)
        cos_tr = np.sqrt(np.maximum(0.0, 1 - sin2_tr))
        rpa = (c - eta * cos_tr) / (c + eta * cos_tr)
        rpe = (eta * c - cos_tr) / (eta * c + cos_tr)
        f = np.where(sin2_tr >= 1, 1.0, 0.5 * (rpa * rpa + rpe * rpe))
    return f, sin2_tr


SPECULAR_REFLECTION, SPECULAR_TRANSMISSION = 4 | 16, 4 | 32  # material.h:18-26


def dielectric_sample_n(base, ior, n, wo, rz):
    """dielectricSample (material.h:159-183) from Snell's law and the Fresnel equations: with probability F the mirror
    direction of wo about n, else the refracted direction (tangential part of wo scaled by 1 / eta and reversed, normal part
    -sign(n.wo) cos(theta_t)) and bsdf / eta^2.  Returns (dir [k, 3], bsdf [k, 3], type [k], F [k], sin^2 theta_t [k])."""
    dot = lambda a, b: np.einsum("ij,ij->i", a, b)
    cos = dot(n, wo)
    eta = np.where(cos < 0, 1.0 / ior, ior)
    f, sin2_tr = fresnel_exact_n(cos, eta)
    reflect = rz < f
    mirror = 2 * cos[:, None] * n - wo
    with np.errstate(all="ignore"):
        tangent = wo - cos[:, None] * n
        t = -tangent / eta[:, None] - (np.sign(cos) * np.sqrt(np.maximum(0.0, 1 - sin2_tr)))[:, None] * n
        t = t / np.linalg.norm(t, axis=1, keepdims=True)
    d = np.where(reflect[:, None], mirror, t)
    bsdf = np.where(reflect[:, None], base, base / (eta * eta)[:, None])
    typ = np.where(reflect, SPECULAR_REFLECTION, SPECULAR_TRANSMISSION)
    return d, bsdf, typ, f, sin2_tr


def lambertian_n(base, n, wi):
    """Lambertian BSDF and pdf (material.h:131-139): base / pi, max(n.wi, 0) / pi."""
    return base / math.pi, np.maximum(np.einsum("ij,ij->i", n, wi), 0) / math.pi


GAMMA_EXPONENT = float(np.float32(1.0) / np.float32(2.2))  # the binary32 constant 1/2.2f both sides multiply by


def pow_gamma_n(x):
    return np.power(np.asarray(x, np.float64), GAMMA_EXPONENT)
