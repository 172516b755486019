"""A float64 numpy statement of the textured, environment-lit path: general triangles, the surface fetch with its four maps
and the procedural colour, the environment map as a light and as what a miss sees, the three full kernels that walk them
(singleKernelPT, PTDirectKernel, renderGBuffer) and the general-geometry scene of tests/restir_model.py — written from the
reference text (src/pathtrace.cu, src/scene.h, src/intersections.h, src/material.h, src/mathUtil.h, src/image.h,
src/gBuffer.cu), vectorised over pixels, one array operation per rule, in a different form from oracle/oracle.cpp and from the
device code, neither of which it reads or calls.

    PathScene(sd)                                              a ModelScene on general triangles with textures and an env map
    intersect / occluded / surface                             intersections.h:20-68, scene.h:303-334, :147-165, :88-112
    PathScene.sample_light(pos, r4, visibility)                scene.h:374-492, both forms
    single_kernel_pt(scene, cam, looper, max_depth, ...)       pathtrace.cu:149-291
    pt_direct(scene, cam, looper, ...)                         pathtrace.cu:293-345
    gbuffer(scene, cam, last_cam)                              gBuffer.cu:3-76

No BVH: every ray meets every triangle, which a scene of a few hundred triangles allows.  `plant` names ONE deliberate
misreading (PLANTS) that the CPU tests switch on to prove that the frozen inputs can see the rule it breaks.

Only the RANGE of binary32 is taken over (restir_model._f32_range), not its rounding; thrust's minstd engine and its
float distribution are stated as tests/test_oracle_kat.py::test_procedural_texture_matches_python_minstd states them."""
import numpy as np

import restir_model as R
from float64_models import dielectric_sample_n, metallic_n
from test_oracle_float64 import _camera_rays_f64, alias_pick, light_pdf_f64, luminance, normalize, sobol_draws

PI = np.pi
FLT_EPSILON = float(np.finfo(np.float32).eps)
LAMBERTIAN, METALLIC_WORKFLOW, DIELECTRIC, LIGHT = 0, 1, 2, 4  # Material::Type (material.h:129)
NULL_TEXTURE, PROCEDURAL_TEXTURE = -1, -2  # material.h:13-15
SPECULAR, INVALID = 1 << 2, 1 << 15  # BSDFSampleType (material.h:18-26)

PLANTS = ("uv_weights_swapped", "normal_map_decode_no_offset", "dielectric_normal_flipped", "specular_cosine",
          "dielectric_nee_draws", "env_nee_no_inv_pi2", "env_pdf_sine", "primary_miss_env_colour", "env_pixel_corner")
# `mapped * 2 - 1` is no misreading at all: it is twice `mapped * 1 - 0.5`, and the decode normalises (scene.h:107-108).
EQUIVALENT_PLANTS = ("normal_map_decode_2x_minus_1",)


def _dot(a, b):
    return np.einsum("...j,...j->...", a, b)


def _fract(x):
    return x - np.floor(x)


# ---------------------------------------------------------------------------------------------------------------------
# environment functions
# ---------------------------------------------------------------------------------------------------------------------
def to_sphere(uv):  # mathUtil.h:138-142
    a, b = uv[..., 0] * 2.0 * PI, uv[..., 1] * PI
    return np.stack([np.cos(a) * np.sin(b), np.cos(b), np.sin(a) * np.sin(b)], -1)


def to_plane(v):  # mathUtil.h:144-147
    return np.stack([_fract(np.arctan2(v[..., 2], v[..., 0]) / PI * 0.5 + 1.0),
                     np.arctan2(np.hypot(v[..., 0], v[..., 2]), v[..., 1]) / PI], -1)


def linear_sample(tex, uv):
    """linearSample (image.h:42-73) on a [h, w, 3] image for rows of uv: wrap by fract, a footprint that starts half a texel LOW
    (the texel whose centre is at or below the sample, decided by `fract(f) > 0.5`), float -> int toward zero, neighbours
    wrapped, weights fract(f + 0.5).  (`width - FLT_MIN` is `width` in binary32.)"""
    h, w, _ = tex.shape
    uv = _fract(uv)
    fx, fy = uv[:, 0] * w + 0.5, uv[:, 1] * h + 0.5
    ix = np.trunc(np.where(_fract(fx) > 0.5, fx, fx - 1.0)).astype(np.int64)
    iy = np.trunc(np.where(_fract(fy) > 0.5, fy, fy - 1.0)).astype(np.int64)
    ix, iy = np.where(ix < 0, ix + w, ix), np.where(iy < 0, iy + h, iy)
    ux, uy = ix + 1, iy + 1
    ux, uy = np.where(ux >= w, ux - w, ux), np.where(uy >= h, uy - h, uy)
    ix, iy = np.minimum(ix, w - 1), np.minimum(iy, h - 1)  # fract() of a binary32 just below 0 is 1: not met in float64
    lx, ly = _fract(fx + 0.5)[:, None], _fract(fy + 0.5)[:, None]
    c1 = tex[iy, ix] * (1.0 - lx) + tex[iy, ux] * lx
    c2 = tex[uy, ix] * (1.0 - lx) + tex[uy, ux] * lx
    return c1 * (1.0 - ly) + c2 * ly


def procedural_texture(uv):
    """DevScene::proceduralTexture (scene.h:77-86): an integer seed per 1/1024 cell, two draws of thrust's default engine
    (minstd: x <- 48271 x mod 2^31 - 1, seeded with seed mod (2^31 - 1) or 1) mapped to [0, 1) as (x - 1) / 2^31, and the product
    of two sines of 10 periods per unit uv."""
    m = 2147483647
    seed = (np.trunc(uv[:, 0] * 1024.0).astype(np.int64) * 1024 + np.trunc(uv[:, 1] * 1024.0).astype(np.int64)) & 0xFFFFFFFF
    x = seed % m
    x = np.where(x == 0, 1, x)
    x = (x * 48271) % m
    rx = (x - 1) / 2147483648.0
    x = (x * 48271) % m
    ry = (x - 1) / 2147483648.0
    f = (np.sin(uv[:, 0] * 10.0 * 2.0 * PI + rx * 2.0 * PI) + 1.0) * 0.5
    g = (np.sin(uv[:, 1] * 10.0 * 2.0 * PI + ry * 2.0 * PI) + 1.0) * 0.5
    return np.repeat((f * g)[:, None], 3, 1)


def local_ref(n):
    """localRefMatrix (mathUtil.h:149-155): the columns (t, b, n), with the helper axis switched where |n.y| > 0.9999."""
    up = np.where((np.abs(n[:, 1]) > 0.9999)[:, None], np.array([0.0, 0.0, 1.0]), np.array([0.0, 1.0, 0.0]))
    b = normalize(np.cross(n, up))
    return np.cross(b, n), b, n


def local_to_world(n, v):  # mathUtil.h:157-159
    t, b, n = local_ref(n)
    return normalize(t * v[:, 0:1] + b * v[:, 1:2] + n * v[:, 2:3])


def _disk(rx, ry):  # the polar "concentricSampleDisk" (mathUtil.h:132-136)
    r, th = np.sqrt(rx), 2.0 * PI * ry
    return r * np.cos(th), r * np.sin(th)


def cosine_sample_hemisphere(n, rx, ry):  # mathUtil.h:161-166
    dx, dy = _disk(rx, ry)
    with np.errstate(invalid="ignore"):
        dz = np.sqrt(1.0 - (dx * dx + dy * dy))
    return local_to_world(n, np.stack([dx, dy, dz], 1))


def ggx_sample(n, wo, alpha, rx, ry):
    """ggxSample (material.h:106-126): the visible-normal construction in the frame of n stretched by alpha."""
    t, b, n = local_ref(n)
    vh = normalize(np.stack([_dot(t, wo) * alpha, _dot(b, wo) * alpha, _dot(n, wo)], 1))  # inverse(mat3(t, b, n)) is its transpose
    len_sq = vh[:, 0] ** 2 + vh[:, 1] ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        t1 = np.where((len_sq > 0.0)[:, None], np.stack([-vh[:, 1], vh[:, 0], np.zeros(len(vh))], 1) / np.sqrt(len_sq)[:, None],
                      np.array([1.0, 0.0, 0.0]))
    b1 = np.cross(vh, t1)
    px, py = _disk(rx, ry)
    s = 0.5 * (vh[:, 2] + 1.0)
    with np.errstate(invalid="ignore"):
        py = (1.0 - s) * np.sqrt(1.0 - px * px) + s * py
    h = t1 * px[:, None] + b1 * py[:, None] + vh * np.sqrt(np.maximum(0.0, 1.0 - (px * px + py * py)))[:, None]
    h = np.stack([h[:, 0] * alpha, h[:, 1] * alpha, np.maximum(0.0, h[:, 2])], 1)
    return normalize(t * h[:, 0:1] + b * h[:, 1:2] + n * h[:, 2:3])


def power_heuristic(f, g):  # mathUtil.h:81-84
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return f * f / (f * f + g * g)


# ---------------------------------------------------------------------------------------------------------------------
# the scene: triangles, materials, textures, the environment map
# ---------------------------------------------------------------------------------------------------------------------
class PathScene(R.ModelScene):
    """restir_model.ModelScene on general geometry: the same interface (intersect, occluded, bsdf, sample_light, the material
    tables), with the surface fetch and the environment branch below."""

    def __init__(self, sd, plant=None):
        assert plant is None or plant in PLANTS + EQUIVALENT_PLANTS, plant
        self.sd, self.plant = sd, plant
        self.V = sd.vertices.astype(np.float64).reshape(-1, 3, 3)
        self.N = sd.normals.astype(np.float64).reshape(-1, 3, 3)
        self.T = sd.texcoords.astype(np.float64).reshape(-1, 3, 2)
        self.tri_mat = sd.material_ids.astype(np.int64)
        m = sd.materials
        self.mat_type = m["type"].astype(np.int64)
        self.mat_color = m["baseColor"].astype(np.float64)
        self.mat_metallic, self.mat_roughness, self.mat_ior = (m[k].astype(np.float64) for k in ("metallic", "roughness", "ior"))
        self.maps = {k: m[k + "MapId"].astype(np.int64) for k in ("baseColor", "normal", "metallic", "roughness")}
        self.textures = [t.astype(np.float64) for t in sd.textures]
        self.env = self.textures[sd.env_map_tex_id] if sd.env_map_tex_id >= 0 else None
        self.sum_light_power_inv = float(sd.sum_light_power_inv)
        self.tri_area = np.linalg.norm(np.cross(self.V[:, 1] - self.V[:, 0], self.V[:, 2] - self.V[:, 0]), axis=1) * 0.5

    # ---- intersections.h:20-68 against every triangle ----
    def _solve(self, org, dirs):
        """(t [rays, triangles] with inf where the triangle is not hit, u, v)."""
        va, e1, e2 = self.V[:, 0], self.V[:, 1] - self.V[:, 0], self.V[:, 2] - self.V[:, 0]
        with np.errstate(all="ignore"):
            p = np.cross(dirs[:, None, :], e2[None])
            det = np.einsum("tj,rtj->rt", e1, p)
            s = org[:, None, :] - va[None]
            u = np.einsum("rtj,rtj->rt", s, p) / det  # the sign change of :41-44 cancels in every quotient
            q = np.cross(s, e1[None])
            v = np.einsum("rj,rtj->rt", dirs, q) / det
            t = np.einsum("tj,rtj->rt", e2, q) / det
            ok = ~(np.abs(det) < FLT_EPSILON) & ~(u < 0.0) & ~(u > 1.0) & ~(v < 0.0) & ~(u + v > 1.0) & (t > 0.0)
        return np.where(ok, t, np.inf), u, v

    def closest(self, org, dirs):
        """scene->intersect without the tree: (hit, primitive, distance, bary.x, bary.y), the smallest distance winning."""
        out = [np.zeros(len(org), bool), np.zeros(len(org), np.int64), np.zeros(len(org)), np.zeros(len(org)), np.zeros(len(org))]
        for lo in range(0, len(org), 4096):
            sl = slice(lo, lo + 4096)
            t, u, v = self._solve(org[sl], dirs[sl])
            k = np.argmin(t, axis=1)
            r = np.arange(len(k))
            out[0][sl], out[1][sl], out[2][sl], out[3][sl], out[4][sl] = np.isfinite(t[r, k]), k, t[r, k], u[r, k], v[r, k]
        out[2] = np.where(out[0], out[2], 0.0)
        return out

    def occluded(self, x, y):
        """testOcclusion (scene.h:303-334) as restir_model._occluded states it: the segment shortened by 1e-4, its origin pushed
        1e-5 along it (makeOffsetedRay, intersections.h:16-18); any triangle nearer than that."""
        d = y - x
        dist = np.linalg.norm(d, axis=1)
        out = np.zeros(len(x), bool)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = d / dist[:, None]
            for lo in range(0, len(x), 4096):
                sl = slice(lo, lo + 4096)
                t, _, _ = self._solve(x[sl] + d[sl] * 1e-5, d[sl])
                out[sl] = (t < (dist[sl] - 1e-4)[:, None]).any(1)
        return out

    # ---- getIntersecGeomInfo (scene.h:147-165) and getTexturedMaterialAndSurface (:88-112) ----
    def surface(self, hit, prim, bu, bv):
        """What a hit knows: pos, the interpolated and normalised normal `geom_norm`, the normal after the normal map `norm`, uv,
        and the material with its maps applied (type, base, metallic, roughness, ior, id).  Rows that are no hit hold triangle 0
        at its first vertex, which nothing reads."""
        prim = np.where(hit, prim, 0)
        bu, bv = np.where(hit, bu, 0.0)[:, None], np.where(hit, bv, 0.0)[:, None]
        bw = 1.0 - bu - bv

        def lerp(a, swap=False):  # vb * bary.x + vc * bary.y + va * (1 - bary.x - bary.y), in this order
            b, c = (a[prim, 2], a[prim, 1]) if swap else (a[prim, 1], a[prim, 2])
            return b * bu + c * bv + a[prim, 0] * bw

        pos, uv = lerp(self.V), lerp(self.T, swap=self.plant == "uv_weights_swapped")
        geom = normalize(lerp(self.N))
        mat = self.tri_mat[prim]
        base, metallic, roughness = self.mat_color[mat].copy(), self.mat_metallic[mat].copy(), self.mat_roughness[mat].copy()
        norm = geom.copy()
        wrapped = np.zeros(len(prim), bool)
        for k in np.unique(self.maps["baseColor"][mat]):  # `!= NullTextureId` (:90), the procedural id chosen first (:92)
            rows = np.flatnonzero(self.maps["baseColor"][mat] == k)
            if k == PROCEDURAL_TEXTURE:
                base[rows] = procedural_texture(uv[rows])
            elif k != NULL_TEXTURE:
                base[rows] = linear_sample(self.textures[k], uv[rows])
                wrapped[rows] = ((uv[rows] < 0.0) | (uv[rows] >= 1.0)).any(1)
        for name, plane in (("metallic", metallic), ("roughness", roughness)):  # `> NullTextureId` (:97, :101), the .r channel
            for k in np.unique(self.maps[name][mat]):
                if k > NULL_TEXTURE:
                    rows = np.flatnonzero(self.maps[name][mat] == k)
                    plane[rows] = linear_sample(self.textures[k], uv[rows])[:, 0]
        mapped_rows = np.zeros(len(prim), bool)
        for k in np.unique(self.maps["normal"][mat]):  # `!= NullTextureId` (:105)
            if k != NULL_TEXTURE:
                rows = np.flatnonzero(self.maps["normal"][mat] == k)
                mapped = linear_sample(self.textures[k], uv[rows])
                # `mapped * 1.f - 0.5f` (:108): half the usual * 2 - 1, and the same direction once normalised
                local = mapped * 2.0 - 1.0 if self.plant == "normal_map_decode_2x_minus_1" else mapped * 1.0 - 0.5
                if self.plant == "normal_map_decode_no_offset":
                    local = mapped
                norm[rows] = local_to_world(geom[rows], normalize(local))
                mapped_rows[rows] = True
        return {"pos": pos, "geom_norm": geom, "norm": norm, "uv": uv, "prim": prim, "mat": mat, "type": self.mat_type[mat],
                "base": base, "metallic": metallic, "roughness": roughness, "ior": self.mat_ior[mat], "normal_mapped": mapped_rows,
                "base_map": self.maps["baseColor"][mat], "wrapped": wrapped}

    def hit_surface(self, org, dirs):
        hit, prim, t, bu, bv = self.closest(org, dirs)
        return hit, self.surface(hit, prim, bu, bv)

    # ---- the environment map ----
    def env_colour(self, dirs):
        return linear_sample(self.env, to_plane(dirs))

    def env_pdf(self, wi):
        """environmentMapPdf (scene.h:374-378): no 1 / pi^2 and no sine, unlike the pdf NEE divides by (:397-398)."""
        h, w, _ = self.env.shape
        pdf = luminance(self.env_colour(wi)) * self.sum_light_power_inv * w * h * 0.5
        if self.plant == "env_pdf_sine":
            pdf = pdf * np.sin(to_plane(wi)[:, 1] * PI)
        return pdf

    def sample_light(self, pos, r4, visibility):
        """sampleDirectLight (scene.h:419-456, visibility) and sampleDirectLightNoVisibility (:458-492): the light's entry by the
        alias table; the LAST entry, when there is an environment sampler, is the map (:426, :466): a pixel by its own alias
        table, the direction of the pixel's centre, the pdf lum * sumLightPowerInv * w * h / pi^2 / 2, occlusion tested to
        pos + wi * 1e6 (:391), dist = 1e10 in the second form (:467).  Every other entry is light_pdf_f64's triangle, occlusion
        tested to the sampled point (before the single-sided test; both reject).
        Returns pdf (-1 rejected), radiance, wi, dist, and the masks is_env, occluded."""
        sd = self.sd
        n = len(pos)
        lid = alias_pick(sd.light_sampler, r4[:, 0], r4[:, 1])
        is_env = (lid == len(sd.light_sampler) - 1) & (len(sd.env_map_sampler) != 0)
        pdf, rad, wi, dist = np.full(n, -1.0), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
        occ = np.zeros(n, bool)
        tri = np.flatnonzero(~is_env)
        if len(tri):
            p, r, w_, d, sampled, valid = light_pdf_f64(sd, pos[tri], r4[tri])
            pdf[tri], rad[tri], wi[tri], dist[tri] = p, r, w_, d
            if visibility:
                occ[tri] = self.occluded(pos[tri], sampled)
        e = np.flatnonzero(is_env)
        if len(e):
            h, w, _ = self.env.shape
            pix = alias_pick(sd.env_map_sampler, r4[e, 2], r4[e, 3])
            y = pix // w
            x = pix - y * w
            half = 0.0 if self.plant == "env_pixel_corner" else 0.5
            rad[e] = self.env[y, x]
            wi[e] = to_sphere(np.stack([(x + half) / w, (y + half) / h], 1))
            scale = 1.0 if self.plant == "env_nee_no_inv_pi2" else 1.0 / (PI * PI)
            pdf[e] = luminance(rad[e]) * self.sum_light_power_inv * w * h * scale * 0.5
            dist[e] = 1e10
            if visibility:
                occ[e] = self.occluded(pos[e], pos[e] + wi[e] * 1e6)
        pdf = np.where(occ, -1.0, pdf)
        return pdf, rad, wi, dist, is_env, occ

    # ---- Material::BSDF / pdf / sample (material.h:131-275) on rows of hits ----
    def eval_bsdf(self, s, base, n, wo, wi):
        """(BSDF, pdf) of the hits `s` with base colour `base`: Lambertian base / pi and satDot / pi, MetallicWorkflow by
        float64_models.metallic_n with the MAPPED metallic and roughness, Dielectric 0 and 0."""
        ty = s["type"]
        bsdf, pdf = np.zeros((len(ty), 3)), np.zeros(len(ty))
        lam = ty == LAMBERTIAN
        bsdf[lam] = base[lam] / PI
        pdf[lam] = np.maximum(_dot(n[lam], wi[lam]), 0.0) / PI
        met = np.flatnonzero(ty == METALLIC_WORKFLOW)
        if len(met):
            b, p, _ = metallic_n(base[met], s["metallic"][met], s["roughness"][met], n[met], wo[met], wi[met])
            bsdf[met], pdf[met] = b, p
        return bsdf, pdf

    def sample_bsdf(self, s, base, n, wo, r3):
        """Material::sample: (dir, bsdf, pdf, type bits, events)."""
        k = len(n)
        ty = s["type"]
        d, bsdf, pdf, bits = np.zeros((k, 3)), np.zeros((k, 3)), np.zeros(k), np.full(k, INVALID)
        ev = {name: np.zeros(k, bool) for name in ("metal_diffuse_lobe", "metal_ggx_lobe", "metal_below_horizon", "refract_enter",
                                                   "refract_leave", "tir_reflects", "tir_invalid", "fresnel_reflects")}
        lam = np.flatnonzero(ty == LAMBERTIAN)
        if len(lam):  # material.h:141-147
            d[lam] = cosine_sample_hemisphere(n[lam], r3[lam, 0], r3[lam, 1])
            bsdf[lam] = base[lam] / PI
            pdf[lam] = np.maximum(_dot(n[lam], d[lam]), 0.0) / PI
            bits[lam] = 1 | 16
        met = np.flatnonzero(ty == METALLIC_WORKFLOW)
        if len(met):  # material.h:215-233
            metallic, rough = s["metallic"][met], s["roughness"][met]
            diffuse = r3[met, 2] > 1.0 / (2.0 - metallic)
            h = ggx_sample(n[met], wo[met], rough * rough, r3[met, 0], r3[met, 1])
            spec = 2.0 * _dot(wo[met], h)[:, None] * h - wo[met]  # -reflect(wo, h)
            dm = np.where(diffuse[:, None], cosine_sample_hemisphere(n[met], r3[met, 0], r3[met, 1]), spec)
            below = _dot(n[met], dm) < 0.0
            b, p, _ = metallic_n(base[met], metallic, rough, n[met], wo[met], dm)
            d[met], bsdf[met], pdf[met] = dm, b, p
            bits[met] = np.where(below, INVALID, 2 | 16)
            ev["metal_diffuse_lobe"][met], ev["metal_ggx_lobe"][met], ev["metal_below_horizon"][met] = diffuse & ~below, ~diffuse & ~below, below
        die = np.flatnonzero(ty == DIELECTRIC)
        if len(die):  # material.h:159-183
            dd, b, typ, f, sin2_tr = dielectric_sample_n(base[die], s["ior"][die], n[die], wo[die], r3[die, 2])
            reflect = r3[die, 2] < f
            tir = sin2_tr >= 1.0  # Math::refract fails (mathUtil.h:177); fresnel() has returned 1 for it (material.h:55-57)
            cos = _dot(n[die], wo[die])
            d[die], bsdf[die], pdf[die] = dd, b, 1.0
            bits[die] = np.where(~reflect & tir, INVALID, typ)
            ev["refract_enter"][die], ev["refract_leave"][die] = ~reflect & ~tir & (cos > 0.0), ~reflect & ~tir & (cos < 0.0)
            ev["tir_reflects"][die], ev["tir_invalid"][die] = reflect & tir, ~reflect & tir
            ev["fresnel_reflects"][die] = reflect & ~tir
        return d, bsdf, pdf, bits, ev

    # ---- the interface restir_model reads ----
    def intersect(self, org, dirs):
        """restir_model's `_intersect`: (hit, surface handle, pos, normal after the maps, material id); the handle keeps the
        mapped metallic and roughness for bsdf()."""
        hit, s = self.hit_surface(org, dirs)
        return hit, s, s["pos"], s["norm"], s["mat"]

    def bsdf(self, handle, rows, n, wo, wi):
        """Material::BSDF with baseColor = 1 (restir.cu:125) at the rows `rows` of an intersect() handle."""
        s = {k: handle[k][rows] for k in ("type", "metallic", "roughness")}
        with np.errstate(all="ignore"):
            out = self.eval_bsdf(s, np.ones((len(n), 3)), n, wo, wi)[0]
        return np.where(wi.any(1)[:, None], out, 0.0)  # the zero sample of a rejected draw: cosI = 0

    def sample_light_no_visibility(self, pos, r4):
        pdf, rad, wi, dist, _, _ = self.sample_light(pos, r4, False)
        return pdf, rad, wi, dist, pdf > -1.0

    def albedo(self, handle):
        return handle["base"]

    def miss_colour(self, dirs):
        """What a ray that hits nothing sees (restir.cu:117-122, gBuffer.cu:61-66, pathtrace.cu:309-313): the map, or black."""
        return self.env_colour(dirs) if self.env is not None else np.zeros((len(dirs), 3))


# ---------------------------------------------------------------------------------------------------------------------
# singleKernelPT
# ---------------------------------------------------------------------------------------------------------------------
def _mean(prev, x, it):  # (prev * iter + x) / (iter + 1)
    return (prev * float(it) + x) / float(it + 1)


def single_kernel_pt(scene, cam, looper, max_depth, iter=0, prev=None):
    """pathtrace.cu:149-291.  prev: (direct, indirect) of the iterations before `iter` (zeros without).  Returns a dict:
    direct, indirect (after hasNanOrInf, HDRToLDR and the running mean), raw_direct, raw_indirect (before them), cursor (the
    draws each pixel consumed) and events: boolean masks per pixel, true where the named rule decided part of the pixel's
    value."""
    W, H = (int(v) for v in cam["resolution"])
    n = W * H
    rows = np.arange(n)
    plant = scene.plant
    u = sobol_draws(scene.sd.sobol, looper, rows, 4 + 7 * max_depth + 7)  # head room for the planted extra draws
    org, dirs = _camera_rays_f64(cam, W, H, u[:, 0:2])  # sample4D (:164); a pinhole reads .x, .y only
    cur = np.full(n, 4)
    hit, s = scene.hit_surface(org, dirs)
    direct, indirect = np.zeros((n, 3)), np.zeros((n, 3))
    ev = {}

    def mark(name, mask):
        ev[name] = ev.get(name, np.zeros(n, bool)) | mask

    miss0 = ~hit
    light0 = hit & (s["type"] == LIGHT)
    direct[miss0 | light0] = 1.0  # :169-172 whatever the map says, :179-182 (baseColor was set to 1 at :177)
    if plant == "primary_miss_env_colour" and scene.env is not None:
        direct[miss0] = scene.env_colour(dirs[miss0])
    mark("primary_miss", miss0)
    mark("emitter_seen_directly", light0)
    alive = hit & ~light0
    base = np.ones((n, 3))  # DENOISER_DEMODULATE (:175-178): the first hit's colour is 1
    thr = np.ones((n, 3))
    wo = -dirs
    norm = s["norm"]
    with np.errstate(all="ignore"):
        for depth in range(1, max_depth + 1):
            delta = s["type"] == DIELECTRIC
            behind = alive & (cur < 4 + 7 * (depth - 1))
            if depth == 3:
                mark("cursor_behind_at_depth_3", behind)
            neg = _dot(norm, wo) < 0.0
            flip = neg if plant == "dielectric_normal_flipped" else ~delta & neg  # :190-193
            mark("normal_map_flip_differs", alive & ~delta & s["normal_mapped"] & (neg != (_dot(s["geom_norm"], wo) < 0.0)))
            norm = np.where(flip[:, None], -norm, norm)
            # ---- next-event estimation (:195-208) ----
            nee = alive & ~delta
            r4 = u[rows[:, None], cur[:, None] + np.arange(4)]
            lpdf, rad, wi, _, is_env, occ = scene.sample_light(s["pos"], r4, True)
            bsdf, bpdf = scene.eval_bsdf(s, base, norm, wo, wi)
            contrib = thr * bsdf * rad * (np.maximum(_dot(norm, wi), 0.0) / lpdf * power_heuristic(lpdf, bpdf))[:, None]
            ok = nee & (lpdf > 0.0)
            (direct if depth == 1 else indirect)[ok] += contrib[ok]
            lit = ok & (contrib != 0.0).any(1)
            mark("env_nee_direct" if depth == 1 else "env_nee_indirect", lit & is_env)
            mark("env_nee_occluded", nee & is_env & occ)
            if depth >= 2:
                mark("base_colour_wrapped_uv", lit & (s["base_map"] > NULL_TEXTURE) & s["wrapped"])
                mark("procedural_at_depth_2_or_more", lit & (s["base_map"] == PROCEDURAL_TEXTURE))
            cur = cur + 4 * (alive if plant == "dielectric_nee_draws" else nee)  # no sample4D for a dielectric
            # ---- the BSDF sample (:210-223) ----
            r3 = u[rows[:, None], cur[:, None] + np.arange(3)]
            cur = cur + 3 * alive
            sdir, sbsdf, spdf, bits, sev = scene.sample_bsdf(s, base, norm, wo, r3)
            for k, v in sev.items():
                mark(k, alive & v)
            alive = alive & (bits != INVALID) & ~(spdf < 1e-8)  # :213-218
            specular = (bits & SPECULAR) != 0
            cos = np.abs(_dot(norm, sdir))
            thr = thr * sbsdf / spdf[:, None] * np.where(specular & (plant != "specular_cosine"), 1.0, cos)[:, None]
            ray_org = s["pos"] + sdir * 1e-5  # makeOffsetedRay (:225)
            cur_pos = s["pos"]
            hit, s = scene.hit_surface(ray_org, sdir)
            wo = -sdir
            # ---- the miss branch (:232-247) ----
            missed = alive & ~hit
            if scene.env is not None and missed.any():
                m = np.flatnonzero(missed)
                w = np.where(specular[m], 1.0, power_heuristic(spdf[m], scene.env_pdf(sdir[m])))
                indirect[m] += scene.env_colour(sdir[m]) * thr[m] * w[:, None]
                mark("miss_into_map_mis", missed & ~specular)
                mark("miss_into_map_after_specular", missed & specular)
            alive = alive & hit
            # ---- the emitter branch (:249-271): the single-sided test on the INTERPOLATED normal ----
            norm = s["norm"]
            base = s["base"]
            is_light = alive & (s["type"] == LIGHT)
            refused = is_light & (_dot(norm, sdir) < 0.0)
            collect = is_light & ~refused
            yx = cur_pos - s["pos"]
            lp = luminance(base) * scene.sum_light_power_inv * scene.tri_area[s["prim"]] * _dot(yx, yx) / np.abs(_dot(norm, normalize(yx)))
            w = np.where(specular, 1.0, power_heuristic(spdf, lp))
            indirect[collect] += (base * thr * w[:, None])[collect]
            mark("emitter_collected", collect)
            mark("emitter_collected_after_specular", collect & specular)
            mark("emitter_refused_single_sided", refused)
            alive = alive & ~is_light
    out = {"raw_direct": direct.copy(), "raw_indirect": indirect.copy(), "cursor": cur, "events": ev}
    prev = (np.zeros((n, 3)), np.zeros((n, 3))) if prev is None else prev
    for k, (x, p) in enumerate(((direct, prev[0]), (indirect, prev[1]))):
        x = R._f32_range(x)
        x = np.where((np.isnan(x) | np.isinf(x)).any(1)[:, None], 0.0, x)  # hasNanOrInf (:279-284)
        x = x / (x + 1.0)  # HDRToLDR (mathUtil.h:49-51)
        out["direct" if k == 0 else "indirect"] = _mean(p, x, iter)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# PTDirectKernel
# ---------------------------------------------------------------------------------------------------------------------
def pt_direct(scene, cam, looper, iter=0, prev=None):
    """pathtrace.cu:293-345: one light sample at the first hit, no MIS, no clean-up and no tone map; a miss shows the map, an
    emitter its colour; a dielectric stays black."""
    W, H = (int(v) for v in cam["resolution"])
    n = W * H
    u = sobol_draws(scene.sd.sobol, looper, np.arange(n), 8)
    org, dirs = _camera_rays_f64(cam, W, H, u[:, 0:2])
    hit, s = scene.hit_surface(org, dirs)
    direct = np.zeros((n, 3))
    direct[~hit] = scene.miss_colour(dirs[~hit])
    light = hit & (s["type"] == LIGHT)
    direct[light] = s["base"][light]
    shade = hit & ~light & (s["type"] != DIELECTRIC)
    wo = -dirs
    norm = np.where((_dot(s["norm"], wo) < 0.0)[:, None], -s["norm"], s["norm"])
    lpdf, rad, wi, _, _, _ = scene.sample_light(s["pos"], u[:, 4:8], True)
    with np.errstate(all="ignore"):
        val = rad * scene.eval_bsdf(s, s["base"], norm, wo, wi)[0] * (np.maximum(_dot(norm, wi), 0.0) / lpdf)[:, None]
    ok = shade & (lpdf > 0.0)
    direct[ok] = val[ok]
    return _mean(np.zeros((n, 3)) if prev is None else prev, direct, iter)


# ---------------------------------------------------------------------------------------------------------------------
# renderGBuffer
# ---------------------------------------------------------------------------------------------------------------------
def gbuffer(scene, cam, last_cam):
    """renderGBuffer (gBuffer.cu:3-76) on general geometry: restir_model.gbuffer with the scene's surface fetch — the albedo is
    the material's colour AFTER its maps, the normal the one AFTER the normal map (:43-46), and a miss stores the map's colour
    as albedo with primId -1, depth 1, motion 0 and a zero normal (:61-74)."""
    return R.gbuffer(scene, cam, last_cam)
