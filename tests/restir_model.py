"""A float64 numpy statement of ReSTIR DI's reuse logic and of the G-buffer planes it reads, written from the reference text
(src/restir.cu, src/restir.h, src/gBuffer.cu, the camera of src/sceneStructs.h) — vectorised over pixels, one array operation per
rule, in a different form from oracle/oracle.cpp and from the device code, neither of which it reads or calls.

Three STEPS, each taking the state before it and returning the state after it:

    gbuffer(scene, cam, last_cam)                                          gBuffer.cu:3-76
    pass1(scene, cam, looper, gb_planes, last_reservoirs, first_frame, reuse, faithful)     restir.cu:109-178, 186-187
    pass2(scene, cam, looper, gb_planes, temp_reservoirs, pass1_state, reuse, iter, image_in)       restir.cu:180-202

What a step reads from EARLIER steps (the G-buffer planes, last frame's reservoirs, the `reservoirTemp` plane, the pixel's own
reservoir) is handed in by the caller from the code under test, so a float32/float64 difference in one discrete choice stays in
the pixel where it arose (tests/restir_model_checks.py drives the sequence).

The reference's kernel has a `__syncthreads()` between storing `reservoirTemp` and reading the neighbours' entries, which orders
only one 8x8 block; the model follows the two-pass reading (every pixel's store before any pixel's spatial reuse).

Geometry is restricted to horizontal quads (two triangles each, one authored normal per quad), so `_hit_quads` is the whole
intersector; no environment map, no textures.  (That restriction is ModelScene's alone: the steps below reach geometry, materials
and lights through the scene's methods only, and tests/path_model.py's PathScene answers them on general triangles with the
surface fetch, the four maps and the environment map — tests/path_model_checks.py runs the same three steps on it.)  Draws rejected by `sampleDirectLightNoVisibility` leave Li, wi and dist at zero
(the reference leaves them uninitialised; the project defines them).
"""
import numpy as np

from test_oracle_float64 import _camera_rays_f64, _hit_quads, light_pdf_f64, luminance, normalize, sobol_draws  # noqa: F401
from test_oracle_kat import _metallic_ref

PI = np.pi
NULL_PRIMITIVE = -1
LAMBERTIAN, METALLIC_WORKFLOW, DIELECTRIC, LIGHT = 0, 1, 2, 4  # Material::Type (src/material.h:129)
RESERVOIR_SIZE = 32  # restir.h:9
TEMPORAL, SPATIAL = 1, 2  # ReservoirReuse bits
MAX_DIMS = 4 + 5 * RESERVOIR_SIZE + 1 + 5 * 3 + 1


# ---------------------------------------------------------------------------------------------------------------------
# scene: a list of horizontal quads read off the scene container's arrays
# ---------------------------------------------------------------------------------------------------------------------
class ModelScene:
    def __init__(self, sd):
        self.sd = sd
        V = sd.vertices.astype(np.float64).reshape(-1, 3, 3)
        N = sd.normals.astype(np.float64).reshape(-1, 3, 3)
        self.quads, mats, nrm = [], [], []
        for q in range(len(V) // 2):
            a, b = V[2 * q], V[2 * q + 1]
            lo, hi = np.minimum(a.min(0), b.min(0)), np.maximum(a.max(0), b.max(0))
            assert lo[1] == hi[1], "horizontal quads only"
            self.quads.append((lo[1], lo[0], hi[0], lo[2], hi[2], q))
            mats.append(int(sd.material_ids[2 * q]))
            nrm.append(N[2 * q, 0])
        self.quad_mat = np.array(mats)
        self.quad_normal = normalize(np.array(nrm))  # getIntersecGeomInfo normalises the interpolated normal (scene.h:162)
        self.mat_type = sd.materials["type"].astype(np.int64)
        self.mat_color = sd.materials["baseColor"].astype(np.float64)
        self.mat_metallic = sd.materials["metallic"].astype(np.float64)
        self.mat_roughness = sd.materials["roughness"].astype(np.float64)

    # What the three steps ask of a scene.  `handle` is whatever intersect() returned second, for all its rays; here the
    # material ids.
    def intersect(self, org, dirs):
        """scene->intersect on quads: (hit, handle, pos, interpolated normal, material id)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            t, q = _hit_quads(org, dirs, self.quads)
        hit = q >= 0
        qq = np.maximum(q, 0)
        pos = org + dirs * np.where(hit, t, 0.0)[:, None]
        return hit, self.quad_mat[qq], pos, self.quad_normal[qq], self.quad_mat[qq]

    def occluded(self, x, y):
        """testOcclusion(x, y) (scene.h:303-334): the segment shortened by 1e-4, its origin pushed 1e-5 along it."""
        d = y - x
        dist = np.linalg.norm(d, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = d / dist[:, None]
            t, _ = _hit_quads(x + d * 1e-5, d, self.quads)
        return t < dist - 1e-4  # a zero-length segment has a NaN direction and hits nothing

    def bsdf(self, handle, rows, n, wo, wi):
        """Material::BSDF with baseColor = 1 (restir.cu:125), rows of (n, wo, wi): Lambertian 1/pi, MetallicWorkflow by the
        float64 statement of tests/test_oracle_kat.py, Dielectric 0 (material.h:131-134, 149-152, 187-204)."""
        mat = handle[rows]
        out = np.zeros((len(mat), 3))
        ty = self.mat_type[mat]
        out[ty == LAMBERTIAN] = 1.0 / PI
        one = np.ones(3)
        for k in np.flatnonzero(ty == METALLIC_WORKFLOW):
            if not wi[k].any():
                continue  # the zero sample of a rejected draw: cosI = 0 and the BSDF is 0
            out[k] = _metallic_ref(one, self.mat_metallic[mat[k]], self.mat_roughness[mat[k]], n[k], wo[k], wi[k])[0]
        return out

    def sample_light_no_visibility(self, pos, r4):
        """sampleDirectLightNoVisibility (scene.h:458-492): (pdf, radiance, wi, dist, accepted)."""
        pdf, rad, wi, dist, _, valid = light_pdf_f64(self.sd, pos, r4)
        return pdf, rad, wi, dist, valid

    def albedo(self, handle):
        return self.mat_color[handle]

    def miss_colour(self, dirs):
        """What a primary ray that hits nothing shows (restir.cu:117-122, gBuffer.cu:61-66): black without an environment map."""
        return np.zeros((len(dirs), 3))


def _dot(a, b):
    return np.einsum("...j,...j->...", a, b)


def _intersect(scene, org, dirs):
    return scene.intersect(org, dirs)


def _occluded(scene, x, y):
    return scene.occluded(x, y)


def _bsdf(scene, handle, rows, n, wo, wi):
    return scene.bsdf(handle, rows, n, wo, wi)


# ---------------------------------------------------------------------------------------------------------------------
# reservoirs as dicts of arrays; restir.h:10-93
# ---------------------------------------------------------------------------------------------------------------------
def empty_reservoirs(n):
    return {"Li": np.zeros((n, 3)), "wi": np.zeros((n, 3)), "dist": np.zeros(n), "numSamples": np.zeros(n, np.int64),
            "weight": np.zeros(n)}


def reservoirs_from_records(rec):
    """RESERVOIR_DTYPE records of the code under test -> float64 arrays."""
    return {"Li": rec["Li"].astype(np.float64), "wi": rec["wi"].astype(np.float64), "dist": rec["dist"].astype(np.float64),
            "numSamples": rec["numSamples"].astype(np.int64), "weight": rec["weight"].astype(np.float64)}


FLT_MAX = float(np.finfo(np.float32).max)


def _f32_range(x):
    """The reference's quantities are binary32: a magnitude past FLT_MAX is an infinity there, and `invalid()`, `hasNanOrInf`
    and every comparison after it see it as one.  (Only the range is taken over, not the rounding.)"""
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) > FLT_MAX, np.copysign(np.inf, x), x)


def _take(r, idx):
    return {k: v[idx].copy() for k, v in r.items()}


def _copy(r):
    return {k: v.copy() for k, v in r.items()}


def _invalid(r):  # restir.h:42
    w = r["weight"]
    with np.errstate(invalid="ignore"):
        return np.isnan(w) | np.isinf(w) | (w < 0.0)


def _check_validity(r):  # restir.h:44-49: clear() zeroes weight and count and keeps the sample
    bad = _invalid(r)
    r["weight"] = np.where(bad, 0.0, r["weight"])
    r["numSamples"] = np.where(bad, 0, r["numSamples"])
    return bad


def _merge(r, rhs, rand, where):
    """restir.h:51-58 on the rows `where`; the others are left alone."""
    with np.errstate(invalid="ignore"):
        w = _f32_range(r["weight"] + rhs["weight"])
        take = where & (rand * w < rhs["weight"])
    r["weight"] = np.where(where, w, r["weight"])
    r["numSamples"] = np.where(where, r["numSamples"] + rhs["numSamples"], r["numSamples"])
    for k in ("Li", "wi"):
        r[k] = np.where(take[:, None], rhs[k], r[k])
    r["dist"] = np.where(take, rhs["dist"], r["dist"])
    return take


def _pre_clamped_merge(r, rhs, rand, where, M=20):  # restir.h:69-77
    rhs = _copy(rhs)
    clamp = (rhs["numSamples"] > 0) & (rhs["numSamples"] > (M - 1) * r["numSamples"]) & (r["numSamples"] > 0)
    scale = (M - 1.0) * r["numSamples"] / np.maximum(rhs["numSamples"], 1)
    rhs["weight"] = np.where(clamp, rhs["weight"] * scale, rhs["weight"])
    rhs["numSamples"] = np.where(clamp, (M - 1) * r["numSamples"], rhs["numSamples"])
    _merge(r, rhs, rand, where)
    return clamp & where


# ---------------------------------------------------------------------------------------------------------------------
# step 1: the G-buffer
# ---------------------------------------------------------------------------------------------------------------------
def raster_coord(cam, pos):
    """Camera::getRasterCoord (sceneStructs.h:22-48): the view direction scaled to unit depth, expressed in (right, up, view),
    divided by the frustum's half extents, mirrored, mapped to [0, 1], times the resolution, converted to int (toward zero)."""
    W, H = (int(v) for v in cam["resolution"])
    right, up, view, eye = (cam[k].astype(np.float64) for k in ("right", "up", "view", "position"))
    d = normalize(pos - eye)
    d = d / _dot(d, view)[:, None]
    inv = np.linalg.inv(np.stack([right, up, view], 1))  # rotationMatInv = inverse(mat3(right, up, view)), columns
    p = d @ inv.T
    tan_fov = np.tan(np.radians(float(cam["fov"][1])))
    uv = -np.stack([p[:, 0] / (W / H * tan_fov), p[:, 1] / tan_fov], 1) * 0.5 + 0.5
    return np.trunc(uv * np.array([W, H], np.float64)).astype(np.int64)


def gbuffer(scene, cam, last_cam):
    """renderGBuffer (gBuffer.cu:3-76).  The centre ray of :11-26 is Camera::sample's with r = (.5, .5).  "primId" holds the
    MATERIAL id (:34, :47), NullPrimitive - 1 for an emitter whichever way it faces (:36; the primId rewrite of :38-40 is read by
    nothing), NullPrimitive for a miss together with depth 1, motion 0 and a zero normal (:61-74).  Without a last camera (the
    first frame; the reference's is uninitialised) the current one is used."""
    W, H = (int(v) for v in cam["resolution"])
    n = W * H
    org, dirs = _camera_rays_f64(cam, W, H, np.full((n, 2), 0.5))
    hit, handle, pos, nrm, mat = _intersect(scene, org, dirs)
    light = scene.mat_type[mat] == LIGHT
    rc = raster_coord(cam if last_cam is None else last_cam, np.where(hit[:, None], pos, org + dirs))
    inside = (rc[:, 0] >= 0) & (rc[:, 0] < W) & (rc[:, 1] >= 0) & (rc[:, 1] < H)
    return {
        "albedo": np.where(hit[:, None], scene.albedo(handle), scene.miss_colour(dirs)),  # :43-45, :61-66
        "normal": np.where(hit[:, None], nrm, 0.0),
        "primId": np.where(hit, np.where(light, NULL_PRIMITIVE - 1, mat), NULL_PRIMITIVE),
        "depth": np.where(hit, np.linalg.norm(pos - org, axis=1), 1.0),
        "motion": np.where(hit, np.where(inside, rc[:, 1] * W + rc[:, 0], -1), 0),
    }


# ---------------------------------------------------------------------------------------------------------------------
# step 2: candidates, shadow test, temporal reuse, the two stores
# ---------------------------------------------------------------------------------------------------------------------
def find_temporal_neighbor(gb, last, idx):
    """findTemporalNeighbor (restir.cu:19-40) for the pixels `idx`: (the reservoirs it returns, which rule decided).
    gb: cur planes "primId", "normal", "motion" and the OTHER half of the double buffer as "lastPrimId", "lastNormal"."""
    prim = gb["primId"][idx]
    last_idx = gb["motion"][idx]
    li = np.maximum(last_idx, 0)
    off = last_idx < 0
    null = ~off & (prim <= NULL_PRIMITIVE)
    changed = ~off & ~null & (gb["lastPrimId"][li] != prim)
    cos = _dot(gb["normal"][idx], gb["lastNormal"][li])
    turned = ~off & ~null & ~changed & (np.abs(cos) < 0.1)  # absDot: a reversed normal is accepted here
    diff = off | null | changed | turned
    r = _take(last, li)
    for k, v in r.items():
        r[k] = np.where(diff.reshape((-1,) + (1,) * (v.ndim - 1)), 0, v)  # T()
    return r, {"off_frame": off, "null_id": null, "changed_id": changed, "normal": turned, "accepted": ~diff,
               "accepted_reversed": ~diff & (cos < 0.0)}


def pass1(scene, cam, looper, gb_planes, last_reservoirs, first_frame, reuse, faithful):
    """restir.cu:109-178 and 186-187.  Returns a dict:
      out, temp   what the pixel stores to reservoirOut / reservoirTemp, rows meaningful where `stored` / `stored_temp`
                  (a miss or an emitter returns before either store, and reservoirTemp is written under Spatial only)
      dims        Sobol dimensions consumed so far
      status      0 shaded, 1 miss, 2 emitter;  pos, normal (flipped to face wo unless Dielectric), wo, mat of the shaded
      live        boolean masks per rule, for the liveness counts"""
    W, H = (int(v) for v in cam["resolution"])
    n = W * H
    c = _candidates(scene, cam, looper, bool(faithful))  # :109-163, the same for every reuse mask
    u, sh, status, mat = c["u"], c["sh"], c["status"], c["mat"]
    r = _copy(c["reservoir"])

    dims = np.full(n, 4)
    dims[sh] = 4 + 5 * RESERVOIR_SIZE
    live = {"flipped": c["flipped"], "shadowed": c["shadowed"]}
    if not first_frame and (reuse & TEMPORAL):  # :165-170
        temporal, why = find_temporal_neighbor(gb_planes, last_reservoirs, sh)
        merge = ~_invalid(temporal)  # T() has weight 0 and is NOT invalid: a rejected neighbour still costs the draw
        clamped = _pre_clamped_merge(r, temporal, u[sh, dims[sh]], merge)
        dims[sh] += merge
        live.update({"temporal_" + k: v for k, v in why.items()})
        live.update({"temporal_skipped": ~merge, "clamped": clamped, "unclamped": why["accepted"] & merge & ~clamped})

    out = _copy(r)  # tempReservoir (:173), stored after checkValidity (:186-187): the PRE-spatial reservoir
    live["cleared_out"] = _check_validity(out)
    temp = _copy(r)
    if reuse & SPATIAL:  # :175-177
        live["cleared_temp"] = _check_validity(temp)

    def full(a):
        o = np.zeros((n,) + a.shape[1:], a.dtype)
        o[sh] = a
        return o

    stored = status == 0
    return {"out": {k: full(v) for k, v in out.items()}, "temp": {k: full(v) for k, v in temp.items()}, "stored": stored,
            "stored_temp": stored & bool(reuse & SPATIAL), "dims": dims, "status": status, "pos": full(c["pos"]),
            "normal": full(c["normal"]), "wo": full(c["wo"]), "mat": mat, "handle": c["handle"], "miss_colour": c["miss_colour"], "live": {k: full(v) for k, v in live.items()}}


_CANDIDATE_CACHE = {}


def _candidates(scene, cam, looper, faithful):
    """The part of pass 1 that reads nothing from earlier frames: primary ray, early exits, normal flip, the 32 candidates and
    the shadow test of the kept one (restir.cu:109-163)."""
    key = (id(scene), cam.tobytes(), looper, faithful)
    if key in _CANDIDATE_CACHE:
        return _CANDIDATE_CACHE[key]
    W, H = (int(v) for v in cam["resolution"])
    n = W * H
    idx = np.arange(n)
    u = sobol_draws(scene.sd.sobol, looper, idx, MAX_DIMS)
    org, dirs = _camera_rays_f64(cam, W, H, u[:, 0:2])  # sample4D: the lens draws .z, .w are unused by a pinhole
    hit, handle, pos, nrm, mat = _intersect(scene, org, dirs)
    status = np.where(~hit, 1, np.where(scene.mat_type[mat] == LIGHT, 2, 0))  # :117-130
    sh = np.flatnonzero(status == 0)
    pos_s, mat_s, wo = pos[sh], mat[sh], -dirs[sh]
    flip = (scene.mat_type[mat_s] != DIELECTRIC) & (_dot(nrm[sh], wo) < 0.0)  # :134-137
    n_s = np.where(flip[:, None], -nrm[sh], nrm[sh])

    r = empty_reservoirs(len(sh))
    for i in range(RESERVOIR_SIZE):  # :140-156
        c = 4 + 5 * i
        pdf, rad, wi, dist, valid = scene.sample_light_no_visibility(pos_s, u[sh, c:c + 4])
        Li = np.where(valid[:, None], rad, 0.0)
        wi = np.where(valid[:, None], wi, 0.0)
        dist = np.where(valid, dist, 0.0)
        p_hat = Li * _bsdf(scene, handle, sh, n_s, wo, wi) * np.maximum(_dot(n_s, wi), 0.0)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.linalg.norm(p_hat / pdf[:, None], axis=1)
        w = np.where(np.isnan(w) | np.isinf(w) | (pdf <= 0.0), 0.0, w)
        rand = u[sh, c + 4]
        # Reservoir::update (restir.h:17-24)
        r["weight"] = _f32_range(r["weight"] + w)
        r["numSamples"] = r["numSamples"] + 1
        if faithful:  # `if (rand * weight / newWeight)`: any float but 0 is true, x / 0 (inf or NaN) included
            take = ~((rand * r["weight"] == 0.0) & (w != 0.0))
        else:  # weighted reservoir sampling, the corrected rule
            take = rand * r["weight"] < w
        r["Li"] = np.where(take[:, None], Li, r["Li"])
        r["wi"] = np.where(take[:, None], wi, r["wi"])
        r["dist"] = np.where(take, dist, r["dist"])
    shadowed = _occluded(scene, pos_s, pos_s + r["wi"] * r["dist"][:, None])  # :158-163
    r["weight"] = np.where(shadowed, 0.0, r["weight"])
    c = {"scene": scene, "u": u, "sh": sh, "status": status, "mat": mat, "handle": handle, "miss_colour": scene.miss_colour(dirs), "reservoir": r, "pos": pos_s, "normal": n_s, "wo": wo, "flipped": flip,
         "shadowed": shadowed}
    _CANDIDATE_CACHE[key] = c
    return c


# ---------------------------------------------------------------------------------------------------------------------
# step 3: spatial reuse, shading, the running mean
# ---------------------------------------------------------------------------------------------------------------------
def find_spatial_neighbor_disk(gb, temp, x, y, W, H, r2):
    """findSpatialNeighborDisk (restir.cu:42-80): (the reservoirs it returns, which rule decided)."""
    radius = 5.0
    rr, theta = np.sqrt(r2[:, 0]), 2.0 * PI * r2[:, 1]  # the polar "concentricSampleDisk" (mathUtil.h:132-136)
    fx = x + 0.5 + rr * np.cos(theta) * radius
    fy = y + 0.5 + rr * np.sin(theta) * radius
    px, py = np.trunc(fx).astype(np.int64), np.trunc(fy).astype(np.int64)  # float -> int truncates toward zero
    idx = y * W + x
    left, right, top, bottom = px < 0, px >= W, py < 0, py >= H
    oob = left | right | top | bottom
    me = ~oob & (px == x) & (py == y)
    p_idx = np.where(oob, 0, py * W + px)
    other = ~oob & ~me & (gb["primId"][p_idx] != gb["primId"][idx])
    rest = ~oob & ~me & ~other
    cos = _dot(gb["normal"][idx], gb["normal"][p_idx])
    turned = rest & (cos < 0.1)  # plain dot: a reversed normal is rejected here
    depth = gb["depth"][idx]
    far = rest & (np.abs(depth - gb["depth"][p_idx]) > depth * 0.1)  # relative to THIS pixel's depth; tested whatever the normals say
    diff = oob | me | other | turned | far
    r = _take(temp, p_idx)
    for k, v in r.items():
        r[k] = np.where(diff.reshape((-1,) + (1,) * (v.ndim - 1)), 0, v)
    why = {"left": left, "right": right, "top": top, "bottom": bottom, "self": me, "other_id": other, "normal": turned,
           "depth": far, "accepted": ~diff, "zero_from_negative": ((fx < 0) & (px == 0)) | ((fy < 0) & (py == 0)), "normal_reversed": turned & (cos < -0.1)}
    return r, why


def pass2(scene, cam, looper, gb_planes, temp_reservoirs, pass1_state, reuse, iter, image_in):
    """restir.cu:180-202.  pass1_state: pass1()'s dict with "own" added — the pixel's own reservoir as it stands after
    restir.cu:177, i.e. the `reservoirTemp` entry under Spatial and the stored `reservoirOut` entry otherwise (whose cleared
    weight shades to 0 exactly as the invalid weight it replaces does, :190-198).  Returns image, dims, live."""
    W, H = (int(v) for v in cam["resolution"])
    n = W * H
    st = pass1_state
    sh = np.flatnonzero(st["status"] == 0)
    x, y = sh % W, sh // W
    u = sobol_draws(scene.sd.sobol, looper, np.arange(n), MAX_DIMS + 1)[sh]
    d = st["dims"][sh].copy()
    r = _take(st["own"], sh)
    live = {}
    if reuse & SPATIAL:
        first_dim = d.copy()
        agg = empty_reservoirs(len(sh))  # mergeSpatialNeighborDirect (:82-95)
        rows = np.arange(len(sh))
        counts = {}
        for i in range(5):
            r2 = np.stack([u[rows, d], u[rows, d + 1]], 1)
            d = d + 2
            nb, why = find_spatial_neighbor_disk(gb_planes, temp_reservoirs, x, y, W, H, r2)
            ok = ~_invalid(nb)
            _merge(agg, nb, u[rows, d], ok)
            d = d + ok
            for k, v in why.items():
                counts[k] = counts.get(k, 0) + v
            counts["neighbour_invalid"] = counts.get("neighbour_invalid", 0) + ~ok
        final = ~_invalid(agg) & ~_invalid(r)  # :182-184
        _merge(r, agg, u[rows, d], final)
        d = d + final
        live = {"spatial_" + k: v for k, v in counts.items()}
        live.update({"final_skipped_own_invalid": _invalid(r) & ~final, "final_skipped_agg_invalid": _invalid(agg),
                     "final_merged": final, "first_spatial_dim": first_dim})
    direct = np.zeros((n, 3))
    direct[st["status"] == 2] = 1.0  # an emitter seen directly: baseColor = 1 (:125-130)
    direct[st["status"] == 1] = st["miss_colour"][st["status"] == 1]  # a miss: the map's colour, 0 without one (:117-122)
    p_hat = r["Li"] * _bsdf(scene, st["handle"], sh, st["normal"][sh], st["wo"][sh], r["wi"]) \
        * np.maximum(_dot(st["normal"][sh], r["wi"]), 0.0)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        Wr = _f32_range(r["weight"] / (np.linalg.norm(p_hat, axis=1) * r["numSamples"]))  # Reservoir::W (restir.h:37-40)
        shaded = np.where(_invalid(r)[:, None], 0.0, _f32_range(p_hat * Wr[:, None]))
    shaded = np.where((np.isnan(shaded) | np.isinf(shaded)).any(1)[:, None], 0.0, shaded)  # :196-198
    direct[sh] = shaded
    direct = direct * gb_planes["albedo"]  # :200
    image = (image_in * float(iter) + direct) / float(iter + 1)  # :201-202
    dims = st["dims"].copy()
    dims[sh] = d

    def full(a):
        o = np.zeros((n,) + a.shape[1:], a.dtype)
        o[sh] = a
        return o

    return {"image": image, "dims": dims, "live": {k: full(np.asarray(v)) for k, v in live.items()}}
