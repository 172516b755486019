"""The lens (rdh_set_lens) restated twice, shared by tests/test_lens_cpu.py and tests/test_gpu_lens.py.

lens_rays_f32: every pixel's primary ray as cameraSample (bsdf.h) computes it, in numpy float32, one array operation per rule of
the semantics (include/radish_hip.h, "the lens") and per operation of Camera::sample (sceneStructs.h:72-91).  numpy's float32
add / sub / mul / div / sqrt are IEEE binary32 operations and never contracted, which is the library's numerics contract
(DESIGN 2); sine and cosine are the oracle library's sincos (orc_sincos_n), the normalise is tests/motion_model.py's, the camera's
tanFovY is motion_model.device_camera's (the host's tanf).  The GPU test holds rdh_debug_primary_rays to it bit for bit.

lens_rays_f64: the same thin lens in float64, written without the float32 code: the aperture point, then the ray from it through
the pixel's point on the focal plane.  tests/path_model.py's evaluations start from these rays (with_lens below).

`plant` puts one mistake into either: "swap_uv" (u and v exchanged), "jy_raw" (jy = r.w, without its remap), "no_flip"
(2u - 1 for 1 - 2u), "dir_pinhole" (the lens offset applied to the origin but not to the direction)."""
import contextlib

import numpy as np

import motion_model as M
from oracle import pyoracle
from test_oracle_float64 import sobol_draws, utilhash

F = np.float32
OFF, DISK, MASK = "off", "disk", "mask"
ONE_BELOW = F(np.nextafter(np.float32(1), np.float32(0)))  # 0x1.fffffep-1f
TWO_PI_F = F(6.2831853071795864769252867665590057683943)
PLANTS = ("swap_uv", "jy_raw", "no_flip", "dir_pinhole")


def draws_f32(sobol, looper, pixel_index, count=4):
    """The first draws of every pixel's Sampler (bsdf.h) as float32: float(table[looper * 200 + k] ^ h_k) * 0x1p-32f."""
    h = utilhash(np.asarray(pixel_index, np.uint64))
    row = sobol[looper].astype(np.uint64)
    out = np.zeros((len(h), count), F)
    for k in range(count):
        out[:, k] = (row[k] ^ h).astype(np.uint32).astype(F) * F(2.0 ** -32)
        h = utilhash(h)
    return out


def mask_weights(texels):
    """luminance of every texel in texel order, float32, operation for operation (bsdf.h luminance)."""
    t = np.ascontiguousarray(texels, F).reshape(-1, 3)
    return (F(0.2126) * t[:, 0] + F(0.7152) * t[:, 1]) + F(0.0722) * t[:, 2]


def mask_table(texels):
    """The host's alias construction over the mask's weights (hostlib.build_alias_table): (table, sum)."""
    from radish_pt_amd import hostlib

    return hostlib.build_alias_table(mask_weights(texels))


def _to_int(f):  # the device's float -> int conversion of a non-negative finite value: towards zero
    return np.trunc(f.astype(np.float64)).astype(np.int64)


def aperture_f32(mode, rz, rw, mask=None, plant=None):
    """pAperture of lensAperture (bsdf.h) for float32 draws rz, rw.  mask: (table, width, height) for MASK.  Returns (ax, ay) and,
    for MASK, the chosen texel and the two in-texel coordinates (k, jx, jy), else None."""
    rz, rw = np.asarray(rz, F), np.asarray(rw, F)
    with np.errstate(all="ignore"):
        if mode == OFF:
            return np.zeros_like(rz), np.zeros_like(rz), None
        if mode == DISK:  # concentricSampleDisk: r = sqrt(x), theta = 2 pi y, (r cos, r sin)
            r = np.sqrt(rz)
            theta = TWO_PI_F * rw
            sc = pyoracle.batch("sincos", theta.view(np.uint32).reshape(-1, 1)).view(F)
            return r * sc[:, 1], r * sc[:, 0], None
        table, w, h = mask
        n = w * h
        prob, fail = table["prob"].astype(F), table["failId"].astype(np.int64)
        fn = F(n) * rz
        k0 = np.minimum(_to_int(fn), n - 1)
        p = prob[k0]
        take = rw < p
        k = np.where(take, k0, fail[k0])
        jx = fn - k0.astype(F)
        jy = np.where(take, rw / p, (rw - p) / (F(1) - p)).astype(F)
        if plant == "jy_raw":
            jy = rw.copy()
        jx = np.where(jx < F(0), F(0), jx)
        jx = np.where(jx > ONE_BELOW, ONE_BELOW, jx)
        jy = np.where(jy < F(0), F(0), jy)
        jy = np.where(jy > ONE_BELOW, ONE_BELOW, jy)
        row = k // w
        col = k - row * w
        u = (col.astype(F) + jx) / F(w)
        v = (row.astype(F) + jy) / F(h)
        if plant == "swap_uv":
            u, v = v, u
        if plant == "no_flip":
            return F(2) * u - F(1), F(2) * v - F(1), (k, jx, jy)
        return F(1) - F(2) * u, F(1) - F(2) * v, (k, jx, jy)


def lens_rays_f32(cam, sobol, looper, mode=OFF, mask=None, plant=None):
    """cameraSample for every pixel in frame order: float32 [n, 6] = {origin, direction}."""
    c = M.device_camera(cam)
    lens_radius = F(np.asarray(cam)["lensRadius"])
    W, H = c["resx"], c["resy"]
    idx = np.arange(W * H)
    r = draws_f32(sobol, looper, idx)
    ax, ay, _ = aperture_f32(mode, r[:, 2], r[:, 3], mask, plant)
    with np.errstate(all="ignore"):
        x, y = (idx % W).astype(F), (idx // W).astype(F)
        aspect = F(W) / F(H)
        px, py = F(1) / F(W), F(1) / F(H)
        ru = (x * px) + px * r[:, 0]
        rv = (y * py) + py * r[:, 1]
        ru = F(1) - ru * F(2)
        rv = F(1) - rv * F(2)
        lx, ly = ax * lens_radius, ay * lens_radius  # pLens = (pAperture * lensRadius, 0)
        fx = (ru * aspect) * c["tanFovY"]
        fy = (rv * F(1)) * c["tanFovY"]
        pf = [fx * c["focalDist"], fy * c["focalDist"], np.full_like(fx, F(1) * c["focalDist"])]
        if plant == "dir_pinhole":
            d = [pf[0] - F(0), pf[1] - F(0), pf[2] - F(0)]
        else:
            d = [pf[0] - lx, pf[1] - ly, pf[2] - F(0)]  # pFocus - pLens
        d = M._normalize(M._mul((c["right"], c["up"], c["view"]), d))
        o = [(c["position"][k] + c["right"][k] * lx) + c["up"][k] * ly for k in range(3)]
    return np.stack(o + d, axis=1).astype(F)


def focus_points_f64(cam, sobol, looper):
    """position + M * pFocus of every pixel in float64, from the float32 draws: the point every lens ray of the pixel passes."""
    cam = np.asarray(cam)
    W, H = (int(v) for v in cam["resolution"])
    idx = np.arange(W * H)
    r = draws_f32(sobol, looper, idx).astype(np.float64)
    tan_fov = float(M.device_camera(cam)["tanFovY"])
    ru = 1.0 - 2.0 * ((idx % W) + r[:, 0]) / W
    rv = 1.0 - 2.0 * ((idx // W) + r[:, 1]) / H
    fd = float(cam["focalDist"])
    right, up, view = (cam[k].astype(np.float64) for k in ("right", "up", "view"))
    return cam["position"].astype(np.float64) + (ru * (W / H) * tan_fov * fd)[:, None] * right + (rv * tan_fov * fd)[:, None] * up + fd * view


def aperture_f64(mode, rz, rw, mask=None):
    """The aperture point in float64.  MASK reads the SAME table (its float32 probabilities are the distribution's definition)."""
    rz, rw = np.asarray(rz, np.float64), np.asarray(rw, np.float64)
    if mode == OFF:
        return np.zeros_like(rz), np.zeros_like(rz)
    if mode == DISK:
        rad, th = np.sqrt(rz), 2.0 * np.pi * rw
        return rad * np.cos(th), rad * np.sin(th)
    table, w, h = mask
    n = w * h
    prob, fail = table["prob"].astype(np.float64), table["failId"].astype(np.int64)
    k0 = np.minimum((n * rz).astype(np.int64), n - 1)
    take = rw < prob[k0]
    k = np.where(take, k0, fail[k0])
    jx = np.clip(n * rz - k0, 0.0, 1.0)
    with np.errstate(all="ignore"):
        jy = np.clip(np.where(take, rw / prob[k0], (rw - prob[k0]) / (1.0 - prob[k0])), 0.0, 1.0)
    u = (k % w + jx) / w
    v = (k // w + jy) / h
    return 1.0 - 2.0 * u, 1.0 - 2.0 * v


def lens_rays_f64(cam, W, H, jitter, zw, mode=OFF, mask=None, plant=None):
    """The thin lens in float64, in the form of test_oracle_float64._camera_rays_f64 (which it equals with mode OFF): (origins,
    directions) for the pixel jitters `jitter` and the lens draws `zw` (both [n, 2])."""
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.reshape(-1).astype(np.float64), y.reshape(-1).astype(np.float64)
    tan_fov = np.tan(np.radians(float(cam["fov"][1])))
    fd, radius = float(cam["focalDist"]), float(cam["lensRadius"])
    ru = 1.0 - 2.0 * (x + jitter[:, 0]) / W
    rv = 1.0 - 2.0 * (y + jitter[:, 1]) / H
    ax, ay = aperture_f64(mode, zw[:, 0], zw[:, 1], mask)
    right, up, view = (cam[k].astype(np.float64) for k in ("right", "up", "view"))
    lens = (ax * radius)[:, None] * right + (ay * radius)[:, None] * up                      # the point on the lens, camera at 0
    focus = (ru * (W / H) * tan_fov * fd)[:, None] * right + (rv * tan_fov * fd)[:, None] * up + fd * view
    d = focus if plant == "dir_pinhole" else focus - lens
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return cam["position"].astype(np.float64) + lens, d


@contextlib.contextmanager
def with_lens(path_model, sobol, looper, mode, mask=None, plant=None):
    """While active, tests/path_model.py's evaluations (single_kernel_pt, pt_direct) of Sobol row `looper` start from
    lens_rays_f64 instead of the pinhole's rays: the module's camera function is replaced, the module's text is not."""
    pinhole = path_model._camera_rays_f64

    def rays(cam, W, H, jitter):
        zw = sobol_draws(sobol, looper, np.arange(W * H), 4)[:, 2:4]
        return lens_rays_f64(cam, W, H, jitter, zw, mode, mask, plant)

    path_model._camera_rays_f64 = rays
    try:
        yield
    finally:
        path_model._camera_rays_f64 = pinhole
