"""float64 restatement of the five denoiser operations (src/denoiser.cu: waveletFilter EAW and SVGF, temporalAccumulate,
estimateVariance, filterVariance), shared by test_denoise_float64.py and test_gpu_denoise.py.

Every quantity is carried as an `R`: its float64 value, computed with np.exp / np.power / np.sqrt from the float32 inputs,
and a first-order bound on how far the float32 computation of the same expression can be from it (running error analysis:
each float32 operation adds u |result| with u = 2^-24, the operands carry their own bounds, decimal literals such as .0983f
carry their float32 representation error).  exp and pow add the recipe errors DESIGN states (`exp_det` 2.4e-7, `pow_det`
8e-6 relative) and exp_det's flush to 0 below -87.3.  Positions are reconstructed in float64 from the 196-byte camera record
(tan(radians(fov.y)), focalDist, right / up / view, position).  Nothing here calls the oracle or the device recipes.

The filters vectorise over the 25 shifted taps with validity masks; `rows=(y0, y1)` restricts the output to a band of rows.
Keyword switches plant deliberate mistakes (`test_denoise_float64.py` checks that each one is caught)."""
import math

import numpy as np

U = 2.0 ** -24         # float32 unit roundoff
ETA = 2.0 ** -150      # half the smallest float32 subnormal: the absolute error of an underflowing product or quotient
FLT_EPSILON = 2.0 ** -23
EXP_REL, POW_REL = 2.4e-7, 8e-6  # exp_det / pow_det relative to the exact function of their float32 argument
EXP_FLUSH = -87.3      # exp_det returns 0 below this argument

G5 = np.array([[.0030, .0133, .0219, .0133, .0030],
               [.0133, .0596, .0983, .0596, .0133],
               [.0219, .0983, .1621, .0983, .0219],
               [.0133, .0596, .0983, .0596, .0133],
               [.0030, .0133, .0219, .0133, .0030]])
G3 = np.array([[.075, .124, .075], [.124, .204, .124], [.075, .124, .075]])
LUM = (0.2126, 0.7152, 0.0722)


def gamma(n):
    """Bound on the relative error of an n-term float32 sum of products (Higham's gamma_n)."""
    return n * U / (1.0 - n * U)


class R:
    """A float64 value and a bound on the error of its float32 evaluation."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.asarray(e, np.float64)

    @staticmethod
    def lit(c):  # a decimal literal written as a float32 constant
        return R(c, abs(float(np.float32(c)) - c))

    def __add__(a, b):
        b = _r(b)
        v = a.v + b.v
        return R(v, a.e + b.e + U * np.abs(v))

    def __radd__(a, b):
        return a + b

    def __sub__(a, b):
        b = _r(b)
        v = a.v - b.v
        return R(v, a.e + b.e + U * np.abs(v))

    def __rsub__(a, b):
        return _r(b) - a

    def __neg__(a):
        return R(-a.v, a.e)

    def __mul__(a, b):
        b = _r(b)
        v = a.v * b.v
        return R(v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e + U * np.abs(v) + ETA)

    def __rmul__(a, b):
        return a * b

    def __truediv__(a, b):
        b = _r(b)
        v = a.v / b.v
        lo = np.maximum(np.abs(b.v) - b.e, np.abs(b.v) * 0.5)
        return R(v, (a.e + np.abs(v) * b.e) / lo + U * np.abs(v) + ETA)

    def sqrt(a):
        v = np.sqrt(a.v)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(v > 0, a.e / (2 * np.where(v > 0, v, 1)), np.sqrt(a.e))
        return R(v, e + U * v)

    def abs(a):
        return R(np.abs(a.v), a.e)

    def clamp0(a):  # gmax(x, 0): 1-Lipschitz
        return R(np.maximum(a.v, 0.0), a.e)

    def __getitem__(a, k):
        return R(a.v[k], np.broadcast_to(a.e, a.v.shape)[k])


def _r(x):
    return x if isinstance(x, R) else R(x)


def dot3(a, b):  # rmath.h dot(v3, v3) = (ax bx + ay by) + az bz
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def luminance(c):
    return (R.lit(LUM[0]) * c[0] + R.lit(LUM[1]) * c[1]) + R.lit(LUM[2]) * c[2]


def exp_w(a, clamp1=False):
    """exp(a) of an argument a <= 0 with error bound a.e: the argument's error (the float32 argument lies in
    [a - a.e, min(a + a.e, 0)]), exp_det's recipe error and its flush to 0."""
    v = np.exp(a.v)
    hi = np.exp(np.minimum(a.v + a.e, 0.0))
    e = np.maximum(hi - v, v - np.exp(a.v - a.e)) + EXP_REL * v + np.where(a.v - a.e < EXP_FLUSH, hi, 0.0)
    return R(np.minimum(v, 1.0) if clamp1 else v, e)


def pow_w(x, y):
    """x^y for x >= 0, y > 0, with the error of x and pow_det's recipe error."""
    v = np.power(x.v, y)
    hi = np.power(x.v + x.e, y) - v
    lo = v - np.power(np.maximum(x.v - x.e, 0.0), y)
    return R(v, np.maximum(hi, lo) + POW_REL * v)


def tan_fov(cam):
    """glm::tan(glm::radians(fov.y)) with the float32 rounding of the radians (constant and product) and 1 ulp of tanf."""
    th = math.radians(float(cam["fov"][1]))
    t = math.tan(th)
    return R(t, (1.0 + t * t) * 2 * U * th + 2 * U * t)


def positions(cam, depth):
    """Camera::getPosition(x, y, depth) of every pixel (sceneStructs.h:50-70 with a pinhole lens): R of 3 x [n]."""
    W, H = int(cam["resolution"][0]), int(cam["resolution"][1])
    n = W * H
    pix = np.arange(n)
    x, y = (pix % W).astype(np.float64), (pix // W).astype(np.float64)
    aspect = R(float(W)) / R(float(H))
    psx, psy = R(1.0) / R(float(W)), R(1.0) / R(float(H))
    ruvx = R(1.0) - (R(x) * psx + psx * R(0.5)) * R(2.0)
    ruvy = R(1.0) - (R(y) * psy + psy * R(0.5)) * R(2.0)
    t = tan_fov(cam)
    fx, fy = (ruvx * aspect) * t, (ruvy * R(1.0)) * t
    fd = R(float(cam["focalDist"]))
    pf = (fx * fd, fy * fd, R(1.0) * fd)
    right, up, view = ([R(float(c)) for c in cam[k]] for k in ("right", "up", "view"))
    d = [(right[k] * pf[0] + up[k] * pf[1]) + view[k] * pf[2] for k in range(3)]
    inv = R(1.0) / dot3(d, d).sqrt()
    dist = R(np.asarray(depth, np.float64))
    return [R(float(cam["position"][k])) + (d[k] * inv) * dist for k in range(3)]


def _taps(W, H, pix, level, step_x_plus1=False):
    """Tap k = 5 (i + 2) + (j + 2) of every output pixel: clipped source index [25, m], validity [25, m], Gaussian (i, j)."""
    step = 1 << level
    sx = step + 1 if step_x_plus1 else step
    x, y = pix % W, pix // W
    idx, ok, ij = [], [], []
    for i in range(-2, 3):
        for j in range(-2, 3):
            qx, qy = x + j * sx, y + i * step
            valid = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            idx.append(np.where(valid, np.clip(qx, 0, W - 1) + np.clip(qy, 0, H - 1) * W, 0))
            ok.append(valid)
            ij.append((i + 2, j + 2))
    return np.array(idx), np.array(ok), ij


def _gauss(ij, gauss_1pct):
    g = G5.copy()
    if gauss_1pct:
        g[1, 2] *= 1.01
    vals = np.array([g[a, b] for a, b in ij])[:, None]
    return R(vals, np.abs(vals.astype(np.float32).astype(np.float64) - vals))


def _pos_diff(pos, pix, idx):
    """posP - posQ of every tap: R of 3 x [25, m]; exactly 0 for the centre tap (the same float32 value twice)."""
    same = idx == pix[None]
    d = [p[pix][None] - p[idx] for p in pos]
    return [R(dk.v, np.where(same, 0.0, dk.e)) for dk in d]


def _pixels(W, H, rows):
    y0, y1 = (0, H) if rows is None else rows
    return np.arange(y0 * W, y1 * W)


def _weighted_mean(w, ok, vals, n_terms=25):
    """sum_q w_q c_q / sum_q w_q over valid taps, and its bound: sum_q dw_q |c_q - out| / sum w (the weights' errors) plus
    gamma_25 (sum_q w_q |c_q| + |out| sum_q w_q) / sum w (the float32 accumulation) plus the final division's rounding.
    w: R [25, m]; vals: float64 [25, m, k].  Returns out [m, k], bound [m, k], sum w, bound of sum w."""
    wv = np.where(ok, w.v, 0.0)
    we = np.where(ok, np.broadcast_to(w.e, wv.shape), 0.0)
    sw = wv.sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (wv[..., None] * vals).sum(0) / sw[:, None]
        g = gamma(n_terms)
        num = (we[..., None] * np.abs(vals - out[None])).sum(0) + g * ((wv[..., None] * np.abs(vals)).sum(0) + np.abs(out) * sw[:, None])
        sw_err = we.sum(0) + g * sw
        bound = num / (sw - sw_err)[:, None] + U * np.abs(out)
    return out, bound, sw, sw_err


def eaw(color, gb, cam, sig_l, sig_n, sig_d, level, rows=None, *, gauss_1pct=False, step_x_plus1=False, no_id_test=False,
        swap_nd=False):
    """waveletFilter, EAW form (denoiser.cu:17-84).  gb: dict with 'normal', 'depth', 'primId' of the current frame.
    Returns (out [m, 3], bound [m, 3]) for the pixels of `rows`."""
    W, H = int(cam["resolution"][0]), int(cam["resolution"][1])
    if swap_nd:
        sig_n, sig_d = sig_d, sig_n
    pix = _pixels(W, H, rows)
    col = np.asarray(color, np.float64).reshape(-1, 3)
    nrm = np.asarray(gb["normal"], np.float64).reshape(-1, 3)
    pid = np.asarray(gb["primId"]).reshape(-1)
    pos = positions(cam, gb["depth"])
    idx, ok, ij = _taps(W, H, pix, level, step_x_plus1)
    if not no_id_test:
        ok = ok & (pid[idx] == pid[pix][None])

    def weight(vp, vq, sig):
        d = [R(vp[k]) - R(vq[k]) for k in range(3)]
        return exp_w(-(dot3(d, d) / R(float(sig))), clamp1=True)

    wc = weight([col[pix, k][None] for k in range(3)], [col[idx, k] for k in range(3)], sig_l)
    wn = weight([nrm[pix, k][None] for k in range(3)], [nrm[idx, k] for k in range(3)], sig_n)
    d = _pos_diff(pos, pix, idx)
    wp = exp_w(-(dot3(d, d) / R(float(sig_d))), clamp1=True)
    w = ((wc * wn) * wp) * _gauss(ij, gauss_1pct)
    out, bound, _, _ = _weighted_mean(w, ok, col[idx])
    bg = pid[pix] <= -1
    out[bg], bound[bg] = col[pix][bg], 0.0
    return out, bound


def svgf(color, variance, var_filtered, gb, cam, sig_l, sig_n, sig_d, level, rows=None, *, gauss_1pct=False,
         step_x_plus1=False, swap_nd=False, no_normal_eps=False, no_sqrt=False):
    """waveletFilter, SVGF form (denoiser.cu:92-173).  Returns (colour [m, 3], colour bound, variance [m], variance bound,
    skip [m]): `skip` marks pixels whose weightSum or weight2Sum lies within its error bound of FLT_EPSILON."""
    W, H = int(cam["resolution"][0]), int(cam["resolution"][1])
    if swap_nd:
        sig_n, sig_d = sig_d, sig_n
    pix = _pixels(W, H, rows)
    col = np.asarray(color, np.float64).reshape(-1, 3)
    var = np.asarray(variance, np.float64).reshape(-1)
    vf = np.asarray(var_filtered, np.float64).reshape(-1)
    nrm = np.asarray(gb["normal"], np.float64).reshape(-1, 3)
    pid = np.asarray(gb["primId"]).reshape(-1)
    pos = positions(cam, gb["depth"])
    idx, ok, ij = _taps(W, H, pix, level, step_x_plus1)
    eps4 = R.lit(1e-4)
    d = _pos_diff(pos, pix, idx)
    wp = exp_w(-(dot3(d, d) / (R(float(sig_d)) + eps4)))
    sat = dot3([R(nrm[pix, k][None]) for k in range(3)], [R(nrm[idx, k]) for k in range(3)]).clamp0()
    wn = pow_w(sat, float(sig_n))
    if not no_normal_eps:
        wn = wn + eps4
    spread = R(np.maximum(vf[pix], 0.0))
    denom = R(float(sig_l)) * (spread if no_sqrt else spread.sqrt()) + eps4
    lp = luminance([R(col[pix, k]) for k in range(3)])
    lq = luminance([R(col[idx, k]) for k in range(3)])
    wcol = exp_w(-((R(lp.v[None], lp.e[None]) - lq).abs() / R(denom.v[None], denom.e[None]))) + eps4
    w = ((wcol * wn) * wp) * _gauss(ij, gauss_1pct)
    w2 = w * w
    out, bound, sw, sw_err = _weighted_mean(w, ok, col[idx])
    vout, vbound, sw2, sw2_err = _weighted_mean(w2, ok, var[idx][..., None])
    vout, vbound = vout[:, 0], vbound[:, 0]
    lowc, lowv = sw < FLT_EPSILON, sw2 < FLT_EPSILON
    out[lowc], bound[lowc] = col[pix][lowc], 0.0
    vout[lowv], vbound[lowv] = var[pix][lowv], 0.0
    skip = (np.abs(sw - FLT_EPSILON) <= sw_err) | (np.abs(sw2 - FLT_EPSILON) <= sw2_err)
    bg = pid[pix] <= -1
    out[bg], bound[bg], vout[bg], vbound[bg], skip[bg] = col[pix][bg], 0.0, var[pix][bg], 0.0, False
    return out, bound, vout, vbound, skip


def temporal_accumulate(color_accum_in, moment_accum_in, color_in, gb, first, *, alpha=0.2):
    """temporalAccumulate (denoiser.cu:208-262).  gb: dict with 'normal', 'lastNormal', 'primId', 'lastPrimId', 'motion'.
    Returns (colour accum R [n, 3], moment accum R [n, 3], skip [n]): `skip` marks pixels whose |dot(normal, lastNormal)|
    lies within its error bound (plus |.1f - .1|) of .1."""
    color = np.asarray(color_in, np.float64).reshape(-1, 3)
    n = len(color)
    last_c = np.asarray(color_accum_in, np.float64).reshape(-1, 3)
    last_m = np.asarray(moment_accum_in, np.float64).reshape(-1, 3)
    pid, lpid = np.asarray(gb["primId"]).reshape(-1), np.asarray(gb["lastPrimId"]).reshape(-1)
    nrm = np.asarray(gb["normal"], np.float64).reshape(-1, 3)
    lnrm = np.asarray(gb["lastNormal"], np.float64).reshape(-1, 3)
    li = np.asarray(gb["motion"]).reshape(-1).astype(np.int64)
    assert li.min() >= -1 and li.max() < n, "motion out of range: the reference reads out of bounds"
    lc = np.maximum(li, 0)
    dt = dot3([R(nrm[:, k]) for k in range(3)], [R(lnrm[lc, k]) for k in range(3)]).abs()
    tested = (li >= 0) & (pid > -1) & (lpid[lc] == pid)
    diff = np.full(n, bool(first)) | ~tested | (dt.v < 0.1)
    skip = tested & ~np.full(n, bool(first)) & (np.abs(dt.v - 0.1) <= dt.e + abs(float(np.float32(0.1)) - 0.1))
    a = R.lit(alpha)
    keep = R(1.0) - a
    lum = luminance([R(color[:, k]) for k in range(3)])
    mixc = [R(last_c[lc, k]) * keep + R(color[:, k]) * a for k in range(3)]
    mixm = [R(last_m[lc, 0]) * keep + lum * a, R(last_m[lc, 1]) * keep + (lum * lum) * a, R(last_m[lc, 2]) + R(1.0)]
    sq = lum * lum
    cv = np.stack([np.where(diff, color[:, k], mixc[k].v) for k in range(3)], 1)
    ce = np.stack([np.where(diff, 0.0, mixc[k].e) for k in range(3)], 1)
    mv = np.stack([np.where(diff, lum.v, mixm[0].v), np.where(diff, sq.v, mixm[1].v), np.where(diff, 0.0, mixm[2].v)], 1)
    me = np.stack([np.where(diff, lum.e, mixm[0].e), np.where(diff, sq.e, mixm[1].e), np.where(diff, 0.0, mixm[2].e)], 1)
    return R(cv, ce), R(mv, me), skip


def estimate_variance(moment, width, height, *, threshold=3.5):
    """estimateVariance (denoiser.cu:264-299): the temporal variance where more than `threshold` frames were accumulated,
    else the spatial variance of the 3x3 neighbourhood's first two moments.  Returns R [n]."""
    m = np.asarray(moment, np.float64).reshape(height, width, 3)
    mp = np.pad(m, ((1, 1), (1, 1), (0, 0)))
    inside = np.pad(np.ones((height, width)), 1)
    sx, sy, cnt = R(np.zeros((height, width))), R(np.zeros((height, width))), np.zeros((height, width))
    for i in range(3):
        for j in range(3):
            mask = inside[i:i + height, j:j + width]
            sx = sx + R(mp[i:i + height, j:j + width, 0])
            sy = sy + R(mp[i:i + height, j:j + width, 1])
            cnt = cnt + mask
    sx, sy = sx / R(cnt), sy / R(cnt)
    spatial = sy - sx * sx
    temporal = R(m[..., 1]) - R(m[..., 0]) * R(m[..., 0])
    use_t = m[..., 2] > threshold
    return R(np.where(use_t, temporal.v, spatial.v).reshape(-1), np.where(use_t, temporal.e, spatial.e).reshape(-1))


def filter_variance(variance, width, height, *, border_div1=False):
    """filterVariance (denoiser.cu:301-328): the 3x3 Gaussian mean over the taps inside the image.  Returns R [n]."""
    v = np.pad(np.asarray(variance, np.float64).reshape(height, width), 1)
    inside = np.pad(np.ones((height, width)), 1)
    s, ws = R(np.zeros((height, width))), R(np.zeros((height, width)))
    for i in range(3):
        for j in range(3):
            g = R.lit(G3[i, j])
            mask = inside[j:j + height, i:i + width]
            s = s + R(v[j:j + height, i:i + width]) * g * R(mask)
            ws = ws + g * R(mask)
    if border_div1:
        ws = R(np.ones((height, width)))
    out = s / ws
    return R(out.v.reshape(-1), out.e.reshape(-1))


# ---- synthetic inputs ------------------------------------------------------------------------------------------------------
REGION_DEPTH = (2.0, 2.3, 2.6, 3.4, 2.05)
REGION_ID = (3, 7, 2 ** 30 + 5, -1, 11)  # -1: background
REGION_NORMAL = ((0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (0.0, -0.8, 0.6), (0.0, 0.0, 1.0), (-0.48, 0.6, 0.64))


def synthetic(W, H, seed):
    """A G-buffer and the denoisers' other inputs at W x H, built so that every planted mistake shows: planar regions at
    different depths with steps between them, per-region normals with small noise (some zero, some opposed), per-region ids
    (a -1 background, ids near 2^30, a second id inside each region), colours made of a gradient, noise and fireflies,
    variances with negative values, moments whose frame counts lie around 4, motion vectors in [-1, W H)."""
    rng = np.random.default_rng(seed)
    n = W * H
    x, y = np.arange(n) % W, np.arange(n) // W
    bx, by = max(1, -(-W // 3)), max(1, -(-H // 2))
    region = (x // bx + 3 * (y // by) + (x + 2 * y) // 7) % 5
    depth = np.array(REGION_DEPTH)[region] + 0.002 * x + 0.001 * y
    normal = np.array(REGION_NORMAL)[region] + rng.normal(0, 0.02, (n, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    r = rng.random(n)
    normal[r < 0.04] = 0.0
    normal[(r >= 0.04) & (r < 0.08)] *= -1.0
    pid = np.array(REGION_ID)[region]
    second = ((x * 5 + y * 3) % 11 == 0) & (pid > -1)
    pid = np.where(second, pid + 1000, pid)
    color = np.stack([x / max(W, 1), y / max(H, 1), 0.5 + 0.25 * np.sin(x + y)], 1) + rng.normal(0, 0.15, (n, 3))
    color = np.abs(color)
    color[rng.random(n) < 0.02] *= 40.0  # fireflies
    variance = rng.uniform(-0.05, 0.6, n)
    var_filtered = rng.uniform(-0.02, 0.4, n)
    var_filtered[rng.random(n) < 0.1] = 0.0
    lum = color @ np.array(LUM)
    moment = np.stack([lum, lum * lum + rng.uniform(0, 0.3, n), rng.choice([0.0, 1.0, 3.0, 4.0, 4.0, 5.0, 9.0], n)], 1)
    motion = np.clip(np.arange(n) + rng.integers(-2, 3, n), -1, n - 1)
    motion[rng.random(n) < 0.1] = -1
    last_pid = np.where(rng.random(n) < 0.1, pid + 1, pid)
    last_normal = np.where(rng.random((n, 1)) < 0.15, np.roll(normal, 1, axis=1), normal)
    last_normal[rng.random(n) < 0.05] = (0.995, 0.0995, 0.0)
    albedo = rng.uniform(-0.1, 1.0, (n, 3))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    i32 = lambda a: np.ascontiguousarray(a, np.int32)  # noqa: E731
    return {
        "color": f32(color), "variance": f32(variance), "var_filtered": f32(var_filtered), "moment": f32(moment),
        "color_accum": f32(color * 0.9 + 0.05), "moment_accum": f32(moment * np.array([1.0, 1.0, 1.0])),
        "normal": f32(normal), "lastNormal": f32(last_normal), "depth": f32(depth), "primId": i32(pid),
        "lastPrimId": i32(last_pid), "motion": i32(motion), "albedo": f32(albedo),
    }


def camera(W, H):
    from radish_pt_amd import hostlib

    return hostlib.make_camera(W, H, eye=(0.3, 1.9, 7.4), rotation=(-91.5, -11.0, 0.0), fovy=19.0)


def host_gbuffer(s, W, H):
    """pyoracle.GBufferHost holding `s` as its current frame (frameIdx 0) and `last*` as the previous one."""
    from oracle import pyoracle

    gb = pyoracle.GBufferHost(W, H)
    gb.albedo[:] = s["albedo"]
    gb.normal[0][:], gb.normal[1][:] = s["normal"], s["lastNormal"]
    gb.depth[0][:] = s["depth"]
    gb.primId[0][:], gb.primId[1][:] = s["primId"], s["lastPrimId"]
    gb.motion[:] = s["motion"]
    return gb


def violations(got, want, bound, skip=None):
    """Elements of `got` (float32, as computed) farther from the model's `want` than its bound; NaN counts as far.
    `skip` [m] excludes pixels next to a branch threshold."""
    got = np.asarray(got, np.float64).reshape(np.shape(want))
    bad = ~(np.abs(got - want) <= bound)
    if skip is not None:
        bad &= ~np.asarray(skip).reshape((-1,) + (1,) * (bad.ndim - 1))
    return int(bad.sum())
