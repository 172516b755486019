"""The denoiser kernels (kernels_denoise.h) at every sigma variant, level and image shape: every launch bit-exact against the
oracle, colour and variance, and within the float64 model's bound (denoise_model.py, test_denoise_float64.py) on finite
cases.  Synthetic G-buffers (denoise_model.synthetic) are copied into an api.GBuffer plane by plane.

All 8 k_eaw_filter<P2L, P2N, P2D> and both k_svgf_filter<P2D> instantiations run; levels 0-16 on small and odd shapes
(classes outside the image are not launched), 0-8 on 301 x 271 (2-3 tiles per residue class at levels 3-4), 0-4 at 1080p."""
import itertools

import numpy as np
import pytest

import denoise_model as M
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (9, 1), (2, 3), (5, 5), (16, 16), (17, 17), (31, 9), (33, 8), (70, 45)]
EAW_SIGMAS = list(itertools.product((64.0, 60.0), (0.25, 0.2), (1.0, 0.7)))  # sigmaIsPow2 patterns 7 .. 0
EDGE = (2.0 ** -125, 2.0 ** 125, 2.0 ** -126, 2.0 ** 126)  # accepted, accepted, refused, refused
NONFINITE_EDGE = (-4.0, 0.0)  # the centre tap's 0/0 is NaN: bit-exact only
EAW_EDGE = [tuple(e if k == pos else r for k, r in enumerate((64.0, 0.2, 1.0))) for pos in range(3) for e in EDGE + NONFINITE_EDGE]
SVGF_SIGMAS = [(4.0, 128.0, sd) for sd in (1.0, 0.9999, 4096.0)]  # 0.9999 + 1e-4f and 4096 + 1e-4f are powers of two


def _torch():
    import torch

    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(n, k=None):
    torch = _torch()
    return torch.full((n, k) if k else (n,), float("nan"), device="cuda")


class Case:
    """One synthetic frame on the device and on the host."""

    def __init__(self, W, H, seed=1, s=None):
        from radish_pt_amd import api

        self.W, self.H, self.n = W, H, W * H
        self.s = M.synthetic(W, H, seed) if s is None else s
        self.cam = M.camera(W, H)
        self.gb_ref = M.host_gbuffer(self.s, W, H)
        self.gb = api.GBuffer()
        self.gb.create(W, H)
        g, s = self.gb, self.s
        g.albedo.copy_(_dev(s["albedo"]))
        g.normal[0].copy_(_dev(s["normal"]))
        g.normal[1].copy_(_dev(s["lastNormal"]))
        g.depth[0].copy_(_dev(s["depth"]))
        g.primId[0].copy_(_dev(s["primId"]))
        g.primId[1].copy_(_dev(s["lastPrimId"]))
        g.motion.copy_(_dev(s["motion"]))
        self.gc = g.c_struct(self.cam)
        self.d = {k: _dev(v) for k, v in s.items()}

    def band(self, a, rows):
        return a if rows is None else a[rows[0] * self.W:rows[1] * self.W]


def _model_rows(W, H):
    """The model is evaluated on every row of small images and on a band across the middle (region boundaries, and the
    tile seams of levels 3-4 at 301 x 271) of larger ones."""
    return None if W * H <= 4096 else (H // 2 - 10, H // 2 + 10)


def assert_bit_equal_nan_class(a, b, what):
    """Bit-equal where the oracle is not NaN, NaN where it is.  When two NaNs meet in one float32 operation (a NaN colour
    times a NaN weight in SVGF), which of them the result carries is fixed neither by IEEE 754 nor by either compiler (both
    may swap the operands of a commutative operation), so the sign of such a NaN is not part of the contract."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"{what}: NaN at {np.argwhere(na != nb)[:5].tolist()} in one of the two only"
    assert_bit_equal(np.where(na, np.float32(0), a), np.where(nb, np.float32(0), b), what)


def _same(nan_class):
    return assert_bit_equal_nan_class if nan_class else assert_bit_equal


def run_eaw(ctx, c, sig, level, model=True, nan_class=False):
    from oracle import pyoracle

    out = _nan(c.n, 3)
    ctx.denoise_eaw(out, c.d["color"], c.gc, c.cam, *sig, level)
    ctx.synchronize()
    got = out.cpu().numpy()
    ref = pyoracle.denoise_eaw(c.s["color"], c.gb_ref, c.cam, *sig, level)
    _same(nan_class)(got, ref, f"EAW {c.W}x{c.H} level {level} sigma {sig}")
    if model:
        rows = _model_rows(c.W, c.H)
        want, bound = M.eaw(c.s["color"], c.s, c.cam, *sig, level, rows)
        assert M.violations(c.band(got, rows), want, bound) == 0, f"EAW {c.W}x{c.H} level {level} sigma {sig} vs float64"


def run_svgf(ctx, c, sig, level, model=True, nan_class=False):
    from oracle import pyoracle

    col, var = _nan(c.n, 3), _nan(c.n)
    ctx.denoise_svgf(col, c.d["color"], var, c.d["variance"], c.d["var_filtered"], c.gc, c.cam, *sig, level)
    ctx.synchronize()
    got_c, got_v = col.cpu().numpy(), var.cpu().numpy()
    ref_c, ref_v = pyoracle.denoise_svgf(c.s["color"], c.s["variance"], c.s["var_filtered"], c.gb_ref, c.cam, *sig, level)
    what = f"SVGF {c.W}x{c.H} level {level} sigma {sig}"
    _same(nan_class)(got_c, ref_c, what + " colour")
    _same(nan_class)(got_v, ref_v, what + " variance")
    if model:
        rows = _model_rows(c.W, c.H)
        out, bound, vout, vbound, skip = M.svgf(c.s["color"], c.s["variance"], c.s["var_filtered"], c.s, c.cam, *sig, level, rows)
        assert M.violations(c.band(got_c, rows), out, bound, skip) == 0, what + " colour vs float64"
        assert M.violations(c.band(got_v, rows), vout, vbound, skip) == 0, what + " variance vs float64"


def run_per_pixel(ctx, c):
    """temporalAccumulate (first and not), estimateVariance, filterVariance, modulate, add: bit-exact and within bound."""
    from oracle import pyoracle

    s, n, W, H = c.s, c.n, c.W, c.H
    for first in (True, False):
        co, mo = _nan(n, 3), _nan(n, 3)
        ctx.denoise_temporal_accumulate(co, c.d["color_accum"], mo, c.d["moment_accum"], c.d["color"], c.gc, first)
        ctx.synchronize()
        rc, rm = pyoracle.denoise_temporal_accumulate(s["color_accum"], s["moment_accum"], s["color"], c.gb_ref, first)
        assert_bit_equal(co.cpu().numpy(), rc, f"temporal colour {W}x{H} first={first}")
        assert_bit_equal(mo.cpu().numpy(), rm, f"temporal moment {W}x{H} first={first}")
        mc, mm, skip = M.temporal_accumulate(s["color_accum"], s["moment_accum"], s["color"], s, first)
        assert M.violations(co.cpu().numpy(), mc.v, mc.e, skip) == 0 and M.violations(mo.cpu().numpy(), mm.v, mm.e, skip) == 0
    var, fvar = _nan(n), _nan(n)
    ctx.denoise_estimate_variance(var, c.d["moment"], W, H)
    ctx.denoise_filter_variance(fvar, c.d["variance"], W, H)
    ctx.synchronize()
    assert_bit_equal(var.cpu().numpy(), pyoracle.denoise_estimate_variance(s["moment"], W, H), f"estimateVariance {W}x{H}")
    assert_bit_equal(fvar.cpu().numpy(), pyoracle.denoise_filter_variance(s["variance"], W, H), f"filterVariance {W}x{H}")
    ev, fv = M.estimate_variance(s["moment"], W, H), M.filter_variance(s["variance"], W, H)
    assert M.violations(var.cpu().numpy(), ev.v, ev.e) == 0 and M.violations(fvar.cpu().numpy(), fv.v, fv.e) == 0
    img = _dev(s["color"])
    ctx.denoise_modulate(img, c.gc)
    ctx.synchronize()
    mod = pyoracle.denoise_modulate(s["color"], c.gb_ref)
    assert_bit_equal(img.cpu().numpy(), mod, f"modulate {W}x{H}")
    out = _nan(n, 3)
    ctx.denoise_add(out, img, c.d["color_accum"], W, H)
    ctx.denoise_add(img, img, c.d["color"], W, H)  # out aliasing in1 (the two-image overload)
    ctx.synchronize()
    assert_bit_equal(out.cpu().numpy(), pyoracle.denoise_add(mod, s["color_accum"], W, H), f"add {W}x{H}")
    assert_bit_equal(img.cpu().numpy(), pyoracle.denoise_add(mod, s["color"], W, H), f"add in place {W}x{H}")


@pytest.mark.parametrize("W,H", SHAPES)
def test_filters_every_sigma_variant_and_level(gpu_ctx, W, H):
    c = Case(W, H)
    for level in range(17):
        for sig in EAW_SIGMAS + EAW_EDGE:
            run_eaw(gpu_ctx, c, sig, level, model=not any(v in NONFINITE_EDGE for v in sig))
        for sig in SVGF_SIGMAS:
            run_svgf(gpu_ctx, c, sig, level)


def test_filters_multi_tile_residue_classes(gpu_ctx):
    c = Case(301, 271)
    for level in range(9):
        for sig in EAW_SIGMAS:
            run_eaw(gpu_ctx, c, sig, level)
        for sig in SVGF_SIGMAS:
            run_svgf(gpu_ctx, c, sig, level)


def test_filters_1080p_reference_sigmas(gpu_ctx):
    c = Case(1920, 1080)
    for level in range(5):
        run_eaw(gpu_ctx, c, (64.0, 0.2, 1.0), level)
        run_svgf(gpu_ctx, c, (4.0, 128.0, 1.0), level)


@pytest.mark.parametrize("W,H", [(33, 8), (70, 45)])
def test_filters_non_finite_inputs(gpu_ctx, W, H):
    """±inf and NaN colours and NaN variances: the packed exp_det2 computes through them and selects afterwards.  Every
    finite output is bit-equal to the oracle and every NaN is where the oracle has one (assert_bit_equal_nan_class)."""
    s = M.synthetic(W, H, 5)
    rng = np.random.default_rng(W)
    k = max(3, W * H // 40)
    for val in (np.inf, -np.inf, np.nan):
        s["color"][rng.integers(0, W * H, k), rng.integers(0, 3, k)] = val
    s["variance"][rng.integers(0, W * H, k)] = np.nan
    s["var_filtered"][rng.integers(0, W * H, k)] = np.nan
    c = Case(W, H, s=s)
    for level in list(range(6)) + [16]:
        for sig in EAW_SIGMAS:
            run_eaw(gpu_ctx, c, sig, level, model=False, nan_class=True)
        for sig in SVGF_SIGMAS:
            run_svgf(gpu_ctx, c, sig, level, model=False, nan_class=True)


@pytest.mark.parametrize("W,H", SHAPES + [(301, 271), (1920, 1080)])
def test_per_pixel_kernels(gpu_ctx, W, H):
    run_per_pixel(gpu_ctx, Case(W, H))


@pytest.mark.parametrize("W,H", [(1, 1), (2, 3), (17, 1)])
def test_filter_classes_three_frames(gpu_ctx, W, H):
    """LeveledEAWFilter and SpatioTemporalFilter over three frames, every intermediate buffer bit-equal to the oracle."""
    from oracle import pyoracle
    from radish_pt_amd import api

    torch = _torch()
    n = W * H
    cam = M.camera(W, H)
    gb, gb_ref = api.GBuffer(), pyoracle.GBufferHost(W, H)
    gb.create(W, H)
    dev = api.DevScene()
    dev.ctx = gpu_ctx
    scene = api.Scene.__new__(api.Scene)
    scene.devScene, scene.camera, scene.data = dev, cam, None
    api.State.scene = scene
    try:
        eaw, stf = api.LeveledEAWFilter(), api.SpatioTemporalFilter()
        eaw.create(W, H, 5)
        stf.create(W, H, 5)
        accC = [np.zeros((n, 3), np.float32) for _ in range(2)]
        accM = [np.zeros((n, 3), np.float32) for _ in range(2)]
        first, fidx = True, 0
        for f in range(3):
            s = M.synthetic(W, H, 10 + f)
            cur = gb.frameIdx
            gb_ref.frameIdx = cur
            for host, plane in ((gb_ref.normal[cur], "normal"), (gb_ref.depth[cur], "depth"), (gb_ref.primId[cur], "primId"),
                                (gb_ref.motion, "motion"), (gb_ref.albedo, "albedo")):
                host[:] = s[plane]
            gb.normal[cur].copy_(_dev(s["normal"]))
            gb.depth[cur].copy_(_dev(s["depth"]))
            gb.primId[cur].copy_(_dev(s["primId"]))
            gb.motion.copy_(_dev(s["motion"]))
            gb.albedo.copy_(_dev(s["albedo"]))
            noisy = s["color"]
            ref = pyoracle.denoise_eaw(noisy, gb_ref, cam, 64.0, 0.2, 1.0, 0)
            for lv in (1, 2, 3, 4):
                ref = pyoracle.denoise_eaw(ref, gb_ref, cam, 64.0, 0.2, 1.0, lv)
            out = eaw.filter(torch.zeros(n, 3, device="cuda"), _dev(noisy), gb, cam)
            gpu_ctx.synchronize()
            assert_bit_equal(out.cpu().numpy(), ref, f"LeveledEAWFilter {W}x{H} frame {f}")
            accC[fidx], accM[fidx] = pyoracle.denoise_temporal_accumulate(accC[fidx ^ 1], accM[fidx ^ 1], noisy, gb_ref, first)
            first = False
            var = pyoracle.denoise_estimate_variance(accM[fidx], W, H)
            fvar = pyoracle.denoise_filter_variance(var, W, H)
            colorOut, tmpVar = pyoracle.denoise_svgf(accC[fidx], var, fvar, gb_ref, cam, 4.0, 128.0, 1.0, 0)
            colorOut, accC[fidx] = accC[fidx], colorOut
            var = tmpVar
            fvar = pyoracle.denoise_filter_variance(var, W, H)
            colorOut, var = pyoracle.denoise_svgf(accC[fidx], var, fvar, gb_ref, cam, 4.0, 128.0, 1.0, 1)
            for lv in (2, 3, 4):
                fvar = pyoracle.denoise_filter_variance(var, W, H)
                colorOut, var = pyoracle.denoise_svgf(colorOut, var, fvar, gb_ref, cam, 4.0, 128.0, 1.0, lv)
            got = stf.filter(torch.zeros(n, 3, device="cuda"), _dev(noisy), gb, cam)
            gpu_ctx.synchronize()
            assert_bit_equal(got.cpu().numpy(), colorOut, f"SpatioTemporalFilter {W}x{H} frame {f}")
            assert_bit_equal(stf.variance.cpu().numpy(), var, f"SVGF variance {W}x{H} frame {f}")
            assert_bit_equal(stf.accumColor[stf.frameIdx].cpu().numpy(), accC[fidx], f"accumColor {W}x{H} frame {f}")
            assert_bit_equal(stf.accumMoment[stf.frameIdx].cpu().numpy(), accM[fidx], f"accumMoment {W}x{H} frame {f}")
            stf.nextFrame()
            fidx ^= 1
            gb.update(cam)
            gb_ref.update(cam)
    finally:
        api.State.scene = None


def test_level_outside_abi_is_rejected_and_context_still_filters(gpu_ctx):
    from radish_pt_amd import api

    c = Case(17, 17)
    col, var = _nan(c.n, 3), _nan(c.n)
    for level in (-1, 17):
        with pytest.raises(api.RadishError, match="bad arguments"):
            gpu_ctx.denoise_eaw(col, c.d["color"], c.gc, c.cam, 64.0, 0.2, 1.0, level)
        with pytest.raises(api.RadishError, match="bad arguments"):
            gpu_ctx.denoise_svgf(col, c.d["color"], var, c.d["variance"], c.d["var_filtered"], c.gc, c.cam, 4.0, 128.0, 1.0, level)
    run_eaw(gpu_ctx, c, (64.0, 0.2, 1.0), 16)
    run_svgf(gpu_ctx, c, (4.0, 128.0, 1.0), 2)
