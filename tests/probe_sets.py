"""What is compared and how, for every function the device probe (tests/probe/device_probe.hip) wraps: one Spec per probe
entry with its input set (tests/probe_inputs.py), the oracle's outputs for it (one batch call, cached) and the comparison rule.
Shared by tests/test_probe_inputs_cpu.py (oracle alone) and tests/test_gpu_device_functions.py (device against oracle).

The three comparison rules:
  1. A NaN equals a NaN of any sign and payload (x86's default NaN is negative, gfx950's positive).  Everything else is compared
     by bits, including the sign of a zero.
  2. Outputs that no caller reads are not compared: bary and dist of a rejected triangle, tMin of a missed box.  Flags always are.
  3. aabbFast, aabbFastPk and boxTest are compared with the device's own aabbIntersect on the same record (and through it with
     the oracle): identical flags, tMin equal as VALUES (-0 == +0) — the latitude the comment above aabbFast claims, no more.
No other function gets latitude.
"""
import functools
import math

import numpy as np

import float64_models as F64
import probe_inputs as P


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def f32(a):
    return np.ascontiguousarray(a).view(np.float32)


def _f64(a):
    with np.errstate(invalid="ignore"):  # signalling NaNs in the sets
        return np.asarray(a).astype(np.float64)


def _is_nan_bits(b):
    return (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def mismatches(got, ref, float_words=True):
    """Boolean array: where two uint32 arrays differ under rule 1 (`float_words`: the words are floats, so NaN == NaN)."""
    got, ref = u32(got), u32(ref)
    bad = got != ref
    if float_words:
        bad &= ~(_is_nan_bits(got) & _is_nan_bits(ref))
    return bad


def check_equal(got, ref, what, float_words=True, where=None, records=None):
    """Assert rule 1 on two arrays of 32-bit words (optionally only where `where`); the message names the first record."""
    bad = mismatches(got, ref, float_words)
    if where is not None:
        bad &= where
    if bad.any():
        idx = np.argwhere(bad)
        first = tuple(idx[0])
        rec = "" if records is None else f"; input record {f32(records)[first[0]]!r}"
        raise AssertionError(f"{what}: {len(idx)} of {bad.size} words differ; first at {first}: "
                             f"{u32(got)[first]:#010x} vs {u32(ref)[first]:#010x}{rec}")


class Spec:
    """One probe entry.  `inputs()` -> uint32 [n, words_in]; `oracle(inp)` -> the oracle's outputs; `device_buffer(inp)` -> the flat
    uint32 array the entry reads; `compare(dev, orc, inp)` asserts the rules on the device's uint32 [n, words_out]."""

    def __init__(self, name, words_in, words_out, inputs, oracle, compare, int_words=(), device_buffer=None):
        self.name, self.words_in, self.words_out = name, words_in, words_out
        self._inputs, self._oracle, self._compare = inputs, oracle, compare
        self.int_words = tuple(int_words)  # output words that are integers (compared by bits without the NaN rule)
        self._device_buffer = device_buffer

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        a = u32(self._inputs()).reshape(-1, self.words_in)
        a.setflags(write=False)
        return a

    @functools.lru_cache(maxsize=None)
    def oracle_outputs(self):
        out = self._oracle(self.inputs())
        return out

    def oracle(self, inp):
        return self._oracle(inp)

    def device_buffer(self, inp):
        return self._device_buffer(inp) if self._device_buffer else np.ascontiguousarray(inp).reshape(-1)

    def compare(self, dev, orc, inp):
        self._compare(self, dev, orc, inp)

    def entry(self):
        return "probe_" + self.name.split("[")[0]


def _compare_all_words(spec, dev, orc, inp):
    dev, orc = u32(dev), u32(orc)
    assert dev.shape == orc.shape
    is_int = np.zeros(dev.shape[1], bool)
    is_int[list(spec.int_words)] = True
    check_equal(dev[:, ~is_int], orc[:, ~is_int], spec.name, True, records=inp)
    if is_int.any():
        check_equal(dev[:, is_int], orc[:, is_int], spec.name + " (integer words)", False, records=inp)


def _batch(name):
    from oracle import pyoracle

    return lambda inp: pyoracle.batch(name, inp)


# ---- boxes ------------------------------------------------------------------------------------------------------------------------
def _box_oracle(inp):
    from oracle import pyoracle

    return pyoracle.aabb_intersect_n(f32(inp))


def _box_compare(spec, dev, orc, inp):
    dev = u32(dev)
    hit_o, t_o = orc
    flags, t, cls = dev[:, 0:4].view(np.int32), dev[:, 4:8], dev[:, 8].view(np.int32)
    rec = f32(inp)
    expect_cls = P.ray_class(rec[:, 6:9], rec[:, 9:12])
    bad = np.flatnonzero(cls != expect_cls)
    assert bad.size == 0, f"cls: {bad.size} records differ from makeRaySlab restated; first {rec[bad[0]]!r}: {cls[bad[0]]} vs {expect_cls[bad[0]]}"
    # aabbIntersect against the oracle: flag always, tMin by bits where the box is hit (rule 2)
    check_equal(flags[:, 0], hit_o, "aabbIntersect hit flag", False, records=inp)
    hit = hit_o == 1
    check_equal(t[:, 0], t_o, "aabbIntersect tMin", True, where=hit, records=inp)
    # the fast tests against the device's own aabbIntersect (rule 3)
    c0 = cls == 0
    tv = t.view(np.float32)
    for k, fn in ((1, "aabbFast"), (2, "aabbFastPk")):
        assert (flags[~c0, k] == -1).all(), f"{fn} was evaluated outside class 0"
        bad = np.flatnonzero(c0 & (flags[:, k] != flags[:, 0]))
        assert bad.size == 0, f"{fn} flag: {bad.size} class-0 records differ from aabbIntersect; first {rec[bad[0]]!r}"
        with np.errstate(invalid="ignore"):
            bad = np.flatnonzero(c0 & hit & ~(tv[:, k] == tv[:, 0]))
        assert bad.size == 0, (f"{fn} tMin: {bad.size} hit class-0 records differ in value from aabbIntersect; first "
                               f"{rec[bad[0]]!r}: {tv[bad[0], k]!r} vs {tv[bad[0], 0]!r}")
    bad = np.flatnonzero(flags[:, 3] != flags[:, 0])
    assert bad.size == 0, f"boxTest flag: {bad.size} records differ from aabbIntersect; first {rec[bad[0]]!r}"
    with np.errstate(invalid="ignore"):
        bad = np.flatnonzero(c0 & hit & ~(tv[:, 3] == tv[:, 0]))
    assert bad.size == 0, f"boxTest tMin (class 0): {bad.size} records differ in value; first {rec[bad[0]]!r}"
    check_equal(t[:, 3], t[:, 0], "boxTest tMin (literal classes)", True, where=hit & ~c0, records=inp)


# ---- triangles --------------------------------------------------------------------------------------------------------------------
def _triangle_compare(spec, dev, orc, inp):
    dev, orc = u32(dev), u32(orc)
    check_equal(dev[:, 0], orc[:, 0], "intersectTriangle hit flag", False, records=inp)
    hit = orc[:, 0] == 1
    check_equal(dev[:, 1:4], orc[:, 1:4], "intersectTriangle bary / dist of accepted hits", True, where=hit[:, None], records=inp)


# ---- display / denoiser recipes ---------------------------------------------------------------------------------------------------
def _pack_rgba_oracle(inp):
    from oracle import pyoracle

    img = f32(inp).reshape(-1, 3)
    return pyoracle.copy_image_to_pbo(img, len(img), 1, 0, 0, 1.0).view(np.uint32).reshape(-1, 1)


def _exp_pow_compare(spec, dev, orc, inp):
    dev, orc = u32(dev), u32(orc)
    check_equal(dev[:, [0, 1, 4]], orc, "exp_det(x), exp_det(y), pow_det(x, y)", True, records=inp)
    check_equal(dev[:, 2:4], dev[:, 0:2], "exp_det2 against exp_det on both halves", True, records=inp)
    assert (dev[:, 5] == 0).all()


# ---- textures ---------------------------------------------------------------------------------------------------------------------
def _linear_sample_spec(width, height):
    from oracle import pyoracle

    tex = P.texture(width, height)

    def buffer(inp):
        head = np.array([width, height, 0, 0], np.int32).view(np.uint32)
        return np.concatenate([head, u32(inp).reshape(-1), u32(tex).reshape(-1)])

    return Spec(f"linear_sample[{width}x{height}]", 2, 3, lambda: P.uv_records(width, height, P.N // 4),
                lambda inp: u32(pyoracle.linear_sample_n(tex, f32(inp))), _compare_all_words, device_buffer=buffer)


SPECS = [
    Spec("box", 12, 9, P.boxes_rays, _box_oracle, _box_compare),
    Spec("triangle", 15, 4, P.triangles_rays, _batch("intersect_triangle"), _triangle_compare),
    Spec("ray", 6, 8, lambda: np.concatenate([P.triples(11), P.triples(12)], axis=1), _batch("ray"), _compare_all_words, int_words=(0, 1)),
    Spec("utilhash", 1, 1, P.hash_words, _batch("utilhash"), _compare_all_words, int_words=(0,)),
    Spec("sincos", 1, 2, P.sincos_arguments, _batch("sincos"), _compare_all_words),
    Spec("atan2", 2, 1, lambda: np.concatenate([P.pairs(21), P.moderate_pairs(22)]), _batch("atan2"), _compare_all_words),
    Spec("to_sphere", 2, 3, P.to_sphere_uv, _batch("to_sphere"), _compare_all_words),
    Spec("to_plane", 3, 2, lambda: P.triples(41), _batch("to_plane"), _compare_all_words),
    Spec("power_heuristic", 2, 1, lambda: P.pairs(51), _batch("power_heuristic"), _compare_all_words),
    Spec("material", 20, 12, P.bsdf_records, _batch("material"), _compare_all_words, int_words=(11,)),
    Spec("procedural_texture", 2, 3, P.procedural_uv, _batch("procedural_texture"), _compare_all_words),
] + [_linear_sample_spec(w, h) for w, h in P.TEXTURE_SIZES] + [
    Spec("pow_gamma", 1, 1, P.all_exponents, _batch("pow_gamma"), _compare_all_words),
    Spec("pack_rgba", 3, 1, P.colours, _pack_rgba_oracle, _compare_all_words, int_words=(0,)),
    Spec("tonemap", 3, 6, P.colours, _batch("tonemap"), _compare_all_words),
    Spec("exp_pow", 2, 6, lambda: P.pairs(61), _batch("exp_pow"), _exp_pow_compare),
    Spec("reservoir", 20, 45, P.reservoir_records, _batch("reservoir"), _compare_all_words, int_words=tuple(range(7, 45, 9))),
    Spec("reservoir_w", 24, 1, P.reservoir_w_records, _batch("reservoir_w"), _compare_all_words),
]
SPEC_BY_NAME = {s.name: s for s in SPECS}


# ---------------------------------------------------------------------------------------------------------------------------------
# Against float64, on the sub-domains where float64 is a fair judge.  Each function below takes the input records and the
# outputs under test (the oracle's on the CPU, the device's on the GPU, same layout) and returns
#   {"errors": {quantity: worst error}, "mismatched flags": count, "domain": records judged or left out, "left out": share of
#    the domain within 1e-4 of a decision threshold}.
# BOUNDS: twice the oracle's worst error over the committed set, measured on the CPU, rounded up to one significant digit (the
# factor of two because the set is a sample and not the supremum).  Measured value | bound, side by side:
# ---------------------------------------------------------------------------------------------------------------------------------
BOUNDS = {
    #  quantity                  measured    bound
    "sincos abs":               (8.93e-8, 2e-7),
    "atan2 abs":                (2.77e-7, 6e-7),
    "pow_gamma rel":            (2.65e-6, 6e-6),
    "box tMin rel":             (1.63e-7, 4e-7),
    "triangle bary abs":        (1.26e-4, 3e-4),
    "triangle dist rel":        (1.34e-5, 3e-5),
    "metallic bsdf rel":        (7.98e-5, 2e-4),
    "metallic pdf rel":         (7.99e-5, 2e-4),
    "dielectric dir abs":       (3.08e-6, 7e-6),
    "dielectric bsdf rel":      (1.35e-7, 3e-7),
    "lambertian bsdf rel":      (8.73e-8, 2e-7),
    "lambertian pdf abs":       (4.82e-8, 1e-7),
}
LEFT_OUT_CAP = 0.05     # of a function's float64 domain (stricter than "of the set": every domain is a part of its set)
JUDGED_FLOOR = 0.05     # of the whole set: what float64 actually judges must not shrink to a token


def _result(errors, domain, left_out, flags=0):
    return {"errors": {k: float(v) for k, v in errors.items()}, "mismatched flags": int(flags), "domain": int(domain.sum()),
            "left out": float(left_out.sum()) / max(int(domain.sum()), 1),
            "judged share of the set": float((domain & ~left_out).sum()) / len(domain)}


def f64_sincos(inp, out):
    """Domain: finite |x| <= 1000 (the path's arguments are 2 pi u, u in [0, 1), with a wide margin).  Nothing left out."""
    x = _f64(f32(inp).reshape(-1))
    o = _f64(f32(out).reshape(-1, 2))
    with np.errstate(invalid="ignore"):
        dom = np.abs(x) <= 1000
    err = np.maximum(np.abs(o[dom, 0] - np.sin(x[dom])), np.abs(o[dom, 1] - np.cos(x[dom])))
    return _result({"sincos abs": err.max()}, dom, np.zeros_like(dom))


def f64_atan2(inp, out):
    """Domain: both arguments finite, non-zero and normal with 1e-30 <= |.| <= 1e30 (y / x neither overflows nor loses bits)."""
    a = _f64(f32(inp).reshape(-1, 2))
    o = _f64(f32(out).reshape(-1))
    with np.errstate(invalid="ignore"):
        dom = ((np.abs(a) >= 1e-30) & (np.abs(a) <= 1e30)).all(axis=1)
    err = np.abs(o[dom] - np.arctan2(a[dom, 0], a[dom, 1]))
    return _result({"atan2 abs": err.max()}, dom, np.zeros_like(dom))


def f64_pow_gamma(inp, out):
    """Domain: positive normal x."""
    x = _f64(f32(inp).reshape(-1))
    o = _f64(f32(out).reshape(-1))
    with np.errstate(invalid="ignore"):
        dom = (x >= 2.0 ** -126) & np.isfinite(x)
    ref = F64.pow_gamma_n(x[dom])
    return _result({"pow_gamma rel": (np.abs(o[dom] - ref) / ref).max()}, dom, np.zeros_like(dom))


def f64_box(inp, hit, t_min):
    """Domain: class-0 rays with 1e-3 <= |d.k| <= 0.999 (tests/test_oracle_kat.py's margin), coordinates of magnitude <= 10,
    boxes of positive thickness on every axis and origins on none of the box's six planes (a hit on a flat box has
    tFar == tNear, an origin on a plane has a t of exactly zero: both ARE decision thresholds, by construction; the bit
    comparison covers them).  Left out: |tFar - tNear| < 1e-4 or |tFar| < 1e-4."""
    r = f32(inp).reshape(-1, 12)
    cls = P.ray_class(r[:, 6:9], r[:, 9:12])
    with np.errstate(invalid="ignore"):
        a = np.abs(r[:, 9:12])
        dom = (cls == 0) & (a.min(axis=1) >= 1e-3) & (a.max(axis=1) <= 0.999) & (np.abs(r[:, :9]).max(axis=1) <= 10) & \
              (np.abs(r[:, :6]).max(axis=1) >= 1e-3) & (r[:, 3:6] > r[:, 0:3]).all(axis=1) & \
              (r[:, 6:9] != r[:, 0:3]).all(axis=1) & (r[:, 6:9] != r[:, 3:6]).all(axis=1)
    expect, tn, tf = F64.slab_n(r)
    with np.errstate(invalid="ignore"):
        left = dom & ((np.abs(tf - tn) < 1e-4) | (np.abs(tf) < 1e-4))
    judge = dom & ~left
    flags = (hit[judge] == 1) != expect[judge]
    h = judge & expect & (hit == 1)
    err = np.abs(t_min[h].astype(np.float64) - tn[h]) / np.maximum(1, np.abs(tn[h]))
    return _result({"box tMin rel": err.max()}, dom, left, flags.sum())


def f64_triangle(inp, out):
    """Domain: coordinates of magnitude in [1e-3, 10] or zero, and a well-conditioned system: |det| >= 1e-2 |e1| |e2| |d| (no sliver,
    no grazing ray).  Left out: u, v, 1 - u - v or t within 1e-4 of zero."""
    r = f32(inp).reshape(-1, 15)
    o = u32(out).reshape(-1, 4)
    u, v, t, det = F64.triangle_solve_n(r)
    r64 = _f64(r)
    e1, e2 = r64[:, 9:12] - r64[:, 6:9], r64[:, 12:15] - r64[:, 6:9]
    with np.errstate(invalid="ignore"):
        mag = np.abs(r64)
        dom = np.isfinite(r64).all(axis=1) & (mag.max(axis=1) <= 10) & ((mag >= 1e-3) | (mag == 0)).all(axis=1) & \
              (np.abs(det) >= 1e-2 * np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) * np.linalg.norm(r64[:, 3:6], axis=1)) & \
              (np.abs(det) > 0)
        left = dom & ((np.abs(u) < 1e-4) | (np.abs(v) < 1e-4) | (np.abs(1 - u - v) < 1e-4) | (np.abs(t) < 1e-4))
        expect = (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    judge = dom & ~left
    flags = (o[judge, 0] == 1) != expect[judge]
    h = judge & expect & (o[:, 0] == 1)
    got = _f64(o[:, 1:4].view(np.float32))
    bary = np.maximum(np.abs(got[h, 0] - u[h]), np.abs(got[h, 1] - v[h]))
    dist = np.abs(got[h, 2] - t[h]) / np.maximum(1, t[h])
    return _result({"triangle bary abs": bary.max(), "triangle dist rel": dist.max()}, dom, left, flags.sum())


def f64_metallic(inp, out):
    """Domain: MetallicWorkflow records with n.wo >= 0.05, n.wi >= 0.05 (grazing is ill-conditioned: tests/test_oracle_kat.py) and
    roughness >= 0.2 (the range tests/test_oracle_kat.py judges).  Nothing left out:
    no decision threshold (cosI cosO < 1e-7, n.h < 1e-6) is within reach of the domain."""
    r = f32(inp).reshape(-1, 20)
    o = _f64(f32(out).reshape(-1, 12))
    typ = u32(inp).reshape(-1, 20)[:, 0].view(np.int32)
    r64 = _f64(r)
    n, wo, wi = r64[:, 7:10], r64[:, 10:13], r64[:, 13:16]
    dot = lambda a, b: np.einsum("ij,ij->i", a, b)
    dom = (typ == P.METALLIC_WORKFLOW) & (dot(n, wo) >= 0.05) & (dot(n, wi) >= 0.05) & (r64[:, 5] >= 0.2)
    bsdf, pdf, _ = F64.metallic_n(r64[dom, 1:4], r64[dom, 4], r64[dom, 5], n[dom], wo[dom], wi[dom])
    eb = np.abs(o[dom, 0:3] - bsdf) / np.abs(bsdf)
    ep = np.abs(o[dom, 3] - pdf) / np.abs(pdf)
    return _result({"metallic bsdf rel": eb.max(), "metallic pdf rel": ep.max()}, dom, np.zeros_like(dom))


def f64_dielectric(inp, out):
    """Domain: Dielectric records (every ior, wo above and below the surface, grazing included) whose r.z is neither 0 nor the
    largest float below 1: those two sit on the reflect / refract threshold by construction wherever F is 0 (ior 1) or 1 (grazing,
    total internal reflection), and the bit comparison covers them.  Left out: r.z within 1e-4 of the
    Fresnel reflectance (the reflect / refract choice) or sin^2(theta_t) within 1e-4 of 1 (total internal reflection sets in).
    Flags: the sample type (reflection / transmission).  materialSample alone: the Dielectric BSDF and pdf are zero by bits."""
    r64 = _f64(f32(inp).reshape(-1, 20))
    o = u32(out).reshape(-1, 12)
    typ = u32(inp).reshape(-1, 20)[:, 0].view(np.int32)
    dom = (typ == P.DIELECTRIC) & (r64[:, 18] > 0) & (r64[:, 18] < float(P.ONE_BELOW))
    d, bsdf, kind, f, sin2_tr = F64.dielectric_sample_n(r64[dom, 1:4], r64[dom, 6], r64[dom, 7:10], r64[dom, 10:13], r64[dom, 18])
    left_d = (np.abs(r64[dom, 18] - f) < 1e-4) | (np.abs(sin2_tr - 1) < 1e-4)
    left = np.zeros_like(dom)
    left[dom] = left_d
    got = o[dom][~left_d]
    flags = got[:, 11] != kind[~left_d]
    same = ~flags
    gf = _f64(got[:, 4:10].view(np.float32))
    e_dir = np.abs(gf[same, 0:3] - d[~left_d][same])
    e_bsdf = np.abs(gf[same, 3:6] - bsdf[~left_d][same]) / bsdf[~left_d][same]
    assert (got[same, 10].view(np.float32) == 1).all()  # pdf of a specular sample
    return _result({"dielectric dir abs": e_dir.max(), "dielectric bsdf rel": e_bsdf.max()}, dom, left, flags.sum())


def f64_lambertian(inp, out):
    """Domain: Lambertian records.  Nothing left out (max(n.wi, 0) is continuous at 0; the pdf error is absolute)."""
    r64 = _f64(f32(inp).reshape(-1, 20))
    o = _f64(f32(out).reshape(-1, 12))
    dom = u32(inp).reshape(-1, 20)[:, 0].view(np.int32) == P.LAMBERTIAN
    bsdf, pdf = F64.lambertian_n(r64[dom, 1:4], r64[dom, 7:10], r64[dom, 13:16])
    return _result({"lambertian bsdf rel": (np.abs(o[dom, 0:3] - bsdf) / bsdf).max(), "lambertian pdf abs": np.abs(o[dom, 3] - pdf).max()},
                   dom, np.zeros_like(dom))


def float64_checks(outputs):
    """`outputs(name)` -> the outputs under test of Spec `name` on its committed inputs.  Returns {function: result}."""
    S = SPEC_BY_NAME
    hit, t = outputs("box")
    return {
        "sincos": f64_sincos(S["sincos"].inputs(), outputs("sincos")),
        "atan2": f64_atan2(S["atan2"].inputs(), outputs("atan2")),
        "pow_gamma": f64_pow_gamma(S["pow_gamma"].inputs(), outputs("pow_gamma")),
        "box": f64_box(S["box"].inputs(), hit, t),
        "triangle": f64_triangle(S["triangle"].inputs(), outputs("triangle")),
        "metallic": f64_metallic(S["material"].inputs(), outputs("material")),
        "dielectric": f64_dielectric(S["material"].inputs(), outputs("material")),
        "lambertian": f64_lambertian(S["material"].inputs(), outputs("material")),
    }


def assert_float64(results):
    for fn, res in results.items():
        print(f"{fn}: {res}")
    for fn, res in results.items():
        assert res["domain"] >= 1000, f"{fn}: only {res['domain']} records in the float64 domain"
        assert res["judged share of the set"] >= JUDGED_FLOOR, f"{fn}: float64 judges only {res['judged share of the set']:.2%} of the set"
        assert res["left out"] <= LEFT_OUT_CAP, f"{fn}: {res['left out']:.3%} of the domain left out, cap {LEFT_OUT_CAP:.0%}"
        assert res["mismatched flags"] == 0, f"{fn}: {res['mismatched flags']} hit flags differ from the float64 model"
        for q, e in res["errors"].items():
            assert math.isfinite(e) and e <= BOUNDS[q][1], f"{q}: worst error {e:.3g} exceeds the bound {BOUNDS[q][1]:.3g}"
