"""CPU side of the per-function comparisons: the input sets of tests/probe_inputs.py cover what they claim, the oracle alone
holds the float64 bounds of tests/probe_sets.py within the 5 % cap, the oracle's batch entries equal its scalar hooks, and the
device probe library exports nothing but its probe_* entries."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import float64_models as F64
import probe_inputs as P
import probe_sets as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_LIB = os.environ.get("RADISH_PROBE_LIB") or os.path.join(ROOT, "tests", "probe", "libradish_probe.so")


def _out(name):
    return S.SPEC_BY_NAME[name].oracle_outputs()


def test_probe_library_exports_only_probe_entries():
    """It shares a process with libradish_hip.so: anything else it defined could shadow or be shadowed by the product's symbols."""
    assert os.path.exists(PROBE_LIB), f"{PROBE_LIB} missing: __graft_entry__.build() (radish_pt_amd._build.build_probe) makes it"
    out = subprocess.run(["nm", "-D", "--defined-only", PROBE_LIB], check=True, capture_output=True, text=True).stdout
    names = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert names and all(n.startswith("probe_") for n in names), names
    assert sorted(set(names)) == sorted({s.entry() for s in S.SPECS})


def test_product_does_not_know_the_probe():
    from radish_pt_amd import api

    assert not [e for e in api.EXPORTS if e.startswith("probe_")]


def test_box_set_coverage():
    rec = P.boxes_rays()
    assert rec.shape == (P.N, 12)
    cls = P.ray_class(rec[:, 6:9], rec[:, 9:12])
    hit, _ = _out("box")
    for c in range(6):
        assert (cls == c).sum() >= 1000, f"class {c}: {(cls == c).sum()} records"
    for c in range(5):
        assert ((cls == c) & (hit == 1)).sum() >= 1000 and ((cls == c) & (hit == 0)).sum() >= 1000, f"class {c} hits / misses"
    taken = np.bincount(P.aabb_return_taken(rec), minlength=len(P.AABB_RETURNS))
    assert (taken > 0).all(), dict(zip(P.AABB_RETURNS, taken))
    lo, hi, o, d = rec[:, 0:3], rec[:, 3:6], rec[:, 6:9], rec[:, 9:12]
    on_plane = ((o == lo) | (o == hi)).sum(axis=1)
    flat = (lo == hi).sum(axis=1)
    mag = np.abs(rec[:, :9])
    with np.errstate(invalid="ignore"):
        claims = {
            "origin on a face": on_plane == 1, "origin on an edge": on_plane == 2, "origin at a corner": on_plane == 3,
            "origin strictly inside": ((o > lo) & (o < hi)).all(axis=1), "origin outside": ((o < lo) | (o > hi)).any(axis=1),
            "flat in x": (flat == 1) & (lo[:, 0] == hi[:, 0]), "flat in y": (flat == 1) & (lo[:, 1] == hi[:, 1]),
            "flat in z": (flat == 1) & (lo[:, 2] == hi[:, 2]), "point box": flat == 3,
            "coordinates near 1e-30": (mag.max(axis=1) < 1e-29) & (mag.max(axis=1) > 0), "coordinates beyond 1e29": mag.max(axis=1) > 1e29,
            "|d.k| == 1e-6": (np.abs(d) == P.EPS).any(axis=1), "|d.k| == 1e-6 + 1 ulp": (np.abs(d) == P.ulp_up(P.EPS)).any(axis=1),
            "|d.k| == 1e-6 - 1 ulp": (np.abs(d) == P.ulp_down(P.EPS)).any(axis=1),
            "|d.k| == 1 - 1e-6": (np.abs(d) == P.ONE_MINUS_EPS).any(axis=1),
            "|d.k| == 1 - 1e-6 + 1 ulp": (np.abs(d) == P.ulp_up(P.ONE_MINUS_EPS)).any(axis=1),
            "|d.k| == 1 - 1e-6 - 1 ulp": (np.abs(d) == P.ulp_down(P.ONE_MINUS_EPS)).any(axis=1),
            "+0 component": ((d == 0) & ~np.signbit(d)).any(axis=1), "-0 component": ((d == 0) & np.signbit(d)).any(axis=1),
            "all-negative direction": (d < 0).all(axis=1), "all-positive direction": (d > 0).all(axis=1),
            "NaN in origin": np.isnan(o).any(axis=1), "inf in origin": np.isinf(o).any(axis=1),
            "NaN in direction": np.isnan(d).any(axis=1), "inf in direction": np.isinf(d).any(axis=1),
            "|d.k| > 1": (np.abs(d) > 1).any(axis=1) & np.isfinite(d).all(axis=1),
        }
    for what, m in claims.items():
        assert m.sum() >= 100, f"{what}: {m.sum()} records"
    # boxes behind the ray: the float64 slab test's far distance is negative
    _, _, tf = F64.slab_n(rec)
    with np.errstate(invalid="ignore"):
        assert (tf < 0).sum() >= 1000


def test_triangle_set_coverage():
    rec = P.triangles_rays()
    out = _out("triangle")
    hit = out[:, 0] == 1
    assert hit.mean() >= 0.10, f"{hit.mean():.1%} hits"
    assert (~hit).sum() >= 1000
    bary, dist = out[:, 1:3].view(np.float32), out[:, 3].view(np.float32)
    u, v, t, det = F64.triangle_solve_n(rec)
    e1, e2 = rec[:, 9:12] - rec[:, 6:9], rec[:, 12:15] - rec[:, 6:9]
    with np.errstate(all="ignore"):
        det32 = np.abs(np.float32(det))  # exact for the constructed records (det = a)
        claims = {
            "bary.x == 0 accepted": hit & (bary[:, 0] == 0), "bary.y == 0 accepted": hit & (bary[:, 1] == 0),
            "u + v == det accepted": hit & (u + v == 1), "t == 0 exactly": (t == 0) & (u > 0) & (v > 0) & (u + v < 1),
            "back faces hit": hit & (det < 0), "front faces hit": hit & (det > 0),
            "|det| == FLT_EPSILON": det32 == P.FLT_EPSILON, "|det| == FLT_EPSILON + 1 ulp": det32 == P.ulp_up(P.FLT_EPSILON),
            "|det| == FLT_EPSILON - 1 ulp": det32 == P.ulp_down(P.FLT_EPSILON),
            "zero area": (np.cross(e1.astype(np.float64), e2.astype(np.float64)) == 0).all(axis=1),
            "slivers": (np.linalg.norm(np.cross(e1.astype(np.float64), e2.astype(np.float64)), axis=1) > 0) &
                       (np.linalg.norm(np.cross(e1.astype(np.float64), e2.astype(np.float64)), axis=1)
                        < 1e-4 * np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)) & (np.abs(rec).max(axis=1) < 10) &
                       (np.abs(e1).max(axis=1) > 1e-3),
            "coordinates beyond 1e29": np.abs(rec).max(axis=1) > 1e29,
            "subnormal edge vectors": (np.abs(e1).max(axis=1) < 2.0 ** -126) & (np.abs(e1).max(axis=1) > 0),
        }
    for what, m in claims.items():
        assert m.sum() >= 100, f"{what}: {m.sum()} records"


def test_bsdf_set_coverage():
    rec = P.bsdf_records()
    typ = rec[:, 0].view(np.int32)
    n, wo, wi, r = rec[:, 7:10].astype(np.float64), rec[:, 10:13].astype(np.float64), rec[:, 13:16].astype(np.float64), rec[:, 16:19]
    cos_o, cos_i = np.einsum("ij,ij->i", n, wo), np.einsum("ij,ij->i", n, wi)
    for t in range(5):
        assert (typ == t).sum() >= 1000
    for what, col, values in (("metallic", 4, P.METALLIC), ("roughness", 5, P.ROUGHNESS), ("ior", 6, P.IOR)):
        for v in values:
            assert (rec[:, col] == np.float32(v)).sum() >= 1000, f"{what} {v}"
    eta = np.where(cos_o < 0, 1 / rec[:, 6].astype(np.float64), rec[:, 6].astype(np.float64))
    claims = {
        "grazing wo": np.abs(cos_o) < 2e-4, "grazing wi": np.abs(cos_i) < 2e-4, "wo below the surface": cos_o < -0.01,
        "wi is the mirror direction": (rec[:, 13:16] == P._reflect32(-rec[:, 10:13], rec[:, 7:10])).all(axis=1),
        "wi == wo": (rec[:, 13:16] == rec[:, 10:13]).all(axis=1),
        "total internal reflection": (typ == P.DIELECTRIC) & ((1 - cos_o * cos_o) / (eta * eta) >= 1),
        "r component == 0": (r == 0).any(axis=1), "r component just below 1": (r == P.ONE_BELOW).any(axis=1),
    }
    for what, m in claims.items():
        assert m.sum() >= 1000, f"{what}: {m.sum()} records"
    # Light and Disney give the zero / no-op results of materialBSDF / materialPdf / materialSample (bsdf.h)
    out = _out("material")
    inert = (typ == P.DISNEY) | (typ == P.LIGHT)
    assert (out[inert, 0:11] == 0).all() and (out[inert, 11] == 1 << 15).all()


def test_one_argument_and_texture_set_coverage():
    a = P.all_exponents()
    b = a.view(np.uint32)
    e, s, m = (b >> 23) & 0xFF, b >> 31, b & 0x7FFFFF
    for ex in range(256):
        for sg in (0, 1):
            sel = (e == ex) & (s == sg)
            assert sel.sum() >= (1 << 12) and (m[sel] == 0).any() and (m[sel] == 0x7FFFFF).any()
    assert np.isin(P.SPECIALS.view(np.uint32), b).all()
    h = P.hash_words()
    assert len(h) >= (1 << 20) and (h == 0).any() and (h == 0xFFFFFFFF).any()
    for w, hgt in P.TEXTURE_SIZES:
        uv = P.uv_records(w, hgt, P.N // 4)
        assert np.isfinite(uv).all()
        for what, sel in {"negative": uv < 0, "exact integer": (uv == np.floor(uv)) & (np.abs(uv) >= 1) & (np.abs(uv) < 10),
                          "just below 1": uv == P.ONE_BELOW, "1e30": uv == np.float32(1e30),
                          "subnormal": (np.abs(uv) < 2.0 ** -126) & (uv != 0)}.items():
            assert sel.sum() >= 100, (w, hgt, what)
        # texel centres ((k + 0.5) / size) and texel boundaries (k / size), each exactly and one ulp to either side
        for axis, size in ((0, w), (1, hgt)):
            u = uv[:, axis]
            k = np.arange(-size, 2 * size + 1)
            for what, base in (("texel centre", np.float32((k + 0.5) / size)), ("texel boundary", np.float32(k / float(size)))):
                for step, val in (("", base), (" + 1 ulp", np.nextafter(base, np.float32(np.inf))),
                                  (" - 1 ulp", np.nextafter(base, np.float32(-np.inf)))):
                    assert np.isin(u, val).sum() >= 100, (w, hgt, axis, what + step)
    assert (np.abs(P.procedural_uv()) < P.PROC_TEX_UV_MAX).all()
    r = P.reservoir_records()
    wgt, cnt = r[:, 8], r[:, 7].view(np.int32)
    with np.errstate(invalid="ignore"):
        for what, sel in {"zero": wgt == 0, "subnormal": (np.abs(wgt) < 2.0 ** -126) & (wgt != 0), "huge": wgt > 1e38,
                          "inf": np.isinf(wgt), "NaN": np.isnan(wgt), "negative": wgt < 0, "M == 0": cnt == 0, "M == 1": cnt == 1,
                          "M at the clamp": cnt == P.RESERVOIR_M, "M above the clamp": cnt > P.RESERVOIR_M,
                          "rnd == 0": r[:, 18] == 0, "rnd just below 1": r[:, 18] == P.ONE_BELOW}.items():
            assert sel.sum() >= 1000, what


def test_oracle_batch_entries_equal_the_scalar_hooks():
    """The _n entries are loops: on a slice of each set they return what the scalar hooks of tests/test_oracle_kat.py return."""
    from oracle import pyoracle

    lib = pyoracle.lib()
    k = slice(0, None, 4099)
    rec = P.boxes_rays()[k]
    hit, t = pyoracle.aabb_intersect_n(rec)
    for i, r in enumerate(rec):
        tt = C.c_float(0)
        b, ry = np.ascontiguousarray(r[:6]), np.ascontiguousarray(r[6:])
        assert lib.orc_aabb_intersect(b.ctypes.data, ry.ctypes.data, C.byref(tt)) == hit[i]
        assert np.float32(tt.value).view(np.uint32) == t[i].view(np.uint32) or (np.isnan(tt.value) and np.isnan(t[i]))
    x = P.all_exponents()[k]
    sc = pyoracle.batch("sincos", x).view(np.float32)
    for i, v in enumerate(x):
        s, c = C.c_float(0), C.c_float(0)
        lib.orc_sincos(float(v), C.byref(s), C.byref(c))
        assert not S.mismatches(np.float32([s.value, c.value]), sc[i]).any() or np.isnan(v)
    hw = P.hash_words()[k]
    assert [lib.orc_utilhash(int(a)) for a in hw] == list(pyoracle.batch("utilhash", hw)[:, 0])
    assert np.array_equal(pyoracle.batch("utilhash", hw)[:, 0], F64.utilhash_n(hw))


def test_oracle_holds_the_float64_bounds():
    """The oracle alone, against the float64 models, over the committed sets: within tests/probe_sets.py:BOUNDS and the 5 % cap."""
    S.assert_float64(S.float64_checks(_out))
    for q, (measured, bound) in S.BOUNDS.items():
        digit = 10.0 ** math.floor(math.log10(2 * measured))
        assert math.isclose(bound, math.ceil(2 * measured / digit) * digit, rel_tol=1e-9), q  # twice the measured worst, rounded up to one digit
