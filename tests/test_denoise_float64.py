"""The denoisers' oracle (oracle.cpp orc_denoise_*) against the float64 model (denoise_model.py), per launch on the same
float32 inputs, over shapes x levels x sigma sets; the model's planted mistakes are each caught; and the tiled filters'
launch grid (kernels_denoise.h denoiseTileGrid) stays within 4 W H workgroups at every accepted level.

Tolerance (denoise_model.py): a first-order bound, not a tuned constant.  For each tap q the float32 argument of every
weight factor carries the running-error bound of its computation (u |result| per float32 operation, the float32
representation error of each decimal literal, positions reconstructed from the camera record with the same accounting);
exp / pow turn it into a bound dw_q on the weight, plus the recipe errors DESIGN states (exp_det 2.4e-7, pow_det 8e-6
relative) and exp_det's flush to 0 below -87.3.  The output's bound is then

    sum_q dw_q |c_q - out| / sum_q w_q  +  gamma_25 (sum_q w_q |c_q| + |out| sum_q w_q) / sum_q w_q  +  u |out|,

the second term being the float32 accumulation of 25 products (Higham's gamma_n = n u / (1 - n u)), the third the final
division.  SVGF pixels whose weightSum or weight2Sum lies within its bound of FLT_EPSILON, and temporal pixels whose
|dot(normal, lastNormal)| lies within its bound (plus |.1f - .1|) of .1, are skipped: the branch taken is not decided by
the model there."""
import itertools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import denoise_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HAVE_HIPCC = shutil.which(HIPCC) is not None or os.path.exists(HIPCC)

SHAPES = [(1, 1), (1, 9), (9, 1), (2, 3), (5, 5), (16, 16), (17, 17), (31, 9), (33, 8), (70, 45)]
EAW_SIGMAS = list(itertools.product((64.0, 60.0), (0.25, 0.2), (1.0, 0.7)))  # all 8 power-of-two patterns
EDGE = (2.0 ** -125, 2.0 ** 125, 2.0 ** -126, 2.0 ** 126)  # accepted / refused by sigmaIsPow2; all finite
EAW_EDGE = [tuple(e if k == pos else r for k, r in enumerate((64.0, 0.2, 1.0))) for pos in range(3) for e in EDGE]
SVGF_SIGMAS = [(4.0, 128.0, sd) for sd in (1.0, 0.9999, 4096.0)]


def _case(W, H, seed=1):
    s = M.synthetic(W, H, seed)
    return s, M.camera(W, H), M.host_gbuffer(s, W, H)


def _band(a, W, rows):
    return a if rows is None else a[rows[0] * W:rows[1] * W]


def eaw_violations(s, cam, gb, sig, level, rows=None, **plant):
    from oracle import pyoracle

    ref = pyoracle.denoise_eaw(s["color"], gb, cam, *sig, level)
    out, bound = M.eaw(s["color"], s, cam, *sig, level, rows, **plant)
    return M.violations(_band(ref, gb.width, rows), out, bound)


def svgf_violations(s, cam, gb, sig, level, rows=None, **plant):
    from oracle import pyoracle

    col, var = pyoracle.denoise_svgf(s["color"], s["variance"], s["var_filtered"], gb, cam, *sig, level)
    out, bound, vout, vbound, skip = M.svgf(s["color"], s["variance"], s["var_filtered"], s, cam, *sig, level, rows, **plant)
    assert skip.mean() < 0.05, "the synthetic inputs should leave the SVGF branches decided"
    W = gb.width
    return M.violations(_band(col, W, rows), out, bound, skip) + M.violations(_band(var, W, rows), vout, vbound, skip)


def temporal_violations(s, gb, first, **plant):
    from oracle import pyoracle

    c, m = pyoracle.denoise_temporal_accumulate(s["color_accum"], s["moment_accum"], s["color"], gb, first)
    mc, mm, skip = M.temporal_accumulate(s["color_accum"], s["moment_accum"], s["color"], s, first, **plant)
    return M.violations(c, mc.v, mc.e, skip) + M.violations(m, mm.v, mm.e, skip)


def variance_violations(s, W, H, **plant):
    from oracle import pyoracle

    v = M.estimate_variance(s["moment"], W, H, **{k: x for k, x in plant.items() if k == "threshold"})
    f = M.filter_variance(s["variance"], W, H, **{k: x for k, x in plant.items() if k == "border_div1"})
    return (M.violations(pyoracle.denoise_estimate_variance(s["moment"], W, H), v.v, v.e)
            + M.violations(pyoracle.denoise_filter_variance(s["variance"], W, H), f.v, f.e))


@pytest.mark.parametrize("W,H", SHAPES)
def test_oracle_filters_within_float64_bound(W, H):
    s, cam, gb = _case(W, H)
    bad = []
    for level in range(17):
        for sig in EAW_SIGMAS + EAW_EDGE:
            if eaw_violations(s, cam, gb, sig, level):
                bad.append(("eaw", level, sig))
        for sig in SVGF_SIGMAS:
            if svgf_violations(s, cam, gb, sig, level):
                bad.append(("svgf", level, sig))
    assert not bad, bad


def test_oracle_filters_within_float64_bound_multi_tile():
    """301 x 271: levels 3 and 4 have 2-3 tiles per residue class in both directions (the model on a band of rows that
    crosses the region boundaries and both tile seams of level 3)."""
    s, cam, gb = _case(301, 271)
    for level in range(9):
        assert eaw_violations(s, cam, gb, (64.0, 0.2, 1.0), level, rows=(124, 144)) == 0, level
        assert svgf_violations(s, cam, gb, (4.0, 128.0, 1.0), level, rows=(124, 144)) == 0, level


@pytest.mark.parametrize("W,H", SHAPES + [(301, 271)])
def test_oracle_per_pixel_kernels_within_float64_bound(W, H):
    s, cam, gb = _case(W, H)
    assert temporal_violations(s, gb, True) == 0
    assert temporal_violations(s, gb, False) == 0
    assert variance_violations(s, W, H) == 0


def test_synthetic_inputs_cover_the_edges():
    """What makes the planted mistakes visible is really in the inputs."""
    s = M.synthetic(70, 45, 1)
    assert (s["primId"] == -1).any() and (s["primId"] > 2 ** 30).any() and len(np.unique(s["primId"])) >= 8
    assert (np.abs(s["normal"]).sum(1) == 0).any() and (s["variance"] < 0).any() and (s["var_filtered"] < 0).any()
    assert (s["moment"][:, 2] == 4.0).any() and (s["moment"][:, 2] == 3.0).any()
    assert s["motion"].min() == -1 and s["motion"].max() < 70 * 45
    assert len(np.unique(s["depth"].round(1))) >= 4


PLANTED = {  # switch -> which comparison must catch it
    "gauss_1pct": ("eaw", "svgf"),
    "step_x_plus1": ("eaw", "svgf"),
    "no_id_test": ("eaw",),
    "no_normal_eps": ("svgf",),
    "no_sqrt": ("svgf",),
    "swap_nd": ("eaw", "svgf"),
}


@pytest.mark.parametrize("switch", sorted(PLANTED))
def test_planted_filter_mistake_is_caught(switch):
    for kind in PLANTED[switch]:
        caught = 0
        for (W, H), level in itertools.product([(17, 17), (70, 45)], (0, 1, 2)):
            s, cam, gb = _case(W, H)
            if kind == "eaw":
                caught += eaw_violations(s, cam, gb, (64.0, 0.2, 1.0), level, **{switch: True})
            else:
                caught += svgf_violations(s, cam, gb, (4.0, 128.0, 1.0), level, **{switch: True})
        assert caught > 0, f"{kind} with {switch} passes the oracle comparison"


@pytest.mark.parametrize("plant", [{"alpha": 0.21}, {"threshold": 4.5}, {"border_div1": True}], ids=str)
def test_planted_per_pixel_mistake_is_caught(plant):
    caught = 0
    for W, H in [(17, 17), (70, 45)]:
        s, cam, gb = _case(W, H)
        if "alpha" in plant:
            caught += temporal_violations(s, gb, False, **plant)
        else:
            caught += variance_violations(s, W, H, **plant)
    assert caught > 0, f"{plant} passes the oracle comparison"


# ---- the launch grid of the tiled filters --------------------------------------------------------------------------------
GRID_TABLE = [(W, H, lv) for W, H in SHAPES + [(301, 271), (1920, 1080)] for lv in range(17)]
PROBE = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "device/kernels_denoise.h"
int main(int argc, char **argv) {  // W H level triples -> W H level gx gy tilesX tilesY; no HIP call is made
    for (int a = 1; a + 2 < argc; a += 3) {
        const int w = atoi(argv[a]), h = atoi(argv[a + 1]), level = atoi(argv[a + 2]);
        const dim3 g = rd::denoiseTileGrid(w, h, level);
        const int step = 1 << level, subW = (w + step - 1) / step, subH = (h + step - 1) / step;
        printf("%d %d %d %u %u %d %d\n", w, h, level, g.x, g.y, (subW + rd::kDT - 1) / rd::kDT, (subH + rd::kDT - 1) / rd::kDT);
    }
    return 0;
}
"""


def grid_table(header_dir, table):
    """Compile the probe against `header_dir` (a csrc tree) with the library's flags for gfx950 and run it on the host."""
    from radish_pt_amd import _build

    flags = [f for f in _build.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "grid_probe.hip"), os.path.join(tmp, "grid_probe")
        with open(src, "w") as f:
            f.write(PROBE)
        r = subprocess.run([HIPCC] + flags + ["-I", header_dir, src, "-o", exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run([exe] + [str(v) for t in table for v in t], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
    return {tuple(int(v) for v in ln.split()[:3]): tuple(int(v) for v in ln.split()[3:]) for ln in r.stdout.splitlines()}


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_denoise_tile_grid_is_bounded():
    rows = grid_table(os.path.join(ROOT, "radish_pt_amd", "csrc"), GRID_TABLE)
    assert len(rows) == len(GRID_TABLE)
    for (W, H, lv), (gx, gy, tx, ty) in rows.items():
        assert gx * gy <= 4 * W * H, (W, H, lv, gx, gy)
        assert gx // tx <= W and gy // ty <= H, (W, H, lv, gx, gy)  # every launched residue class holds a pixel
        assert gx % tx == 0 and gy % ty == 0
        step = 1 << lv
        assert gx // tx == min(step, W) and gy // ty == min(step, H), (W, H, lv)  # and every class that holds one is launched
    assert rows[(1, 1, 16)][:2] == (1, 1)
    assert rows[(70, 45, 16)][0] * rows[(70, 45, 16)][1] == 3150
    for lv in range(5):  # unchanged where step <= width, height: 1080p at the levels the filter classes use
        step, sub = 1 << lv, lambda n: -(-n // (1 << lv))
        assert rows[(1920, 1080, lv)][:2] == (-(-sub(1920) // 16) * step, -(-sub(1080) // 16) * step), lv


def test_denoise_grid_comment_and_design_agree():
    src = open(os.path.join(ROOT, "radish_pt_amd", "csrc", "device", "kernels_denoise.h")).read()
    assert re.search(r"[Ll]evels 0-16", src)
    hip = open(os.path.join(ROOT, "radish_pt_amd", "csrc", "radish_hip.hip")).read()
    assert hip.count("level < 0 || level > 16") == 2  # both filters accept exactly levels 0-16
