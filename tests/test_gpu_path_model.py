"""The HIP kernels against tests/path_model.py, the float64 statement of the textured, environment-lit path — directly, pixel by
pixel, not by way of the oracle agreeing with both.  Scene, cameras, loopers, tolerance and cap are those of
tests/test_path_model_cpu.py (tests/path_model_checks.py holds them, and evaluates the model once for all structures): 48x36,
depth 3, iterations 0 and 1; three cameras for the G-buffer and ReSTIR.  The pixels left out under the cap must be the very pixels
the oracle's run leaves out, the two being bit-identical."""
import numpy as np
import pytest

import path_model_checks as C
import restir_model_checks as RC
from test_gpu_restir_model import _run_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]


def _torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def setup():
    sd, ms, cams = C.setup()
    return {"sd": sd, "ms": ms, "cams": cams}


def _use(ctx, setup):
    ctx.set_partition(0, 1, 64)
    ctx.upload_scene(setup["sd"])
    ctx.set_camera(setup["cams"][0])


def _check_path_trace(tested, what):
    want = C.oracle_excluded()["path_trace"]
    for it, e in enumerate(C.path_trace_excluded(tested)):
        print(what, it, {k: v.tolist() for k, v in e.items()})
        for k, px in e.items():
            C.assert_within_cap(px, f"{what}, iteration {it}, {k}")
            assert px.tolist() == want[it][k].tolist(), f"{what}, iteration {it}, {k}: not the pixels the oracle's run leaves out"
    assert tested[1][0].max() > 0.3 and tested[1][1].max() > 0.3


@pytest.mark.parametrize("structure", ["mega", "wavefront", "wavefront_sort", "persistent", "persistent_threaded", "wavefront_threaded", "auto"])
def test_path_trace_vs_model(gpu_ctx, setup, structure):
    from radish_pt_amd import api

    torch = _torch()
    flags = {"mega": api.RDH_PT_MEGAKERNEL, "wavefront": api.RDH_PT_WAVEFRONT,
             "wavefront_sort": api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL, "persistent": api.RDH_PT_PERSISTENT,
             "persistent_threaded": api.RDH_PT_PERSISTENT | api.RDH_PT_NO_PAIRS,
             "wavefront_threaded": api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_NO_PAIRS, "auto": api.RDH_PT_AUTO}[structure]
    _use(gpu_ctx, setup)
    d, i = torch.zeros(C.N, 3, device="cuda"), torch.zeros(C.N, 3, device="cuda")
    tested = []
    for it, looper in enumerate(C.LOOPERS):
        gpu_ctx.path_trace(d, i, it, looper, C.MAX_DEPTH, flags)
        tested.append((d.cpu().numpy(), i.cpu().numpy()))
    _check_path_trace(tested, structure)


def test_path_trace_samples_vs_model(gpu_ctx, setup):
    """Both iterations as two samples of ONE wavefront pass (the loopers are consecutive for this): only the end is seen, and it
    is the model's mean over its own iteration 0."""
    from radish_pt_amd import api

    torch = _torch()
    assert C.LOOPERS[1] == C.LOOPERS[0] + 1
    _use(gpu_ctx, setup)
    d, i = torch.zeros(C.N, 3, device="cuda"), torch.zeros(C.N, 3, device="cuda")
    gpu_ctx.path_trace_samples(d, i, 0, C.LOOPERS[0], 2, C.MAX_DEPTH, api.RDH_PT_WAVEFRONT, samples_per_pass=2)
    got = (d.cpu().numpy(), i.cpu().numpy())
    want = C.oracle_excluded()["path_trace"][1]
    m = C.model_path_trace()[1]
    for k, g in (("direct", got[0]), ("indirect", got[1])):
        px = np.flatnonzero(C.far(g, m[k]))
        print("samples", k, px.tolist())
        C.assert_within_cap(px, f"path_trace_samples, {k}")
        assert px.tolist() == want[k].tolist()
    assert got[1].max() > 0.3


def test_path_trace_direct_vs_model(gpu_ctx, setup):
    torch = _torch()
    _use(gpu_ctx, setup)
    d = torch.zeros(C.N, 3, device="cuda")
    tested = []
    for it, looper in enumerate(C.LOOPERS):
        gpu_ctx.path_trace_direct(d, it, looper)
        tested.append(d.cpu().numpy())
    want = C.oracle_excluded()["pt_direct"]
    for it, px in enumerate(C.images_excluded(tested, C.model_pt_direct())):
        print("direct", it, px.tolist())
        C.assert_within_cap(px, f"path_trace_direct, iteration {it}")
        assert px.tolist() == want[it].tolist()
    assert tested[1].max() > 1.0


@pytest.mark.parametrize("kernel", ["packets", "packets_budget_4", "persistent", "one_lane_per_pixel"])
def test_gbuffer_kernels_vs_model(gpu_ctx, setup, kernel):
    """The planes of every G-buffer kernel over the three cameras: id and motion exactly, normal (after the normal map), depth and
    albedo (after the maps; the sky's colour on a miss) within the tolerance."""
    from radish_pt_amd import api

    flags = {"one_lane_per_pixel": api.RDH_PT_MEGA_GBUFFER, "persistent": api.RDH_PT_NO_PACKETS, "packets": 0,
             "packets_budget_4": api.RDH_PT_WF_SMALL_LISTS}[kernel]
    frames = _run_gpu(gpu_ctx, setup, 0, 1, 0, gbuffer_flags=flags, restir=False)
    want = C.oracle_excluded()["gbuffer"]
    for f, px in enumerate(C.gbuffer_excluded([t["planes"] for t in frames])):
        print(kernel, f, px.tolist())
        C.assert_within_cap(px, f"{kernel}, camera {f}")
        assert px.tolist() == want[f].tolist()
        assert (frames[f]["planes"]["primId"] == -1).sum() > 100 and (frames[f]["planes"]["primId"] == -2).sum() > 30


@pytest.mark.parametrize("structure", ["split", "fused", "no_packets"])
@pytest.mark.parametrize("reuse,faithful", C.RESTIR_CASES)
def test_restir_kernels_vs_model(gpu_ctx, setup, reuse, faithful, structure):
    from radish_pt_amd import api

    flags = {"split": 0, "fused": api.RDH_PT_RESTIR_FUSED, "no_packets": api.RDH_PT_NO_PACKETS}[structure]
    want = C.oracle_restir_excluded(reuse, faithful)
    frames = _run_gpu(gpu_ctx, setup, reuse, faithful, flags)
    for f, t in enumerate(frames):
        ex, p1, _ = RC.check_frame(setup["ms"], f, setup["cams"], reuse, faithful, t)
        what = f"{structure}, reuse {reuse}, faithful {faithful}, frame {f}"
        print(what, {k: v.tolist() for k, v in ex.items()})
        RC.assert_within_cap(ex, what)
        for step in ex:
            assert ex[step].tolist() == want[f][0][step].tolist(), f"{what}, {step}: not the pixels the oracle's run leaves out"
        assert t["image"].max() > 0 and p1["stored"].sum() > 1000
