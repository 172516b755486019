"""The path's shading step (csrc/device/path_step.h) on a scene where every branch of it is live, through every kernel structure.

cornell_textured with its environment map has Lambertian, textured metallic and dielectric surfaces, an emitter and an environment:
misses with and without the MIS weight, emitter hits, NEE through every BSDF class, specular and diffuse samples.  Depth 1 makes the
depth bound cut every path right after its first bounce body; depth 3 lets the later branches run.  Images are compared bit for bit
and the five work counters exactly, over two accumulated iterations, with no tolerance and no pixel left out."""
import numpy as np
import pytest

from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

W, H = 40, 28
DEPTHS = (1, 3)
ITERS = ((0, 60), (1, 61))  # (iter, looper)
COUNTERS = ("closestRays", "anyRays", "nodeVisits", "triTests", "closestHits")


def _oracle_frames(sd, cam, depth):
    from oracle import pyoracle

    o = pyoracle.OracleScene(sd)
    d, i = np.zeros((W * H, 3), np.float32), np.zeros((W * H, 3), np.float32)
    for it, looper in ITERS:
        o.path_trace(cam, d, i, it, looper, depth)
    return d, i, o.stats()


@pytest.fixture(scope="module")
def reference():
    """Computed once, from the oracle alone: the frames the kernels must reproduce, and proof that these inputs reach the step's
    environment branches and its depth bound (else the comparison below would pass without running them)."""
    from radish_pt_amd import scenes

    cam = scenes.cornell_camera(W, H)
    sd = scenes.cornell_textured(segments=12, bands=8, env=True)
    ref = {depth: _oracle_frames(sd, cam, depth) for depth in DEPTHS}
    no_env = scenes.cornell_textured(segments=12, bands=8, env=False)
    for depth in DEPTHS:
        d, i, _ = ref[depth]
        assert d.max() > 0 and i.max() > 0
        assert np.any(i != _oracle_frames(no_env, cam, depth)[1], axis=1).sum() > 0, f"the environment adds nothing at depth {depth}"
    assert np.any(ref[1][1] != ref[3][1], axis=1).sum() > 0, "the depth bound cuts nothing"
    return sd, cam, ref


@pytest.fixture(scope="module")
def textured_gpu(gpu_ctx, reference):
    sd, cam, _ = reference
    gpu_ctx.set_partition(0, 1, 64)
    gpu_ctx.upload_scene(sd)
    gpu_ctx.set_camera(cam)
    return gpu_ctx


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("flags_name", ["mega", "wavefront", "wavefront_sort", "persistent", "persistent_threaded", "wavefront_threaded", "auto"])
def test_path_step_bit_exact(textured_gpu, reference, flags_name, depth):
    import torch

    from radish_pt_amd import api

    flags = {"mega": api.RDH_PT_MEGAKERNEL, "wavefront": api.RDH_PT_WAVEFRONT,
             "wavefront_sort": api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL,
             "persistent": api.RDH_PT_PERSISTENT,
             "persistent_threaded": api.RDH_PT_PERSISTENT | api.RDH_PT_NO_PAIRS,
             "wavefront_threaded": api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_NO_PAIRS,
             "auto": api.RDH_PT_AUTO}[flags_name] | api.RDH_PT_COUNT
    ref_d, ref_i, stats = reference[2][depth]
    d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
    textured_gpu.counters_reset()
    for it, looper in ITERS:
        textured_gpu.path_trace(d, i, it, looper, depth, flags)
    assert_bit_equal(d.cpu().numpy(), ref_d, f"{flags_name} direct, depth {depth}")
    assert_bit_equal(i.cpu().numpy(), ref_i, f"{flags_name} indirect, depth {depth}")
    ct = textured_gpu.counters()
    for key in COUNTERS:
        assert ct[key] == stats[key], (flags_name, depth, key)
