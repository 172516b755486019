"""The HIP G-buffer and ReSTIR DI kernels against tests/restir_model.py, the float64 statement of the reference's rules — directly,
step by step and pixel by pixel, not by way of the oracle agreeing with both.  Scene, sequence, tolerance and cap are those of
tests/test_restir_model_cpu.py (tests/restir_model_checks.py holds them): frames 0-2 from the zeroed buffers under a moving camera,
frame 3 from seeded last-frame reservoirs, every reuse mask, both `update` rules, and every kernel structure of pass 1 (split,
fused, lane by lane) and of the G-buffer (packets, packets with a budget of 4 visits, persistent, one lane per pixel).

Each step of the model runs on the kernels' OWN earlier state: the `api.GBuffer` planes, `restir_read(1)` before the frame (last
frame's reservoirs), `restir_read(2)` after it (reservoirTemp).  The pixels left out under the cap must be the very pixels the
oracle's run leaves out, the two being bit-identical."""
import numpy as np
import pytest

import restir_model as M
import restir_model_checks as C

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def setup():
    sd = C.build_scene()
    return {"sd": sd, "ms": M.ModelScene(sd), "cams": C.cameras(), "oracle": {}}


def _oracle_excluded(setup, reuse, faithful):
    """Per frame, the pixels the ORACLE's run leaves out per step (computed once per case on the CPU)."""
    key = (reuse, faithful)
    if key not in setup["oracle"]:
        frames = C.run_oracle(setup["sd"], setup["cams"], reuse, faithful)
        setup["oracle"][key] = [C.check_frame(setup["ms"], f, setup["cams"], reuse, faithful, t)[0] for f, t in enumerate(frames)]
    return setup["oracle"][key]


def _planes(gb, half):
    return {"albedo": gb.albedo.cpu().numpy(), "normal": gb.normal[half].cpu().numpy(), "primId": gb.primId[half].cpu().numpy(),
            "depth": gb.depth[half].cpu().numpy(), "motion": gb.motion.cpu().numpy()}


def _write_last_reservoirs(ctx, rec):
    """Last frame's reservoirs <- rec, through the reservoir exchange's receive side (one rank, one 64x64 tile: the gathered
    buffer is the tile's records, 9 words each, row by row)."""
    torch = _torch()
    assert (ctx.world, ctx.tile, ctx.tiles_per_rank()) == (1, 64, 1) and C.W <= 64 and C.H <= 64
    tile = np.zeros((64, 64, 9), np.float32)
    tile[:C.H, :C.W] = np.ascontiguousarray(rec).view(np.float32).reshape(C.H, C.W, 9)
    gathered = torch.from_numpy(tile.reshape(-1, 9)).cuda()
    torch.cuda.synchronize()
    ctx.restir_exchange_unpack(gathered)
    ctx.synchronize()
    assert ctx.restir_read(1).tobytes() == rec.tobytes()


def _run_gpu(ctx, setup, reuse, faithful, restir_flags, gbuffer_flags=0, restir=True):
    """The frames as check_frame reads them, from Context.gbuffer_render / api.GBuffer and Context.restir_direct."""
    from radish_pt_amd import api

    torch = _torch()
    cams = setup["cams"]
    w, h = (int(v) for v in cams[0]["resolution"])  # tests/test_gpu_path_model.py drives its own scene and size through here
    ctx.set_partition(0, 1, 64)
    ctx.upload_scene(setup["sd"])
    ctx.set_camera(cams[0])
    gb = api.GBuffer()
    gb.create(w, h)
    img = torch.zeros(w * h, 3, device="cuda")
    if restir:
        ctx.restir_init()
    frames = []
    try:
        for f, cam in enumerate(cams):
            ctx.set_camera(cam)
            ctx.gbuffer_render(gb.c_struct(cam_fallback=cam), gbuffer_flags)
            ctx.synchronize()
            t = {"planes": _planes(gb, gb.frameIdx), "last_planes": _planes(gb, gb.frameIdx ^ 1)}
            if restir:
                if f == C.SEEDED_FRAME:
                    _write_last_reservoirs(ctx, C.seed_last(ctx.restir_read(1)))
                t.update(last=ctx.restir_read(1), prior_out=ctx.restir_read(0), prior_temp=ctx.restir_read(2), image_in=img.cpu().numpy())
                ctx.restir_direct(img, f, C.LOOPERS[f], gb.c_struct(cam), reuse, faithful_ris=faithful, flags=restir_flags)
                ctx.synchronize()
                t.update(out=ctx.restir_read(1), temp=ctx.restir_read(2), image=img.cpu().numpy())  # read after the swap
            frames.append(t)
            gb.update(cam)
    finally:
        if restir:
            ctx.restir_free()
        gb.destroy()
    return frames


@pytest.mark.parametrize("structure", ["split", "fused", "no_packets"])
@pytest.mark.parametrize("reuse", [0, 1, 2, 3])
@pytest.mark.parametrize("faithful", [1, 0])
def test_restir_kernels_vs_model(gpu_ctx, setup, faithful, reuse, structure):
    from radish_pt_amd import api

    flags = {"split": 0, "fused": api.RDH_PT_RESTIR_FUSED, "no_packets": api.RDH_PT_NO_PACKETS}[structure]
    want = _oracle_excluded(setup, reuse, faithful)
    frames = _run_gpu(gpu_ctx, setup, reuse, faithful, flags)
    for f, t in enumerate(frames):
        ex, p1, _ = C.check_frame(setup["ms"], f, setup["cams"], reuse, faithful, t)
        what = f"{structure}, reuse {reuse}, faithful {faithful}, frame {f}"
        print(what, {k: v.tolist() for k, v in ex.items()})
        C.assert_within_cap(ex, what)
        for step in ex:
            assert ex[step].tolist() == want[f][step].tolist(), f"{what}, {step}: not the pixels the oracle's run leaves out"
        assert t["image"].max() > 0 and p1["stored"].sum() > 1000


@pytest.mark.parametrize("kernel", ["packets", "packets_budget_4", "persistent", "one_lane_per_pixel"])
def test_gbuffer_kernels_vs_model(gpu_ctx, setup, kernel):
    """The planes of every G-buffer kernel over the four cameras: id and motion exactly, normal, depth, albedo within the tolerance."""
    from radish_pt_amd import api

    flags = {"one_lane_per_pixel": api.RDH_PT_MEGA_GBUFFER, "persistent": api.RDH_PT_NO_PACKETS, "packets": 0,
             "packets_budget_4": api.RDH_PT_WF_SMALL_LISTS}[kernel]
    want = _oracle_excluded(setup, 0, 1)
    frames = _run_gpu(gpu_ctx, setup, 0, 1, 0, gbuffer_flags=flags, restir=False)
    for f, t in enumerate(frames):
        gb = M.gbuffer(setup["ms"], setup["cams"][f], setup["cams"][f - 1] if f else None)
        bad = np.flatnonzero(C.gbuffer_bad(gb, t["planes"]))
        assert len(bad) <= C.CAP, f"{kernel}, frame {f}: {len(bad)} pixels differ from the float64 model; first {bad[:12]}"
        assert bad.tolist() == want[f]["gbuffer"].tolist()
        assert (t["planes"]["primId"] >= 0).mean() > 0.5 and (t["planes"]["primId"] == -2).sum() > 5
