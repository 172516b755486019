"""The oracle's G-buffer and two-pass ReSTIR DI against tests/restir_model.py, a float64 statement of the same rules written from
the reference text in another form — per frame, per step and per pixel, under a moving camera.  The oracle and the device code
are one author's two restatements of the reference and agree bit for bit; what this closes is a misreading the two share in the
rules that decide WHICH pixels exchange samples: findTemporalNeighbor, findSpatialNeighborDisk, the conditional Sobol draws, the
two stores, the planes of renderGBuffer.  (tests/test_gpu_restir_model.py holds the HIP kernels to the same model.)

Figures on this scene (the oracle's; the GPU test asserts that the kernels' are the same sets).  Pixels left out per frame, of 1665
with a cap of 6 — all in pass 1, none in any G-buffer or pass-2 step; each is a component of `wi` below the tolerance's floor of
1e-3, where binary32's absolute rounding of the hit position exceeds 2e-4 * 1e-3:

    reference's update, every reuse mask:   frame 0 {373, 980}     frame 1 {}          frame 2 {}           frame 3 {169}
    corrected update, reuse 0 and 2:        frame 0 {1336, 1349}   frame 1 {304, 516}  frame 2 {167, 1270}  frame 3 {169, 290, 482}
    corrected update, reuse 1 and 3:        frame 0 {1336, 1349}   frame 1 {516}       frame 2 {}           frame 3 {169}
"""
import numpy as np
import pytest

import restir_model as M
import restir_model_checks as C


@pytest.fixture(scope="module")
def setup():
    sd = C.build_scene()
    return sd, M.ModelScene(sd), C.cameras()


@pytest.fixture(scope="module")
def liveness(setup):
    """How often each rule decides, from the model alone with its own state carried forward (reuse 3, the reference's update).
    Each threshold is about half of what the scene gives; the counts are in the comments, frames 0-2 summed unless noted.
    A comparison that passes because a branch never ran is what this prevents."""
    _, ms, cams = setup
    per_frame = C.model_only_counts(ms, cams, 3, 1)
    nat = {k: sum(c.get(k, 0) for c in per_frame[:C.SEEDED_FRAME]) for k in per_frame[-1]}
    seeded = per_frame[C.SEEDED_FRAME]
    floor = {
        # renderGBuffer
        "gb_miss": 500, "gb_emitter": 48, "gb_motion_off_frame": 35, "gb_motion_moved": 1250,          # 1017, 96, 70, 2515
        # pass 1
        "early_miss": 500, "early_emitter": 39, "flipped": 22, "shadowed": 250, "metallic": 145,       # 1022, 78, 45, 498, 292
        "temporal_off_frame": 34, "temporal_null_id": 12, "temporal_changed_id": 50,                   # 69, 24, 103
        "temporal_normal": 16, "temporal_accepted": 1150, "unclamped": 1150,                           # 32, 2360, 2360
        # pass 2
        "spatial_left": 30, "spatial_right": 180, "spatial_top": 100, "spatial_bottom": 345,           # 62, 366, 208, 691
        "spatial_self": 135, "spatial_other_id": 2000, "spatial_normal": 900, "spatial_depth": 900,    # 277, 4038, 1823, 1879
        "spatial_normal_reversed": 160,  # 321: the plain dot rejects a reversed normal that |dot| would accept
        "spatial_accepted": 5000, "spatial_zero_from_negative": 95, "final_merged": 1900,              # 10544, 193, 3895
    }
    for k, least in floor.items():
        assert nat[k] >= least, (k, nat[k], least)
    # |dot| accepts a reversed normal in the temporal test: 5 pixels in frames 0-2 and 6 in frame 3
    assert nat["temporal_accepted_reversed"] + seeded["temporal_accepted_reversed"] >= 5
    # Reachable only from the seeded last-frame reservoirs of frame 3 (restir_model_checks.seed_last says why): the pre-clamp, a
    # skipped temporal merge — whose pixel then starts its spatial draws one dimension before a neighbour — and a final merge
    # skipped because the spatial aggregate is invalid.
    for k, least in {"clamped": 88, "unclamped": 330, "temporal_skipped": 130, "spatial_draws_one_dim_early": 130,  # 177, 676, 268, 268
                     "final_skipped_agg_invalid": 100}.items():                                                      # 216
        assert seeded[k] >= least, (k, seeded[k], least)
        assert k == "unclamped" or nat[k] == 0, k
    # Unreachable by any input, and asserted so: `reservoir.checkValidity()` (restir.cu:176) directly precedes the final merge's
    # `!reservoir.invalid()` (:182), so that test cannot fail; and a weight turns invalid in pass 1 only by a sum of finite
    # non-negative terms overflowing binary32 (candidates are scrubbed one by one at :152, an invalid temporal neighbour is not
    # merged, the clamp only scales down), which needs a term near 1e31.  checkValidity therefore clears nothing, and no
    # stored neighbour is invalid.
    for k in ("final_skipped_own_invalid", "cleared_out", "cleared_temp", "spatial_neighbour_invalid"):
        assert all(c.get(k, 0) == 0 for c in per_frame), k
    return per_frame


@pytest.fixture(scope="module", params=[(r, f) for f in (1, 0) for r in (0, 1, 2, 3)], ids=lambda p: f"reuse{p[0]}-faithful{p[1]}")
def oracle_frames(request, setup):
    sd, _, cams = setup
    return request.param + (C.run_oracle(sd, cams, *request.param),)


@pytest.mark.parametrize("f", range(4))
def test_oracle_vs_model(setup, liveness, oracle_frames, f):
    """Frames 0-2 from the zeroed buffers; frame 3 from seeded last-frame reservoirs.  Per step: the G-buffer's id and motion planes
    exactly and its normal, depth and albedo within 2e-4 relative (floor 1e-3); reservoirOut and reservoirTemp with numSamples
    exactly and weight, Li, wi, dist within the same, untouched where the pixel returned early; the image within the same.
    At most 6 of the 1665 pixels per step may differ (a ray classified differently at a quad's border, a tie)."""
    _, ms, cams = setup
    reuse, faithful, frames = oracle_frames
    ex, p1, _ = C.check_frame(ms, f, cams, reuse, faithful, frames[f])
    print({k: v.tolist() for k, v in ex.items()})
    C.assert_within_cap(ex, f"oracle, reuse {reuse}, faithful {faithful}, frame {f}")
    assert frames[f]["image"].max() > 0 and p1["stored"].sum() > 1000


def test_model_reads_no_device_code_and_calls_no_oracle_entry():
    import ast
    import inspect

    tree = ast.parse(inspect.getsource(M))
    names = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name)} | {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute)}
    mods = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names} | \
           {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert mods == {"numpy", "test_oracle_float64", "test_oracle_kat"}, mods
    assert not {n for n in names if n.startswith("orc_")} and "pyoracle" not in names and "lib" not in names
