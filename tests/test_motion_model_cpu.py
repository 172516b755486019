"""motion_model.py against the oracle, before any GPU sees it (rdh_scene_track_motion).

With equal previous and current vertices the model must give the oracle's own motion plane at every pixel, and its depth the
oracle's depth plane bit for bit: that pins the primary ray, the interpolation and the projection.  Hand values pin the sign and
the size of a known motion.  The last test shows that the moving scene of test_gpu_motion.py can fail: on the model alone, most of
the moved object's pixels get another index with tracking than without."""
import numpy as np
import pytest

import motion_model
from helpers import assert_bit_equal


def _oracle_planes(o, cam, last_cam, W, H):
    from oracle import pyoracle

    gb = pyoracle.GBufferHost(W, H)
    gb.lastCam = last_cam.copy()
    o.gbuffer_render(cam, gb)
    return gb


@pytest.mark.parametrize("size", [(151, 91), (64, 48)])
@pytest.mark.parametrize("literal", [False, True])
def test_model_equals_oracle_when_nothing_moved(cornell_small, size, literal):
    from oracle import pyoracle

    W, H = size
    o = pyoracle.OracleScene(cornell_small)
    cams = motion_model.moving_cameras(W, H, frames=3, literal=literal)
    for last_cam, cam in ((cams[0], cams[0]), (cams[0], cams[1]), (cams[1], cams[2])):
        gb = _oracle_planes(o, cam, last_cam, W, H)
        _, _, hits = motion_model.trace(o, cam)
        assert np.array_equal(hits["primId"] >= 0, gb.primId[0] != -1), "the model's rays hit other pixels than the oracle's"
        v = cornell_small.vertices
        motion = motion_model.motion_plane(o, v, v, cam, last_cam, hits)
        bad = np.flatnonzero(motion != gb.motion)
        assert len(bad) == 0, f"{len(bad)} pixels differ, first {bad[:4].tolist()}: {motion[bad[:4]].tolist()} vs {gb.motion[bad[:4]].tolist()}"
        assert_bit_equal(motion_model.depth_plane(o, v, cam, hits), gb.depth[0], "depth")
        assert (gb.primId[0] != -1).mean() > 0.05, "the camera sees too little of the scene for the comparison to mean anything"


def _one_triangle(shift):
    """A triangle that covers the whole view of a camera at (0, 0, 5) looking down -z, moved by `shift` in world units."""
    from radish_pt_amd import scenes

    base = scenes.tiny()
    v = np.array([[-400.0, -300.0, 0.0], [400.0, -300.0, 0.0], [0.0, 500.0, 0.0]], np.float32) + np.asarray(shift, np.float32)
    return scenes.SceneData("one", v, np.tile(base.normals[:3], (1, 1)), np.tile(base.texcoords[:3], (1, 1)),
                            np.full(1, base.material_ids[0], np.int32), base.materials)


@pytest.mark.parametrize("kx,ky", [(3, 0), (0, 2), (-4, 5), (100, 0), (0, -100)])
def test_hand_values(kx, ky):
    """The camera looks at a plane 5 units away; one pixel is 2 * 5 * tanFovY / H world units there.  A surface that moved by
    kx pixels' worth along the camera's right vector appears kx pixels to the LEFT (the raster x runs against `right`), so the
    point under the centre of pixel (x, y) was at raster position (x + kx + 0.5, y + ky + 0.5) last frame.  The index rule
    converts towards zero, as the reference's cast does: raster positions in (-1, 0) land in pixel 0 rather than outside.
    Farther out the point was out of frame (-1)."""
    from oracle import pyoracle
    from radish_pt_amd import hostlib

    W, H = 64, 48
    cam = hostlib.make_camera(W, H, eye=(0.0, 0.0, 5.0), rotation=(-90.0, 0.0, 0.0), fovy=20.0)
    right, up, view = (np.asarray(cam[k], np.float64) for k in ("right", "up", "view"))
    assert abs(view[2] + 1.0) < 1e-6 and abs(abs(right[0]) - 1.0) < 1e-6 and abs(abs(up[1]) - 1.0) < 1e-6, (right, up, view)
    pixel = 2.0 * 5.0 * float(motion_model.device_camera(cam)["tanFovY"]) / H
    shift = pixel * (kx * right + ky * up)
    prev, cur = _one_triangle((0, 0, 0)), _one_triangle(shift)
    o = pyoracle.OracleScene(cur)
    motion = motion_model.motion_plane(o, cur.vertices, prev.vertices, cam, cam).reshape(H, W)
    y, x = np.mgrid[0:H, 0:W]
    lx, ly = np.trunc(x + kx + 0.5).astype(int), np.trunc(y + ky + 0.5).astype(int)
    want = np.where((lx >= 0) & (lx < W) & (ly >= 0) & (ly < H), ly * W + lx, -1)
    assert np.array_equal(motion, want), np.argwhere(motion != want)[:4].tolist()
    static = motion_model.motion_plane(o, cur.vertices, cur.vertices, cam, cam).reshape(H, W)
    assert np.array_equal(static, y * W + x), "an unmoved point under an unmoved camera stays in its pixel"


@pytest.mark.parametrize("literal", [False, True])
def test_moving_scene_can_tell_tracking_from_none(cornell_small, literal):
    """The deformation of test_gpu_motion.py, on the model alone: on every frame at least a fifth of the moved object's pixels
    get a tracked index that differs from the untracked one (in fact most do)."""
    from oracle import pyoracle

    W, H = 151, 91
    cams = motion_model.moving_cameras(W, H, literal=literal)
    prev, last_cam = cornell_small, cams[0]
    for f, cam in enumerate(cams):
        cur = motion_model.deformed(cornell_small, f + 1)
        o = pyoracle.OracleScene(cur)
        _, _, hits = motion_model.trace(o, cam)
        tracked = motion_model.motion_plane(o, cur.vertices, prev.vertices, cam, last_cam, hits)
        untracked = motion_model.motion_plane(o, cur.vertices, cur.vertices, cam, last_cam, hits)
        moved = (hits["primId"] >= 0) & (cur.material_ids[np.where(hits["primId"] >= 0, hits["primId"], 0)] == motion_model.MOVED_MATERIAL)
        assert moved.sum() >= (30 if literal else 150), f"frame {f}: the moved object covers {moved.sum()} pixels"
        assert np.array_equal(tracked[~moved], untracked[~moved]), "pixels of unmoved triangles must not change"
        share = (tracked[moved] != untracked[moved]).mean()
        print(f"frame {f} literal={literal}: {moved.sum()} moved pixels, {share:.2f} with another index")
        assert share >= 0.2
        prev, last_cam = cur, cam
