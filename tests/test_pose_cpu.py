"""Objects and their rest pose on the host (rdh_object_transform, rdh_scene_parse_objects), CPU only.

The scene file is pose_scene's: three OBJ meshes, six Object blocks.  What pins the device kernel to the loader is checked here on
the host side: pose_model (the kernel's four expression lines in numpy float32) applied to the rest pose the parser returns, with
hostlib.object_transform of each object's own Translate / Rotate / Scale, gives the parsed vertices and normals bit for bit."""
import numpy as np
import pytest

import pose_model
import pose_scene
from helpers import assert_bit_equal

F = np.float32


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from radish_pt_amd import hostlib

    d = str(tmp_path_factory.mktemp("pose_scene"))
    pose_scene.write_meshes(d)
    return d, hostlib.parse_scene(pose_scene.write_scene(d, "scene.txt"))


def test_objects_tile_the_scene_in_file_order(scene):
    _, p = scene
    objs = p["objects"]
    assert len(objs) == 6
    sizes = [pose_scene.MESH_PRIMS[o[0]] for o in pose_scene.OBJECTS]
    assert objs["numPrims"].tolist() == sizes == [200, 21, 1, 200, 21, 200]
    assert objs["firstPrim"].tolist() == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    assert int(objs["firstPrim"][-1] + objs["numPrims"][-1]) == len(p["material_ids"]) == 643
    # rest ranges in order of first use: rev 0..200, cone 200..221, tri 221..222; instances share them
    assert objs["restFirstPrim"].tolist() == [0, 200, 221, 0, 200, 0]
    assert p["rest_vertices"].shape == p["rest_normals"].shape == (3 * 222, 3)
    for o, (_, _, t, r, s) in zip(objs, pose_scene.OBJECTS):
        assert o["translate"].tolist() == list(t) and o["rotate"].tolist() == list(r) and o["scale"].tolist() == list(s)
        first = int(o["firstPrim"])
        assert (p["material_ids"][first:first + int(o["numPrims"])] == o["materialId"]).all()
    assert p["materials"]["type"][objs["materialId"][4]] == 4  # the emissive object


def test_rest_pose_is_the_meshes_own_floats(scene):
    """The identity object (explicit zeros and ones) is the rest pose itself, and an instance's rest range is the mesh as written."""
    _, p = scene
    o = p["objects"][2]
    a, r = 3 * int(o["firstPrim"]), 3 * int(o["restFirstPrim"])
    assert_bit_equal(p["vertices"][a:a + 3], p["rest_vertices"][r:r + 3], "identity object")
    assert np.array_equal(p["rest_vertices"][r:r + 3], np.array([[-9, 0, -9], [0, 0, 11], [9, 0, -9]], F))
    assert np.array_equal(p["rest_normals"][r:r + 3], np.array([[0, 1, 0]] * 3, F))
    assert np.array_equal(p["rest_vertices"][3 * 200], np.array([0, 0.5, 0], F))  # cone.obj's apex: `f 1//1 ...`


def test_model_on_rest_pose_equals_the_loader(scene):
    from radish_pt_amd import hostlib

    _, p = scene
    objs = p["objects"]
    xf = np.stack([hostlib.object_transform(o["translate"], o["rotate"], o["scale"]) for o in objs])
    v, n = pose_model.pose(p["rest_vertices"], p["rest_normals"], objs, xf)
    assert_bit_equal(v, p["vertices"], "vertices")
    assert_bit_equal(n, p["normals"], "normals")
    dets = [np.linalg.det(x[:16].reshape(4, 4).astype(np.float64)) for x in xf]
    assert dets[3] < 0 and all(d > 0 for k, d in enumerate(dets) if k != 3)  # the mirrored object is the mirrored one
    assert np.array_equal(xf[2], np.concatenate([np.eye(4, dtype=F).reshape(-1)] * 2))  # zeros and ones: the identity, exactly
    # and for the second file, which carries the TRS rows the GPU tests pose to
    d, _ = scene
    q = hostlib.parse_scene(pose_scene.write_scene(d, "posed.txt", pose_scene.POSED))
    assert np.array_equal(q["objects"][["firstPrim", "numPrims", "restFirstPrim"]], objs[["firstPrim", "numPrims", "restFirstPrim"]])
    assert_bit_equal(q["rest_vertices"], p["rest_vertices"], "rest pose of the second file")
    v2, n2 = pose_model.pose(p["rest_vertices"], p["rest_normals"], objs, pose_scene.xforms(pose_scene.POSED))
    assert_bit_equal(v2, q["vertices"], "posed vertices")
    assert_bit_equal(n2, q["normals"], "posed normals")
    assert not np.array_equal(v2, v)


def test_object_transform_equals_hand_written_matrices():
    from radish_pt_amd import hostlib

    x = hostlib.object_transform((1.5, -2.0, 0.25), (0, 0, 0), (1, 1, 1))
    T = np.eye(4, dtype=F)
    T[3, :3] = (1.5, -2.0, 0.25)  # [col][row]: the translation is column 3
    Ti = np.eye(4, dtype=F)
    Ti[3, :3] = (-1.5, 2.0, -0.25)
    assert np.array_equal(x[:16].reshape(4, 4), T) and np.array_equal(x[16:].reshape(4, 4), Ti)
    # 90 degrees about z: x -> y, y -> -x.  cosf(pi/2 in float32) is not 0 but -4.371139e-08, and it stays in the matrix
    r = hostlib.object_transform((0, 0, 0), (0, 0, 90), (1, 1, 1))
    c = F(np.cos(np.float64(F(90.0) * F(3.1415926535897932) / F(180.0))))
    R = np.eye(4, dtype=F)
    R[0, :2] = (c, 1.0)
    R[1, :2] = (-1.0, c)
    assert np.array_equal(r[:16].reshape(4, 4), R), r[:16].reshape(4, 4)
    assert np.allclose(r[16:].reshape(4, 4), R.T, atol=1e-7)
    v, n = pose_model.transform(np.array([[1, 0, 0], [0, 2, 0]], F), np.array([[1, 0, 0], [0, 1, 0]], F), r)
    assert np.allclose(v, [[0, 1, 0], [-2, 0, 0]], atol=1e-6) and np.allclose(n, [[0, 1, 0], [-1, 0, 0]], atol=1e-6)


def test_singular_scale_is_refused():
    import ctypes as C

    from radish_pt_amd import hostlib

    with pytest.raises(ValueError):
        hostlib.object_transform((0, 0, 0), (0, 0, 0), (0, 1, 1))
    out = np.ones(32, F)
    a = [np.array(v, F) for v in ((0, 0, 0), (0, 0, 0), (0, 1, 1))]
    rc = hostlib.lib().rdh_object_transform(*[C.c_void_p(x.ctypes.data) for x in a], C.c_void_p(out.ctypes.data))
    assert rc == -1  # RDH_HOST_ERR_ARGS
    assert hostlib.lib().rdh_object_transform(None, None, None, None) == -1


def test_skipped_model_yields_no_object(scene):
    from radish_pt_amd import hostlib, scenes

    d, p = scene
    extra = pose_scene.object_block(6, "missing.obj", "steel", (9, 9, 9), (0, 0, 0), (1, 1, 1)) + \
        pose_scene.object_block(7, "tri.obj", "green", (0, 1, 0), (0, 0, 0), (2, 2, 2))
    q = hostlib.parse_scene(pose_scene.write_scene(d, "skipped.txt", extra_objects=extra))
    assert len(q["objects"]) == 7  # six + the second ground triangle; missing.obj left nothing
    last = q["objects"][-1]
    assert (int(last["firstPrim"]), int(last["numPrims"]), int(last["restFirstPrim"])) == (643, 1, 221)
    assert len(q["material_ids"]) == 644 and len(q["rest_vertices"]) == 3 * 222
    # load_scene_file hands the table on; procedural scenes have none
    sd, _, _ = scenes.load_scene_file(pose_scene.write_scene(d, "scene.txt"))
    assert np.array_equal(sd.objects, p["objects"]) and np.array_equal(sd.rest_vertices, p["rest_vertices"])
    assert np.array_equal(sd.rest_normals, p["rest_normals"])
    assert scenes.tiny().objects is None
