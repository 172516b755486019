"""numpy float32 restatement of k_pose_objects (kernels_pose.h) and of the loop at the end of the loader's loadModel
(csrc/host/scene_load.cpp), shared by test_pose_cpu.py and test_gpu_pose.py.

The four expression lines, elementwise and in the order written; numpy's float32 mul / add / div / sqrt are IEEE binary32
operations and are never contracted (the library's numerics contract):

    w[r]  = X[0][r]*p.x + X[1][r]*p.y + X[2][r]*p.z + X[3][r]*1.0f
    nn[r] = Xi[r][0]*n.x + Xi[r][1]*n.y + Xi[r][2]*n.z
    inv   = 1.f / sqrtf((nn0*nn0 + nn1*nn1) + nn2*nn2)
    n'    = nn*inv

xforms32 rows are hostlib.object_transform's: X column-major ([col][row] at 4*col + row), then inverse(X) likewise."""
import numpy as np

F = np.float32


def transform(p, n, xform32):
    """p, n: float32 [k, 3] object-space vertices and normals -> their world-space images under one transform."""
    X = np.asarray(xform32, F)[:16].reshape(4, 4)   # X[col][row]
    Xi = np.asarray(xform32, F)[16:].reshape(4, 4)
    p, n = np.asarray(p, F), np.asarray(n, F)
    with np.errstate(all="ignore"):
        w = [((X[0][r] * p[:, 0] + X[1][r] * p[:, 1]) + X[2][r] * p[:, 2]) + X[3][r] * F(1.0) for r in range(3)]
        nn = [(Xi[r][0] * n[:, 0] + Xi[r][1] * n[:, 1]) + Xi[r][2] * n[:, 2] for r in range(3)]
        inv = F(1.0) / np.sqrt((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2])
        out_n = [nn[r] * inv for r in range(3)]
    return np.stack(w, axis=1).astype(F), np.stack(out_n, axis=1).astype(F)


def pose(rest_vertices, rest_normals, objects, xforms32, ids=None, world=None):
    """World vertices and normals ([3N, 3] float32 each) after posing objects `ids` (default: all, in table order) with the rows of
    xforms32.  objects: records with firstPrim / numPrims / restFirstPrim.  world: the (vertices, normals) the pose starts from —
    needed when `ids` leaves triangles out; without it the arrays span exactly the triangles the table covers and start as zeros."""
    rv = np.asarray(rest_vertices, F).reshape(-1, 3)
    rn = np.asarray(rest_normals, F).reshape(-1, 3)
    ids = list(range(len(objects))) if ids is None else [int(i) for i in ids]
    xf = np.asarray(xforms32, F).reshape(-1, 32)
    assert len(xf) == len(ids)
    if world is None:
        total = max(int(o["firstPrim"]) + int(o["numPrims"]) for o in objects)
        v, n = np.zeros((3 * total, 3), F), np.zeros((3 * total, 3), F)
    else:
        v, n = np.array(world[0], F).reshape(-1, 3).copy(), np.array(world[1], F).reshape(-1, 3).copy()
    for j, i in enumerate(ids):
        o = objects[i]
        a, k, r = 3 * int(o["firstPrim"]), 3 * int(o["numPrims"]), 3 * int(o["restFirstPrim"])
        v[a:a + k], n[a:a + k] = transform(rv[r:r + k], rn[r:r + k], xf[j])
    return v, n
