"""The scene file of the pose tests (test_pose_cpu.py, test_gpu_pose.py): three small OBJ meshes and six Object blocks, written
into a directory in the grammar the loader accepts (as tests/test_scene_loader.py does).

Meshes: tri.obj (1 triangle, the ground), cone.obj (21 triangles: a cone's side, one triangle per segment, with vertex normals)
and rev.obj (a revolved profile of 10 segments x 10 bands = 200 triangles, with normals and texcoords).  cone.obj is instanced
twice and rev.obj three times; object 4 is emissive.  The transforms cover a pure translation, a three-axis rotation, explicit
zeros and ones (the identity), a mirrored scale (negative determinant) and non-uniform scale plus rotation."""
import os

import numpy as np

F = np.float32

# (mesh, material, translate, rotate in degrees, scale) in file order
OBJECTS = [
    ("rev.obj", "red", (-1.25, 0.0, 0.5), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),          # pure translation
    ("cone.obj", "steel", (0.25, 0.75, -0.5), (25.0, 40.0, -15.0), (1.0, 1.0, 1.0)),  # three-axis rotation
    ("tri.obj", "white", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),          # explicit zeros and ones
    ("rev.obj", "glass", (1.5, 0.0, 0.25), (0.0, 30.0, 0.0), (-1.0, 1.25, 0.75)),     # mirrored: negative determinant
    ("cone.obj", "lamp", (0.0, 2.5, 0.5), (180.0, 10.0, 0.0), (1.5, 0.5, 1.25)),      # emissive; non-uniform scale + rotation
    ("rev.obj", "green", (0.0, 0.0, -1.75), (10.0, -35.0, 5.0), (0.5, 1.5, 0.75)),    # non-uniform scale + rotation
]
MESH_PRIMS = {"tri.obj": 1, "cone.obj": 21, "rev.obj": 200}
# TRS rows the tests pose the six objects to (every one differs from OBJECTS)
POSED = [
    ((-1.0, 0.25, 0.75), (0.0, 20.0, 0.0), (1.0, 1.0, 1.0)),
    ((0.5, 1.0, -0.25), (-35.0, 10.0, 50.0), (1.25, 1.25, 1.25)),
    ((0.125, -0.0625, 0.0), (0.0, 3.0, 0.0), (1.0, 1.0, 1.0)),
    ((1.25, 0.125, 0.5), (5.0, -45.0, 0.0), (0.75, 1.0, -1.0)),
    ((0.25, 2.25, 0.25), (170.0, 0.0, 15.0), (1.0, 0.75, 1.5)),
    ((-0.25, 0.0, -1.5), (0.0, 60.0, -10.0), (0.75, 1.0, 0.5)),
]

MATERIALS = """Material white
Type Lambertian
BaseColor 0.73 0.73 0.73
Metallic 0
Roughness 1
Ior 1.5
NormalMap Null

Material red
Type Lambertian
BaseColor 0.63 0.065 0.05
Metallic 0
Roughness 1
Ior 1.5
NormalMap Null

Material green
Type Lambertian
BaseColor 0.14 0.45 0.091
Metallic 0
Roughness 1
Ior 1.5
NormalMap Null

Material steel
Type MetallicWorkflow
BaseColor 0.9 0.8 0.7
Metallic 1
Roughness 0.3
Ior 1.5
NormalMap Null

Material glass
Type Dielectric
BaseColor 1 1 1
Metallic 0
Roughness 0
Ior 1.5
NormalMap Null

Material lamp
Type Light
BaseColor 12 10 8
Metallic 0
Roughness 1
Ior 1
NormalMap Null

"""

CAMERA = """Camera
Resolution 64 48
FovY 20
LensRadius 0.0
FocalDist 5
ApertureMask Null
Sample 1
Depth 3
File pose_out
Eye 0.2 1.6 5
Rotation -92 -12 0
Up 0 1 0
"""


def _fmt(x):
    return "%.9g" % float(F(x))  # nine digits: strtof gives the float32 back


def tri_obj():
    return "v -9 0 -9\nv 0 0 11\nv 9 0 -9\nvn 0 1 0\nf 1//1 2//1 3//1\n"


def cone_obj(segments=21):
    lines = ["v 0 0.5 0"]
    for s in range(segments):
        a = 2.0 * np.pi * s / segments
        lines.append(f"v {_fmt(0.4 * np.cos(a))} 0 {_fmt(0.4 * np.sin(a))}")
    for s in range(segments):  # one normal per rim vertex, tilted outwards; the apex takes the normal of its triangle's first rim vertex
        a = 2.0 * np.pi * s / segments
        lines.append(f"vn {_fmt(0.8 * np.cos(a))} 0.6 {_fmt(0.8 * np.sin(a))}")
    for s in range(segments):
        i, j = 2 + s, 2 + (s + 1) % segments
        lines.append(f"f 1//{1 + s} {j}//{1 + (s + 1) % segments} {i}//{1 + s}")
    return "\n".join(lines) + "\n"


def rev_obj(segments=10, bands=10):
    """A vase: radius 0.3 + 0.12 sin(3 h) over height 0..0.9, open at both ends."""
    lines, idx = [], {}
    for b in range(bands + 1):
        h = 0.9 * b / bands
        r = 0.3 + 0.12 * np.sin(3.0 * h / 0.9 * 2.0)
        dr = 0.12 * np.cos(3.0 * h / 0.9 * 2.0) * 6.0 / 0.9
        for s in range(segments):
            a = 2.0 * np.pi * s / segments
            idx[(b, s)] = len(idx) + 1
            lines.append(f"v {_fmt(r * np.cos(a))} {_fmt(h)} {_fmt(r * np.sin(a))}")
            nrm = np.array([np.cos(a), -dr, np.sin(a)])
            nrm /= np.linalg.norm(nrm)
            lines.append(f"vn {_fmt(nrm[0])} {_fmt(nrm[1])} {_fmt(nrm[2])}")
            lines.append(f"vt {_fmt(s / segments)} {_fmt(b / bands)}")
    for b in range(bands):
        for s in range(segments):
            p00, p01 = idx[(b, s)], idx[(b, (s + 1) % segments)]
            p10, p11 = idx[(b + 1, s)], idx[(b + 1, (s + 1) % segments)]
            lines.append(f"f {p00}/{p00}/{p00} {p10}/{p10}/{p10} {p11}/{p11}/{p11}")
            lines.append(f"f {p00}/{p00}/{p00} {p11}/{p11}/{p11} {p01}/{p01}/{p01}")
    return "\n".join(lines) + "\n"


def object_block(k, mesh, material, t, r, s):
    v = lambda a: " ".join(_fmt(x) for x in a)
    return f"Object {k}\n{mesh}\nMaterial {material}\nTranslate {v(t)}\nRotate {v(r)}\nScale {v(s)}\n\n"


def write_meshes(d):
    for name, text in (("tri.obj", tri_obj()), ("cone.obj", cone_obj()), ("rev.obj", rev_obj())):
        with open(os.path.join(d, name), "w") as f:
            f.write(text)


def write_scene(d, name, trs=None, extra_objects=""):
    """Writes `name` into directory d (the meshes must be there): OBJECTS with their own transforms, or with the rows of `trs`
    ((translate, rotate, scale) per object).  Returns the path."""
    rows = [(o[2], o[3], o[4]) for o in OBJECTS] if trs is None else trs
    text = MATERIALS
    for k, (o, (t, r, s)) in enumerate(zip(OBJECTS, rows)):
        text += object_block(k, o[0], o[1], t, r, s)
    text += extra_objects + CAMERA
    path = os.path.join(d, name)
    with open(path, "w") as f:
        f.write(text)
    return path


def trs_array(rows):
    """(translate, rotate, scale) rows -> float32 [count, 9], Context.pose_objects' `trs`."""
    return np.array([list(t) + list(r) + list(s) for t, r, s in rows], F)


def xforms(rows):
    from radish_pt_amd import hostlib

    return np.stack([hostlib.object_transform(t, r, s) for t, r, s in rows])
