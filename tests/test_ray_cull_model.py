"""The emitter-box test (ray_cull.h, restated in tests/ray_cull_model.py) never drops a ray that the traversal would report as a hit.

Scenes made of emissive triangles only, so that the oracle's closest hit IS "some intersectTriangle against an emissive triangle
returned a hit with dist > 0": a large quad, a sliver, and a triangle in an axis plane (a box of zero thickness).  The root box of
such a scene is the emitters' own box.  Per scene 500 000 rays (1.5 million in all), binary32 with unit directions as the
path tracer's are, aimed at and just past edges and vertices:
  - from ordinary distances, and grazing the triangle's plane at angles from 1e-1 down to 1e-5 rad;
  - from origins on the padded box's faces and inside the box;
  - from origins 1e3 extents away;
  - with one and with two direction components near 1.1e-6 of the length, on either side of the threshold;
  - with a direction within 1e-7 .. 1e-5 of an axis, on either side of AABB::intersect's 1 - 1e-6.
Condition: no ray for which the oracle's trace_closest reports a hit is dropped.  That is the walk through the tree, as every
kernel makes it: a triangle is tested only after its leaf's box has passed AABB::intersect, and that is what the box test leans
on (ray_cull.h).  The brute-force loop over the triangles (`naive`) is NOT the reference here: for rays that graze the plane at
1e-5 rad and less, intersectTriangle alone reports hits for rays that pass the triangle at 1e-3 to 1e-2 extents (measured on the
large quad: 6 of the 50 000 rays of the finest grazing family); no walk reports them, and the test prints how many there are.
The random rays of the last family are aimed at nothing; the test states how many of them the box drops and asserts a share that
follows from the geometry (below), so it cannot pass by dropping nothing."""
import numpy as np
import pytest

from ray_cull_model import F, may_reach, padded_box

N_PER_FAMILY = 50_000


def _emitter_scene(name, tris):
    from radish_pt_amd import layouts as L, scenes

    v = np.asarray(tris, F).reshape(-1, 3)
    n = np.zeros_like(v)
    n[:, 1] = 1.0
    return scenes.SceneData(name, v, n, np.zeros((v.shape[0], 2), F), np.zeros(v.shape[0] // 3, np.int32),
                            np.array([L.make_material(L.LIGHT, (5.0, 5.0, 5.0))], dtype=L.MATERIAL_DTYPE))


SCENES = {
    "large": [[(-1, 0.5, -1), (1, 0.5, -1), (1, 1.5, 1)], [(-1, 0.5, -1), (1, 1.5, 1), (-1, 1.5, 1)]],
    "sliver": [[(0, 0, 0), (1, 0.3, 0.2), (1.0001, 0.3001, 0.2)]],
    "axis_plane": [[(-0.75, 1.5, -0.75), (0.75, 1.5, -0.75), (0.2, 1.5, 0.75)]],
}


def _unit(d):
    d = np.asarray(d, np.float64)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _targets(rng, tris, n, ext):
    """Points on the edges and at the vertices of random triangles of the scene, pushed in the triangle's plane by 0 or
    +-ext * 10^[-8, -2] across the edge; also each triangle's unit normal and an in-plane unit vector."""
    t = np.asarray(tris, np.float64)[rng.integers(0, len(tris), n)]
    e = rng.integers(0, 3, n)
    a, b, c = t[np.arange(n), e], t[np.arange(n), (e + 1) % 3], t[np.arange(n), (e + 2) % 3]
    s = rng.uniform(0, 1, n)
    s[rng.uniform(0, 1, n) < 0.3] = 0.0  # a vertex
    p = a + (b - a) * s[:, None]
    nrm = _unit(np.cross(b - a, c - a))
    along = _unit(b - a)
    across = np.cross(nrm, along)  # in the plane, pointing inwards
    push = ext * 10.0 ** rng.uniform(-8, -2, n) * rng.choice([-1.0, 0.0, 1.0], n)
    return p + across * push[:, None], nrm, along, across


def _rays(rng, tris, box, ext):
    """{family: (o, d)} in float32."""
    n = N_PER_FAMILY
    lo, hi = (np.asarray(x, np.float64) for x in box)
    out = {}

    def aimed(o, p):
        o32 = o.astype(F)
        return o32, _unit(p - o32.astype(np.float64)).astype(F)

    p, nrm, along, across = _targets(rng, tris, n, ext)
    out["ordinary"] = aimed(p + _unit(rng.normal(size=(n, 3))) * (ext * 10.0 ** rng.uniform(-1, 1, n))[:, None], p)
    for lo_e, hi_e, name in ((-3, -1, "grazing"), (-5, -3, "grazing_fine")):
        p, nrm, along, across = _targets(rng, tris, n, ext)
        th, phi = 10.0 ** rng.uniform(lo_e, hi_e, n) * rng.choice([-1.0, 1.0], n), rng.uniform(0, 2 * np.pi, n)
        t = along * np.cos(phi)[:, None] + across * np.sin(phi)[:, None]
        back = t * np.cos(th)[:, None] + nrm * np.sin(th)[:, None]
        out[name] = aimed(p + back * (ext * 10.0 ** rng.uniform(-1, 1, n))[:, None], p)
    p, *_ = _targets(rng, tris, n, ext)
    o = rng.uniform(lo, hi, (n, 3))
    ax, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    o32 = o.astype(F)
    o32[np.arange(n), ax] = np.where(side == 0, box[0][ax], box[1][ax])  # exactly on a face of the padded box
    out["on_faces"] = (o32, _unit(p - o32.astype(np.float64)).astype(F))
    p, *_ = _targets(rng, tris, n, ext)
    out["inside"] = aimed(rng.uniform(lo, hi, (n, 3)), p)
    p, *_ = _targets(rng, tris, n, ext)
    out["far"] = aimed(p + _unit(rng.normal(size=(n, 3))) * (ext * 1e3 * rng.uniform(0.5, 2.0, n))[:, None], p)
    for k, name in ((1, "one_small_component"), (2, "two_small_components")):
        p, *_ = _targets(rng, tris, n, ext)
        d = _unit(rng.normal(size=(n, 3)))
        first = rng.integers(0, 3, n)
        for j in range(k):
            d[np.arange(n), (first + j) % 3] = 1.1e-6 * rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
        d = _unit(d)
        o32 = (p - d * (ext * 10.0 ** rng.uniform(-1, 1, n))[:, None]).astype(F)
        out[name] = (o32, d.astype(F))
    p, *_ = _targets(rng, tris, n, ext)
    d = _unit(rng.normal(size=(n, 3))) * (10.0 ** rng.uniform(-3.5, -2.5, n))[:, None]  # |d_k| of 1 - 1e-7 .. 1 - 1e-5 on the axis
    d[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n)
    d = _unit(d)
    out["near_an_axis"] = ((p - d * (ext * 10.0 ** rng.uniform(-1, 1, n))[:, None]).astype(F), d.astype(F))
    mid = (lo + hi) / 2
    out["random"] = ((mid + rng.uniform(-4 * ext, 4 * ext, (n, 3))).astype(F), _unit(rng.normal(size=(n, 3))).astype(F))
    return out


@pytest.mark.parametrize("name", sorted(SCENES))
def test_no_hit_is_culled(name):
    from oracle import pyoracle

    tris = SCENES[name]
    sd = _emitter_scene(name, tris)
    assert sd.num_lights == len(tris)
    v = sd.vertices
    root_lo, root_hi = v.min(axis=0), v.max(axis=0)
    box = padded_box(v, root_lo, root_hi)
    ext = float(np.max(root_hi - root_lo))
    if name == "axis_plane":
        assert root_lo[1] == root_hi[1] and box[0][1] < root_lo[1] < box[1][1]
    orc = pyoracle.OracleScene(sd)
    rng = np.random.default_rng(20260 + len(name))
    total = 0
    for family, (o, d) in _rays(rng, tris, box, ext).items():
        assert o.dtype == F and d.dtype == F and np.isfinite(o).all() and np.isfinite(d).all()
        rays = np.concatenate([o, d], axis=1)
        hit = orc.trace_closest(rays)["primId"] >= 0
        brute = orc.trace_closest(rays, naive=True)["primId"] >= 0
        keep = may_reach(box, o, d)
        total += len(o)
        print(f"{name:10s} {family:22s} rays {len(o)}  oracle hits {int(hit.sum())}  culled {int((~keep).sum())}  "
              f"culled with a brute-force hit {int((brute & ~keep).sum())}")
        bad = hit & ~keep
        assert not bad.any(), (name, family, int(bad.sum()), rays[bad][:4])
        if family in ("ordinary", "inside", "on_faces"):
            assert hit.sum() > len(o) // 20, (family, int(hit.sum()))  # the aimed rays do meet the triangles
        if family in ("inside", "on_faces"):
            assert keep.all(), family  # kept whatever the direction
        if "small_component" in family:
            dd = d.astype(np.float64)
            small = (np.abs(dd) < 1.0e-6 * np.linalg.norm(dd, axis=1, keepdims=True)).any(axis=1)
            assert small.sum() > len(o) // 10 and keep[small].all()
        if family == "near_an_axis":
            dd = np.abs(d.astype(np.float64)).max(axis=1)
            assert (dd > 1 - 1e-6).sum() > len(o) // 10 and keep[dd > 1 - 1e-6].all() and (dd < 1 - 2e-6).sum() > len(o) // 10
        if family == "random":
            # Origins uniform in a cube of edge 8 ext around the box, directions uniform: the padded box lies inside a ball of radius
            # 0.9 ext around its centre (half its diagonal, at most sqrt(3) / 2 ext, plus the padding), which an origin at distance r sees under the solid-angle share
            # (1 - sqrt(1 - (0.9 ext / r)^2)) / 2 < 0.07 once r > 2 ext, and at most 7 % of the cube lies within 2 ext of the centre
            # (4/3 pi 2^3 / 8^3).  So fewer than 0.07 + 0.07 of these rays can meet the box, and the test must drop over 80 %.
            share = float((~keep).mean())
            print(f"{name}: {share:.3f} of the random rays are culled")
            assert share > 0.8, share
    assert total >= 400_000


def test_no_emitters_culls_everything():
    o = np.zeros((4, 3), F)
    d = np.array([[1, 0, 0], [0, 1, 0], [0.6, 0.8, 0], [0.577, 0.577, 0.577]], F)
    assert padded_box(np.zeros((0, 3), F), (0, 0, 0), (1, 1, 1)) is None
    assert not may_reach(None, o, d).any()
