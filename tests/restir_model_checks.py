"""The scene, the three-frame sequence and the per-step comparison shared by tests/test_restir_model_cpu.py (the oracle against
tests/restir_model.py) and tests/test_gpu_restir_model.py (the HIP kernels against the same model).

Every step of the model is run on the TESTED code's own earlier state (its G-buffer planes, its last-frame reservoirs, its
reservoirTemp plane), so a discrete choice that float32 and float64 make differently stays in the pixel where it arose; by
induction from the zeroed buffers the whole sequence is pinned all the same."""
import numpy as np

import restir_model as M
from radish_pt_amd import hostlib, layouts as L, scenes

W, H = 45, 37  # not a multiple of the 8x8 packet
N = W * H
LOOPERS = (40, 977, 5003, 8191)
SEEDED_FRAME = 3  # frames 0-2 run from the zeroed buffers; frame 3 reads last-frame reservoirs edited by seed_last()
REL, FLOOR = 2e-4, 1e-3  # the tolerance of the project's float64 comparisons (test_oracle_statistics.py)
CAP = 6  # 0.4 % of 1665 pixels, per frame and per step


# ---------------------------------------------------------------------------------------------------------------------
# scene and cameras
# ---------------------------------------------------------------------------------------------------------------------
SIDEWAYS = (1.0, 0.08, 0.15)  # authored normal of the "sideways" patch: dot with +y is 0.079 after normalisation, below 0.1

OPPOSED = (-1.0, 0.08, -0.15)  # dot with SIDEWAYS is -0.99 and with +y 0.079

LIGHTS = [  # (centre x, z, half x, z, height, colour); winding faces the floor
    (-1.05, 0.55, 0.16, 0.13, 1.30, (6.0, 5.0, 3.0)),
    (0.75, 0.25, 0.14, 0.17, 1.45, (3.0, 6.0, 7.0)),
    (0.05, -0.95, 0.22, 0.12, 1.55, (7.0, 7.0, 6.0)),
    (-0.55, 1.25, 0.12, 0.12, 1.20, (4.0, 2.5, 6.5)),
    (1.35, -1.6, 0.25, 0.2, 1.70, (8.0, 4.0, 2.0)),
    (-1.5, -2.6, 0.3, 0.25, 1.90, (2.5, 7.5, 4.0)),
]


def build_scene():
    """Horizontal quads only.  A long Lambertian floor (open sky beside and behind it), a patch of ANOTHER material and a patch of
    the FLOOR'S OWN material with sideways authored normals 2 mm above it, a MetallicWorkflow patch, a hovering occluder and six
    emissive quads between the camera and the floor (seen directly from behind: the -2 entries)."""
    mats = [L.make_material(L.LAMBERTIAN, (0.75, 0.6, 0.5)), L.make_material(L.LAMBERTIAN, (0.3, 0.5, 0.7)),
            L.make_material(L.METALLIC_WORKFLOW, (0.9, 0.8, 0.4), metallic=0.6, roughness=0.5),
            L.make_material(L.LAMBERTIAN, (0.5, 0.7, 0.4))]
    verts, norms, ids = [], [], []

    def quad(x0, x1, z0, z1, y, n, mat, down=False):
        p = [(x0, y, z0), (x0, y, z1), (x1, y, z1), (x1, y, z0)]  # winding normal +y
        if down:
            p = p[::-1]
        verts.extend([p[0], p[1], p[2], p[0], p[2], p[3]])
        norms.extend([n] * 6)
        ids.extend([mat, mat])

    quad(-2.0, 2.0, -7.0, 2.2, 0.0, (0, 1, 0), 0)
    quad(-1.6, -0.5, -1.0, 0.6, 0.002, (0, 1, 0), 1)
    quad(0.5, 1.0, -0.9, 0.5, 0.002, SIDEWAYS, 0)
    quad(1.0, 1.5, -0.9, 0.5, 0.002, OPPOSED, 0)  # adjoining, normal reversed: |dot| passes where the plain dot does not
    quad(-0.3, 1.8, -2.3, -1.95, 0.002, SIDEWAYS, 0)  # a strip of the same: more border for the normal tests
    quad(0.5, 1.5, 0.5, 0.85, 0.002, OPPOSED, 0)
    quad(-0.4, 0.45, 0.7, 1.5, 0.003, (0, 1, 0), 2)
    quad(-0.45, 0.35, -0.6, 0.1, 0.9, (0, 1, 0), 3)
    for (cx, cz, hx, hz, y, col) in LIGHTS:
        mats.append(L.make_material(L.LIGHT, col))
        quad(cx - hx, cx + hx, cz - hz, cz + hz, y, (0, -1, 0), len(mats) - 1, down=True)
    v, n = np.array(verts, np.float32), np.array(norms, np.float32)
    return scenes.SceneData("restir_model", v, n, np.zeros((len(v), 2), np.float32), np.array(ids, np.int32),
                            np.array(mats, dtype=L.MATERIAL_DTYPE))


def cameras():
    """The camera translates and turns each frame: the leading image edge reprojects outside the last frame and the occluder's
    parallax uncovers floor."""
    return [hostlib.make_camera(W, H, eye=(0.15 + 0.22 * f, 2.5, 2.3 - 0.08 * f), rotation=(-92.0 + 3.0 * f, -48.0 - 2.5 * f, 0.0),
                                fovy=30.0) for f in range(4)]


def seed_last(rec):
    """Last-frame reservoirs that no run from zeroed buffers can hold, for the branches such a run cannot reach: every stored
    reservoir has passed checkValidity and has at most 32 samples per frame, so within a few frames no temporal neighbour is
    invalid, none has 19 times the pixel's own count, and no sum of weights overflows.  By pixel index: NaN, negative and
    infinite weights (the temporal merge and its draw are skipped), counts times 40 (the pre-clamp applies) and weights of 2e38
    (two such neighbours overflow binary32 in the spatial sum, which makes the aggregate invalid and skips the final merge)."""
    out = rec.copy()
    i = np.arange(len(rec))
    out["weight"][i % 7 == 3] = np.nan
    out["weight"][i % 7 == 5] = -1.0
    out["weight"][i % 14 == 1] = np.inf
    out["numSamples"][i % 5 == 0] *= 40
    out["weight"][i % 3 == 2] = 2e38
    return out


# ---------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------
def far(got, want):
    """Per row: any component outside 2e-4 relative with a floor of 1e-3 (NaN on either side only matches NaN)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got - want) <= REL * np.maximum(np.abs(want), FLOOR)) & ~(np.isnan(got) & np.isnan(want))
    return bad.reshape(len(bad), -1).any(1)


def planes_for_model(cur, last):
    """The tested code's planes as the model reads them: this frame's and the other half of the double buffer."""
    p = {k: np.asarray(v).astype(np.int64 if k in ("primId", "motion") else np.float64) for k, v in cur.items()}
    p["lastPrimId"] = np.asarray(last["primId"]).astype(np.int64)
    p["lastNormal"] = np.asarray(last["normal"]).astype(np.float64)
    return p


def gbuffer_bad(model, tested):
    """The id and motion planes exactly; normal, depth and albedo within the tolerance."""
    bad = (model["primId"] != tested["primId"]) | (model["motion"] != tested["motion"])
    for k in ("normal", "depth", "albedo"):
        bad |= far(tested[k], model[k])
    return bad


def reservoirs_bad(model, rec, rows):
    bad = model["numSamples"] != rec["numSamples"]
    for k in ("weight", "Li", "wi", "dist"):
        bad |= far(rec[k], model[k])
    return bad & rows


def records_from_reservoirs(r):
    rec = np.zeros(len(r["weight"]), L.RESERVOIR_DTYPE)
    for k in rec.dtype.names:
        rec[k] = r[k]
    return rec


def _raw(rec):
    return np.ascontiguousarray(rec).view(np.uint8).reshape(len(rec), -1)


_MEMO = {}


def _memo(key, inputs, fn):
    """The model's steps are deterministic in their inputs: a step is computed once per distinct input state (the GPU's state is
    the oracle's bit for bit, so the kernel structures share one evaluation; a state that differed would be evaluated afresh)."""
    key = key + tuple(np.ascontiguousarray(a).tobytes() for a in inputs)
    h = hash(key)
    if h not in _MEMO or _MEMO[h][0] != key:
        _MEMO[h] = (key, fn())
    return _MEMO[h][1]


def check_frame(ms, f, cams, reuse, faithful, t):
    """One frame of the tested code `t` (a dict: planes, last_planes, last, prior_out, prior_temp, out, temp, image_in, image;
    reservoirs as RESERVOIR_DTYPE records) against the model's three steps.  Returns {step: excluded pixel indices}."""
    cam, last_cam = cams[f], (cams[f - 1] if f else None)
    ex = {}
    tag = (f, reuse, faithful, id(ms))  # the scene too: tests/path_model_checks.py runs the same sequence on another one
    gb = _memo(("gb", f, id(ms)), (), lambda: M.gbuffer(ms, cam, last_cam))
    ex["gbuffer"] = np.flatnonzero(gbuffer_bad(gb, t["planes"]))
    planes = planes_for_model(t["planes"], t["last_planes"])  # the tested code's planes from here on

    p1_in = (t["last"], t["planes"]["primId"], t["planes"]["motion"], t["planes"]["normal"], t["last_planes"]["primId"],
             t["last_planes"]["normal"])
    p1 = _memo(("p1",) + tag, p1_in, lambda: M.pass1(ms, cam, LOOPERS[f], planes, M.reservoirs_from_records(t["last"]), f == 0, reuse, faithful))
    bad = reservoirs_bad(p1["out"], t["out"], p1["stored"])
    bad |= ~p1["stored"] & (_raw(t["out"]) != _raw(t["prior_out"])).any(1)  # a miss or an emitter stores nothing
    bad |= reservoirs_bad(p1["temp"], t["temp"], p1["stored_temp"])
    bad |= ~p1["stored_temp"] & (_raw(t["temp"]) != _raw(t["prior_temp"])).any(1)
    ex["pass1"] = np.flatnonzero(bad)

    own = t["temp"] if reuse & M.SPATIAL else t["out"]
    st = dict(p1, own=M.reservoirs_from_records(own))
    p2 = _memo(("p2",) + tag, p1_in + (t["temp"], own, t["image_in"], t["planes"]["albedo"], t["planes"]["depth"]), lambda: M.pass2(ms, cam, LOOPERS[f], planes, M.reservoirs_from_records(t["temp"]), st, reuse, f, t["image_in"].astype(np.float64)))
    ex["pass2"] = np.flatnonzero(far(t["image"], p2["image"]))
    return ex, p1, p2


def assert_within_cap(ex, what):
    for step, px in ex.items():
        assert len(px) <= CAP, f"{what}, {step}: {len(px)} pixels differ from the float64 model (cap {CAP}); first {px[:12]}"


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's sequence
# ---------------------------------------------------------------------------------------------------------------------
def host_planes(gb, half):
    return {"albedo": gb.albedo.copy(), "normal": gb.normal[half].copy(), "primId": gb.primId[half].copy(),
            "depth": gb.depth[half].copy(), "motion": gb.motion.copy()}


def run_oracle(sd, cams, reuse, faithful):
    """The frames as check_frame reads them, from pyoracle's gbuffer_render and restir_direct."""
    from oracle import pyoracle

    w, h = (int(v) for v in cams[0]["resolution"])
    o = pyoracle.OracleScene(sd)
    gb = pyoracle.GBufferHost(w, h)
    res = [np.zeros(w * h, L.RESERVOIR_DTYPE) for _ in range(3)]  # cur, last, temp (restir.cu:4-7)
    img = np.zeros((w * h, 3), np.float32)
    frames = []
    for f, cam in enumerate(cams):
        o.gbuffer_render(cam, gb)
        t = {"planes": host_planes(gb, gb.frameIdx), "last_planes": host_planes(gb, gb.frameIdx ^ 1), "last": res[1].copy(),
             "prior_out": res[0].copy(), "prior_temp": res[2].copy(), "image_in": img.copy()}
        if f == SEEDED_FRAME:
            res[1][:] = t["last"] = seed_last(res[1])
        o.restir_direct(cam, img, f, LOOPERS[f], res[0], res[1], res[2], gb, f == 0, reuse, faithful)
        res[0], res[1] = res[1], res[0]  # std::swap(directReservoir, lastDirectReservoir)
        t.update(out=res[1].copy(), temp=res[2].copy(), image=img.copy())
        frames.append(t)
        gb.update(cam)
    return frames


# ---------------------------------------------------------------------------------------------------------------------
# liveness: how often each rule decides, from the model alone (its own state carried forward)
# ---------------------------------------------------------------------------------------------------------------------
def model_only_counts(ms, cams, reuse=3, faithful=1):
    """One dict of counts per frame."""
    zero_planes = {"albedo": np.zeros((N, 3)), "normal": np.zeros((N, 3)), "primId": np.zeros(N, np.int64), "depth": np.zeros(N),
                   "motion": np.zeros(N, np.int64)}
    res = [M.empty_reservoirs(N) for _ in range(3)]
    img = np.zeros((N, 3))
    last_planes = zero_planes
    per_frame = []

    def add(name, mask):
        counts[name] = counts.get(name, 0) + int(np.sum(mask))

    def store(buf, new, rows):
        for k in buf:
            buf[k][rows] = new[k][rows]

    for f, cam in enumerate(cams):
        counts = {}
        per_frame.append(counts)
        cur = M.gbuffer(ms, cam, cams[f - 1] if f else None)
        planes = planes_for_model(cur, last_planes)
        add("gb_miss", cur["primId"] == -1)
        add("gb_emitter", cur["primId"] == -2)
        add("gb_motion_off_frame", cur["motion"] < 0)
        add("gb_motion_moved", (cur["primId"] >= 0) & (cur["motion"] >= 0) & (cur["motion"] != np.arange(N)))
        if f == SEEDED_FRAME:
            res[1] = M.reservoirs_from_records(seed_last(records_from_reservoirs(res[1])))
        p1 = M.pass1(ms, cam, LOOPERS[f], planes, res[1], f == 0, reuse, faithful)
        store(res[0], p1["out"], p1["stored"])
        store(res[2], p1["temp"], p1["stored_temp"])
        st = dict(p1, own=res[2] if reuse & M.SPATIAL else res[0])
        p2 = M.pass2(ms, cam, LOOPERS[f], planes, res[2], st, reuse, f, img)
        img = p2["image"]
        sh = p1["status"] == 0
        add("metallic", sh & (ms.mat_type[p1["mat"]] == M.METALLIC_WORKFLOW))
        add("early_miss", p1["status"] == 1)
        add("early_emitter", p1["status"] == 2)
        for k, v in p1["live"].items():
            add(k, v & sh)
        for k, v in p2["live"].items():
            if k == "first_spatial_dim":
                # a pixel whose spatial draws start one dimension earlier than those of a shaded 4-neighbour
                d = np.where(sh, v, -1).reshape(H, W)
                early = np.zeros((H, W), bool)
                early[:, :-1] |= (d[:, :-1] >= 0) & (d[:, 1:] == d[:, :-1] + 1)
                early[:, 1:] |= (d[:, 1:] >= 0) & (d[:, :-1] == d[:, 1:] + 1)
                early[:-1] |= (d[:-1] >= 0) & (d[1:] == d[:-1] + 1)
                early[1:] |= (d[1:] >= 0) & (d[:-1] == d[1:] + 1)
                add("spatial_draws_one_dim_early", early)
            else:
                add(k, np.where(sh, v, 0))
        res[0], res[1] = res[1], res[0]
        last_planes = cur
    return per_frame
