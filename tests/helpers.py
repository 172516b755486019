import numpy as np


def random_rays(n, seed, lo=(-1.2, -0.2, -1.2), hi=(1.2, 2.2, 4.5)):
    """Origins in a box around the Cornell scene, unit directions; a few axis-parallel and tiny-component
    directions so every branch of AABB::intersect is exercised."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32)
    k = max(n // 16, 1)
    for axis in range(3):  # exactly axis-parallel
        idx = rng.choice(n, k, replace=False)
        d[idx] = 0
        d[idx, axis] = rng.choice([-1.0, 1.0], k)
    idx = rng.choice(n, k, replace=False)  # one tiny component
    d[idx, rng.integers(0, 3, k)] = 1e-7
    idx = rng.choice(n, k, replace=False)  # one exactly-zero component
    d[idx, rng.integers(0, 3, k)] = 0.0
    return np.concatenate([o, d], axis=1).astype(np.float32)


def random_segments(n, seed, lo=(-1.0, 0.0, -1.0), hi=(1.0, 2.0, 1.0)):
    rng = np.random.default_rng(seed)
    x = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    y = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    return np.concatenate([x, y], axis=1).astype(np.float32)


def bits(a):
    """View float arrays as uint32 so comparisons are bit-exact (NaN == NaN, +0 != -0)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_equal(a, b, what=""):
    ba, bb = bits(a), bits(b)
    if not np.array_equal(ba, bb):
        bad = np.argwhere(ba != bb)
        first = tuple(bad[0])
        raise AssertionError(
            f"{what}: {len(bad)} of {ba.size} floats differ bitwise; first at {first}: "
            f"{np.asarray(a, np.float32)[first]!r} vs {np.asarray(b, np.float32)[first]!r}"
        )


def chain_scene(n_stack):
    """n_stack coincident triangles with alternating materials over a floor, under a lamp: the SAH builder has nothing to split on
    and returns a CHAIN (one leaf and one inner child per level), and every ray that hits one of the triangles hits all of them at
    the same distance."""
    from radish_pt_amd import layouts as L, scenes

    mats = [L.make_material(L.LAMBERTIAN, (0.8, 0.3, 0.2)), L.make_material(L.LAMBERTIAN, (0.2, 0.7, 0.9)),
            L.make_material(L.METALLIC_WORKFLOW, (0.9, 0.9, 0.9), metallic=0.6, roughness=0.35), L.make_material(L.LIGHT, (7.0, 6.5, 6.0))]
    tri = np.array([[-1.2, -0.4, 0.1], [1.3, -0.5, -0.2], [0.1, 1.4, 0.3]], np.float32)
    nrm = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    nrm = np.tile((nrm / np.linalg.norm(nrm)).astype(np.float32), (3, 1))
    uv = np.array([[0, 0], [1, 0], [0, 1]], np.float32)
    floor = np.array([[-3, -0.8, -3], [3, -0.8, -3], [3, -0.8, 3], [-3, -0.8, -3], [3, -0.8, 3], [-3, -0.8, 3]], np.float32)
    lamp = np.array([[-0.6, 2.4, -0.6], [0.6, 2.4, -0.6], [0.6, 2.4, 0.6], [-0.6, 2.4, -0.6], [0.6, 2.4, 0.6], [-0.6, 2.4, 0.6]], np.float32)  # facing down
    v = np.concatenate([np.tile(tri, (n_stack, 1)), floor, lamp])
    n = np.concatenate([np.tile(nrm, (n_stack, 1)), np.tile(np.array([0, 1, 0], np.float32), (6, 1)), np.tile(np.array([0, -1, 0], np.float32), (6, 1))])
    t = np.tile(uv, (n_stack + 4, 1))
    ids = np.array([i % 3 for i in range(n_stack)] + [0, 0, 3, 3], np.int32)
    return scenes.SceneData(f"chain{n_stack}", v, n, t, ids, np.array(mats, dtype=L.MATERIAL_DTYPE))


def count_literal_primary_rays(cam):
    """How many un-jittered centre rays of `cam` have a direction component below the box test's Eps (bvh.h:138-148)."""
    W, H = int(cam["resolution"][0]), int(cam["resolution"][1])
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ru = 1.0 - (x + 0.5) / W * 2.0
    rv = 1.0 - (y + 0.5) / H * 2.0
    t = float(cam["tanFovY"])
    d = (ru * (W / H) * t)[..., None] * cam["right"].astype(np.float64) + (rv * t)[..., None] * cam["up"].astype(np.float64) \
        + cam["view"].astype(np.float64)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return int((np.abs(d) < 5e-7).any(axis=-1).sum())


def restir_partition_run(gpu_ctx, sd, W, H, cams, world, tile, reuse):
    """ReSTIR frames on `world` virtual ranks (one rdh_ctx each, all on this GPU): whole-frame G-buffer, rdh_restir_direct per
    rank into its packed tiles, reservoir exchange (pack -> simulated all-gather -> unpack), rdh_untile.  Returns the frames and
    every rank's `last` reservoirs after each frame."""
    from radish_pt_amd import api

    import torch
    n = W * H
    dev = api.DevScene()
    ctxs = []
    for rank in range(world):
        c = gpu_ctx if world == 1 else api.Context(0)
        c.upload_scene(sd)
        c.set_partition(rank, world, tile)
        c.set_camera(cams[0])
        c.restir_init()
        ctxs.append(c)
    gb = api.GBuffer()
    gb.create(W, H)
    frames, resv = [], []
    tpr = ctxs[0].tiles_per_rank()
    imgs = [torch.zeros(n if world == 1 else tpr * tile * tile, 3, device="cuda") for _ in ctxs]
    for f, cam in enumerate(cams):
        dev.ctx = ctxs[0]
        gb.render(dev, cam)  # whole frame regardless of the partition
        for c, img in zip(ctxs, imgs):
            c.set_camera(cam)
            c.restir_direct(img, 0, 40 + f, gb.c_struct(cam), reuse)
        if world == 1:
            frames.append(imgs[0].cpu().numpy().copy())
        else:
            packs = []
            for c in ctxs:
                pk = torch.zeros(tpr * tile * tile, 9, device="cuda")
                c.restir_exchange_pack(pk)
                packs.append(pk)
            gathered = torch.cat(packs).contiguous()
            for c in ctxs:
                c.restir_exchange_unpack(gathered)
            frame = torch.zeros(n, 3, device="cuda")
            ctxs[0].untile(torch.cat(imgs).contiguous(), frame)
            ctxs[0].synchronize()
            frames.append(frame.cpu().numpy().copy())
        resv.append([c.restir_read(1).tobytes() for c in ctxs])
        gb.update(cam)
    for c in ctxs:
        c.restir_free()
        if c is not gpu_ctx:
            c.close()
    return frames, resv


def oracle_path_trace_mt(sd, cam, direct, indirect, iter, looper, depth, stride=1, threads=None):
    """The oracle's pathTrace on every `stride`-th pixel of the frame, spread over host threads (one oracle handle per thread,
    pixels dealt round-robin; the ctypes call releases the GIL).  Fills the sampled rows of direct / indirect in place and
    returns (pixel indices, summed work counters)."""
    import os
    import threading

    from oracle import pyoracle

    w, h = (int(v) for v in cam["resolution"])
    n = w * h
    if threads is None:
        threads = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))
    handles = [pyoracle.OracleScene(sd) for _ in range(threads)]
    ts = [threading.Thread(target=handles[t].path_trace, args=(cam, direct, indirect, iter, looper, depth),
                           kwargs={"pix": (t * stride, n, threads * stride)}) for t in range(threads)]
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    stats = {}
    for hd in handles:
        for k, v in hd.stats().items():
            stats[k] = stats.get(k, 0) + v
    return np.arange(0, n, stride), stats
