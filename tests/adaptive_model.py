"""numpy float32 restatements of the adaptive-sampling kernels (radish_pt_amd/csrc/device/kernels_adaptive.h): the finish fold with
its moments (k_ad_finish), the plan rule (k_ad_plan) and the slot layout of a request plane (k_ad_count / k_ad_scan / k_ad_scatter).
Every expression is evaluated in the kernels' order, one float32 operation at a time, so the results can be compared by bits."""
import numpy as np

F = np.float32
MAX_REQUEST = 16
OWNER_SHIFT = 4
# The threshold at which the plan is tested on rendered moments: chosen on the CPU oracle's 8-sample moments of the 52x36 Cornell
# frame so that the plan splits the frame (tests/test_adaptive_cpu.py: 19 of 35 blocks active)
PLAN_THRESHOLD = 0.15


# ---- the finish fold ---------------------------------------------------------------------------------------------------------
def luminance(c):
    """bsdf.h: 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z, left to right."""
    c = np.asarray(c, F)
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def running_mean(mean, x, n):
    """storeRunningMean's expression at iter n: (mean * float(n) + x) / float(n + 1); n may be an array."""
    n = np.asarray(n)
    return ((np.asarray(mean, F) * n.astype(F) + np.asarray(x, F)) / (n + 1).astype(F)).astype(F)


def fold(direct, indirect, count, moments, samples_d, samples_i, request):
    """k_ad_finish on planes [P, 3], [P, 3], [P], [P, 2] (moments may be None) — changed in place.  samples_d / samples_i[k] are the
    FINISHED samples (finishSample applied) of sample index k of every pixel, [K, P, 3]; pixel p folds k = count[p] .. count[p] +
    request[p] - 1, each at its own iter, and the moments fold L = luminance(d + i) and L * L alike."""
    with np.errstate(all="ignore"):
        for j in range(int(request.max()) if request.size else 0):
            on = np.flatnonzero(request > j)
            n = count[on] + j
            sd, si = samples_d[n, on], samples_i[n, on]
            direct[on] = running_mean(direct[on], sd, n[:, None])
            indirect[on] = running_mean(indirect[on], si, n[:, None])
            if moments is not None:
                L = luminance((sd + si).astype(F))
                moments[on, 0] = running_mean(moments[on, 0], L, n)
                moments[on, 1] = running_mean(moments[on, 1], (L * L).astype(F), n)
    count += request
    return direct, indirect, count, moments


# ---- the plan ----------------------------------------------------------------------------------------------------------------
def wants(count, moments, min_samples, threshold):
    """Per pixel: n < minSamples, or err2 > tol * tol (false for NaN) with var = m2 - m1 * m1, err2 = var / float(n),
    tol = threshold * (m1 + 0.01f)."""
    m1, m2 = np.asarray(moments[:, 0], F), np.asarray(moments[:, 1], F)
    with np.errstate(all="ignore"):
        var = (m2 - (m1 * m1).astype(F)).astype(F)
        err2 = (var / count.astype(F)).astype(F)
        tol = (F(threshold) * (m1 + F(0.01)).astype(F)).astype(F)
        over = err2 > (tol * tol).astype(F)
    return (count < min_samples) | over


def plan(count, moments, W, H, min_samples, max_samples, step, threshold):
    """k_ad_plan: (request [P] int32, {"samplesRequested", "activeBlocks", "wantingPixels"}).  The blocks are the frame's 8x8 blocks
    (tiles are multiples of 8 pixels, so PixelMap's blocks are these whatever the tile size)."""
    w = wants(count, moments, min_samples, threshold).reshape(H, W)
    by, bx = (H + 7) // 8, (W + 7) // 8
    padded = np.zeros((by * 8, bx * 8), bool)
    padded[:H, :W] = w
    active_blocks = padded.reshape(by, 8, bx, 8).any(axis=(1, 3))
    active = np.repeat(np.repeat(active_blocks, 8, axis=0), 8, axis=1)[:H, :W].reshape(-1)
    room = max_samples - count.astype(np.int64)
    request = np.where(active & (room > 0), np.minimum(step, room), 0).astype(np.int32)
    return request, {"samplesRequested": int(request.sum(dtype=np.int64)), "activeBlocks": int(active_blocks.sum()),
                     "wantingPixels": int(w.sum())}


# ---- the slot layout -----------------------------------------------------------------------------------------------------------
def work_order(W, H, tile=64):
    """Pixel index (y * W + x, or -1 off the frame) of every pixel work index of a single-rank PixelMap: tiles row-major, the 8x8
    blocks of a 64-pixel tile in Morton order (row-major for other tile sizes), a block's pixels row-major (mapPixel)."""
    bpe = tile // 8
    tiles_x, tiles_y = (W + tile - 1) // tile, (H + tile - 1) // tile
    out = np.full(tiles_x * tiles_y * bpe * bpe * 64, -1, np.int64)
    lane = np.arange(64)
    for t in range(tiles_x * tiles_y):
        for b in range(bpe * bpe):
            if bpe == 8:
                bx = (b & 1) | ((b >> 1) & 2) | ((b >> 2) & 4)
                by = ((b >> 1) & 1) | ((b >> 2) & 2) | ((b >> 3) & 4)
            else:
                bx, by = b % bpe, b // bpe
            x = (t % tiles_x) * tile + bx * 8 + (lane & 7)
            y = (t // tiles_x) * tile + by * 8 + (lane >> 3)
            ok = (x < W) & (y < H)
            out[(t * bpe * bpe + b) * 64 + lane] = np.where(ok, y * W + x, -1)
    return out


def slot_layout(request, W, H, tile=64):
    """(slotBase per pixel work index, owner per slot, T): the exclusive prefix of the requests in work order; slot slotBase + j of a
    pixel is owned by (work index << 4) | j."""
    order = work_order(W, H, tile)
    r = np.where(order >= 0, request[np.maximum(order, 0)], 0).astype(np.int64)
    base = np.cumsum(r) - r
    total = int(r.sum())
    owner = np.zeros(total, np.int64)
    work = np.repeat(np.arange(len(order)), r)
    owner[:] = (work << OWNER_SHIFT) | (np.arange(total) - np.repeat(base, r))
    return base, owner, total


# ---- hand-made planes for the plan (tests/test_adaptive_cpu.py pins what each block must give; the GPU plan is held to the model on them)
HAND_W, HAND_H = 52, 36  # 7 x 5 blocks, the last column 4 pixels wide, the last row 4 pixels high
HAND_PARAMS = {"min_samples": 4, "max_samples": 8, "step": 4, "threshold": 0.15}


def hand_made_planes():
    """(count [P] int32, moments [P, 2] float32) over a 52x36 frame, one case per 8x8 block of the top row and one in the corner:
      block 0  n = 2, below the minimum: every pixel wants
      block 1  wanting pixels at n = 8 (the maximum) and, in its first two rows, n = 9 (above it): active, but they get nothing; its
               last row has n = 6 and gets min(4, 8 - 6)
      block 2  zero mean, zero second moment: nobody wants
      block 3  zero mean and one pixel with a second moment: that pixel wants, the block gets samples
      block 4  m2 < m1 * m1, a negative variance: nobody wants
      block 5  NaN moments: nobody wants
      block 6  (4 pixels wide) one wanting pixel
      corner   (4x4 pixels) one wanting pixel, the frame's last
    everything else is quiet: n = 5, a constant luminance of 0.5."""
    W, H = HAND_W, HAND_H
    count = np.full((H, W), 5, np.int32)
    m = np.zeros((H, W, 2), F)
    m[..., 0], m[..., 1] = F(0.5), F(0.25)
    count[0:8, 0:8] = 2
    m[0:8, 0:8] = 0
    count[0:8, 8:16] = 8
    count[0:2, 8:16] = 9
    count[7, 8:16] = 6
    m[0:8, 8:16] = (F(0.5), F(1.0))
    count[0:8, 16:32] = 6
    m[0:8, 16:32] = 0
    m[3, 27, 1] = F(1e-3)
    m[0:8, 32:40] = (F(1.0), F(0.5))
    m[0:8, 40:48] = np.nan
    m[5, 50] = (F(0.5), F(1.0))
    m[35, 51] = (F(0.5), F(1.0))
    return count.reshape(-1), m.reshape(-1, 2)
