"""The numpy statement of the motion-estimation specification (include/lsfa_hip.h, lsfa_luma_u8 / lsfa_mv_estimate; DESIGN.md "Motion
estimation").  It is what the device kernels are compared with bit for bit; tests/test_me_cpu.py pins it against hand-made cases and
against clips with known motion.  Written for clarity: vectorised over the macroblocks, one Python iteration per candidate, visited in the
order of the tie-break so that "strictly smaller cost replaces" IS the lexicographic minimum (no packed key, unlike the kernel)."""
import numpy as np


def luma(bgr):
    """(H, W, 3) uint8 BGR -> (H, W) uint8, Y = (29 B + 150 G + 77 R + 128) >> 8"""
    b = bgr.astype(np.int64)
    return ((29 * b[..., 0] + 150 * b[..., 1] + 77 * b[..., 2] + 128) >> 8).astype(np.uint8)


def estimate(y_cur, y_ref, search=16, lam=4, max_sad=0):
    """(H, W) uint8 planes -> rows (mbh * mbw, 7) int32 {-1, 16, 16, src_x, src_y, dst_x, dst_y}, sad (mbh, mbw) int32 (the winner's SAD)"""
    assert y_cur.dtype == np.uint8 and y_ref.dtype == np.uint8 and y_cur.shape == y_ref.shape and y_cur.ndim == 2
    assert 1 <= search <= 32 and lam >= 0 and max_sad >= 0
    H, W = y_cur.shape
    R = int(search)
    mbh, mbw = -(-H // 16), -(-W // 16)
    PH, PW = mbh * 16, mbw * 16
    cur = np.zeros((PH, PW), np.int32)
    cur[:H, :W] = y_cur
    covered = np.zeros((PH, PW), np.int32)
    covered[:H, :W] = 1
    ref = np.zeros((PH + 2 * R, PW + 2 * R), np.int32)        # the frame at (R, R); what lies outside it is never part of a valid sum
    ref[R:R + H, R:R + W] = y_ref
    x0 = 16 * np.arange(mbw)[None, :]
    y0 = 16 * np.arange(mbh)[:, None]
    x1 = np.minimum(x0 + 16, W) - 1            # last covered column / row of the block
    y1 = np.minimum(y0 + 16, H) - 1
    best_cost = np.full((mbh, mbw), np.iinfo(np.int64).max, np.int64)
    best_sad = np.zeros((mbh, mbw), np.int64)
    best_dx = np.zeros((mbh, mbw), np.int64)
    best_dy = np.zeros((mbh, mbw), np.int64)
    cands = sorted(((abs(dx) + abs(dy), dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)))
    for length, dy, dx in cands:
        valid = (x0 + dx >= 0) & (x1 + dx <= W - 1) & (y0 + dy >= 0) & (y1 + dy <= H - 1)
        if not valid.any():
            continue
        shifted = ref[R + dy:R + dy + PH, R + dx:R + dx + PW]
        sad = (np.abs(cur - shifted) * covered).reshape(mbh, 16, mbw, 16).sum(axis=(1, 3)).astype(np.int64)
        cost = sad + lam * length
        take = valid & (cost < best_cost)       # candidates come in (|dx| + |dy|, dy, dx) order: equal cost keeps the earlier one
        best_cost = np.where(take, cost, best_cost)
        best_sad = np.where(take, sad, best_sad)
        best_dx = np.where(take, dx, best_dx)
        best_dy = np.where(take, dy, best_dy)
    if max_sad > 0:
        intra = best_sad > max_sad
        best_dx = np.where(intra, 0, best_dx)
        best_dy = np.where(intra, 0, best_dy)
    rows = np.empty((mbh, mbw, 7), np.int32)
    rows[..., 0] = -1
    rows[..., 1] = 16
    rows[..., 2] = 16
    rows[..., 3] = x0 + 8 + best_dx
    rows[..., 4] = y0 + 8 + best_dy
    rows[..., 5] = x0 + 8
    rows[..., 6] = y0 + 8
    return rows.reshape(mbh * mbw, 7), best_sad.astype(np.int32)


def vectors(rows, mbh, mbw):
    """rows -> (mbh, mbw, 2) int: (dst_x - src_x, dst_y - src_y), the block's displacement from the reference frame to the current one"""
    return np.stack([rows[:, 5] - rows[:, 3], rows[:, 6] - rows[:, 4]], axis=1).reshape(mbh, mbw, 2)


def translated_clip(n, width, height, m, seed=0, sigma=0.0):
    """n frames (H, W, 3) uint8 cut out of one uniform random texture; the content moves by m = (mx, my) pixels per frame
    (frame f shows the world at offset -m * f); sigma: per-frame Gaussian noise added before rounding"""
    rs = np.random.RandomState(seed)
    mx, my = m
    pad_x, pad_y = abs(mx) * (n - 1), abs(my) * (n - 1)
    world = rs.randint(0, 256, (height + 2 * pad_y, width + 2 * pad_x, 3)).astype(np.uint8)
    frames = []
    for f in range(n):
        oy, ox = pad_y - my * f, pad_x - mx * f
        fr = world[oy:oy + height, ox:ox + width]
        if sigma > 0:
            fr = np.clip(np.rint(fr.astype(np.float64) + rs.randn(*fr.shape) * sigma), 0, 255).astype(np.uint8)
        frames.append(np.ascontiguousarray(fr))
    return frames
