"""The numpy statement of the stale-key-frame specification (include/lsfa_hip.h, lsfa_mv_key_sad / lsfa_mv_key_sad_accu; DESIGN.md "Stale key
frames"), built on tests/ref_me_segment.py (the walk back to the key frame) and tests/ref_me_cut.py (the decision, unchanged): the SAD of
every macroblock of frame f against the KEY frame, compensated with the accumulated vectors - `res_diff` before its resize, per block.  It
is what the device kernels are compared with bit for bit; tests/test_me_stale_cpu.py pins it by cases with a known answer.  Integer
arithmetic throughout, one answer per input."""
import numpy as np

import ref_me_cut
import ref_me_segment

BIAS, PERCENT = 4, 50


def key_sad_accu(cur, key, accu):
    """cur, key (H, W) uint8; accu (H, W, 2) int32, the (x, y) in the key frame every pixel comes from -> (mbh, mbw) int32: per macroblock
    the sum over its covered pixels p of |cur[p] - key[accu[p]]|; a source position outside the plane reads as 0"""
    assert cur.dtype == np.uint8 and key.dtype == np.uint8 and cur.shape == key.shape and accu.shape == cur.shape + (2,)
    H, W = cur.shape
    mbh, mbw = -(-H // 16), -(-W // 16)
    qx, qy = accu[..., 0].astype(np.int64), accu[..., 1].astype(np.int64)
    inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
    src = np.where(inside, key[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)].astype(np.int64), 0)
    diff = np.zeros((mbh * 16, mbw * 16), np.int64)
    diff[:H, :W] = np.abs(cur.astype(np.int64) - src)
    return diff.reshape(mbh, 16, mbw, 16).sum(axis=(1, 3)).astype(np.int32)


def key_sad(planes, rows):
    """planes (C, F + 1, H, W) uint8, plane 0 of a chain its key frame; rows (C, F, mbh * mbw, 7) int32, the level-0 rows of frames 1..F ->
    keysad (C, F, mbh, mbw) int32: key_sad_accu(P_f, P_0, q_f) with q_f = ref_me_segment.walk's position in the key frame"""
    C, F1, H, W = planes.shape
    assert rows.shape[:2] == (C, F1 - 1)
    out = []
    for c in range(C):
        accu = ref_me_segment.walk(rows[c], W, H)
        out.append(np.stack([key_sad_accu(planes[c, f], planes[c, 0], accu[f - 1]) for f in range(1, F1)]))
    return np.stack(out)


def key_score(planes, rows, bias=BIAS):
    """-> keysad, intra (C, F, mbh, mbw) int32 and unmatched (C, F) int32: ref_me_cut.cut_score with keysad in the place of the search's sad"""
    sad = key_sad(planes, rows)
    cost, un = ref_me_cut.cut_score(planes, sad, bias)
    return sad, cost, un


def first_flagged(*flag_rows):
    """flag arrays (C, F) of several rules -> per chain the first f (1-based) that any of them flags, or None"""
    flags = np.logical_or.reduce([np.asarray(f, bool) for f in flag_rows])
    return [int(np.argmax(row)) + 1 if row.any() else None for row in flags]


def plan(ys, interval, search, cut=None, stale=None, lam=4):
    """The key frames of a clip of luma planes `ys`, as the loader finds them: segment by segment from each key frame, ref_me.estimate's rows
    and SADs of every pair of the segment, the pair rule on the SADs (cut=(bias, percent) or None), the key rule on the walk back to the
    segment's key frame (stale=(bias, percent) or None), the first frame either flags becoming the next key frame.  -> (keys, {key frame:
    (pair counts, key counts)} of every segment estimated), counts as lists over the segment's frames"""
    import ref_me
    L = len(ys)
    H, W = ys[0].shape
    blocks = int(ref_me_cut.block_pixels(H, W).size)
    keys, counts = [0], {}
    while keys[-1] < L - 1:
        k = keys[-1]
        n = min(k + interval - 1, L - 2) - k
        flagged = None
        if n >= 1:
            est = [ref_me.estimate(ys[f], ys[f - 1], search, lam, 0) for f in range(k + 1, k + n + 1)]
            rows = np.stack([r for r, _ in est])[None]
            sad = np.stack([s for _, s in est])[None]
            stack = np.stack(ys[k:k + n + 1])[None]
            flags, pair_un, key_un = [], None, None
            if cut is not None:
                _, pair_un = ref_me_cut.cut_score(stack, sad, cut[0])
                flags.append(ref_me_cut.is_cut(pair_un, blocks, cut[1]))
            if stale is not None:
                _, _, key_un = key_score(stack, rows, stale[0])
                flags.append(ref_me_cut.is_cut(key_un, blocks, stale[1]))
            counts[k] = (None if pair_un is None else pair_un[0].tolist(), None if key_un is None else key_un[0].tolist())
            flagged = first_flagged(*flags)[0] if flags else None
        keys.append(k + flagged if flagged is not None else min(k + interval, L - 1))
    return keys, counts


# ---- the clips the tests share (tests/test_me_stale_cpu.py records the reference's counts on them and checks their margin; tests/test_me_stale_gpu.py
# runs the estimators on them).  Grey frames: lsfa_luma_u8 of (v, v, v) is v, so a plane is its own luma --------------------------------------------
def smooth_texture(seed, height, width, k=5):
    """(H, W) float64: uniform noise under a k x k box filter, scaled to mean 128 and standard deviation 50"""
    r = np.random.RandomState(seed)
    a = r.uniform(0, 255, (height + k - 1, width + k - 1))
    c = np.cumsum(np.cumsum(np.pad(a, ((1, 0), (1, 0))), 0), 1)
    b = (c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]) / (k * k)
    return (b - b.mean()) / b.std() * 50 + 128


def noisy(img, seed, sigma=2.0):
    """the plane as uint8 under Gaussian noise of its own seed"""
    r = np.random.RandomState(seed)
    return np.clip(np.rint(img + r.randn(*img.shape) * sigma), 0, 255).astype(np.uint8)


def dissolve_clip(width=96, height=64, length=5):
    """eight planes for length = 5: two of scene A, `length` frames of a linear blend (weight (i + 1) / (length + 1) of scene B), one of B"""
    a, b = smooth_texture(1, height, width), smooth_texture(2, height, width)
    ys = [noisy(a, 10), noisy(a, 9)]
    for i in range(length):
        w = (i + 1) / (length + 1.0)
        ys.append(noisy((1 - w) * a + w * b, 11 + i))
    return ys + [noisy(b, 40)]


def cut_clip(width=96, height=64):
    """seven planes: four of scene A, three of scene B - a hard cut at frame 4"""
    a, b = smooth_texture(1, height, width), smooth_texture(2, height, width)
    return [noisy(a, 10 + i) for i in range(4)] + [noisy(b, 20 + i) for i in range(3)]


def pan_clip(width=250, height=130, frames=9, m=(2, -1)):
    """a window that moves by m per frame over one texture: content pans in along two edges"""
    pad = 20
    big = smooth_texture(3, height + 2 * pad, width + 2 * pad)
    return [noisy(big[pad - m[1] * f:pad - m[1] * f + height, pad - m[0] * f:pad - m[0] * f + width], 30 + f) for f in range(frames)]


def chain_counts(ys, search, lam=4, bias=BIAS):
    """a chain of luma planes, plane 0 its key frame -> (the pair rule's counts, the key rule's counts) per frame f = 1.., and the blocks of a plane"""
    import ref_me
    est = [ref_me.estimate(ys[f], ys[f - 1], search, lam, 0) for f in range(1, len(ys))]
    rows, sad = np.stack([r for r, _ in est])[None], np.stack([s for _, s in est])[None]
    stack = np.stack(ys)[None]
    pair_un = ref_me_cut.cut_score(stack, sad, bias)[1]
    key_un = key_score(stack, rows, bias)[2]
    return pair_un[0].tolist(), key_un[0].tolist(), int(ref_me_cut.block_pixels(*ys[0].shape).size)


def bgr(y):
    """a luma plane as the grey (H, W, 3) uint8 frame whose lsfa_luma_u8 it is"""
    return np.ascontiguousarray(np.repeat(y[:, :, None], 3, axis=2))
