"""The numpy statement of the scene-cut specification (include/lsfa_hip.h, lsfa_mv_cut_score; DESIGN.md "Scene cuts"), built on tests/ref_me.py:
a macroblock's intra cost (the sum of |p - mean| over its covered pixels of the CURRENT plane), the count of blocks whose search residual
exceeds it, the frame decision and the key-frame plan the loader follows.  It is what the device kernels are compared with bit for bit;
tests/test_me_cut_cpu.py pins it by cases with a known answer.  Integer arithmetic throughout, one answer per input."""
import numpy as np

BIAS, PERCENT = 4, 50


def block_pixels(height, width):
    """(mbh, mbw) int64: the covered pixels n_b of every macroblock of the level-0 grid (256, fewer at the right and bottom edges)"""
    mbh, mbw = -(-height // 16), -(-width // 16)
    bh = np.minimum(16, height - 16 * np.arange(mbh))[:, None]
    bw = np.minimum(16, width - 16 * np.arange(mbw))[None, :]
    return (bh * bw).astype(np.int64)


def intra(y):
    """(H, W) uint8 plane -> (mbh, mbw) int32: m_b = (sum p + n_b / 2) / n_b in integers, intra_b = sum |p - m_b|, both over the covered pixels"""
    assert y.dtype == np.uint8 and y.ndim == 2
    H, W = y.shape
    mbh, mbw = -(-H // 16), -(-W // 16)
    n = block_pixels(H, W)
    p = np.zeros((mbh * 16, mbw * 16), np.int64)
    p[:H, :W] = y
    covered = np.zeros((mbh * 16, mbw * 16), np.int64)
    covered[:H, :W] = 1
    total = p.reshape(mbh, 16, mbw, 16).sum(axis=(1, 3))
    mean = (total + n // 2) // n
    dev = np.abs(p - np.repeat(np.repeat(mean, 16, axis=0), 16, axis=1)) * covered
    return dev.reshape(mbh, 16, mbw, 16).sum(axis=(1, 3)).astype(np.int32)


def unmatched_blocks(sad, intra_cost, height, width, bias=BIAS):
    """(mbh, mbw) bool: inter_b > intra_b + bias * n_b"""
    assert 0 <= bias <= 255
    return sad.astype(np.int64) > intra_cost.astype(np.int64) + bias * block_pixels(height, width)


def cut_score(planes, sad, bias=BIAS):
    """planes (C, F + 1, H, W) uint8, sad (C, F, mbh, mbw) int32 as a search wrote it -> intra (C, F, mbh, mbw) int32 (of plane f = 1..F),
    unmatched (C, F) int32"""
    C, F1, H, W = planes.shape
    cost = np.stack([np.stack([intra(planes[c, f]) for f in range(1, F1)]) for c in range(C)])
    assert sad.shape == cost.shape
    un = np.stack([np.stack([unmatched_blocks(sad[c, f], cost[c, f], H, W, bias).sum() for f in range(F1 - 1)]) for c in range(C)])
    return cost, un.astype(np.int32)


def is_cut(unmatched, blocks, percent=PERCENT):
    """unmatched * 100 > percent * mbh * mbw, elementwise"""
    assert 1 <= percent <= 100
    return np.asarray(unmatched, np.int64) * 100 > percent * int(blocks)


def first_cuts(unmatched, blocks, percent=PERCENT):
    """unmatched (C, F) -> per chain the first f (1-based) whose pair is a cut, or None"""
    flags = is_cut(unmatched, blocks, percent)
    return [int(np.argmax(row)) + 1 if row.any() else None for row in flags]


def key_plan_brute(length, interval, cuts):
    """The key frames of a video of `length` frames, frame by frame: frame f is a key frame iff it is the first or the last frame, a cut
    frame, or `interval` frames behind the key frame in front of it.  (The restatement lsfa_amd.core.loader.key_plan is tested against.)"""
    keys, last = [], None
    for f in range(length):
        if f == 0 or f == length - 1 or f in cuts or f - last == interval:
            keys.append(f)
            last = f
    return keys


# the end-to-end clip (tests/test_me_cut_cpu.py: the margin check; tests/test_me_cut_gpu.py: the loader and both frame loops on it).  At
# 96 x 160 the synthetic clip's rectangles, which wrap around the frame's edges, left up to 36 of 60 blocks unmatched inside a scene;
# at 128 x 192 with search 8 every pair lies far from the decision (the margin check states how far).
E2E = dict(clip_id=0, frames=24, height=128, width=192, interval=10, cuts=(4, 17), search=8, keys=[0, 4, 14, 17, 23])


def e2e_unmatched():
    """the E2E clip's luma planes through ref_me.estimate and this module: unmatched per pair f = 1..frames - 1, and the blocks of a plane"""
    import ref_me
    from lsfa_amd.utils.synthetic import SyntheticClip
    e = E2E
    clip = SyntheticClip(e['clip_id'], e['frames'], e['height'], e['width'], e['interval'], cuts=e['cuts'])
    ys = [ref_me.luma(clip.frame_u8(f).numpy()) for f in range(e['frames'])]
    counts = []
    for f in range(1, e['frames']):
        _, sad = ref_me.estimate(ys[f], ys[f - 1], e['search'], 4, 0)
        counts.append(int(unmatched_blocks(sad, intra(ys[f]), e['height'], e['width'], BIAS).sum()))
    return counts, int(block_pixels(e['height'], e['width']).size)
