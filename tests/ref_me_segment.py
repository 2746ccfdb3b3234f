"""The numpy statement of the walk lsfa_mv_segment_inputs rests on (include/lsfa_hip.h; DESIGN.md "Motion estimation"): the accumulated source
map of frame f from the macroblock rows of frames 1..f alone, without accumulating frame by frame.

The rows of lsfa_mv_estimate[_chain] (tests/ref_me.py) partition the frame into their destination blocks, so the block that contains a pixel
is its last writer and
    accu_f[p] = accu_{f-1}[p + src - dst of frame f's row at p's block] = ... :
    q = p;  for k = f .. 1:  q' = q + (row[3] - row[5], row[4] - row[6]),  row = rows[k - 1][(q.y >> 4) * mbw + (q.x >> 4)];
    the step is not taken where q' lies outside the frame (the accumulation does not write a pixel whose source is outside).
tests/test_me_segment_cpu.py pins this against oracle.coviar_accumulate chained over ref_me.estimate rows."""
import numpy as np


def walk(rows, width, height):
    """rows (F, mbh * mbw, 7) int32, one row per macroblock in grid order -> [accu_1, .., accu_F], each (H, W, 2) int32 = the (x, y) in the
    key frame that pixel (x, y) of frame f comes from (what oracle.coviar_accumulate leaves after frames 1..f)"""
    rows = np.asarray(rows)
    mbh, mbw = -(-height // 16), -(-width // 16)
    assert rows.ndim == 3 and rows.shape[1:] == (mbh * mbw, 7)
    ys, xs = np.mgrid[0:height, 0:width]
    out = []
    for f in range(1, rows.shape[0] + 1):
        qx, qy = xs.astype(np.int64), ys.astype(np.int64)
        for k in range(f, 0, -1):
            row = rows[k - 1][(qy >> 4) * mbw + (qx >> 4)].astype(np.int64)              # (H, W, 7): the row of the block that contains q
            nx, ny = qx + (row[..., 3] - row[..., 5]), qy + (row[..., 4] - row[..., 6])
            inside = (nx >= 0) & (nx < width) & (ny >= 0) & (ny < height)
            qx, qy = np.where(inside, nx, qx), np.where(inside, ny, qy)
        out.append(np.stack([qx, qy], axis=-1).astype(np.int32))
    return out


def field(accu):
    """mv = p - q, (H, W, 2) int32: lsfa_mv_field / oracle.coviar_mv"""
    height, width = accu.shape[:2]
    ys, xs = np.mgrid[0:height, 0:width]
    return np.stack([xs - accu[..., 0], ys - accu[..., 1]], axis=-1).astype(np.int32)


def residual(cur, key, accu):
    """res = cur[p] - key[q], (H, W, 3) int32: lsfa_mv_residual / oracle.coviar_residual"""
    return cur.astype(np.int32) - key[accu[..., 1], accu[..., 0]].astype(np.int32)
