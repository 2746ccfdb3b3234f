"""The numpy statement of the 10-bit YUV 4:2:0 intake specification (include/lsfa_hip.h, lsfa_yuv420p10_to_bgr_u8 and its two fused forms;
DESIGN.md "YUV intake", "10-bit planes").  It is what the device kernels are compared with bit for bit; tests/test_yuv10_cpu.py pins it by
cases with known answers and ties it to tests/ref_yuv.py: planes that are exactly 4 x an 8-bit plane give that specification's BGR.
int64 intermediates throughout; `>>` on numpy integers is arithmetic (it floors), as the specification asks.

A sample is a 16-bit word w and s = (w >> shift) & 1023: shift 6 is P010 (the value in the high ten bits), shift 0 is yuv420p10le (the value
in the low ten bits).  Planes may be int16 or uint16 arrays: the word's bits count, not its sign."""
import numpy as np

import ref_yuv

MATRICES = ref_yuv.MATRICES
SHIFTS = {'p010': 6, 'yuv420p10le': 0}
chroma_shape = ref_yuv.chroma_shape
split_uv = ref_yuv.split_uv
transform = ref_yuv.transform


def samples(words, shift):
    """16-bit words (int16 / uint16, or any integer array of values 0..65535) -> the ten-bit samples as int64"""
    assert shift in (0, 6), shift
    w = np.asarray(words)
    if w.dtype == np.int16:
        w = w.view(np.uint16)
    w = w.astype(np.int64)
    assert w.min(initial=0) >= 0 and w.max(initial=0) <= 0xFFFF
    return (w >> shift) & 1023


def convert(Y, U, V, matrix=0):
    """ten-bit samples Y, U, V of one shape (one chroma sample per pixel already) -> uint8 BGR (..., 3): the 8-bit table with the offsets
    times four, rounding constant 512 and shift 10"""
    o, cy, rv, gu, gv, bu = ref_yuv.COEF[MATRICES.get(matrix, matrix)]
    C = np.asarray(Y).astype(np.int64) - 4 * o
    D = np.asarray(U).astype(np.int64) - 512
    E = np.asarray(V).astype(np.int64) - 512
    terms = (cy * C + rv * E + 512, cy * C - gu * D - gv * E + 512, cy * C + bu * D + 512)
    assert all(np.abs(t).max(initial=0) < 1 << 20 for t in terms)
    r, g, b = (np.clip(t >> 10, 0, 255) for t in terms)
    return np.stack([b, g, r], axis=-1).astype(np.uint8)


def y_packed(y, shift):
    """the 8-bit luma plane the search reads: min(255, (Y + 2) >> 2)"""
    return np.minimum(255, (samples(y, shift) + 2) >> 2).astype(np.uint8)


def to_bgr(y, uv=None, u=None, v=None, matrix=0, shift=6):
    """y (H, W) [or (N, H, W)] words and either uv (ch, 2 cw) or u, v (ch, cw), all possibly pitched views -> (H, W, 3) uint8 BGR: pixel
    (x, y) takes Y[y][x] and the chroma sample (x >> 1, y >> 1)"""
    if uv is not None:
        assert u is None and v is None
        u, v = split_uv(uv)
    H, W = y.shape[-2:]
    ch, cw = chroma_shape(H, W)
    assert u.shape[-2:] == (ch, cw) and v.shape[-2:] == (ch, cw), (y.shape, u.shape, v.shape)
    yy, xx = np.arange(H)[:, None] >> 1, np.arange(W)[None, :] >> 1
    return convert(samples(y, shift), samples(u, shift)[..., yy, xx], samples(v, shift)[..., yy, xx], matrix)


# ---- test inputs only -------------------------------------------------------------------------------------------------------------------------
CORNERS = (0, 1, 63, 64, 65, 511, 512, 513, 939, 940, 941, 959, 960, 1022, 1023)


def widen(plane8, shift, low_bits=0):
    """an 8-bit plane as words whose sample is exactly 4 x the byte; low_bits fills what the alignment ignores (shift 6: the low six bits;
    shift 0: the high six)"""
    s = np.asarray(plane8).astype(np.uint16) << 2
    junk = np.uint16(low_bits & 63)
    return ((s << 6) | junk) if shift == 6 else (s | (junk << 10))


def random_words(rs, shape):
    """uniform random full 16-bit words with the corner samples (in both alignments) mixed in"""
    w = rs.randint(0, 1 << 16, shape).astype(np.uint16)
    flat = w.reshape(-1)
    if flat.size >= 4:
        k = max(1, flat.size // 4)
        idx = rs.choice(flat.size, k, replace=False)
        c = np.asarray(CORNERS, np.uint16)[rs.randint(0, len(CORNERS), k)]
        flat[idx] = np.where(rs.randint(0, 2, k) == 1, c << 6, c)
    return w


def interleave(u, v):
    """U, V (ch, cw) words -> the semi-planar (ch, 2 cw) plane"""
    uv = np.empty(u.shape[:-1] + (2 * u.shape[-1],), u.dtype)
    uv[..., 0::2] = u
    uv[..., 1::2] = v
    return uv


def raw_frame_bytes(y, u, v, fmt):
    """one frame as `-f rawvideo -pix_fmt p010le | yuv420p10le` writes it: little-endian words, planes back to back, no pitch, no header"""
    le = lambda a: np.ascontiguousarray(a).astype('<u2').tobytes()          # noqa: E731
    if fmt == 'p010':
        return le(y) + le(interleave(u, v))
    assert fmt == 'yuv420p10le'
    return le(y) + le(u) + le(v)
