"""The numpy statement of the YUV intake's other chroma formats (include/lsfa_hip.h, "YUV intake, other chroma formats": lsfa_yuv_to_bgr_u8
and its two fused forms; DESIGN.md "YUV intake", "Other chroma formats").  It is what the device kernels are compared with bit for bit;
tests/test_yuvfmt_cpu.py pins it by derived answers.  The conversions are tests/ref_yuv.py's `convert` (bytes) and tests/ref_yuv10.py's
`samples`, `convert` and `y_packed` (words); only the chroma ADDRESS is stated here.

A format is code = sub | layout << 4 | sample << 8:
  sub     0: 4:2:0, 1: 4:2:2, 2: 4:4:4 - pixel (x, y) takes Y[y][x] and the chroma sample (x >> sx, y >> sy), SHIFTS[sub] = (sx, sy)
  layout  0: planes U, V   1: interleaved U, V   2: interleaved V, U   3: packed Y0 U Y1 V   4: packed U Y0 V Y1 (3, 4: sub 1, sample 0 only)
  sample  0: bytes   1: words, the value in the low ten bits (ref_yuv10's shift 0)   2: in the high ten bits (shift 6)"""
import numpy as np

import ref_yuv
import ref_yuv10

MATRICES = ref_yuv.MATRICES
transform = ref_yuv.transform
SHIFTS = {0: (1, 1), 1: (1, 0), 2: (0, 0)}
PLANAR, UV, VU, YUYV, UYVY = range(5)


def code(sub, layout, sample):
    return sub | layout << 4 | sample << 8


def fields(c):
    return c & 15, (c >> 4) & 15, (c >> 8) & 15


def valid(c):
    sub, layout, sample = fields(c)
    return 0 <= c < 1 << 12 and sub <= 2 and layout <= 4 and sample <= 2 and (layout < 3 or (sub == 1 and sample == 0))


ALL = [c for c in range(1 << 12) if valid(c)]          # 27 + 2
assert len(ALL) == 29

# the names lsfa_amd.yuvfmt.FORMATS gives (libav's pix_fmt names where there is one)
NAMES = {
    'nv12': code(0, UV, 0), 'i420': code(0, PLANAR, 0), 'nv21': code(0, VU, 0), 'yuv422p': code(1, PLANAR, 0), 'nv16': code(1, UV, 0),
    'nv61': code(1, VU, 0), 'yuyv422': code(1, YUYV, 0), 'yuy2': code(1, YUYV, 0), 'uyvy422': code(1, UYVY, 0), 'yuv444p': code(2, PLANAR, 0),
    'nv24': code(2, UV, 0), 'nv42': code(2, VU, 0), 'p010': code(0, UV, 2), 'yuv420p10le': code(0, PLANAR, 1), 'yuv422p10le': code(1, PLANAR, 1),
    'p210': code(1, UV, 2), 'yuv444p10le': code(2, PLANAR, 1), 'p410': code(2, UV, 2),
}


def chroma_shape(c, H, W):
    sx, sy = SHIFTS[fields(c)[0]]
    return -(-H // (1 << sy)), -(-W // (1 << sx))


def split(c, y, uv=None, u=None, v=None, width=None):
    """the planes as the format lays them out -> Y (.., H, W), U, V (.., ch, cw) of raw samples (bytes or words), and W"""
    _, layout, _ = fields(c)
    if layout >= YUYV:
        assert uv is None and u is None and v is None and y.shape[-1] % 4 == 0
        g = y.reshape(y.shape[:-1] + (y.shape[-1] // 4, 4))
        W = 2 * g.shape[-2] if width is None else width
        assert -(-W // 2) == g.shape[-2]
        yi, ui, vi = ((0, 2), 1, 3) if layout == YUYV else ((1, 3), 0, 2)
        Y = g[..., yi].reshape(y.shape[:-1] + (2 * g.shape[-2],))[..., :W]          # with odd W the last group's second Y is dropped
        return Y, g[..., ui], g[..., vi], W
    W = y.shape[-1]
    assert width in (None, W)
    if layout == PLANAR:
        assert uv is None
        return y, u, v, W
    assert u is None and v is None
    first, second = uv[..., 0::2], uv[..., 1::2]
    return (y, first, second, W) if layout == UV else (y, second, first, W)


def to_bgr(c, y, uv=None, u=None, v=None, matrix=0, width=None):
    """-> (.., H, W, 3) uint8 BGR: pixel (x, y) takes Y[y][x] and the chroma sample (x >> sx, y >> sy)"""
    assert valid(c), c
    sub, _, sample = fields(c)
    Y, U, V, W = split(c, y, uv, u, v, width)
    H = Y.shape[-2]
    assert U.shape[-2:] == chroma_shape(c, H, W) == V.shape[-2:], (Y.shape, U.shape, V.shape)
    sx, sy = SHIFTS[sub]
    yy, xx = np.arange(H)[:, None] >> sy, np.arange(W)[None, :] >> sx
    if sample == 0:
        return ref_yuv.convert(Y, U[..., yy, xx], V[..., yy, xx], matrix)
    shift = 0 if sample == 1 else 6
    return ref_yuv10.convert(ref_yuv10.samples(Y, shift), ref_yuv10.samples(U, shift)[..., yy, xx], ref_yuv10.samples(V, shift)[..., yy, xx], matrix)


def y_packed(c, y, width=None):
    """the 8-bit luma plane the search reads: Y of bytes, ref_yuv10's rule of words"""
    _, layout, sample = fields(c)
    Y = split(c, y, width=width)[0] if layout >= YUYV else y
    return np.ascontiguousarray(Y).astype(np.uint8) if sample == 0 else ref_yuv10.y_packed(Y, 0 if sample == 1 else 6)


# ---- test inputs only -------------------------------------------------------------------------------------------------------------------------
def dtype(c):
    return np.uint8 if fields(c)[2] == 0 else np.uint16


def lay_out(c, Y, U, V):
    """Y (.., H, W) and U, V (.., ch, cw) of raw samples -> the format's planes as the keyword arguments y, uv | u, v; with odd W the packed
    layouts' spare Y byte holds 0x5A"""
    _, layout, _ = fields(c)
    if layout == PLANAR:
        return dict(y=Y, u=U, v=V)
    if layout in (UV, VU):
        uv = np.empty(U.shape[:-1] + (2 * U.shape[-1],), U.dtype)
        uv[..., 0::2], uv[..., 1::2] = (U, V) if layout == UV else (V, U)
        return dict(y=Y, uv=uv)
    gn = U.shape[-1]
    Y2 = np.full(Y.shape[:-1] + (2 * gn,), 0x5A, np.uint8)
    Y2[..., :Y.shape[-1]] = Y
    g = np.empty(Y.shape[:-1] + (gn, 4), np.uint8)
    yi, ui, vi = ((0, 2), 1, 3) if layout == YUYV else ((1, 3), 0, 2)
    g[..., yi[0]], g[..., yi[1]], g[..., ui], g[..., vi] = Y2[..., 0::2], Y2[..., 1::2], U, V
    return dict(y=g.reshape(Y.shape[:-1] + (4 * gn,)))


def random_samples(c, rs, H, W, n=None):
    """Y, U, V of raw samples for one frame (or n): uniform bytes, or ref_yuv10.random_words"""
    lead = () if n is None else (n,)
    shapes = [lead + (H, W)] + [lead + chroma_shape(c, H, W)] * 2
    if fields(c)[2] == 0:
        return tuple(rs.randint(0, 256, s).astype(np.uint8) for s in shapes)
    return tuple(ref_yuv10.random_words(rs, s) for s in shapes)


def plane_bytes(c, H, W):
    """the bytes of each plane of one frame without pitch, in file order"""
    b = np.dtype(dtype(c)).itemsize
    if fields(c)[1] >= YUYV:
        return [H * 4 * -(-W // 2)]
    ch, cw = chroma_shape(c, H, W)
    return [b * H * W, b * ch * cw, b * ch * cw]


def raw_frame_bytes(c, Y, U, V):
    """one frame as `-f rawvideo -pix_fmt X` writes it: little-endian, planes back to back, no pitch, no header"""
    p = lay_out(c, Y, U, V)
    le = lambda a: np.ascontiguousarray(a).astype('<u2' if a.dtype.itemsize == 2 else np.uint8).tobytes()          # noqa: E731
    return b"".join(le(p[k]) for k in ("y", "uv", "u", "v") if k in p)


def upsample(U, V, sub, H, W):
    """4:2:0 chroma planes -> the chroma planes of `sub` that address the same samples: rows written twice (cut to H), for 4:4:4 columns too"""
    if sub >= 1:
        U, V = np.repeat(U, 2, axis=-2)[..., :H, :], np.repeat(V, 2, axis=-2)[..., :H, :]
    if sub == 2:
        U, V = np.repeat(U, 2, axis=-1)[..., :W], np.repeat(V, 2, axis=-1)[..., :W]
    return U, V
