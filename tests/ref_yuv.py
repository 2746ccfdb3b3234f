"""The numpy statement of the YUV 4:2:0 intake specification (include/lsfa_hip.h, lsfa_yuv420_to_bgr_u8 and its two fused forms; DESIGN.md
"YUV intake").  It is what the device kernels are compared with bit for bit; tests/test_yuv_cpu.py pins it by cases with known answers.
int64 intermediates throughout; `>>` on numpy integers is arithmetic (it floors), as the specification asks.

`forward` is NOT part of the specification: a float BGR -> YUV 4:2:0 conversion (rounded, clipped, the chroma of each 2 x 2 block averaged)
that only makes test inputs."""
import numpy as np

MATRICES = {'bt601': 0, 'bt709': 1, 'jpeg': 2}
# matrix: (o, cy, rv, gu, gv, bu):  R = clip((cy C + rv E + 128) >> 8), G = clip((cy C - gu D - gv E + 128) >> 8), B = clip((cy C + bu D + 128) >> 8)
COEF = {0: (16, 298, 409, 100, 208, 516), 1: (16, 298, 459, 55, 136, 541), 2: (0, 256, 359, 88, 183, 454)}


def convert(Y, U, V, matrix=0):
    """Y, U, V integer arrays of one shape (one chroma sample per pixel already) -> uint8 BGR (..., 3)"""
    o, cy, rv, gu, gv, bu = COEF[MATRICES.get(matrix, matrix)]
    C = np.asarray(Y).astype(np.int64) - o
    D = np.asarray(U).astype(np.int64) - 128
    E = np.asarray(V).astype(np.int64) - 128
    r = np.clip((cy * C + rv * E + 128) >> 8, 0, 255)
    g = np.clip((cy * C - gu * D - gv * E + 128) >> 8, 0, 255)
    b = np.clip((cy * C + bu * D + 128) >> 8, 0, 255)
    return np.stack([b, g, r], axis=-1).astype(np.uint8)


def chroma_shape(H, W):
    return -(-H // 2), -(-W // 2)


def split_uv(uv):
    """NV12's interleaved (ch, 2 cw) plane -> U, V (ch, cw)"""
    return uv[..., 0::2], uv[..., 1::2]


def to_bgr(y, uv=None, u=None, v=None, matrix=0):
    """y (H, W) [or (N, H, W)] uint8 and either uv (ch, 2 cw) or u, v (ch, cw), all possibly pitched views -> (H, W, 3) uint8 BGR:
    pixel (x, y) takes Y[y][x] and the chroma sample (x >> 1, y >> 1)"""
    if uv is not None:
        assert u is None and v is None
        u, v = split_uv(uv)
    H, W = y.shape[-2:]
    ch, cw = chroma_shape(H, W)
    assert u.shape[-2:] == (ch, cw) and v.shape[-2:] == (ch, cw), (y.shape, u.shape, v.shape)
    yy, xx = np.arange(H)[:, None] >> 1, np.arange(W)[None, :] >> 1
    return convert(y, u[..., yy, xx], v[..., yy, xx], matrix)


def transform(bgr, pixel_means, pixel_scale):
    """(..., H, W, 3) uint8 BGR -> (..., 3, H, W) float32, channel i = (bgr[2 - i] - pixel_means[2 - i]) * pixel_scale in float64, rounded once"""
    x = bgr.astype(np.float64)
    out = np.stack([(x[..., 2 - i] - float(pixel_means[2 - i])) * float(pixel_scale) for i in range(3)], axis=-3)
    return out.astype(np.float32)


# ---- test inputs only -------------------------------------------------------------------------------------------------------------------------
_FWD = {
    # (offset, Y row over (R, G, B), U row, V row); the limited-range rows are the full-range ones times 219 / 255 (luma), 224 / 255 (chroma)
    0: (16.0, (0.299, 0.587, 0.114)),
    1: (16.0, (0.2126, 0.7152, 0.0722)),
    2: (0.0, (0.299, 0.587, 0.114)),
}


def forward_pixels(bgr, matrix=0):
    """(..., 3) BGR (any real dtype) -> float Y, U, V per pixel (not rounded)"""
    m = MATRICES.get(matrix, matrix)
    off, (kr, kg, kb) = _FWD[m]
    x = np.asarray(bgr, dtype=np.float64)
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    yf = kr * r + kg * g + kb * b
    pb, pr = (b - yf) / (2.0 * (1.0 - kb)), (r - yf) / (2.0 * (1.0 - kr))
    if m == 2:
        return yf, 128.0 + pb, 128.0 + pr
    return off + yf * 219.0 / 255.0, 128.0 + pb * 224.0 / 255.0, 128.0 + pr * 224.0 / 255.0


def _round_u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def forward(bgr, matrix=0):
    """(H, W, 3) uint8 BGR -> y (H, W), u, v (ceil(H / 2), ceil(W / 2)) uint8: rounded, clipped, the chroma of each 2 x 2 block (what of it
    lies inside the frame) averaged"""
    H, W = bgr.shape[:2]
    ch, cw = chroma_shape(H, W)
    yf, uf, vf = forward_pixels(bgr, matrix)

    def pool(a):
        p = np.full((2 * ch, 2 * cw), np.nan)
        p[:H, :W] = a
        return np.nanmean(p.reshape(ch, 2, cw, 2), axis=(1, 3))

    return _round_u8(yf), _round_u8(pool(uf)), _round_u8(pool(vf))


def interleave(u, v):
    """U, V (ch, cw) -> NV12's (ch, 2 cw) plane"""
    uv = np.empty(u.shape[:-1] + (2 * u.shape[-1],), np.uint8)
    uv[..., 0::2] = u
    uv[..., 1::2] = v
    return uv


def pitched(plane, pitch, fill=0xA5):
    """a (..., rows, cols) plane as a view of rows `pitch` bytes long (the tail holds `fill`): what a decoder's surface looks like"""
    assert pitch >= plane.shape[-1]
    buf = np.full(plane.shape[:-1] + (pitch,), fill, np.uint8)
    buf[..., :plane.shape[-1]] = plane
    return buf[..., :plane.shape[-1]]


def raw_frame_bytes(y, u, v, fmt):
    """one frame as `-f rawvideo -pix_fmt nv12 | yuv420p` writes it: planes back to back, no pitch, no header"""
    if fmt == 'nv12':
        return y.tobytes() + interleave(u, v).tobytes()
    assert fmt == 'i420'
    return y.tobytes() + np.ascontiguousarray(u).tobytes() + np.ascontiguousarray(v).tobytes()
