"""tests/ref_yuv.py - the numpy statement of the YUV 4:2:0 intake specification - pinned by cases with known answers: greys, the range's
anchor points, saturated colours, the clip at both ends, a round trip, and the plane geometry (odd sizes, NV12 against I420, pitched
against packed).  tests/test_yuv_gpu.py compares the kernels with ref_yuv bit for bit."""
import numpy as np
import pytest

import ref_yuv

ALL = ('bt601', 'bt709', 'jpeg')


def one(Y, U, V, matrix):
    return tuple(int(c) for c in ref_yuv.convert(np.array([Y]), np.array([U]), np.array([V]), matrix)[0])


@pytest.mark.parametrize("matrix", ALL)
def test_neutral_chroma_is_grey(matrix):
    """U = V = 128: B == G == R at every Y"""
    Y = np.arange(256)
    bgr = ref_yuv.convert(Y, np.full(256, 128), np.full(256, 128), matrix)
    assert (bgr[:, 0] == bgr[:, 1]).all() and (bgr[:, 1] == bgr[:, 2]).all()
    assert (np.diff(bgr[:, 0].astype(int)) >= 0).all()


def test_range_anchor_points():
    for matrix in ('bt601', 'bt709'):
        for Y, want in ((16, 0), (126, 128), (235, 255), (255, 255), (0, 0)):
            assert one(Y, 128, 128, matrix) == (want,) * 3, (matrix, Y)
    assert (ref_yuv.convert(np.arange(256), np.full(256, 128), np.full(256, 128), 'jpeg')[:, 1] == np.arange(256)).all()


def test_saturated_colours_and_both_clip_ends():
    assert one(81, 90, 240, 'bt601') == (0, 0, 255)           # pure red
    # (0, 0, 255): C = -16, D = -128, E = 127: every sum but R's is negative - the arithmetic shift floors, the clip takes 0
    assert one(0, 0, 255, 'bt601') == (0, 0, 184)
    # (255, 255, 0): B and G far above 255, R = (71222 - 52352 + 128) >> 8 = 74
    assert one(255, 255, 0, 'bt601') == (255, 255, 74)
    # the same by hand, unclipped: floor division IS the arithmetic shift
    C, D, E = 0 - 16, 0 - 128, 255 - 128
    assert (298 * C + 409 * E + 128) // 256 == 184 and (298 * C + 516 * D + 128) // 256 < 0


def test_matrix_numbers_and_names_agree():
    rs = np.random.RandomState(0)
    Y, U, V = rs.randint(0, 256, (3, 1000))
    for name, num in ref_yuv.MATRICES.items():
        assert (ref_yuv.convert(Y, U, V, name) == ref_yuv.convert(Y, U, V, num)).all()
    assert not (ref_yuv.convert(Y, U, V, 0) == ref_yuv.convert(Y, U, V, 1)).all()


@pytest.mark.parametrize("matrix", ALL)
def test_round_trip_within_two_levels(matrix):
    """2 x 10^6 seeded random colours -> float forward conversion, rounded -> the specification: every channel within 2 levels.  The bound
    follows from the coefficients: rounding Y, U, V moves each by at most 1/2, which the largest row (B: 298 / 256 * 1/2 + 516 / 256 * 1/2
    = 1.59 for BT.601, 1.64 for BT.709) turns into less than 2 levels, the 8-bit coefficients add less than 0.3 over the range, and the
    final floor(x + 1/2) keeps an error below 2.5 at 2."""
    rs = np.random.RandomState(1234)
    bgr = rs.randint(0, 256, (2000000, 3)).astype(np.uint8)
    yf, uf, vf = ref_yuv.forward_pixels(bgr, matrix)
    back = ref_yuv.convert(np.clip(np.rint(yf), 0, 255), np.clip(np.rint(uf), 0, 255), np.clip(np.rint(vf), 0, 255), matrix)
    err = np.abs(back.astype(np.int64) - bgr.astype(np.int64)).max(axis=0)
    print("round trip %s: max |error| B, G, R = %s" % (matrix, err.tolist()))
    assert (err <= 2).all(), err


def frame(H, W, seed, matrix='bt601'):
    rs = np.random.RandomState(seed)
    return ref_yuv.forward(rs.randint(0, 256, (H, W, 3)).astype(np.uint8), matrix)


@pytest.mark.parametrize("size", [(5, 7), (4, 6), (1, 1), (3, 2), (2, 3)])
def test_odd_sizes_use_ceil_chroma_planes(size):
    H, W = size
    y, u, v = frame(H, W, seed=H * 10 + W)
    ch, cw = -(-H // 2), -(-W // 2)
    assert y.shape == (H, W) and u.shape == (ch, cw) and v.shape == (ch, cw)
    bgr = ref_yuv.to_bgr(y, u=u, v=v)
    assert bgr.shape == (H, W, 3) and bgr.dtype == np.uint8
    for yy in range(H):
        for xx in range(W):
            assert tuple(bgr[yy, xx]) == one(y[yy, xx], u[yy >> 1, xx >> 1], v[yy >> 1, xx >> 1], 'bt601')
    with pytest.raises(AssertionError):
        ref_yuv.to_bgr(y, u=u[:, :cw - 1] if cw > 1 else u[:0], v=v)


@pytest.mark.parametrize("matrix", ALL)
def test_nv12_i420_pitched_and_packed_forms_agree(matrix):
    H, W = 5, 7
    rs = np.random.RandomState(3)
    y = rs.randint(0, 256, (H, W)).astype(np.uint8)
    u, v = rs.randint(0, 256, (2, 3, 4)).astype(np.uint8)
    want = ref_yuv.to_bgr(y, u=u, v=v, matrix=matrix)
    uv = ref_yuv.interleave(u, v)
    assert uv.shape == (3, 8) and (uv[:, 0::2] == u).all() and (uv[:, 1::2] == v).all()
    assert (ref_yuv.to_bgr(y, uv=uv, matrix=matrix) == want).all()
    yp, uvp, up, vp = ref_yuv.pitched(y, 16), ref_yuv.pitched(uv, 16), ref_yuv.pitched(u, 9), ref_yuv.pitched(v, 9)
    assert yp.strides == (16, 1) and not yp.flags['C_CONTIGUOUS']
    assert (ref_yuv.to_bgr(yp, uv=uvp, matrix=matrix) == want).all()
    assert (ref_yuv.to_bgr(yp, u=up, v=vp, matrix=matrix) == want).all()
    # batched
    ys, us, vs = np.stack([y, y[::-1]]), np.stack([u, v]), np.stack([v, u])
    got = ref_yuv.to_bgr(ys, u=us, v=vs, matrix=matrix)
    assert (got[0] == want).all() and (got[1] == ref_yuv.to_bgr(y[::-1], u=v, v=u, matrix=matrix)).all()


def test_transform_is_the_float64_formula():
    bgr = np.array([[[0, 128, 255]]], np.uint8)
    means, ps = (102.9801, 115.9465, 122.7717), 0.0125
    out = ref_yuv.transform(bgr, means, ps)
    assert out.shape == (3, 1, 1) and out.dtype == np.float32
    assert out[0, 0, 0] == np.float32((255.0 - 122.7717) * 0.0125) and out[2, 0, 0] == np.float32((0.0 - 102.9801) * 0.0125)


def test_raw_frame_bytes_layout():
    y, u, v = frame(4, 6, seed=9)
    nv12, i420 = ref_yuv.raw_frame_bytes(y, u, v, 'nv12'), ref_yuv.raw_frame_bytes(y, u, v, 'i420')
    assert len(nv12) == len(i420) == 24 + 12
    assert nv12[:24] == y.tobytes() and nv12[24] == u[0, 0] and nv12[25] == v[0, 0]
    assert i420[24:30] == u.tobytes() and i420[30:] == v.tobytes()
