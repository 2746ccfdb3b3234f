"""tests/ref_yuv10.py (the numpy statement of the 10-bit YUV 4:2:0 intake) pinned without a GPU: its tie to tests/ref_yuv.py on planes that are
4 x an 8-bit plane, cases with known answers, the bits each alignment ignores; and the refusals of lsfa_amd/yuv10.py's wrappers under the spy
and the stand-in CUDA tensors of tests/binding_contract.py: nothing may be recorded as launched."""
import numpy as np
import pytest
import torch

import binding_contract as bc
import ref_yuv
import ref_yuv10
from lsfa_amd import hip, yuv10

MATRICES = ("bt601", "bt709", "jpeg")
SHIFTS = (6, 0)


def colours():
    """2 x 10^6 random 8-bit (Y, U, V) triples and every combination of the corner bytes"""
    rs = np.random.RandomState(10)
    c = np.array([0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 239, 240, 254, 255], np.uint8)
    corners = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([rs.randint(0, 256, (2000000, 3)).astype(np.uint8), corners])


@pytest.mark.parametrize("matrix", MATRICES)
def test_four_times_an_8_bit_plane_gives_the_8_bit_specification(matrix):
    yuv8 = colours()
    want = ref_yuv.convert(yuv8[:, 0], yuv8[:, 1], yuv8[:, 2], matrix)
    rs = np.random.RandomState(11)
    for shift in SHIFTS:
        junk = rs.randint(0, 64, yuv8.shape)
        w = [ref_yuv10.widen(yuv8[:, i], shift) | (junk[:, i] if shift == 6 else junk[:, i] << 10).astype(np.uint16) for i in range(3)]
        s = [ref_yuv10.samples(p, shift) for p in w]
        assert all((s[i] == 4 * yuv8[:, i].astype(np.int64)).all() for i in range(3))
        np.testing.assert_array_equal(ref_yuv10.convert(s[0], s[1], s[2], matrix), want)
        np.testing.assert_array_equal(ref_yuv10.y_packed(w[0], shift), yuv8[:, 0])
    assert want.min() == 0 and want.max() == 255


@pytest.mark.parametrize("matrix", MATRICES)
def test_every_intermediate_stays_below_2_to_the_20(matrix):
    """the extremes of all three samples (the terms are linear in each): |term| < 2^20, so int32 holds them with room to spare"""
    e = np.array([0, 1023], np.int64)
    Y, U, V = np.meshgrid(e, e, e, indexing="ij")
    o, cy, rv, gu, gv, bu = ref_yuv.COEF[ref_yuv.MATRICES[matrix]]
    C, D, E = Y - 4 * o, U - 512, V - 512
    for term in (cy * C + rv * E + 512, cy * C - gu * D - gv * E + 512, cy * C + bu * D + 512):
        assert np.abs(term).max() < 1 << 20
    ref_yuv10.convert(Y, U, V, matrix)              # ... and the reference asserts the same on whatever it is given


@pytest.mark.parametrize("matrix", MATRICES)
def test_neutral_chroma_is_grey_at_every_luma(matrix):
    Y = np.arange(1024)
    bgr = ref_yuv10.convert(Y, np.full(1024, 512), np.full(1024, 512), matrix)
    assert (bgr[:, 0] == bgr[:, 1]).all() and (bgr[:, 1] == bgr[:, 2]).all()
    assert (np.diff(bgr[:, 0].astype(int)) >= 0).all() and bgr[0, 0] == 0 and bgr[-1, 0] == 255


def test_limited_range_black_white_and_above():
    for matrix in ("bt601", "bt709"):
        bgr = ref_yuv10.convert(np.array([64, 940, 1023]), np.full(3, 512), np.full(3, 512), matrix)
        assert bgr.tolist() == [[0, 0, 0], [255, 255, 255], [255, 255, 255]]
    # full range maps Y to round(Y / 4), saturated
    bgr = ref_yuv10.convert(np.array([0, 2, 512, 1021, 1023]), np.full(5, 512), np.full(5, 512), "jpeg")
    assert bgr[:, 0].tolist() == [0, 1, 128, 255, 255]
    assert ref_yuv10.y_packed(np.array([0, 1, 2, 64, 940, 1020, 1021, 1022, 1023], np.uint16), 0).tolist() == [0, 0, 1, 16, 235, 255, 255, 255, 255]


@pytest.mark.parametrize("shift", SHIFTS)
def test_the_bits_an_alignment_ignores_are_ignored(shift):
    """random full 16-bit words against the same words with the ignored six bits cleared, set and re-drawn: one frame, both layouts"""
    rs = np.random.RandomState(12 + shift)
    H, W = 9, 14
    ch, cw = ref_yuv10.chroma_shape(H, W)
    y, u, v = (rs.randint(0, 1 << 16, s).astype(np.uint16) for s in ((H, W), (ch, cw), (ch, cw)))
    ignored = np.uint16(0x003F if shift == 6 else 0xFC00)
    want = ref_yuv10.to_bgr(y, u=u, v=v, matrix="bt709", shift=shift)
    for change in (lambda a: a & ~ignored, lambda a: a | ignored, lambda a: (a & ~ignored) | (rs.randint(0, 1 << 16, a.shape).astype(np.uint16) & ignored)):
        y2, u2, v2 = change(y), change(u), change(v)
        np.testing.assert_array_equal(ref_yuv10.to_bgr(y2, u=u2, v=v2, matrix="bt709", shift=shift), want)
        np.testing.assert_array_equal(ref_yuv10.to_bgr(y2, uv=ref_yuv10.interleave(u2, v2), matrix="bt709", shift=shift), want)
        np.testing.assert_array_equal(ref_yuv10.y_packed(y2, shift), ref_yuv10.y_packed(y, shift))
    # int16 views of the same words are the same input
    np.testing.assert_array_equal(ref_yuv10.to_bgr(y.view(np.int16), u=u.view(np.int16), v=v.view(np.int16), matrix="bt709", shift=shift), want)
    # the other alignment reads other bits: not the same picture
    assert (ref_yuv10.to_bgr(y, u=u, v=v, matrix="bt709", shift=6 - shift) != want).any()


def test_raw_frame_bytes_are_little_endian_words():
    y, u, v = np.array([[0x0102, 0x0304]], np.uint16), np.array([[0x0506]], np.uint16), np.array([[0x0708]], np.uint16)
    assert ref_yuv10.raw_frame_bytes(y, u, v, "p010") == bytes([2, 1, 4, 3, 6, 5, 8, 7])
    assert ref_yuv10.raw_frame_bytes(y, u, v, "yuv420p10le") == bytes([2, 1, 4, 3, 6, 5, 8, 7])
    y = np.arange(8, dtype=np.uint16).reshape(2, 4)
    u, v = np.array([[10, 11]], np.uint16), np.array([[20, 21]], np.uint16)
    assert np.frombuffer(ref_yuv10.raw_frame_bytes(y, u, v, "p010"), "<u2").tolist() == list(range(8)) + [10, 20, 11, 21]
    assert np.frombuffer(ref_yuv10.raw_frame_bytes(y, u, v, "yuv420p10le"), "<u2").tolist() == list(range(8)) + [10, 11, 20, 21]


# ---- the wrappers under the spy ---------------------------------------------------------------------------------------------------------
H, W = 6, 10
WRAPPERS = (yuv10.yuv420p10_to_bgr_u8, yuv10.image_transform_yuv420p10, yuv10.image_resize_transform_yuv420p10)


@pytest.fixture()
def spied(monkeypatch):
    spy = bc.Spy(hip.lib())
    monkeypatch.setattr(hip, "lib", lambda: spy)
    with bc.fake_cuda(monkeypatch):
        yield spy


def words(*shape, dtype=torch.int16):
    return torch.zeros(shape, dtype=dtype).as_subclass(bc.FakeCuda)


def planes(semi=True, dtype=torch.int16):
    if semi:
        return dict(y=words(H, W, dtype=dtype), uv=words(3, 10, dtype=dtype))
    return dict(y=words(H, W, dtype=dtype), u=words(3, 5, dtype=dtype), v=words(3, 5, dtype=dtype))


def short_pitch(rows, cols):
    """(rows, cols) words whose rows start cols - 2 words apart: a pitch below the row"""
    return torch.as_strided(words(rows * cols), (rows, cols), (cols - 2, 1))


def refused(spy, fn, **kw):
    del spy.calls[:]
    with pytest.raises(hip.LsfaError):
        fn(**kw)
    assert not spy.calls, "%s launched %s before refusing" % (fn.__name__, spy.launched())


def test_well_formed_calls_reach_their_exports_with_byte_pitches_and_the_shift(spied):
    big = words(H, W + 6)
    y = big[:, :W]                                     # a pitched row view: 16 words = 32 bytes from row to row
    assert yuv10.yuv420p10_to_bgr_u8(y, uv=words(3, 10)).shape == (H, W, 3)
    got = spied.values("lsfa_yuv420p10_to_bgr_u8")
    assert (got["y_pitch"], got["c_pitch"], got["N"], got["H"], got["W"], got["matrix"], got["shift"], got["v"]) == (32, 20, 1, H, W, 0, 6, None)
    del spied.calls[:]
    out = yuv10.image_transform_yuv420p10(matrix="bt709", msb_aligned=False, **planes(semi=False, dtype=torch.uint16))
    got = spied.values("lsfa_image_transform_yuv420p10")
    assert tuple(out.shape) == (1, 3, H, W) and (got["y_pitch"], got["c_pitch"], got["matrix"], got["shift"]) == (20, 10, 1, 0) and got["v"] is not None
    del spied.calls[:]
    n3 = dict(y=words(3, H, W), uv=words(3, 3, 10))
    out = yuv10.image_resize_transform_yuv420p10(im_scale=1.25, stride=16, **n3)
    got = spied.values("lsfa_image_resize_transform_yuv420p10")
    assert tuple(out.shape) == (3, 3, 16, 16) and (got["N"], got["y_frame_stride"], got["c_frame_stride"], got["h1"], got["w1"]) == (3, 120, 60, 8, 12)
    assert spied.launched() == ["lsfa_image_resize_transform_yuv420p10"]


@pytest.mark.parametrize("fn", WRAPPERS, ids=[f.__name__ for f in WRAPPERS])
def test_bad_planes_are_refused_before_anything_is_launched(spied, fn):
    semi, planar = planes(), planes(semi=False)
    host = {k: bc.plain(t).clone() for k, t in semi.items()}
    refused(spied, fn, **host)                                                                  # host tensors
    refused(spied, fn, y=host["y"], uv=semi["uv"])
    refused(spied, fn, y=semi["y"], uv=host["uv"])
    refused(spied, fn, y=planar["y"], u=planar["u"], v=bc.plain(planar["v"]).clone())
    refused(spied, fn, y=words(H, W, dtype=torch.uint8), uv=words(3, 10, dtype=torch.uint8))    # 8-bit planes belong to hip.*yuv420*
    refused(spied, fn, y=semi["y"], uv=words(3, 10, dtype=torch.uint8))
    refused(spied, fn, y=words(H, W, dtype=torch.float32), uv=semi["uv"])                       # a float plane
    refused(spied, fn, y=words(H, W, dtype=torch.int32), uv=semi["uv"])
    refused(spied, fn, y=semi["y"], uv=words(3, 5))                                             # wrong chroma shapes
    refused(spied, fn, y=semi["y"], uv=words(2, 10))
    refused(spied, fn, y=semi["y"], u=words(3, 10), v=words(3, 10))
    refused(spied, fn, y=semi["y"], u=planar["u"], v=words(3, 4))
    refused(spied, fn, y=semi["y"], uv=words(1, 3, 10))                                         # ranks differ
    refused(spied, fn, y=words(2, H, W), uv=words(3, 3, 10))                                    # frame counts differ
    refused(spied, fn, y=short_pitch(H, W), uv=semi["uv"])                                      # a pitch below its row
    refused(spied, fn, y=semi["y"], uv=short_pitch(3, 10))
    refused(spied, fn, y=semi["y"], u=short_pitch(3, 5), v=short_pitch(3, 5))
    refused(spied, fn, y=words(H, 2 * W)[:, ::2], uv=semi["uv"])                                # a last dimension that is not dense
    refused(spied, fn, y=semi["y"], u=planar["u"], v=words(3, 8)[:, :5])                        # u and v of different pitch
    refused(spied, fn, y=semi["y"], uv=semi["uv"], u=planar["u"], v=planar["v"])                # both uv and u
    refused(spied, fn, y=semi["y"], uv=semi["uv"], u=planar["u"])
    refused(spied, fn, y=semi["y"], u=planar["u"])
    refused(spied, fn, y=semi["y"])
    refused(spied, fn, matrix="bt2020", **semi)
    refused(spied, fn, msb_aligned=6, **semi)
    refused(spied, fn, y=None, uv=semi["uv"])


def test_bad_outputs_are_refused_before_anything_is_launched(spied):
    semi = planes()
    f32 = lambda *s: words(*s, dtype=torch.float32)          # noqa: E731
    u8 = lambda *s: words(*s, dtype=torch.uint8)             # noqa: E731
    fn = yuv10.yuv420p10_to_bgr_u8
    refused(spied, fn, out=u8(H, W + 1, 3), **semi)                                             # wrong shape
    refused(spied, fn, out=u8(1, H, W, 3), **semi)
    refused(spied, fn, out=f32(H, W, 3), **semi)                                                # wrong dtype
    refused(spied, fn, out=u8(H, W, 4)[:, :, :3], **semi)                                       # not contiguous
    refused(spied, fn, out=bc.plain(u8(H, W, 3)), **semi)                                       # on the host
    refused(spied, fn, out=u8(H, W, 3), y_packed=u8(H, W + 2)[:, :W], **semi)
    refused(spied, fn, out=u8(H, W, 3), y_packed=words(H, W), **semi)
    refused(spied, fn, out=u8(H, W, 3), y_packed=u8(1, H, W), **semi)
    fn = yuv10.image_transform_yuv420p10
    refused(spied, fn, out=f32(3, H, W), **semi)
    refused(spied, fn, out=u8(1, 3, H, W), **semi)
    refused(spied, fn, out=f32(1, 3, H, W + 1)[:, :, :, :W], **semi)
    refused(spied, fn, out=bc.plain(f32(1, 3, H, W)), **semi)
    fn = yuv10.image_resize_transform_yuv420p10
    refused(spied, fn, im_scale=1.25, stride=16, out=f32(1, 3, 8, 12), **semi)                  # the unpadded size
    refused(spied, fn, im_scale=1.25, stride=16, out=words(1, 3, 16, 16, dtype=torch.float64), **semi)
    refused(spied, fn, im_scale=1.25, stride=16, out=f32(1, 3, 16, 32)[:, :, :, ::2], **semi)
    refused(spied, fn, im_scale=0.0, **semi)
    refused(spied, fn, im_scale=1.0, stride=-16, **semi)
    # ... and the good outputs pass
    out, yp = u8(H, W, 3), u8(H, W)
    assert yuv10.yuv420p10_to_bgr_u8(out=out, y_packed=yp, **semi) is out and spied.launched() == ["lsfa_yuv420p10_to_bgr_u8"]


def test_the_estimators_refuse_bad_planes_before_anything_is_launched(spied):
    me = yuv10.MotionEstimator10(32, 16, bc.CUDA0, search=4)
    del spied.calls[:]
    for bad in (dict(y=words(16, 32, dtype=torch.uint8), uv=words(8, 32, dtype=torch.uint8)), dict(y=words(16, 32), uv=words(8, 16)),
                dict(y=words(8, 32), uv=words(4, 32)), dict(y=bc.plain(words(16, 32)), uv=words(8, 32)), dict(y=words(16, 32))):
        refused(spied, me.key_frame_yuv, **bad)
        refused(spied, me.next_frame_yuv, **bad)
    me.key_frame_yuv(y=words(16, 32), uv=words(8, 32))
    assert spied.launched()[0] == "lsfa_yuv420p10_to_bgr_u8" and spied.values("lsfa_yuv420p10_to_bgr_u8")["shift"] == 6
    assert "lsfa_yuv420_to_bgr_u8" not in spied.launched()
    sme = yuv10.SegmentMotionEstimator10(32, 16, frames=2, device=bc.CUDA0, search=4, msb_aligned=False, luma_from='y')
    refused(spied, sme.segment_yuv, y=words(3, 16, 32, dtype=torch.uint8), uv=words(3, 8, 32, dtype=torch.uint8))
    refused(spied, sme.segment_yuv, y=words(3, 16, 32), uv=words(3, 8, 30))
    del spied.calls[:]
    sme.segment_yuv(y=words(3, 16, 32), u=words(3, 8, 16), v=words(3, 8, 16))
    got = spied.values("lsfa_yuv420p10_to_bgr_u8")
    assert (got["N"], got["shift"]) == (3, 0) and got["y_packed"] is not None and "lsfa_luma_u8" not in spied.launched()
    with pytest.raises(hip.LsfaError):
        yuv10.MotionEstimator10(32, 16, bc.CUDA0, msb_aligned=1)


def test_the_8_bit_estimators_still_convert_through_the_8_bit_export(spied):
    """the hook is a pure refactor: uint8 planes reach lsfa_yuv420_to_bgr_u8, from both estimators"""
    u8 = lambda *s: words(*s, dtype=torch.uint8)             # noqa: E731
    me = hip.MotionEstimator(32, 16, bc.CUDA0, search=4)
    del spied.calls[:]
    me.key_frame_yuv(y=u8(16, 32), uv=u8(8, 32))
    assert spied.launched()[0] == "lsfa_yuv420_to_bgr_u8"
    sme = hip.SegmentMotionEstimator(32, 16, frames=2, device=bc.CUDA0, search=4)
    del spied.calls[:]
    sme.segment_yuv(y=u8(3, 16, 32), uv=u8(3, 8, 32))
    assert spied.launched()[0] == "lsfa_yuv420_to_bgr_u8" and not any("p10" in n for n in spied.launched())


def test_demo_knows_the_10_bit_formats(tmp_path):
    from lsfa_amd import demo
    path = tmp_path / "clip.p010"
    path.write_bytes(bytes(2 * 3 * (8 * 6 * 3 // 2)))
    assert demo.yuv_file_frames(str(path), 8, 6) == (72, 432, 6)                # three arguments: bytes
    assert demo.yuv_file_frames(str(path), 8, 6, 2) == (144, 432, 3)
    for fmt in ("p010", "yuv420p10le"):
        args = demo.parse_args(["--yuv", str(path), "--size", "8x6", "--yuv-format", fmt])
        assert args.yuv_format == fmt
    with pytest.raises(SystemExit):
        demo.parse_args(["--yuv", str(path), "--size", "10x6", "--yuv-format", "p010"])
