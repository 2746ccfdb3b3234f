"""tests/ref_yuvfmt.py - the numpy statement of the YUV intake's other chroma formats - pinned by derived answers, and what can be said of
lsfa_amd/yuvfmt.py, the header and the demo without a GPU: the format table against the header's #defines, the frame-size rule, the
prototypes, the wrappers' validation under binding_contract's spy.  The kernels are tests/test_yuvfmt_gpu.py's."""
import os
import re

import numpy as np
import pytest
import torch

import binding_contract as bc
import ref_yuv
import ref_yuv10
import ref_yuvfmt as ref
from lsfa_amd import hip, yuvfmt

MATRICES = ("bt601", "bt709", "jpeg")
SIZES = ((1, 1), (1, 2), (3, 5), (6, 8))
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "lsfa_hip.h")


def planar(sub, sample=0):
    return ref.code(sub, ref.PLANAR, sample)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", (0, 1, 2))
@pytest.mark.parametrize("H,W", SIZES)
def test_every_pixel_takes_the_chroma_sample_its_subsampling_names(sub, H, W):
    """chroma planes that hold their own coordinates: U = cx & 255, V = cy & 255, constant Y"""
    c = planar(sub)
    ch, cw = ref.chroma_shape(c, H, W)
    sx, sy = ref.SHIFTS[sub]
    assert (ch, cw) == (-(-H // (1 << sy)), -(-W // (1 << sx)))
    Y = np.full((H, W), 120, np.uint8)
    U = np.broadcast_to((np.arange(cw) & 255).astype(np.uint8)[None, :], (ch, cw))
    V = np.broadcast_to((np.arange(ch) & 255).astype(np.uint8)[:, None], (ch, cw))
    for matrix in MATRICES:
        got = ref.to_bgr(c, Y, u=U, v=V, matrix=matrix)
        gu = np.array([[x >> sx for x in range(W)] for _ in range(H)])
        gv = np.array([[y >> sy for _ in range(W)] for y in range(H)])
        np.testing.assert_array_equal(got, ref_yuv.convert(Y, gu, gv, matrix))


@pytest.mark.parametrize("H,W", SIZES + ((7, 9),))
def test_doubled_chroma_gives_the_4_2_0_frame(H, W):
    """4:2:2 planes made by writing each 4:2:0 chroma row twice (cut to H) and 4:4:4 planes doubled both ways == ref_yuv.to_bgr"""
    rs = np.random.RandomState(H * 10 + W)
    Y, U, V = ref.random_samples(planar(0), rs, H, W)
    for matrix in MATRICES:
        want = ref_yuv.to_bgr(Y, u=U, v=V, matrix=matrix)
        np.testing.assert_array_equal(ref.to_bgr(planar(0), Y, u=U, v=V, matrix=matrix), want)
        for sub in (1, 2):
            u2, v2 = ref.upsample(U, V, sub, H, W)
            assert u2.shape == ref.chroma_shape(planar(sub), H, W)
            np.testing.assert_array_equal(ref.to_bgr(planar(sub), Y, u=u2, v=v2, matrix=matrix), want)


@pytest.mark.parametrize("sample", (0, 1, 2))
@pytest.mark.parametrize("sub", (0, 1, 2))
def test_interleaved_v_u_of_swapped_planes_is_interleaved_u_v(sub, sample):
    rs = np.random.RandomState(sub + 3 * sample)
    uv, vu = ref.code(sub, ref.UV, sample), ref.code(sub, ref.VU, sample)
    for H, W in SIZES:
        Y, U, V = ref.random_samples(uv, rs, H, W, n=2)
        a = ref.to_bgr(uv, matrix=1, **ref.lay_out(uv, Y, U, V))
        np.testing.assert_array_equal(ref.to_bgr(vu, matrix=1, **ref.lay_out(vu, Y, U, V)), a)
        np.testing.assert_array_equal(ref.to_bgr(vu, Y, uv=ref.lay_out(uv, Y, V, U)["uv"], matrix=1), a)
        np.testing.assert_array_equal(ref.to_bgr(planar(sub, sample), Y, u=U, v=V, matrix=1), a)
        if sub == 0 and sample == 0:
            np.testing.assert_array_equal(ref_yuv.to_bgr(Y, uv=ref.lay_out(uv, Y, U, V)["uv"], matrix=1), a)


def test_packed_frames_equal_their_planes_odd_widths_included():
    rs = np.random.RandomState(11)
    p = planar(1)
    for H, W in SIZES + ((4, 7), (2, 3)):
        Y, U, V = ref.random_samples(p, rs, H, W)
        want = ref.to_bgr(p, Y, u=U, v=V, matrix=2)
        for layout in (ref.YUYV, ref.UYVY):
            c = ref.code(1, layout, 0)
            packed = ref.lay_out(c, Y, U, V)["y"]
            assert packed.shape == (H, 4 * -(-W // 2))
            np.testing.assert_array_equal(ref.to_bgr(c, packed, matrix=2, width=W), want)
            np.testing.assert_array_equal(ref.y_packed(c, packed, W), Y)
            if W % 2:                   # the last group's second Y is no part of the result
                other = packed.copy()
                other[:, -2 if layout == ref.YUYV else -1] ^= 0xFF
                np.testing.assert_array_equal(ref.to_bgr(c, other, matrix=2, width=W), want)
    # the byte order itself
    y = np.array([[1, 2, 3, 4]], np.uint8)
    Yq, Uq, Vq, _ = ref.split(ref.code(1, ref.YUYV, 0), y)
    assert (Yq.tolist(), Uq.tolist(), Vq.tolist()) == ([[1, 3]], [[2]], [[4]])
    Yq, Uq, Vq, _ = ref.split(ref.code(1, ref.UYVY, 0), y)
    assert (Yq.tolist(), Uq.tolist(), Vq.tolist()) == ([[2, 4]], [[1]], [[3]])


@pytest.mark.parametrize("sample,shift", ((1, 0), (2, 6)))
def test_words_that_are_four_times_a_byte_plane_equal_the_byte_format(sample, shift):
    rs = np.random.RandomState(sample)
    for sub in (0, 1, 2):
        for layout in (ref.PLANAR, ref.UV, ref.VU):
            for H, W in SIZES:
                c8, c10 = ref.code(sub, layout, 0), ref.code(sub, layout, sample)
                p8 = ref.random_samples(c8, rs, H, W)
                p10 = [ref_yuv10.widen(p, shift, low_bits=int(rs.randint(0, 64))) for p in p8]
                for matrix in MATRICES:
                    np.testing.assert_array_equal(ref.to_bgr(c10, matrix=matrix, **ref.lay_out(c10, *p10)), ref.to_bgr(c8, matrix=matrix, **ref.lay_out(c8, *p8)))
                np.testing.assert_array_equal(ref.y_packed(c10, p10[0]), p8[0])
    # and the 4:2:0 word formats are ref_yuv10's
    Y, U, V = ref.random_samples(planar(0, sample), rs, 5, 7)
    np.testing.assert_array_equal(ref.to_bgr(planar(0, sample), Y, u=U, v=V), ref_yuv10.to_bgr(Y, u=U, v=V, shift=shift))


# ---- the table, the frame size, the header ------------------------------------------------------------------------------------------------
def header_defines():
    text = open(HEADER).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (LSFA_YUV_\w+) (\d+)\s*$", text, flags=re.M)}, text


def test_the_format_table_is_the_headers():
    d, text = header_defines()
    assert (d["LSFA_YUV_420"], d["LSFA_YUV_422"], d["LSFA_YUV_444"]) == (yuvfmt.SUB_420, yuvfmt.SUB_422, yuvfmt.SUB_444) == (0, 1, 2)
    assert tuple(d["LSFA_YUV_" + n] for n in ("PLANAR", "UV", "VU", "YUYV", "UYVY")) == (yuvfmt.PLANAR, yuvfmt.UV, yuvfmt.VU, yuvfmt.YUYV, yuvfmt.UYVY)
    assert tuple(d["LSFA_YUV_" + n] for n in ("U8", "LO10", "HI10")) == (yuvfmt.U8, yuvfmt.LO10, yuvfmt.HI10) == (0, 1, 2)
    assert "#define LSFA_YUV_FORMAT(sub, layout, sample) ((sub) | (layout) << 4 | (sample) << 8)" in text
    f = lambda s, l, b: d["LSFA_YUV_" + s] | d["LSFA_YUV_" + l] << 4 | d["LSFA_YUV_" + b] << 8          # noqa: E731,E741
    want = {'nv12': f("420", "UV", "U8"), 'i420': f("420", "PLANAR", "U8"), 'nv21': f("420", "VU", "U8"), 'yuv422p': f("422", "PLANAR", "U8"),
            'nv16': f("422", "UV", "U8"), 'nv61': f("422", "VU", "U8"), 'yuyv422': f("422", "YUYV", "U8"), 'yuy2': f("422", "YUYV", "U8"),
            'uyvy422': f("422", "UYVY", "U8"), 'yuv444p': f("444", "PLANAR", "U8"), 'nv24': f("444", "UV", "U8"), 'nv42': f("444", "VU", "U8"),
            'yuv422p10le': f("422", "PLANAR", "LO10"), 'p210': f("422", "UV", "HI10"), 'yuv444p10le': f("444", "PLANAR", "LO10"),
            'p410': f("444", "UV", "HI10"), 'p010': f("420", "UV", "HI10"), 'yuv420p10le': f("420", "PLANAR", "LO10")}
    assert yuvfmt.FORMATS == want == ref.NAMES
    for c in range(-2, 1 << 13):
        if ref.valid(c):
            assert yuvfmt.fields(c) == (c,) + ref.fields(c)
        else:
            with pytest.raises(hip.LsfaError):
                yuvfmt.fields(c)
    for bad in ("yvyu422", None, 1.0, True):
        with pytest.raises(hip.LsfaError):
            yuvfmt.fields(bad)


def test_the_frame_size_is_the_sum_of_the_planes():
    rs = np.random.RandomState(5)
    for name, c in sorted(yuvfmt.FORMATS.items()):
        for H, W in SIZES + ((23, 37), (600, 1000)):
            assert yuvfmt.frame_bytes(name, W, H) == sum(ref.plane_bytes(c, H, W)), (name, H, W)
            assert yuvfmt.chroma_shape(name, H, W) == ref.chroma_shape(c, H, W)
        Y, U, V = ref.random_samples(c, rs, 3, 5)
        assert len(ref.raw_frame_bytes(c, Y, U, V)) == yuvfmt.frame_bytes(name, 5, 3), name
    assert yuvfmt.frame_bytes('nv12', 8, 6) == 72 and yuvfmt.frame_bytes('yuyv422', 5, 3) == 36 and yuvfmt.frame_bytes('yuv444p10le', 5, 3) == 90
    assert yuvfmt.frame_bytes('yuv422p', 5, 3) == 15 + 2 * 9 and yuvfmt.frame_bytes('p210', 4, 2) == 32


def test_the_header_declares_the_three_exports():
    protos = hip._PROTOTYPES
    for name, arity in (("lsfa_yuv_to_bgr_u8", 15), ("lsfa_image_transform_yuv", 16), ("lsfa_image_resize_transform_yuv", 22)):
        ret, params = protos[name]
        ten = protos[name.replace("lsfa_yuv_to", "lsfa_yuv420p10_to") if "to_bgr" in name else name + "420p10"][1]
        assert ret.strip() == "int" and len(params) == arity == len(ten), name
        # the 10-bit prototype argument for argument, `format` where it has `shift`
        assert [" ".join(p.split()) for p in params] == [" ".join(p.split()).replace("int shift", "int format") for p in ten], name


def test_demo_takes_every_format_name(tmp_path):
    from lsfa_amd import demo
    for name in sorted(yuvfmt.FORMATS):
        path = tmp_path / ("clip." + name)
        path.write_bytes(bytes(2 * yuvfmt.frame_bytes(name, 6, 4)))
        args = demo.parse_args(["--yuv", str(path), "--size", "6x4", "--yuv-format", name])
        assert args.yuv_format == name
        assert demo.yuv_file_frames(str(path), 6, 4, fmt=name) == (yuvfmt.frame_bytes(name, 6, 4), 2 * yuvfmt.frame_bytes(name, 6, 4), 2)
    with pytest.raises(SystemExit):
        demo.parse_args(["--yuv", str(path), "--size", "6x4", "--yuv-format", "yvyu422"])
    with pytest.raises(SystemExit):          # a yuyv422 file is not a whole number of nv12 frames of another size
        demo.parse_args(["--yuv", str(tmp_path / "clip.yuyv422"), "--size", "10x4", "--yuv-format", "yuyv422"])


# ---- the wrappers under the spy -----------------------------------------------------------------------------------------------------------
H, W = 6, 10
WRAPPERS = (yuvfmt.yuv_to_bgr_u8, yuvfmt.image_transform_yuv, yuvfmt.image_resize_transform_yuv)


@pytest.fixture()
def spied(monkeypatch):
    spy = bc.Spy(hip.lib())
    monkeypatch.setattr(hip, "lib", lambda: spy)
    with bc.fake_cuda(monkeypatch):
        yield spy


def z(*shape, dtype=torch.uint8):
    return torch.zeros(shape, dtype=dtype).as_subclass(bc.FakeCuda)


def refused(spy, fn, *a, **kw):
    del spy.calls[:]
    with pytest.raises(hip.LsfaError) as e:
        fn(*a, **kw)
    if fn in WRAPPERS:
        assert fn.__name__ in str(e.value)          # the message names the function
    assert not spy.calls, "%s launched %s before refusing" % (fn.__name__, spy.launched())


def test_well_formed_calls_reach_their_exports_with_byte_pitches_and_the_format(spied):
    y = z(H, W + 6)[:, :W]
    assert yuvfmt.yuv_to_bgr_u8("nv16", y, uv=z(H, W)).shape == (H, W, 3)
    got = spied.values("lsfa_yuv_to_bgr_u8")
    assert (got["y_pitch"], got["c_pitch"], got["N"], got["H"], got["W"], got["matrix"], got["format"], got["v"]) == (16, 10, 1, H, W, 0, 0x011, None)
    del spied.calls[:]
    out = yuvfmt.image_transform_yuv("yuv444p10le", z(2, H, W, dtype=torch.uint16), u=z(2, H, W, dtype=torch.uint16), v=z(2, H, W, dtype=torch.uint16), matrix="bt709")
    got = spied.values("lsfa_image_transform_yuv")
    assert tuple(out.shape) == (2, 3, H, W) and (got["y_pitch"], got["c_pitch"], got["y_frame_stride"], got["matrix"], got["format"]) == (20, 20, 120, 1, 0x102)
    assert got["v"] is not None
    del spied.calls[:]
    out = yuvfmt.image_resize_transform_yuv("uyvy422", z(H, 20), im_scale=1.25, stride=16, width=9)
    got = spied.values("lsfa_image_resize_transform_yuv")
    assert tuple(out.shape) == (1, 3, 16, 16) and (got["W"], got["y_pitch"], got["u_or_uv"], got["v"], got["c_pitch"], got["c_frame_stride"]) == (9, 20, None, None, 0, 0)
    assert got["format"] == 0x041 and spied.launched() == ["lsfa_image_resize_transform_yuv"]
    del spied.calls[:]
    yuvfmt.yuv_to_bgr_u8("yuy2", z(3, H, 20))
    got = spied.values("lsfa_yuv_to_bgr_u8")
    assert (got["N"], got["W"], got["y_frame_stride"], got["format"]) == (3, 10, 120, 0x031)
    del spied.calls[:]
    yuvfmt.yuv_to_bgr_u8(yuvfmt.code(0, yuvfmt.VU, yuvfmt.LO10), z(H, W, dtype=torch.int16), uv=z(3, 10, dtype=torch.int16))
    assert spied.values("lsfa_yuv_to_bgr_u8")["format"] == 0x120 and spied.values("lsfa_yuv_to_bgr_u8")["c_pitch"] == 20


@pytest.mark.parametrize("fn", WRAPPERS, ids=[f.__name__ for f in WRAPPERS])
def test_bad_planes_are_refused_before_anything_is_launched(spied, fn):
    y, uv, u, v = z(H, W), z(H, W), z(H, 5), z(H, 5)
    w16 = lambda *s: z(*s, dtype=torch.int16)          # noqa: E731
    refused(spied, fn, "nv16", bc.plain(y).clone(), uv=uv)                          # on the host
    refused(spied, fn, "nv16", y, uv=bc.plain(uv).clone())
    refused(spied, fn, "nv16", y, u=u, v=v)                                         # the layout's own planes
    refused(spied, fn, "yuv422p", y, uv=uv)
    refused(spied, fn, "yuv422p", y, u=u)
    refused(spied, fn, "nv16", y, uv=uv, u=u, v=v)
    refused(spied, fn, "nv16", y)
    refused(spied, fn, "yuyv422", z(H, 2 * W), uv=uv)                               # a packed frame has no chroma planes
    refused(spied, fn, "yuyv422", z(H, 2 * W), u=u, v=v)
    refused(spied, fn, "yuyv422", z(H, 2 * W + 2))                                  # not whole groups
    refused(spied, fn, "yuyv422", z(H, 2 * W), width=W + 1)                         # a width of another group count
    refused(spied, fn, "yuyv422", z(H, 2 * W), width=W - 2)
    refused(spied, fn, "yuyv422", w16(H, 2 * W))                                    # packed words do not exist
    refused(spied, fn, "nv16", y, uv=uv, width=W + 1)
    refused(spied, fn, "nv16", w16(H, W), uv=w16(H, W))                             # the sample's dtype
    refused(spied, fn, "p210", y, uv=uv)
    refused(spied, fn, "p210", w16(H, W), uv=uv)
    refused(spied, fn, "nv16", z(H, W, dtype=torch.float32), uv=uv)
    refused(spied, fn, "nv16", y, uv=z(3, W))                                       # 4:2:2 chroma has H rows
    refused(spied, fn, "nv12", y, uv=uv)                                            # ... and 4:2:0 half of them
    refused(spied, fn, "nv24", y, uv=uv)                                            # 4:4:4 interleaved is 2 W wide
    refused(spied, fn, "yuv444p", y, u=u, v=v)
    refused(spied, fn, "yuv422p", y, u=u, v=z(H, 4))
    refused(spied, fn, "nv16", y, uv=z(1, H, W))                                    # ranks, frame counts
    refused(spied, fn, "nv16", z(2, H, W), uv=z(3, H, W))
    refused(spied, fn, "nv16", torch.as_strided(z(H * W), (H, W), (W - 2, 1)), uv=uv)          # a pitch below its row
    refused(spied, fn, "nv16", y, uv=torch.as_strided(z(H * W), (H, W), (W - 2, 1)))
    refused(spied, fn, "nv16", z(H, 2 * W)[:, ::2], uv=uv)                          # a last dimension that is not dense
    refused(spied, fn, "yuv422p", y, u=u, v=z(H, 8)[:, :5])                         # u and v of different pitch
    refused(spied, fn, "nv16", y, uv=uv, matrix="bt2020")
    refused(spied, fn, "yvyu422", y, uv=uv)                                         # no such format
    refused(spied, fn, 0x131, z(H, 2 * W))
    refused(spied, fn, 0x003, y, uv=uv)
    refused(spied, fn, "nv16", None, uv=uv)


def test_bad_outputs_are_refused_before_anything_is_launched(spied):
    k = dict(y=z(H, W), uv=z(H, W))
    f32 = lambda *s: z(*s, dtype=torch.float32)          # noqa: E731
    fn = yuvfmt.yuv_to_bgr_u8
    refused(spied, fn, "nv16", out=z(H, W + 1, 3), **k)
    refused(spied, fn, "nv16", out=f32(H, W, 3), **k)
    refused(spied, fn, "nv16", out=z(H, W, 4)[:, :, :3], **k)
    refused(spied, fn, "nv16", out=bc.plain(z(H, W, 3)), **k)
    refused(spied, fn, "nv16", out=z(H, W, 3), y_packed=z(H, W + 2)[:, :W], **k)
    refused(spied, fn, "yuyv422", z(H, 2 * W), out=z(H, 2 * W, 3))                  # the frame's width, not the plane's
    refused(spied, fn, "yuyv422", z(H, 2 * W), y_packed=z(H, 2 * W))
    refused(spied, yuvfmt.image_transform_yuv, "nv16", out=f32(3, H, W), **k)
    refused(spied, yuvfmt.image_transform_yuv, "nv16", out=z(1, 3, H, W), **k)
    fn = yuvfmt.image_resize_transform_yuv
    refused(spied, fn, "nv16", im_scale=1.25, stride=16, out=f32(1, 3, 8, 12), **k)
    refused(spied, fn, "nv16", im_scale=0.0, **k)
    refused(spied, fn, "nv16", im_scale=1.0, stride=-16, **k)
    out, yp = z(H, W, 3), z(H, W)
    assert yuvfmt.yuv_to_bgr_u8("nv16", out=out, y_packed=yp, **k) is out and spied.launched() == ["lsfa_yuv_to_bgr_u8"]


def test_the_estimators_check_the_plane_their_format_has(spied):
    """a packed frame's y is (H, 4 ceil(W / 2)); every other format's (H, W); the shipped classes keep their check and their message"""
    me = yuvfmt.MotionEstimatorYuv(32, 16, bc.CUDA0, fmt="uyvy422", search=4)
    del spied.calls[:]
    refused(spied, me.key_frame_yuv, y=z(16, 32))
    refused(spied, me.next_frame_yuv, y=z(16, 64), uv=z(16, 32))
    me.key_frame_yuv(y=z(16, 64))
    got = spied.values("lsfa_yuv_to_bgr_u8")
    assert spied.launched()[0] == "lsfa_yuv_to_bgr_u8" and (got["format"], got["W"], got["H"]) == (0x041, 32, 16)
    me = yuvfmt.MotionEstimatorYuv(32, 16, bc.CUDA0, fmt="yuv444p10le", search=4, luma_from='y')
    del spied.calls[:]
    w16 = lambda *s: z(*s, dtype=torch.int16)          # noqa: E731
    refused(spied, me.key_frame_yuv, y=w16(16, 64), u=w16(16, 32), v=w16(16, 32))
    refused(spied, me.key_frame_yuv, y=z(16, 32), u=z(16, 32), v=z(16, 32))
    me.key_frame_yuv(y=w16(16, 32), u=w16(16, 32), v=w16(16, 32))
    assert spied.values("lsfa_yuv_to_bgr_u8")["y_packed"] is not None and "lsfa_luma_u8" not in spied.launched()
    sme = yuvfmt.SegmentMotionEstimatorYuv(32, 16, frames=2, device=bc.CUDA0, fmt="yuy2", search=4)
    refused(spied, sme.segment_yuv, y=z(3, 16, 32))
    del spied.calls[:]
    sme.segment_yuv(y=z(3, 16, 64))
    assert (spied.values("lsfa_yuv_to_bgr_u8")["N"], spied.values("lsfa_yuv_to_bgr_u8")["format"]) == (3, 0x031)
    with pytest.raises(hip.LsfaError, match="MotionEstimatorYuv"):
        yuvfmt.MotionEstimatorYuv(32, 16, bc.CUDA0, fmt="yvyu422")
    with pytest.raises(hip.LsfaError, match=r"a \(16, 32\) uint8 Y plane"):
        hip.MotionEstimator(32, 16, bc.CUDA0, search=4).key_frame_yuv(y=z(16, 64), uv=z(8, 32))
    with pytest.raises(hip.LsfaError, match=r"a \(1 \* \(n \+ 1\), 16, 32\) uint8 Y stack"):
        hip.SegmentMotionEstimator(32, 16, frames=2, device=bc.CUDA0, search=4).segment_yuv(y=z(3, 16, 64), uv=z(3, 8, 32))


# ---- the compiled kernels -----------------------------------------------------------------------------------------------------------------
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not in this image")
def test_no_half_register_pack_in_the_format_kernels(tmp_path):
    """v_ashr_pk_u8_i32 writes half of its destination and the back end uses the whole: the four-pixel BGR kernels gave 0xFF in two bytes
    wherever a blue had clipped to 0 (DESIGN.md "Other chroma formats").  yuvfmt.hip, the one intake source, clamps before it shifts so that
    the instruction is not formed; this looks at what was compiled: the 46 yuvfmt kernels are every intake kernel of the library - the
    4:2:0 exports' own kernels (yuv420_*, yuv420p10_*, resize_transform_yuv420*), which held the instruction, are gone - and hold none"""
    import glob
    import shutil
    import subprocess
    lib = os.path.join(os.path.dirname(HEADER), "..", "lsfa_amd", "liblsfa_hip.so")
    if not os.path.exists(lib):
        from lsfa_amd import build
        build.build_hip()
    work = tmp_path / "liblsfa_hip.so"
    shutil.copy(lib, work)
    subprocess.run([OBJDUMP, "--offloading", str(work)], check=True, capture_output=True)
    found, kernels, old = [], 0, []
    for o in glob.glob(str(work) + ".*gfx950*"):
        asm = subprocess.run([OBJDUMP, "-d", o], check=True, capture_output=True, text=True).stdout
        for body in re.split(r"^[0-9a-f]+ <", asm, flags=re.M)[1:]:
            name = body.split(">:", 1)[0]
            if "yuv420" in name:
                old.append(name)
            if "yuv" in name:          # every intake kernel: they are all yuvfmt's
                assert "yuvfmt" in name, name
                kernels += 1
                found += ["%s: %s" % (name, m) for m in re.findall(r"v_ashr_pk_u8_i32[^\n]*", body)]
    assert not old, old
    assert kernels == 46, kernels
    assert not found, "%d, e.g. %s" % (len(found), found[0])
