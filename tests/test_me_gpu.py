"""lsfa_luma_u8 / lsfa_mv_estimate (lsfa_amd/csrc/me.hip) and hip.MotionEstimator on the GPU against tests/ref_me.py, bit for bit: the
rows AND the SAD of every macroblock; then the chain behind them (accumulation, field, residual, transform_mv_res) against the oracle,
graph capture, the error paths and the demo's --estimate-mv / --dump-mv / --mv round trip.  tests/test_me_cpu.py pins the reference."""
import json

import numpy as np
import pytest
import torch

import oracle
import ref_me
from me_util import t
from oracle import np_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [(1000, 600), (96, 64), (37, 23), (250, 130)]        # (width, height)
SMALL = SIZES[1:]
MEANS = (102.9801, 115.9465, 122.7717)


def plane_pair(kind, width, height, seed):
    """two (H, W) uint8 luma planes (current, reference) of the named kind"""
    rs = np.random.RandomState(seed)
    if kind in ("translated", "translated_noise"):
        f0, f1 = ref_me.translated_clip(2, width, height, (3, -2), seed=seed, sigma=3.0 if kind == "translated_noise" else 0.0)
        return ref_me.luma(f1), ref_me.luma(f0)
    if kind == "noise":                                       # pure noise against pure noise: near-ties everywhere
        return rs.randint(0, 256, (height, width)).astype(np.uint8), rs.randint(0, 256, (height, width)).astype(np.uint8)
    if kind == "flat":
        return np.full((height, width), 93, np.uint8), np.full((height, width), 93, np.uint8)
    if kind == "half_flat":                                   # left half flat, right half moving texture
        f0, f1 = ref_me.translated_clip(2, width, height, (-2, 1), seed=seed)
        cur, ref = ref_me.luma(f1), ref_me.luma(f0)
        cur[:, :width // 2] = 120
        ref[:, :width // 2] = 120
        return cur, ref
    if kind == "stripes":                                     # saturated 0 / 255 stripes, shifted by 3 between the frames: SADs at their maximum
        x = np.arange(width + 3)
        line = np.where((x // 5) % 2 == 0, 0, 255).astype(np.uint8)
        return np.tile(line[3:], (height, 1)), np.tile(line[:width], (height, 1))
    if kind == "synthetic":                                   # weak texture under noise: the lambda term decides
        from lsfa_amd.utils.synthetic import SyntheticClip
        clip = SyntheticClip(seed % 7, 3, height, width)
        return ref_me.luma(clip.frame_u8(2).numpy()), ref_me.luma(clip.frame_u8(1).numpy())
    raise ValueError(kind)


KINDS = ["translated", "translated_noise", "noise", "flat", "half_flat", "stripes", "synthetic"]


def check_estimate(hip, cur, ref, search, lam, max_sad, tag):
    want_rows, want_sad = ref_me.estimate(cur, ref, search, lam, max_sad)
    rows, sad = hip.mv_estimate(t(cur), t(ref), search=search, lam=lam, max_sad=max_sad, return_sad=True)
    assert rows.dtype == torch.int32 and tuple(rows.shape) == want_rows.shape and tuple(sad.shape) == want_sad.shape
    np.testing.assert_array_equal(sad.cpu().numpy(), want_sad, err_msg="SAD " + tag)
    np.testing.assert_array_equal(rows.cpu().numpy(), want_rows, err_msg="rows " + tag)
    # without the optional output
    np.testing.assert_array_equal(hip.mv_estimate(t(cur), t(ref), search=search, lam=lam, max_sad=max_sad).cpu().numpy(), want_rows)


@pytest.mark.parametrize("size", SIZES)
def test_luma_u8_equals_the_reference(hip, size):
    """lsfa_luma_u8 on random frames, plus the extremes of every channel"""
    width, height = size
    rs = np.random.RandomState(width)
    bgr = rs.randint(0, 256, (height, width, 3)).astype(np.uint8)
    bgr[0, :8] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]]
    got = hip.luma_u8(t(bgr))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (height, width)
    np.testing.assert_array_equal(got.cpu().numpy(), ref_me.luma(bgr))
    out = torch.zeros((height, width), dtype=torch.uint8, device=DEV)
    assert hip.luma_u8(t(bgr), out=out) is out
    np.testing.assert_array_equal(out.cpu().numpy(), ref_me.luma(bgr))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SMALL)
def test_mv_estimate_bit_exact_small(hip, size, kind):
    """lsfa_mv_estimate rows and SAD == ref_me over R in {1, 4, 16, 32}, lambda in {0, 4, 50}, max_sad off / on.  The small sizes carry the
    sweep: 96 x 64 (whole blocks), 37 x 23 (one partial row and column; R = 16 and 32 exceed the frame) and 250 x 130 (partial blocks of
    10 columns / 2 rows)."""
    width, height = size
    cur, ref = plane_pair(kind, width, height, seed=width + len(kind))
    for search, lam, max_sad in ((1, 4, 0), (4, 0, 0), (4, 50, 1500), (16, 4, 0), (16, 0, 3000), (16, 50, 0), (32, 4, 0), (32, 0, 20000)):
        check_estimate(hip, cur, ref, search, lam, max_sad, "%s %dx%d R=%d lambda=%d max_sad=%d" % (kind, width, height, search, lam, max_sad))


@pytest.mark.parametrize("kind,search,lam,max_sad", [("translated_noise", 16, 4, 0), ("noise", 16, 0, 0), ("synthetic", 16, 4, 0),
                                                     ("half_flat", 32, 4, 12000)])
def test_mv_estimate_bit_exact_full_size(hip, kind, search, lam, max_sad):
    """... and at 1000 x 600 (63 x 38 blocks, the last column 8 wide, the last row 8 high): few cases, each costs seconds on the host"""
    cur, ref = plane_pair(kind, 1000, 600, seed=3)
    check_estimate(hip, cur, ref, search, lam, max_sad, "%s 1000x600 R=%d" % (kind, search))


def test_translation_recovered_on_the_device(hip):
    """what tests/test_me_cpu.py derives for the reference, on the kernel's own output: 2,294 of 2,394 blocks return exactly m"""
    m = (-5, 7)
    f0, f1 = ref_me.translated_clip(2, 1000, 600, m, seed=21, sigma=3.0)
    rows = hip.mv_estimate(hip.luma_u8(t(f1)), hip.luma_u8(t(f0))).cpu().numpy()
    v = ref_me.vectors(rows, 38, 63)
    x0, y0 = 16 * np.arange(63)[None, :], 16 * np.arange(38)[:, None]
    x1, y1 = np.minimum(x0 + 16, 1000) - 1, np.minimum(y0 + 16, 600) - 1
    inside = (x0 - m[0] >= 0) & (x1 - m[0] <= 999) & (y0 - m[1] >= 0) & (y1 - m[1] <= 599)
    assert int(inside.sum()) == 2294
    assert int(((v[..., 0] == m[0]) & (v[..., 1] == m[1]) & inside).sum()) == 2294


def reference_chain(frames, search, lam, max_sad=0):
    """key frame + P-frames through ref_me and the oracle: the accumulated source map after every frame"""
    height, width = frames[0].shape[:2]
    accu = oracle.coviar_identity(width, height)
    lum = [ref_me.luma(f) for f in frames]
    accus = [accu]
    for f in range(1, len(frames)):
        rows, _ = ref_me.estimate(lum[f], lum[f - 1], search, lam, max_sad)
        accu = oracle.coviar_accumulate(rows, accu)
        accus.append(accu)
    return accus


@pytest.mark.parametrize("size,search", [((1000, 600), 8), ((250, 130), 16)])
def test_motion_estimator_chain(hip, size, search):
    """MotionEstimator over a key frame + 9 frames == coviar_accumulate of the reference rows frame by frame; network_inputs ==
    np_ref.transform_mv_res(-coviar_mv, coviar_residual) bit for bit.  On the translated texture, m = (3, -2): the residual against the key
    frame is exactly 0 on pixels at least 48 from the border (a wrong border block reaches 16 + 9 * 3 = 43 pixels inward through the
    chain) and sum |res| is strictly below the zero-motion residual's."""
    width, height = size
    m = (3, -2)
    frames = ref_me.translated_clip(10, width, height, m, seed=width)
    accus = reference_chain(frames, search, 4)
    me = hip.MotionEstimator(width, height, DEV, search=search, lam=4)
    dev_frames = [t(f) for f in frames]
    me.key_frame(dev_frames[0])
    np.testing.assert_array_equal(me.acc.accu.cpu().numpy(), accus[0])
    sc, ps = 1.25, 0.5
    for f in range(1, 10):
        rows = me.next_frame(dev_frames[f])
        assert tuple(rows.shape) == (me.mbh * me.mbw, 7)
        np.testing.assert_array_equal(me.acc.accu.cpu().numpy(), accus[f], err_msg="frame %d" % f)
        if f in (1, 5, 9):
            want_mv, want_res = np_ref.transform_mv_res(-oracle.coviar_mv(accus[f]).astype(np.float32),
                                                        oracle.coviar_residual(frames[f], frames[0], accus[f]).astype(np.float32), sc, MEANS, ps)
            got_mv, got_res = me.network_inputs(dev_frames[f], dev_frames[0], sc, MEANS, ps)
            np.testing.assert_array_equal(got_mv.cpu().numpy(), want_mv.astype(np.float32), err_msg="frame %d" % f)
            np.testing.assert_array_equal(got_res.cpu().numpy(), want_res.astype(np.float32), err_msg="frame %d" % f)
    res = me.acc.residual(dev_frames[9], dev_frames[0]).cpu().numpy()
    mv = me.acc.motion_vectors().cpu().numpy()
    assert (res[48:height - 48, 48:width - 48] == 0).all()
    assert (mv[48:height - 48, 48:width - 48] == np.array([9 * m[0], 9 * m[1]])).all()
    zero_motion = np.abs(frames[9].astype(np.int64) - frames[0].astype(np.int64)).sum()
    assert np.abs(res.astype(np.int64)).sum() < zero_motion
    # a new key frame starts over
    me.key_frame(dev_frames[3])
    np.testing.assert_array_equal(me.acc.accu.cpu().numpy(), accus[0])
    me.next_frame(dev_frames[4])
    want = oracle.coviar_accumulate(ref_me.estimate(ref_me.luma(frames[4]), ref_me.luma(frames[3]), search, 4)[0], accus[0])
    np.testing.assert_array_equal(me.acc.accu.cpu().numpy(), want)


def test_motion_estimator_graph_capture(hip):
    """key_frame + next_frame + network_inputs captured with torch.cuda.graph on one stream (no parallel branches), replayed on NEW frame
    contents written into the same buffers == the eager result on those contents."""
    width, height = 250, 130
    clips = [ref_me.translated_clip(2, width, height, (3, -2), seed=1), ref_me.translated_clip(2, width, height, (-4, 5), seed=2, sigma=3.0)]
    key_buf, cur_buf = t(clips[0][0]).clone(), t(clips[0][1]).clone()
    me = hip.MotionEstimator(width, height, DEV, search=16, lam=4)

    def step():
        me.key_frame(key_buf)
        me.next_frame(cur_buf)
        return me.network_inputs(cur_buf, key_buf, 1.0, MEANS, 1.0)

    step()                                   # warm-up: network_inputs allocates its outputs at the first call for a scale
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_mv, out_res = step()
    for k, clip in enumerate(clips[::-1] + clips):
        key_buf.copy_(t(clip[0]))
        cur_buf.copy_(t(clip[1]))
        g.replay()
        torch.cuda.synchronize()
        got = out_mv.clone(), out_res.clone(), me.rows.clone(), me.sad.clone()
        eager = hip.MotionEstimator(width, height, DEV, search=16, lam=4)
        eager.key_frame(t(clip[0]))
        rows = eager.next_frame(t(clip[1]))
        e_mv, e_res = eager.network_inputs(t(clip[1]), t(clip[0]), 1.0, MEANS, 1.0)
        assert torch.equal(got[2], rows) and torch.equal(got[3], eager.sad), k
        assert torch.equal(got[0], e_mv) and torch.equal(got[1], e_res), k
        want_rows, want_sad = ref_me.estimate(ref_me.luma(clip[1]), ref_me.luma(clip[0]), 16, 4)
        np.testing.assert_array_equal(got[2].cpu().numpy(), want_rows)
        np.testing.assert_array_equal(got[3].cpu().numpy(), want_sad)
    assert not torch.equal(t(clips[0][1]), t(clips[1][1]))


def test_error_paths(hip):
    y = torch.zeros((64, 96), dtype=torch.uint8, device=DEV)
    bgr = torch.zeros((64, 96, 3), dtype=torch.uint8, device=DEV)
    for bad in (dict(search=0), dict(search=33), dict(lam=-1), dict(max_sad=-1)):
        with pytest.raises(hip.LsfaError):
            hip.mv_estimate(y, y, **bad)
    with pytest.raises(hip.LsfaError):
        hip.mv_estimate(y.float(), y.float())                 # wrong dtype
    with pytest.raises(hip.LsfaError):
        hip.mv_estimate(y, y[:32])                            # planes differ
    with pytest.raises(hip.LsfaError):
        hip.mv_estimate(bgr, bgr)                             # wrong rank
    with pytest.raises(hip.LsfaError):
        hip.mv_estimate(y.cpu(), y.cpu())                     # not on the device
    with pytest.raises(hip.LsfaError):
        hip.luma_u8(bgr.float())
    with pytest.raises(hip.LsfaError):
        hip.luma_u8(y)                                        # (H, W): no channel axis
    with pytest.raises(hip.LsfaError):
        hip.luma_u8(bgr[:, :, :2])
    with pytest.raises(hip.LsfaError):
        hip.MotionEstimator(96, 64, DEV, search=40)
    me = hip.MotionEstimator(96, 64, DEV)
    with pytest.raises(hip.LsfaError):
        me.key_frame(bgr[:32])
    with pytest.raises(hip.LsfaError):
        me.next_frame(bgr.int())
    # the C entry points themselves: NULL pointers and bad sizes come back as error codes with a message
    import ctypes
    L = hip.lib()
    assert L.lsfa_luma_u8(None, 96, 64, ctypes.c_void_p(y.data_ptr()), None) != 0 and b"lsfa_luma_u8" in L.lsfa_last_error()
    assert L.lsfa_luma_u8(ctypes.c_void_p(bgr.data_ptr()), 0, 64, ctypes.c_void_p(y.data_ptr()), None) != 0
    assert L.lsfa_mv_estimate(ctypes.c_void_p(y.data_ptr()), None, 96, 64, 16, 4, 0, ctypes.c_void_p(y.data_ptr()), None, None) != 0
    assert b"lsfa_mv_estimate" in L.lsfa_last_error()
    assert L.lsfa_mv_estimate(ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(y.data_ptr()), 96, -1, 16, 4, 0, ctypes.c_void_p(y.data_ptr()), None, None) != 0
    torch.cuda.synchronize()


def test_prof_scope_counts_the_launches(hip):
    y = torch.zeros((64, 96), dtype=torch.uint8, device=DEV)
    hip.prof_enable(True, ops=["mv_estimate"])
    try:
        hip.mv_estimate(y, y)
        hip.mv_estimate(y, y)
        ms, n = hip.prof_read()["mv_estimate"]
    finally:
        hip.prof_enable(False)
    assert n == 2 and ms > 0.0


def write_clip(directory, n, width, height, m, seed):
    from PIL import Image
    frames = ref_me.translated_clip(n, width, height, m, seed=seed)
    directory.mkdir()
    for i, f in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(str(directory / ("%06d.png" % i)))        # PNG holds RGB; the frames are BGR
    return frames


def test_frame_dir_clip_estimates_like_the_direct_chain(hip, tmp_path):
    """FrameDirClip(..., estimate).mv_res(i, 0) == the direct MotionEstimator chain on the decoded frames"""
    from lsfa_amd import demo
    from lsfa_amd.config.config import lsfa_test_config
    cfg = lsfa_test_config()
    frames = write_clip(tmp_path / "frames", 10, 200, 120, (3, -2), seed=4)
    clip = demo.FrameDirClip(str(tmp_path / "frames"), None, cfg, dict(search=16, lam=4), DEV)
    me = hip.MotionEstimator(200, 120, DEV, search=16, lam=4)
    dev_frames = [t(f) for f in frames]
    me.key_frame(dev_frames[0])
    for i in range(1, 10):
        me.next_frame(dev_frames[i])
        want_mv, want_res = me.network_inputs(dev_frames[i], dev_frames[0], clip.im_scale, cfg.network.PIXEL_MEANS, cfg.network.PIXEL_SCALE)
        got_mv, got_res = clip.mv_res(i, 0)
        assert torch.equal(got_mv, want_mv) and torch.equal(got_res, want_res), i
        assert tuple(got_mv.shape) == (1, 2, -(-clip.height // 16), -(-clip.width // 16))
    assert float(got_mv.abs().max()) > 0
    # asking for a later frame first walks the chain from the key frame; a step back starts over
    clip2 = demo.FrameDirClip(str(tmp_path / "frames"), None, cfg, dict(search=16, lam=4), DEV)
    a_mv, a_res = clip2.mv_res(9, 0)
    assert torch.equal(a_mv, got_mv) and torch.equal(a_res, got_res)
    b_mv, _ = clip2.mv_res(2, 0)
    assert torch.equal(b_mv, clip.mv_res(2, 0)[0])
    with pytest.raises(ValueError):
        demo.FrameDirClip(str(tmp_path / "frames"), str(tmp_path), cfg, dict(search=16, lam=4), DEV)


def test_demo_estimate_dump_and_read_back(tmp_path, monkeypatch):
    """lsfa_amd.demo --estimate-mv --dump-mv DIR, then --mv DIR: the same detections JSON (the dumped mv / res files round-trip exactly), and
    the motion vectors a non-key frame receives are non-zero where the plain --frames demo passes zeros."""
    from lsfa_amd import demo
    write_clip(tmp_path / "frames", 10, 200, 120, (3, -2), seed=6)
    seen = {}
    plain = demo.FrameDirClip.mv_res

    def recording(self, i, key_i):
        mv, res = plain(self, i, key_i)
        seen.setdefault(seen["run"], {})[i] = (mv.detach().cpu().clone(), res.detach().cpu().clone())
        return mv, res

    monkeypatch.setattr(demo.FrameDirClip, "mv_res", recording)
    outs = {}
    for run, extra in (("estimate", ["--estimate-mv", "--dump-mv", str(tmp_path / "mv")]), ("read", ["--mv", str(tmp_path / "mv")]), ("zero", [])):
        seen["run"] = run
        out = tmp_path / (run + ".json")
        demo.main(["--frames", str(tmp_path / "frames"), "--interval", "5", "--score", "0.05", "--out", str(out)] + extra)
        outs[run] = json.loads(out.read_text())
    assert sorted(p.name for p in (tmp_path / "mv").iterdir()) == ["%06d.npz" % i for i in (1, 2, 3, 4, 6, 7, 8, 9)]
    assert [r["key"] for r in outs["estimate"]] == [i % 5 == 0 for i in range(10)]
    for i in (1, 2, 3, 4, 6, 7, 8, 9):
        e_mv, e_res = seen["estimate"][i]
        r_mv, r_res = seen["read"][i]
        assert torch.equal(e_mv, r_mv) and torch.equal(e_res, r_res), i          # host and device transform_mv_res agree bit for bit
        assert float(e_mv.abs().max()) > 0 and float(seen["zero"][i][0].abs().max()) == 0
    assert outs["estimate"] == outs["read"]
    assert sum(len(r["dets"]) for r in outs["estimate"]) > 0
