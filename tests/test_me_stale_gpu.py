"""lsfa_mv_key_sad / lsfa_mv_key_sad_accu (lsfa_amd/csrc/me_key.hip), hip.SegmentMotionEstimator / hip.MotionEstimator with stale= and
TestLoader(estimate_mv=dict(stale=...)) on the GPU: both kernels through the C ABI against tests/ref_me_stale.py bit for bit at the smallest
shapes at which they can go wrong, the refusals, rows and source maps that point outside the frame (defined behaviour on valid buffers),
the estimators with the mode on against the same estimators with it off, graph capture, a synthetic clip with a dissolve and a hard cut
through both frame loops, and the two command lines once each.  tests/test_me_stale_cpu.py pins the reference and the margins the
expectations rest on."""
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import me_util
import ref_me
import ref_me_cut as rc
import ref_me_stale as rs
import test_me_stale_cpu as cpu
from me_util import plane_stack, t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEANS = (102.9801, 115.9465, 122.7717)
PIXEL_SCALE = 0.5


def lumas(n, width, height, seed):
    return [ref_me.luma(f) for f in me_util.clip(n, width, height, seed)]


def key_sad(hip, luma_ptr, stride, C, F, width, height, rows):
    """lsfa_mv_key_sad through the C ABI into a buffer of exactly the promised size between two guard words -> (C, F, mbh, mbw) host array"""
    mbh, mbw = -(-height // 16), -(-width // 16)
    n = C * F * mbh * mbw
    buf = torch.full((n + 2,), -7, dtype=torch.int32, device=DEV)
    assert tuple(rows.shape) == (C, F, mbh * mbw, 7) and rows.is_contiguous() and rows.dtype == torch.int32
    code = hip.lib().lsfa_mv_key_sad(luma_ptr, stride, C, F, width, height, rows.data_ptr(), buf[1:].data_ptr(), None)
    assert code == 0, hip.lib().lsfa_last_error()
    torch.cuda.synchronize()
    assert int(buf[0]) == -7 and int(buf[-1]) == -7
    return buf[1:-1].view(C, F, mbh, mbw).cpu().numpy()


def check_key_sad(hip, planes, chains, rows, stack=None):
    """lsfa_mv_key_sad on plane_stack(planes, chains) and `rows` == ref_me_stale.key_sad on the same planes and rows, bit for bit"""
    stack = plane_stack(planes, chains) if stack is None else stack
    host = np.stack([np.stack([planes[i] for i in chain]) for chain in chains])
    C, F1, H, W = host.shape
    got = key_sad(hip, stack.data_ptr(), stack.stride(1), C, F1 - 1, W, H, rows)
    want = rs.key_sad(host, rows.cpu().numpy())
    np.testing.assert_array_equal(got, want)
    assert want.max() <= 65280
    return got


# ---- lsfa_mv_key_sad -------------------------------------------------------------------------------------------------------------------------------
def test_key_sad_small_unaligned_plane(hip):
    """37 x 23, R = 4, F = 3: rows that are not dword aligned, blocks cut by both edges, planes a padded size apart"""
    planes = lumas(4, 37, 23, seed=1)
    stack = plane_stack(planes, [[0, 1, 2, 3]])
    got = check_key_sad(hip, planes, [[0, 1, 2, 3]], hip.mv_estimate_chain(stack, 4, 4, 0), stack)
    assert got.any()


@pytest.mark.parametrize("levels", [0, 1])
def test_key_sad_two_chains(hip, levels):
    """250 x 130 (10-pixel and 2-row edge blocks), two chains, F = 4, on the full search's rows and on the pyramid's (L = 1) level-0 rows; the
    second chain crosses a scene change"""
    width, height = 250, 130
    planes = lumas(3, width, height, seed=1) + lumas(2, width, height, seed=2)
    chains = [[0, 1, 2, 1, 0], [1, 2, 3, 4, 3]]
    stack = plane_stack(planes, chains)
    if levels == 0:
        rows = hip.mv_estimate_chain(stack, 8, 4, 0)
    else:
        p1 = hip.luma_pyramid(stack.reshape(10, height, width), 1)[0]
        rows = hip.mv_refine_chain(stack, hip.mv_estimate_chain(p1.view(2, 5, p1.shape[1], p1.shape[2]), 8, 4, 0), 2, 4, 0)
    check_key_sad(hip, planes, chains, rows, stack)


def test_key_sad_longest_walk(hip):
    """96 x 64, F = 9: nine steps back from the last frame"""
    planes = lumas(10, 96, 64, seed=3)
    chains = [list(range(10))]
    stack = plane_stack(planes, chains)
    got = check_key_sad(hip, planes, chains, hip.mv_estimate_chain(stack, 8, 4, 0), stack)
    assert got[0, 8].any()


def test_key_sad_on_a_stack_stored_in_reverse(hip):
    """96 x 64, F = 3, the key frame LAST in memory and the planes 12 bytes further apart than they are large: the negative stride"""
    width, height = 96, 64
    planes = lumas(4, width, height, seed=4)
    rows = hip.mv_estimate_chain(plane_stack(planes, [[0, 1, 2, 3]]), 8, 4, 0)
    stride = width * height + 12
    memory = plane_stack(planes, [[3, 2, 1, 0]], stride=stride)[0]
    assert memory.stride(0) == stride
    got = key_sad(hip, memory[3].data_ptr(), -stride, 1, 3, width, height, rows)
    np.testing.assert_array_equal(got, rs.key_sad(np.stack(planes)[None], rows.cpu().numpy()))


def test_key_sad_tiny_plane(hip):
    """5 x 3, F = 1: one block of 15 pixels, a plane smaller than two dwords of a row"""
    planes = [np.random.RandomState(s).randint(0, 256, (3, 5)).astype(np.uint8) for s in (1, 2)]
    stack = plane_stack(planes, [[0, 1]])
    check_key_sad(hip, planes, [[0, 1]], hip.mv_estimate_chain(stack, 2, 4, 0), stack)


def test_key_sad_refuses_what_the_chain_search_refuses(hip):
    """a stack or stride lsfa_mv_estimate_chain refuses is refused by lsfa_mv_key_sad with the same code, and nothing is launched"""
    L = hip.lib()
    W, H = 96, 64
    luma = torch.zeros((1, 3, H, W), dtype=torch.uint8, device=DEV)
    rows = torch.zeros((1, 2, 24, 7), dtype=torch.int32, device=DEV)
    out = torch.full((1, 2, 4, 6), -7, dtype=torch.int32, device=DEV)
    mvs = torch.full((1, 2, 24, 7), -7, dtype=torch.int32, device=DEV)
    for kw, text in ((dict(luma=None), b"NULL"), (dict(W=0), b"bad frame size"), (dict(H=-1), b"bad frame size"), (dict(C=0), b"at least 1"),
                     (dict(F=0), b"at least 1"), (dict(stride=W * H - 4), b"plane stride"), (dict(stride=-(W * H - 4)), b"plane stride"),
                     (dict(stride=W * H + 2), b"multiple of 4"), (dict(stride=1 << 36), b"2^36"), (dict(luma=luma.data_ptr() + 1), b"4-byte aligned"),
                     (dict(C=1 << 16, F=1 << 12), b"exceed one grid")):
        a = dict(luma=luma.data_ptr(), stride=W * H, C=1, F=2, W=W, H=H)
        a.update(kw)
        want = L.lsfa_mv_estimate_chain(a['luma'], a['stride'], a['C'], a['F'], a['W'], a['H'], 4, 4, 0, mvs.data_ptr(), None, None)
        got = L.lsfa_mv_key_sad(a['luma'], a['stride'], a['C'], a['F'], a['W'], a['H'], rows.data_ptr(), out.data_ptr(), None)
        msg = L.lsfa_last_error()
        assert got == want != 0 and text in msg and b"lsfa_mv_key_sad" in msg, (kw, got, want, msg)
    for kw in (dict(rows=None), dict(out=None)):
        assert L.lsfa_mv_key_sad(luma.data_ptr(), W * H, 1, 2, W, H, kw.get('rows', rows.data_ptr()), kw.get('out', out.data_ptr()), None) != 0
        assert b"NULL" in L.lsfa_last_error()
    acc = torch.zeros((H, W, 2), dtype=torch.int32, device=DEV)
    for args, text in (((None, luma.data_ptr(), acc.data_ptr(), W, H, out.data_ptr()), b"NULL"), ((luma.data_ptr(), luma.data_ptr(), acc.data_ptr(), 0, H, out.data_ptr()), b"bad frame size"),
                       ((luma.data_ptr() + 2, luma.data_ptr(), acc.data_ptr(), W, H, out.data_ptr()), b"aligned"),
                       ((luma.data_ptr(), luma.data_ptr(), acc.data_ptr() + 4, W, H, out.data_ptr()), b"aligned")):
        assert L.lsfa_mv_key_sad_accu(*(args + (None,))) != 0
        msg = L.lsfa_last_error()
        assert text in msg and b"lsfa_mv_key_sad_accu" in msg, msg
    torch.cuda.synchronize()
    assert (out == -7).all() and (mvs == -7).all()          # nothing was launched


def test_rows_that_point_outside_the_frame(hip):
    """hand-made rows (not the estimator's): steps that would leave the frame by a little, by a lot and by more than an int holds are not
    taken, as the reference says - defined behaviour, every read inside the planes and the table"""
    width, height = 96, 64
    planes = lumas(3, width, height, seed=5)
    rows = np.stack([ref_me.estimate(planes[f], planes[f - 1], 4, 4, 0)[0] for f in (1, 2)])[None].copy()
    rows[0, 0, 0, 3:5] -= (5, 3)                     # frame 1, block (0, 0): its first columns / rows would come from outside
    rows[0, 0, 23, 3:5] += (40, 0)                   # the last block: wholly outside
    rows[0, 1, 7, 3:7] = (2 ** 31 - 1, -2 ** 31, -2 ** 31, 2 ** 31 - 1)          # differences beyond 32 bits
    rows[0, 1, 8, 3:5] = (-100000, 100000)
    rows[0, 1, 9, 3:5] += (0, -64)                   # straight up and out
    dev = t(rows)
    got = check_key_sad(hip, planes, [[0, 1, 2]], dev)
    assert got.any()


# ---- lsfa_mv_key_sad_accu ----------------------------------------------------------------------------------------------------------------------------
def key_sad_accu(hip, cur, key, accu, width, height):
    mbh, mbw = -(-height // 16), -(-width // 16)
    buf = torch.full((mbh * mbw + 2,), -7, dtype=torch.int32, device=DEV)
    code = hip.lib().lsfa_mv_key_sad_accu(cur.data_ptr(), key.data_ptr(), accu.data_ptr(), width, height, buf[1:].data_ptr(), None)
    assert code == 0, hip.lib().lsfa_last_error()
    torch.cuda.synchronize()
    assert int(buf[0]) == -7 and int(buf[-1]) == -7
    return buf[1:-1].view(mbh, mbw).cpu().numpy()


def test_accu_form_equals_the_segment_form(hip):
    """250 x 130, F = 4: on the source map MotionVectorAccumulator holds after frames 1..f, lsfa_mv_key_sad_accu equals frame f of
    lsfa_mv_key_sad - the walk-back identity on the device - for every f"""
    width, height = 250, 130
    planes = lumas(3, width, height, seed=1) + lumas(2, width, height, seed=2)
    chains = [[0, 1, 2, 3, 4]]
    stack = plane_stack(planes, chains)
    rows = hip.mv_estimate_chain(stack, 8, 4, 0)
    want = check_key_sad(hip, planes, chains, rows, stack)
    acc = hip.MotionVectorAccumulator(width, height, DEV)
    for f in range(1, 5):
        acc.add_frame(rows[0, f - 1], max_block_area=256)
        np.testing.assert_array_equal(key_sad_accu(hip, stack[0, f], stack[0, 0], acc.accu, width, height), want[0, f - 1], err_msg="frame %d" % f)


def test_accu_entries_outside_the_plane_read_as_zero(hip):
    """a hand-made source map with entries outside the plane (the accumulator never makes one): they read as 0, as the reference says"""
    width, height = 37, 23
    cur, key = lumas(2, width, height, seed=6)
    r = np.random.RandomState(8)
    accu = np.stack([r.randint(-3, width + 3, (height, width)), r.randint(-3, height + 3, (height, width))], axis=-1).astype(np.int32)
    accu[0, 0], accu[1, 1], accu[2, 2] = (-2 ** 31, 0), (0, 2 ** 31 - 1), (width, height)
    inside = (accu[..., 0] >= 0) & (accu[..., 0] < width) & (accu[..., 1] >= 0) & (accu[..., 1] < height)
    assert inside.any() and not inside.all()
    stack = plane_stack([cur, key], [[0, 1]])
    got = key_sad_accu(hip, stack[0, 0], stack[0, 1], t(accu), width, height)
    np.testing.assert_array_equal(got, rs.key_sad_accu(cur, key, accu))


# ---- the estimators --------------------------------------------------------------------------------------------------------------------------------
def dissolve_stack():
    """the dissolve clip of tests/test_me_stale_cpu.py forwards and backwards, two clips in lock step: (2, 8, 64, 96, 3) grey frames and their planes"""
    ys = rs.dissolve_clip()
    chains = [ys, ys[::-1]]
    return t(np.stack([np.stack([rs.bgr(y) for y in chain]) for chain in chains])), np.stack([np.stack(chain) for chain in chains])


@pytest.mark.parametrize("levels", [0, 1])
def test_segment_estimator_with_stale(hip, levels):
    """stale= changes nothing the estimator returned before - rows, SAD, motion_vector and res_diff equal the same estimator's without it, bit
    for bit - and adds .keysad / .key_unmatched == the reference on the estimator's own rows; first_cuts() on the dissolve gives the
    reference's frame with stale alone and with cut + stale, None with cut alone; a short segment; one captured graph replayed twice"""
    width, height = 96, 64
    stack, host = dissolve_stack()
    kw = dict(frames=7, clips=2, device=DEV, search=4, lam=4, levels=levels)
    plain, stale = hip.SegmentMotionEstimator(width, height, **kw), hip.SegmentMotionEstimator(width, height, stale=dict(), **kw)
    both, cut = hip.SegmentMotionEstimator(width, height, cut=dict(), stale=dict(), **kw), hip.SegmentMotionEstimator(width, height, cut=dict(), **kw)
    assert plain.stale is None and plain.keysad is None and stale.stale == (rs.BIAS, rs.PERCENT) and stale.cut is None and cut.stale is None
    want_mv, want_res = [x.clone() for x in plain.segment(stack, 1.25, MEANS, PIXEL_SCALE)]
    for est in (stale, both, cut):
        mv, res = est.segment(stack, 1.25, MEANS, PIXEL_SCALE)
        assert torch.equal(mv, want_mv) and torch.equal(res, want_res) and torch.equal(est.rows, plain.rows) and torch.equal(est.sad, plain.sad)
    want_sad, want_intra, want_un = rs.key_score(host, stale.rows.cpu().numpy())
    pair_un = rc.cut_score(host, plain.sad.cpu().numpy())[1]
    for est in (stale, both):
        assert tuple(est.keysad.shape) == (2, 7, 4, 6) and tuple(est.key_unmatched.shape) == (2, 7)
        np.testing.assert_array_equal(est.keysad.cpu().numpy(), want_sad)
        np.testing.assert_array_equal(est.key_unmatched.cpu().numpy(), want_un)
    np.testing.assert_array_equal(both.unmatched.cpu().numpy(), pair_un)
    np.testing.assert_array_equal(both.intra.cpu().numpy(), want_intra)
    key_flags, pair_flags = rc.is_cut(want_un, 24), rc.is_cut(pair_un, 24)
    want_first = rs.first_flagged(key_flags)
    assert not pair_flags.any() and want_first[0] is not None and want_first[1] is not None
    if levels == 0:
        assert want_un[0].tolist() == cpu.DISSOLVE[1] and want_first[0] == 5           # the figures tests/test_me_stale_cpu.py records
    assert stale.first_cuts() == want_first == both.first_cuts() and cut.first_cuts() == [None, None]
    assert stale.first_cuts(want_first[0] - 1)[0] is None
    with pytest.raises(hip.LsfaError, match="first_cuts"):
        plain.first_cuts()

    # one graph, no parallel branch: replayed on new contents and on the first contents again
    buf = stack.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_mv, g_res = both.segment(buf, 1.25, MEANS, PIXEL_SCALE)
    other = stack.flip(0).contiguous()
    e_mv, e_res = [x.clone() for x in plain.segment(other, 1.25, MEANS, PIXEL_SCALE)]
    for contents, w_mv, w_res, w_un in ((other, e_mv, e_res, want_un[::-1]), (stack, want_mv, want_res, want_un)):
        buf.copy_(contents)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_mv, w_mv) and torch.equal(g_res, w_res)
        np.testing.assert_array_equal(both.key_unmatched.cpu().numpy(), w_un)
    assert not np.array_equal(want_un[0], want_un[1])

    # the short segment in front of a clip's last frame: one clip, n = 3 of a stack of eight frames, parameters of its own
    one = hip.SegmentMotionEstimator(width, height, frames=7, clips=1, device=DEV, search=4, lam=4, levels=levels, stale=dict(bias=0, percent=10))
    one.segment(stack[:1], 1.0, MEANS, PIXEL_SCALE, n=3)
    assert tuple(one.key_unmatched.shape) == (1, 3) and tuple(one.keysad.shape) == (1, 3, 4, 6)
    w_sad, _, w_un = rs.key_score(host[:1, :4], one.rows.cpu().numpy(), 0)
    np.testing.assert_array_equal(one.keysad.cpu().numpy(), w_sad)
    np.testing.assert_array_equal(one.key_unmatched.cpu().numpy(), w_un)
    assert one.first_cuts() == rs.first_flagged(rc.is_cut(w_un, 24, 10))


@pytest.mark.parametrize("levels", [0, 1])
def test_motion_estimator_with_stale(hip, levels):
    """frame by frame over the dissolve: rows and SAD of the estimator without stale=, .keysad / .key_unmatched equal to the segment form's
    frame by frame, is_cut() true from the same frame on; nothing is allocated after construction"""
    width, height = 96, 64
    stack, host = dissolve_stack()
    seg = hip.SegmentMotionEstimator(width, height, frames=7, clips=2, device=DEV, search=4, lam=4, levels=levels, stale=dict())
    seg.segment(stack, 1.0, MEANS, PIXEL_SCALE)
    want_sad, want_un = seg.keysad.cpu().numpy(), seg.key_unmatched.cpu().numpy()
    np.testing.assert_array_equal(want_un, rs.key_score(host, seg.rows.cpu().numpy())[2])
    first = seg.first_cuts()
    for c in (0, 1):
        plain = hip.MotionEstimator(width, height, DEV, search=4, lam=4, levels=levels)
        me = hip.MotionEstimator(width, height, DEV, search=4, lam=4, levels=levels, stale=dict())
        assert plain.key_unmatched is None and tuple(me.key_unmatched.shape) == (1,) and me.unmatched is None
        plain.key_frame(stack[c, 0])
        me.key_frame(stack[c, 0])
        flags = []
        for f in range(1, 8):
            cur = stack[c, f]
            if f == 2:           # around the second frame: every buffer of the mode was allocated at construction
                gc.collect()
                before = torch.cuda.memory_allocated()
            rows = me.next_frame(cur)
            if f == 2:
                assert torch.cuda.memory_allocated() == before
            assert torch.equal(rows, plain.next_frame(stack[c, f])) and torch.equal(me.sad, plain.sad), (c, f)
            np.testing.assert_array_equal(me.keysad.cpu().numpy(), want_sad[c, f - 1], err_msg="clip %d frame %d" % (c, f))
            assert me.key_unmatched.tolist() == [int(want_un[c, f - 1])], (c, f)
            flags.append(me.is_cut())
        assert flags.index(True) + 1 == first[c] and flags == rc.is_cut(want_un[c], 24).tolist()
    with pytest.raises(hip.LsfaError, match="without cut"):
        plain.is_cut()


def test_motion_estimator_with_stale_on_decoder_planes(hip):
    """key_frame_yuv / next_frame_yuv with luma_from='y': the search and the key rule read the decoder's Y plane, so on Y = the dissolve's
    planes the counts are the segment form's on those planes; cut + stale together, is_cut() the union"""
    width, height = 96, 64
    ys = rs.dissolve_clip()
    host = np.stack(ys)[None]
    uv = torch.full((height // 2, width), 128, dtype=torch.uint8, device=DEV)
    me = hip.MotionEstimator(width, height, DEV, search=4, lam=4, luma_from='y', cut=dict(), stale=dict())
    me.key_frame_yuv(t(ys[0]), uv=uv)
    rows, counts, flags = [], [], []
    for f in range(1, 8):
        me.next_frame_yuv(t(ys[f]), uv=uv)
        rows.append(me.rows.cpu().numpy().copy())
        counts.append(int(me.key_unmatched[0]))
        assert int(me.unmatched[0]) == 0
        flags.append(me.is_cut())
    want_un = rs.key_score(host, np.stack(rows)[None])[2]
    assert counts == want_un[0].tolist() == cpu.DISSOLVE[1] and flags == rc.is_cut(want_un[0], 24).tolist()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------
def test_clip_with_a_dissolve_and_a_cut_through_both_frame_loops(hip, monkeypatch):
    """The 24-frame synthetic clip of test_me_stale_cpu.E2E (K = 10, a dissolve over frames 3..5, a new scene at frame 18; decisive by that
    file's margin check) with the key rule alone: the loader's flags are the plan the CPU test derived in the serial loop and in both
    pipelined forms, every frame delivers its detections, pred_eval_pipelined frame by frame equals pred_eval bit for bit, and with whole
    segments batched and three key frames grouped the bank check (the key frames upcoming_key_frames announced are the ones handed out) does
    not raise."""
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.core.loader import TestLoader
    from lsfa_amd.function import test_rcnn as T
    from lsfa_amd.symbols import params as P
    from lsfa_amd.utils.synthetic import synthetic_roidb
    e = cpu.E2E
    assert e['clip_id'] == 0
    cfg = lsfa_test_config(key_frame_interval=e['interval'])
    arg, aux = P.init_params(cfg, seed=3)
    roidb = synthetic_roidb(1, e['frames'], e['height'], e['width'], e['interval'], cuts=e['cuts'], dissolves=e['dissolves'])
    cfg.TEST.ESTIMATE_MV = dict(search=e['search'], lam=4, stale=dict())
    want_flags = [(0 if f == 0 else 1) if f in e['keys'] else 2 for f in range(e['frames'])]
    runs = []

    class FlagLoader(TestLoader):
        def __init__(self, *a, **kw):
            self.flags = []
            runs.append(self)
            TestLoader.__init__(self, *a, **kw)

        def next(self):
            out = TestLoader.next(self)
            self.flags.append(out[1])
            return out

    monkeypatch.setattr(T, "TestLoader", FlagLoader)
    rows_serial, ids_serial = T.test_rcnn(cfg, roidb, arg, aux, device=DEV, pipeline=False)
    rows_frame, ids_frame = T.test_rcnn(cfg, roidb, arg, aux, device=DEV, pipeline=True, segment=0, key_group=1)
    rows_batch, ids_batch = T.test_rcnn(cfg, roidb, arg, aux, device=DEV, pipeline=True, segment=e['interval'] - 1, key_group=3)
    assert [r.flags for r in runs] == [want_flags] * 3
    assert all(r.cut and not r._segments for r in runs)
    assert sorted(np.asarray(ids_serial).tolist()) == list(range(e['frames']))          # every frame was delivered
    np.testing.assert_array_equal(ids_frame, ids_serial)
    np.testing.assert_array_equal(ids_batch, ids_serial)
    assert len(rows_serial) > 0 and len(rows_batch) > 0
    np.testing.assert_array_equal(rows_frame, rows_serial)


def child(args, timeout):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m"] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


@pytest.mark.subprocess
def test_test_command_line_with_stale_key(hip, tmp_path):
    """python -m lsfa_amd.test --estimate-mv --stale-key --synthetic-dissolves in a child process: the clip of E2E's first twelve frames runs
    through, and the options that do not go together are refused"""
    out = tmp_path / "dets.npy"
    child(["lsfa_amd.test", "--clips", "1", "--frames", "12", "--height", "128", "--width", "192", "--interval", "10", "--estimate-mv", "--search", "8",
           "--stale-key", "--stale-bias", "4", "--scene-cut", "--synthetic-dissolves", "3:3", "--out", str(out)], 600)
    rows = np.load(str(out))
    assert rows.ndim == 2 and rows.shape[1] == 7 and len(rows) > 0
    from lsfa_amd import test as test_cli
    for bad in (["--stale-key"], ["--estimate-mv", "--stale-key", "0"], ["--estimate-mv", "--stale-key", "--stale-bias", "256"],
                ["--synthetic-dissolves", "3"], ["--synthetic-dissolves", "a:b"]):
        monkey = pytest.MonkeyPatch()
        monkey.setattr(sys, "argv", ["test"] + bad)
        with pytest.raises(SystemExit):
            test_cli.parse_args()
        monkey.undo()


@pytest.mark.subprocess
def test_demo_command_line_with_stale_key(hip, tmp_path):
    """python -m lsfa_amd.demo --frames DIR --estimate-mv --stale-key in a child process on the dissolve clip as eight PNG frames (interval
    10): the loop's key frames are frame 0 and the frames hip.MotionEstimator's is_cut() reports - from the numpy reference: every chain
    starts over at its stale frame"""
    from PIL import Image
    ys = rs.dissolve_clip()
    (tmp_path / "frames").mkdir()
    for i, y in enumerate(ys):
        Image.fromarray(rs.bgr(y)).save(str(tmp_path / "frames" / ("%06d.png" % i)))
    keys, last = [0], 0
    for f in range(1, len(ys)):
        key_un = rs.chain_counts(ys[last:f + 1], 4)[1]
        assert key_un[-1] * 100 <= 30 * 24 or key_un[-1] * 100 >= 70 * 24, (last, f, key_un)          # decisive, as in the CPU test
        if rc.is_cut(key_un[-1], 24):
            keys.append(f)
            last = f
    assert keys[:2] == [0, 5]
    out = tmp_path / "stale.json"
    child(["lsfa_amd.demo", "--frames", str(tmp_path / "frames"), "--estimate-mv", "--search", "4", "--stale-key", "--interval", "10", "--score", "0.05",
           "--out", str(out)], 600)
    got = json.loads(out.read_text())
    assert [r["key"] for r in got] == [f in keys for f in range(len(ys))]
    from lsfa_amd import demo
    for bad in (["--stale-key"], ["--frames", str(tmp_path / "frames"), "--estimate-mv", "--stale-key", "101"]):
        with pytest.raises(SystemExit):
            demo.parse_args(bad)
