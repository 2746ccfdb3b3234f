"""The segment form of the motion front end, without a device: the walk-back identity lsfa_mv_segment_inputs rests on (tests/ref_me_segment.py
against oracle.coviar_accumulate chained over tests/ref_me.py rows), the two exports' declarations and derived bindings, and the segment
boundaries of TestLoader(estimate_mv=...) on a stub estimator.  tests/test_me_segment_gpu.py compares the kernels with these references."""
import os
import re

import numpy as np
import pytest
import torch

import oracle
import ref_me
import ref_me_segment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chain_rows(frames, search, lam, max_sad):
    lum = [ref_me.luma(f) for f in frames]
    return np.stack([ref_me.estimate(lum[f], lum[f - 1], search, lam, max_sad)[0] for f in range(1, len(frames))])


@pytest.mark.parametrize("width,height,search,max_sad,sigma", [(250, 130, 16, 0, 0.0),        # partial blocks of 10 columns / 2 rows
                                                               (37, 23, 4, 0, 3.0),           # one partial row and column, search cut by the frame
                                                               (96, 64, 8, 900, 3.0)])        # zero vectors inside a chain
def test_walk_equals_the_chained_accumulation(width, height, search, max_sad, sigma):
    """accu_f from the rows of frames 1..f alone == oracle.coviar_accumulate frame by frame, f = 1..5, bit for bit"""
    frames = ref_me.translated_clip(6, width, height, (3, -2), seed=width, sigma=sigma)
    rows = chain_rows(frames, search, 4, max_sad)
    if max_sad:
        v = rows[:, :, 3:5] - rows[:, :, 5:7]
        zero = (v == 0).all(axis=2)
        assert zero.any() and not zero.all()                   # the threshold bites: zero and non-zero vectors in one chain
    walked = ref_me_segment.walk(rows, width, height)
    accu = oracle.coviar_identity(width, height)
    for f in range(1, 6):
        accu = oracle.coviar_accumulate(rows[f - 1], accu)
        np.testing.assert_array_equal(walked[f - 1], accu, err_msg="frame %d" % f)
        np.testing.assert_array_equal(ref_me_segment.field(walked[f - 1]), oracle.coviar_mv(accu))
        np.testing.assert_array_equal(ref_me_segment.residual(frames[f], frames[0], walked[f - 1]), oracle.coviar_residual(frames[f], frames[0], accu))
    assert any((w != oracle.coviar_identity(width, height)).any() for w in walked)


def test_a_step_that_leaves_the_frame_is_not_taken():
    """rows that are not the estimator's: the walk's own rule, against the accumulation (which does not write such a pixel either)"""
    width, height = 96, 64
    rows = ref_me.estimate(np.zeros((height, width), np.uint8), np.zeros((height, width), np.uint8), 4, 0)[0][None].copy()
    rows[0, 0, 3:5] -= (5, 3)                     # block (0, 0): source 5 left, 3 up: its first columns / rows come from outside
    rows[0, 23, 3:5] += (40, 0)                   # the last block: source 40 to the right, wholly outside
    got = ref_me_segment.walk(rows, width, height)[0]
    np.testing.assert_array_equal(got, oracle.coviar_accumulate(rows[0], oracle.coviar_identity(width, height)))
    assert (got[0, 0] == (0, 0)).all() and (got[3, 5] == (0, 0)).all() and (got[2, 9] == (9, 2)).all() and (got[63, 95] == (95, 63)).all()


def test_header_declares_and_the_binding_derives_both_exports():
    text = open(os.path.join(ROOT, "include", "lsfa_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("lsfa_mv_estimate_chain", "lsfa_mv_segment_inputs"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    from lsfa_amd import hip
    import ctypes
    for name, count in (("lsfa_mv_estimate_chain", 12), ("lsfa_mv_segment_inputs", 18)):
        ret, params = hip._PROTOTYPES[name]
        assert ret.strip() == "int" and len(params) == count, (name, params)
    chain = [hip._ctype(p) for p in hip._PROTOTYPES["lsfa_mv_estimate_chain"][1]]
    assert chain == [ctypes.c_void_p, ctypes.c_longlong] + [ctypes.c_int] * 7 + [ctypes.c_void_p] * 3
    seg = [hip._ctype(p) for p in hip._PROTOTYPES["lsfa_mv_segment_inputs"][1]]
    assert seg == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong] + [ctypes.c_int] * 4 + [ctypes.c_double] + [ctypes.c_int] * 3 + \
        [ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    for name in ("mv_estimate_chain", "mv_segment_inputs", "SegmentMotionEstimator"):
        assert hasattr(hip, name), name


class StubEstimator(object):
    """stands in for hip.SegmentMotionEstimator: records every call and returns tensors that name the frame they belong to"""

    def __init__(self, log):
        self.log = log
        self.buf = {}

    def segment(self, stack, im_scale, pixel_means, pixel_scale):
        n = int(stack.shape[1]) - 1
        self.log.append((tuple(stack.shape), stack.clone(), float(im_scale)))
        # like the real one: buffers reused from call to call - the loader must not hand these out as they are
        mv, res = self.buf.setdefault(n, (torch.empty((n, 1, 2, 2, 3)), torch.empty((n, 1, 3, 2, 3))))
        for f in range(n):
            mv[f] = float(stack[0, f + 1].sum())
            res[f] = float(stack[0, 0].sum()) + f + 1
        return mv, res


@pytest.mark.parametrize("K,n", [(10, 24), (4, 11), (4, 9), (3, 7), (1, 4)])
def test_loader_estimates_segment_by_segment(K, n):
    """TestLoader(estimate_mv=...) over two synthetic clips: one estimator call per key frame that has non-key frames behind it, on the uint8
    frames key .. key + m with m = K - 1, fewer in front of the video's last frame (a key frame by the loader's rule); the frame after a key
    frame receives slice f = 1, every non-key frame its own, and a segment's tensors survive the next segment's call."""
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.core.loader import TestLoader
    from lsfa_amd.utils.synthetic import synthetic_roidb
    cfg = lsfa_test_config(key_frame_interval=K)
    log, made = [], []

    class Loader(TestLoader):
        def _segment_estimator(self, width, height):
            made.append((width, height))
            return StubEstimator(log)

    roidb = synthetic_roidb(2, n, 32, 48, K)
    loader = Loader(roidb, cfg, device='cpu', estimate_mv=dict(search=8, lam=2))
    assert loader.estimate_mv == dict(search=8, lam=2)
    keys = sorted(set(list(range(0, n, K)) + [n - 1]))
    held, i = [], 0
    for im_info, flag, batch in loader:
        d = dict(zip(loader.data_name, batch.data[0]))
        v, f = divmod(i, n)
        clip = roidb[v]['clip']
        assert (flag != 2) == (f in keys), (K, n, f, flag)
        if flag == 2:
            key_f = max(k for k in keys if k < f)
            assert tuple(d['motion_vector'].shape) == (1, 2, 2, 3) and tuple(d['res_diff'].shape) == (1, 3, 2, 3)
            assert float(d['motion_vector'].flatten()[0]) == float(clip.frame_u8(f).sum()), (K, n, f)
            assert float(d['res_diff'].flatten()[0]) == float(clip.frame_u8(key_f).sum()) + (f - key_f), (K, n, f)
            held.append((d['motion_vector'], d['motion_vector'].clone(), d['res_diff'], d['res_diff'].clone()))
        else:
            assert torch.equal(d['motion_vector'], clip.motion_vector(f, f // K * K, 'cpu')) and torch.equal(d['res_diff'], clip.res_diff(f, 'cpu'))       # key frames: the clip's own, as ever
        i += 1
    assert i == 2 * n
    for a, a0, b, b0 in held:                     # nothing handed out was overwritten by a later segment's call
        assert torch.equal(a, a0) and torch.equal(b, b0)
    want = []
    for v in range(2):
        for k in keys:
            m = min(k + K - 1, n - 2) - k
            if m >= 1:
                want.append((v, k, m))
    assert len(log) == len(want), (K, n, [s for s, _, _ in log], want)
    for (shape, stack, scale), (v, k, m) in zip(log, want):
        assert shape == (1, m + 1, 32, 48, 3) and stack.dtype == torch.uint8 and scale == 1.0
        for g in range(m + 1):
            assert torch.equal(stack[0, g], roidb[v]['clip'].frame_u8(k + g)), (K, n, v, k, g)
    assert made == ([(48, 32)] if want else [])


def test_loader_takes_the_option_from_the_config():
    """config.TEST.ESTIMATE_MV reaches a loader built without the argument (test_rcnn builds its own); the argument, when given, wins"""
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.core.loader import TestLoader
    from lsfa_amd.utils.synthetic import synthetic_roidb
    cfg = lsfa_test_config(key_frame_interval=3)
    assert cfg.TEST.ESTIMATE_MV is None
    cfg.TEST.ESTIMATE_MV = dict(search=8, lam=2)
    log = []

    class Loader(TestLoader):
        def _segment_estimator(self, width, height):
            return StubEstimator(log)

    roidb = synthetic_roidb(1, 5, 32, 48, 3)
    assert Loader(roidb, cfg, device='cpu').estimate_mv == dict(search=8, lam=2) and len(log) == 1
    assert Loader(roidb, cfg, device='cpu', estimate_mv=dict(search=4)).estimate_mv == dict(search=4)


def test_loader_default_is_the_clip_path():
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.core.loader import TestLoader
    from lsfa_amd.utils.synthetic import synthetic_roidb
    roidb = synthetic_roidb(1, 5, 32, 48, 3)
    loader = TestLoader(roidb, lsfa_test_config(key_frame_interval=3), device='cpu')
    assert loader.estimate_mv is None
    for i, (im_info, flag, batch) in enumerate(loader):
        d = dict(zip(loader.data_name, batch.data[0]))
        key_f = 0 if i < 3 else 3
        assert torch.equal(d['motion_vector'], roidb[0]['clip'].motion_vector(i, key_f, 'cpu'))
        assert torch.equal(d['res_diff'], roidb[0]['clip'].res_diff(i, 'cpu'))
