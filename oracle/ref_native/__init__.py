"""oracle/_ref: the reference's own PSROI pooling, MultiProposal and motion-vector accumulation, compiled for
the host.  TEST INFRASTRUCTURE ONLY, like the rest of ``oracle``.

``build()`` cuts the functions out of the reference tree (``slice.py``) into ``oracle/_ref/*.inc`` and compiles
the committed drivers around them.  Neither the slices nor the objects are ever committed, and where the
reference tree is absent ``build()`` does nothing.  The tests do not need ``oracle/_ref``: they read what the
`on` build computed from ``tests/golden/ref_native.npz`` (``tests/golden/make_native_golden.py``).

Three shared objects come from the same slices, differing only in the floating-point contraction flag, because
the reference's text does not fix it: ``on`` (a*b + c fuses inside one expression; the rule claimed for nvcc's
default, and the authoritative build), ``off`` and ``fast``.
"""
import ctypes
import os
import subprocess

import numpy as np

from . import slice as _slice

_HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(_HERE), "_ref")
MODES = ("on", "off", "fast")
CXX = os.environ.get("LSFA_REF_CXX", "/opt/rocm/llvm/bin/clang++")
CC = os.environ.get("LSFA_REF_CC", "/opt/rocm/llvm/bin/clang")


def reference_root():
    return os.environ.get("LSFA_REFERENCE", "/root/reference")


def available():
    return os.path.isdir(os.path.join(reference_root(), _slice.OPS))


def ops_so(mode):
    return os.path.join(OUT, "libref_ops_%s.so" % mode)


def coviar_so():
    return os.path.join(OUT, "libref_coviar.so")


def build(force=False):
    """Slice and compile into oracle/_ref.  Returns the directory, or None where there is no reference tree."""
    if not available():
        return None
    wanted = [ops_so(m) for m in MODES] + [coviar_so()]
    if not force and all(os.path.exists(p) for p in wanted):
        return OUT
    _slice.write(reference_root(), OUT)
    common = ["-O2", "-fPIC", "-shared", "-fno-fast-math", "-I", OUT, "-I", _HERE]
    for mode in MODES:
        subprocess.check_call([CXX, "-std=c++14", "-mfma", "-ffp-contract=%s" % mode] + common +
                              ["-o", ops_so(mode), os.path.join(_HERE, "ref_ops_driver.cpp"), "-lpthread", "-lm"])
    subprocess.check_call([CC, "-std=gnu11"] + common + ["-o", coviar_so(), os.path.join(_HERE, "ref_coviar_driver.c")])
    return OUT


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


_ci, _cf = ctypes.c_int, ctypes.c_float


class Ops(object):
    """ctypes face of one libref_ops_<mode>.so, with the signatures of the oracle's functions of the same name."""

    def __init__(self, mode="on"):
        self.mode = mode
        self.lib = ctypes.CDLL(ops_so(mode))

    def generate_anchors(self, feature_stride=16, ratios=(0.5, 1, 2), scales=(8, 16, 32)):
        r, s = _f32(ratios), _f32(scales)
        out = np.empty((len(r) * len(s), 5), np.float32)
        n = self.lib.ref_generate_anchors(_ci(feature_stride), _p(r), _ci(len(r)), _p(s), _ci(len(s)), _p(out))
        assert n == out.shape[0]
        return out

    def psroi_pool(self, data, rois, spatial_scale, output_dim, pooled_size, group_size):
        data, rois = _f32(data), _f32(rois)
        _, C, H, W = data.shape
        R = rois.shape[0]
        out = np.empty((R, output_dim, pooled_size, pooled_size), np.float32)
        mc = np.empty_like(out)
        rc = self.lib.ref_psroi_pool(_p(data), _p(rois), _ci(C), _ci(H), _ci(W), _ci(R), _cf(spatial_scale), _ci(output_dim),
                                     _ci(pooled_size), _ci(group_size), _p(out), _p(mc))
        assert rc == 0, "launch geometry would run a thread's loop body twice"
        return out, mc

    def proposal(self, cls_prob, bbox_pred, im_info, feature_stride=16, scales=(8, 16, 32), ratios=(0.5, 1, 2),
                 rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300, threshold=0.7, rpn_min_size=0):
        """-> dict(decode (B, count, 5), order (B, pre_n), keep (B, pre_n; -1 past nkeep), nkeep (B), rois, scores)"""
        cls_prob, bbox_pred, im_info = _f32(cls_prob), _f32(bbox_pred), _f32(im_info)
        B, A2, H, W = cls_prob.shape
        A = A2 // 2
        count = A * H * W
        pre_n = min(rpn_pre_nms_top_n if rpn_pre_nms_top_n > 0 else count, count)
        post_n = min(rpn_post_nms_top_n, pre_n)
        s, r = _f32(scales), _f32(ratios)
        rois = np.empty((B * post_n, 5), np.float32)
        scores = np.empty((B * post_n, 1), np.float32)
        decode = np.empty((B, count, 5), np.float32)
        order = np.empty((B, pre_n), np.int32)
        keep = np.full((B, pre_n), -1, np.int32)
        nkeep = np.empty(B, np.int32)
        self.lib.ref_multi_proposal(_p(cls_prob), _p(bbox_pred), _p(im_info), _ci(B), _ci(A), _ci(H), _ci(W), _ci(feature_stride),
                                    _p(s), _ci(len(s)), _p(r), _ci(len(r)), _ci(rpn_pre_nms_top_n), _ci(rpn_post_nms_top_n),
                                    _cf(threshold), _ci(rpn_min_size), _p(rois), _p(scores), _p(decode), _p(order), _p(keep), _p(nkeep))
        return dict(decode=decode, order=order, keep=keep, nkeep=nkeep, rois=rois, scores=scores)


def coviar_gop(frames, width, height, bgr_ref, bgr_cur):
    """frames: list of (n, 7) int32 block lists.  -> accu (F, H, W, 2) after every frame, mv (H, W, 2), res (H, W, 3), all
    int32 and in the PROJECT's layout: the reference's x-major maps are transposed here."""
    lib = ctypes.CDLL(coviar_so())
    rows = np.ascontiguousarray(np.concatenate([np.asarray(f, np.int32).reshape(-1, 7) for f in frames]), np.int32)
    counts = np.array([len(f) for f in frames], np.int32)
    bgr = np.ascontiguousarray(np.stack([bgr_ref, bgr_cur]), np.uint8)
    out = {}
    for rep, name in ((1, "mv"), (2, "res")):          # the loader's two representations, one decode each
        accu = np.empty((len(frames), width, height, 2), np.int32)
        mv = np.zeros((height, width, 2), np.int32)
        res = np.zeros((height, width, 3), np.int32)
        rc = lib.ref_coviar_gop(_p(rows), _p(counts), _ci(len(frames)), _ci(width), _ci(height), _ci(rep), _p(bgr), _p(accu),
                                _p(mv), _p(res))
        assert rc == 0, "a block row exceeds AVMotionVector's field widths"
        out[name] = mv if rep == 1 else res
        out.setdefault("accu", np.ascontiguousarray(accu.transpose(0, 2, 1, 3)))
        assert np.array_equal(out["accu"], accu.transpose(0, 2, 1, 3))
    return out["accu"], out["mv"], out["res"]
