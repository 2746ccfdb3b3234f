"""The specification of the one-piece (bf16) convolution form, in numpy / torch-on-CPU float64, for tests/test_conv_bf16_gpu.py.

lsfa_conv_fwd with pieces = 1 is specified in two lines of lsfa_amd/csrc/conv_split_kernel.h (the header comment and the comment above
PiecesN): BOTH operands are rounded to ONE bf16 value, to nearest even; their products are formed on the matrix pipe, where the product of
two bf16 values (8 x 8 significant bits) is exact in fp32; the sum is accumulated in fp32.  With the input's bn + ReLU applied at the cut
(in_scale / in_shift) the value that is rounded is max(x * in_scale + in_shift, 0) evaluated in fp32 with two roundings.

So the reference here is a float64 convolution of the ROUNDED operands: the operand rounding (2^-9 per operand, what the tests against a
float64 convolution of the unrounded operands have to allow for) is taken out of the comparison, and what is left between kernel and
reference is the fp32 accumulation alone.  bf16_rne is written with integer arithmetic on the bit pattern - not with torch's cast and
not with anything of lsfa_amd - and tests/test_ref_bf16_cpu.py pins it to torch's cast, conv_ref to a six-loop numpy statement and
deconv_crop_ref to conv_transpose2d + slicing.

The bounds (bound_ratios), both asserted wherever a kernel is compared with this reference:

  gamma   per element, |got - ref| <= gamma(K + 3, u) * ref_abs, gamma(n, u) = n u / (1 - n u) (tests/ref64.py; Higham, Accuracy and
          Stability of Numerical Algorithms, section 3.1), ref_abs the same sum over |x'|, |w|, |bias|, |residual|, K = kh * kw * Cin.
          The products are exact, so a term passes through at most K - 1 additions whatever their order; the two-level accumulation
          (one more addition per 12 chunks of 32), the K slices and the reduce pass stay within K; + 3 for bias, residual and the
          LeakyReLU multiply.  u = 2^-23, NOT 2^-24: the project states nowhere how the matrix instruction rounds its internal
          additions, and 2^-23 holds for any faithful rounding (to nearest or not).  Derived, not measured, and without margin.
  fp32    max|got - ref| < 2e-6 * sqrt(K) * max(max|ref|, 1): the project's own criterion for its fp32 forms
          (tests/test_hip_ops.py::test_conv_split_vs_float64_and_fp32_mfma), applied against the rounded-operand reference.
"""
import numpy as np
import torch
import torch.nn.functional as F

import ref64

U_FAITHFUL = 2.0 ** -23


def bf16_rne(a):
    """float32 -> float32 holding the nearest bf16 value, ties to even: u + 0x7FFF + ((u >> 16) & 1) on the bit pattern, low half cleared.
    (A value above the largest finite bf16 by half a step or more carries into the exponent 255: infinity.  NaN stays the NaN it was.)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return np.where(np.isnan(a), a, r.view(np.float32))


def activate(v, act):
    """0 none, 1 ReLU, 2 LeakyReLU(0.1)"""
    if act == 1:
        return np.maximum(v, 0.0)
    if act == 2:
        return np.where(v > 0, v, v * 0.1)
    assert act == 0
    return v


def input_at_the_cut(x_nhwc, in_scale=None, in_shift=None):
    """what the kernel rounds: x, or max(x * in_scale + in_shift, 0) in float32 with two roundings (per input channel)"""
    x = np.asarray(x_nhwc, np.float32)
    if in_scale is None:
        return x
    prod = x * np.asarray(in_scale, np.float32)               # first rounding
    return np.maximum(prod + np.asarray(in_shift, np.float32), np.float32(0))      # second rounding; the maximum is exact


def _conv64(x_nhwc, w, stride, pad_hw, dil):
    y = F.conv2d(torch.from_numpy(np.ascontiguousarray(x_nhwc, dtype=np.float64)).permute(0, 3, 1, 2), torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)),
                 None, stride, tuple(pad_hw), dil)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def conv_ref(x_nhwc, w, bias, stride, pad_hw, dil, act, residual=None, in_scale=None, in_shift=None):
    """x (N, H, W, Cin) float32, w (Cout, Cin, kh, kw) float32, bias (Cout) or None, pad_hw (pad_h, pad_w), residual (N, Ho, Wo, Cout) or
    None -> (ref, ref_abs), (N, Ho, Wo, Cout) float64: ref = act(conv(bf16_rne(x'), bf16_rne(w)) + bias + residual), ref_abs the same sum
    over |x'|, |w|, |bias|, |residual| without the activation."""
    xr, wr = bf16_rne(input_at_the_cut(x_nhwc, in_scale, in_shift)), bf16_rne(w)
    ref, ref_abs = _conv64(xr, wr, stride, pad_hw, dil), _conv64(np.abs(xr), np.abs(wr), stride, pad_hw, dil)
    for extra in (bias, residual):
        if extra is not None:
            ref = ref + np.asarray(extra, np.float64)
            ref_abs = ref_abs + np.abs(np.asarray(extra, np.float64))
    return activate(ref, act), ref_abs


def deconv_crop_ref(x_nhwc, wt, bias, Hc, Wc, act):
    """Deconvolution(4x4, stride 2) + Crop(offset 1) to Hc x Wc on rounded operands.  x (N, Hi, Wi, Cin), wt (Cin, Cout, 4, 4) (the
    Deconvolution weight layout) -> (ref, ref_abs) (N, Hc, Wc, Cout) float64.  The scatter form of tests/ref64.py: every input pixel
    into the full map, cropped afterwards."""
    ref, ref_abs = ref64.upsample_flow_ref(bf16_rne(x_nhwc), bf16_rne(wt), bias, Hc, Wc)
    return activate(ref, act), ref_abs


def bound_ratios(got, ref, ref_abs, K):
    """-> (worst err / gamma bound over the elements, max err / the fp32 criterion); both must be <= 1 (the second < 1)"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape == ref_abs.shape, (got.shape, ref.shape, ref_abs.shape)
    assert np.isfinite(got).all()
    err, bound = np.abs(got - ref), ref64.gamma(K + 3, U_FAITHFUL) * ref_abs
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()), float(err.max() / (2e-6 * np.sqrt(K) * max(float(np.abs(ref).max()), 1.0)))
