"""Float64 statements of FlowNet's small operators and the layout copies, for tests/test_hip_ops_direct.py.

Written from the operator definitions the reference's symbol uses (dff_rfcn/symbols/resnet_v1_101_flownet_rfcn.py:150-207:
Convolution pad 1; Deconvolution kernel 4 stride 2 + Crop offset (1, 1); Pooling 2x2 / 2 avg pooling_convention='full';
Pooling 3x3 / 2 pad 1 max) as plain index arithmetic on channels-last numpy arrays - NOT from the kernels' code: the
deconvolution scatters every input pixel into the full map and crops afterwards (the kernel gathers into the cropped one), the
poolings walk window offsets over strided views (the kernels walk clipped windows per output).  tests/test_ref64_cpu.py pins each
of them to the torch-CPU float64 operator, so what the GPU tests compare with is checked by something that is neither the kernel nor
written from it.

The convolution and the deconvolution also return the same operation on |x|, |w|, |bias|: the operand of the a-priori error
bound of a fixed-order fp32 sum, |fl(sum) - sum| <= gamma(n) * sum|terms|, gamma(n) = n u / (1 - n u), u = 2^-24, n the longest chain
of roundings a term passes through (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1 / 4.2).
"""
import numpy as np

U32 = 2.0 ** -24


def gamma(n, u=U32):
    return n * u / (1.0 - n * u)


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def _conv3x3_pad1(x, w, bias):
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    xp = np.zeros((N, H + 2, W + 2, Cin), np.float64)
    xp[:, 1:H + 1, 1:W + 1] = x
    out = np.zeros((N, H, W, Cout), np.float64)
    for ky in range(3):
        for kx in range(3):
            # out[n, y, x, o] += sum_c in[n, y + ky - 1, x + kx - 1, c] * w[o, ky, kx, c]
            out += np.einsum('nhwc,oc->nhwo', xp[:, ky:ky + H, kx:kx + W], w[:, ky, kx])
    if bias is not None:
        out += bias
    return out


def head_conv3x3_ref(x_nhwc, w, bias=None, mul=1.0):
    """Convolution(kernel 3, pad 1) * mul.  x (N, H, W, Cin), w (Cout, 3, 3, Cin), bias (Cout) or None ->
    (ref, ref_abs), both (N, H, W, Cout) float64; ref_abs is the convolution of |x|, |w| plus |bias| (no mul)."""
    x, w, bias = _f64(x_nhwc), _f64(w), _f64(bias)
    ref = _conv3x3_pad1(x, w, bias) * float(mul)
    ref_abs = _conv3x3_pad1(np.abs(x), np.abs(w), None if bias is None else np.abs(bias))
    return ref, ref_abs


def _deconv4x4s2_crop1(x, w, bias, Hc, Wc):
    N, Hi, Wi, C = x.shape
    Co = w.shape[1]
    full = np.zeros((N, 2 * Hi + 2, 2 * Wi + 2, Co), np.float64)           # (Hi - 1) * 2 + 4
    for ky in range(4):
        for kx in range(4):
            # full[n, 2 * iy + ky, 2 * ix + kx, o] += sum_i in[n, iy, ix, i] * w[i, o, ky, kx]
            full[:, ky:ky + 2 * Hi:2, kx:kx + 2 * Wi:2] += np.einsum('nhwi,io->nhwo', x, w[:, :, ky, kx])
    if bias is not None:
        full += bias
    if not (0 < Hc <= 2 * Hi + 1 and 0 < Wc <= 2 * Wi + 1):
        raise ValueError("crop (%d, %d) at offset 1 does not fit the %d x %d deconvolution" % (Hc, Wc, 2 * Hi + 2, 2 * Wi + 2))
    return np.ascontiguousarray(full[:, 1:1 + Hc, 1:1 + Wc])


def upsample_flow_ref(x_nhwc, w, bias, Hc, Wc):
    """Deconvolution(kernel 4, stride 2, no pad) + Crop(offset (1, 1)) to Hc x Wc.  x (N, Hi, Wi, C), w (C, Co, 4, 4) (input channel first,
    the Deconvolution weight layout), bias (Co) or None -> (ref, ref_abs) (N, Hc, Wc, Co) float64."""
    x, w, bias = _f64(x_nhwc), _f64(w), _f64(bias)
    ref = _deconv4x4s2_crop1(x, w, bias, Hc, Wc)
    ref_abs = _deconv4x4s2_crop1(np.abs(x), np.abs(w), None if bias is None else np.abs(bias), Hc, Wc)
    return ref, ref_abs


def avgpool2_full_ref(x_nhwc):
    """Pooling(2x2, stride 2, avg, 'full'): ceil(H / 2) x ceil(W / 2) outputs, an edge window holds only the pixels inside the map
    and is divided by their number.  -> (avg, avg of |x|), float64."""
    x = _f64(x_nhwc)
    N, H, W, C = x.shape
    Ho, Wo = -(-H // 2), -(-W // 2)
    s, sa, cnt = np.zeros((N, Ho, Wo, C)), np.zeros((N, Ho, Wo, C)), np.zeros((1, Ho, Wo, 1))
    for dy in range(2):
        for dx in range(2):
            sub = x[:, dy::2, dx::2]
            h, w = sub.shape[1:3]
            s[:, :h, :w] += sub
            sa[:, :h, :w] += np.abs(sub)
            cnt[:, :h, :w] += 1
    return s / cnt, sa / cnt


def avgpool2_full_f32_in_order(x_nhwc):
    """The same pooling in float32, in the order flownet.hip states: the window's pixels added row by row (rows, then columns) onto 0,
    then ONE division by the window's own size.  Every step is a correctly rounded fp32 operation, so numpy's float32 gives the bits."""
    x = np.asarray(x_nhwc, np.float32)
    N, H, W, C = x.shape
    Ho, Wo = -(-H // 2), -(-W // 2)
    s, cnt = np.zeros((N, Ho, Wo, C), np.float32), np.zeros((1, Ho, Wo, 1), np.float32)
    for dy in range(2):
        for dx in range(2):
            sub = x[:, dy::2, dx::2]
            h, w = sub.shape[1:3]
            s[:, :h, :w] = s[:, :h, :w] + sub
            cnt[:, :h, :w] += np.float32(1)
    return s / cnt


def maxpool3x3s2_pad1_ref(x_nhwc):
    """Pooling(3x3, stride 2, pad 1, max): (H - 1) // 2 + 1 outputs per axis; the padding is "no value" (-inf), never a candidate.
    A maximum is exact in any format, so the result keeps the input's dtype (float32 in, float32 bits out)."""
    x = np.asarray(x_nhwc)
    N, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.full((N, 2 * Ho + 1, 2 * Wo + 1, C), -np.inf, x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    out = np.full((N, Ho, Wo, C), -np.inf, x.dtype)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, xp[:, dy:dy + 2 * Ho - 1:2, dx:dx + 2 * Wo - 1:2])
    return out


def nchw_slice_to_nhwc_ref(x_nchw, c0=0, c=None):
    """channels [c0, c0 + c) of (N, Ctot, H, W) as a contiguous (N, H, W, c) array, values untouched."""
    x = np.asarray(x_nchw)
    c = x.shape[1] - c0 if c is None else c
    out = np.empty((x.shape[0], x.shape[2], x.shape[3], c), x.dtype)
    for k in range(c):
        out[..., k] = x[:, c0 + k]
    return out
