"""tests/ref64.py pinned on the CPU: every float64 reference the direct kernel tests (tests/test_hip_ops_direct.py) compare with equals the
torch-CPU float64 operator of the same name, at the shapes those tests use, and composed the way oracle/graph_ref.get_flownet composes
its flow heads they reproduce that function's float64 flow.  Neither side of these comparisons is a kernel or written from one."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref64
from oracle import graph_ref

HEAD_SHAPES = [(5, 8, 1024), (10, 16, 1026), (19, 32, 770), (38, 63, 386), (38, 63, 194), (1, 1, 3), (2, 7, 255), (3, 3, 257), (4, 5, 1)]
UPFLOW_SHAPES = [((5, 8), (10, 16)), ((10, 16), (19, 32)), ((19, 32), (38, 63)), ((38, 63), (75, 125)), ((6, 10), (12, 20)),
                 ((1, 1), (1, 1)), ((1, 1), (3, 3)), ((2, 3), (5, 7)), ((3, 2), (5, 3))]
AVG_SHAPES = [(75, 125), (150, 250), (1, 1), (1, 7), (7, 1), (2, 2), (3, 5)]
MAX_SHAPES = [(300, 500), (37, 50), (1, 1), (2, 2), (9, 8), (71, 131)]
NHWC_SHAPES = [(1, 1024, 38, 63, 512, 512), (9, 1024, 38, 63, 0, 1024), (2, 70, 5, 13, 3, 65), (1, 1, 1, 1, 0, 1), (3, 130, 9, 7, 64, 66),
               (1, 64, 64, 1, 0, 64)]


def close(got, want, rel=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= rel * max(np.abs(want).max(), 1e-300), np.abs(got - want).max() / np.abs(want).max()


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).transpose(0, 3, 1, 2)))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def test_gamma_is_the_textbook_constant():
    assert ref64.U32 == 2.0 ** -24
    assert ref64.gamma(1) == 2.0 ** -24 / (1 - 2.0 ** -24)
    assert ref64.gamma(53) == 53 * 2.0 ** -24 / (1 - 53 * 2.0 ** -24)


@pytest.mark.parametrize("shape", HEAD_SHAPES)
@pytest.mark.parametrize("cout", [1, 2, 3, 4])
def test_head_conv3x3_ref_is_conv2d_pad1(shape, cout):
    H, W, Cin = shape
    N = 2 if H * W * Cin < 200000 else 1
    rs = np.random.RandomState(H * 100 + cout)
    x, w, b = rs.randn(N, H, W, Cin), rs.randn(cout, 3, 3, Cin), rs.randn(cout)
    wt = torch.from_numpy(np.ascontiguousarray(w.transpose(0, 3, 1, 2)))             # (Cout, Cin, 3, 3)
    for bias, mul in ((b, 2.5), (None, 1.0)):
        ref, ref_abs = ref64.head_conv3x3_ref(x, w, bias, mul)
        bt = None if bias is None else torch.from_numpy(bias)
        close(ref, nhwc(F.conv2d(nchw(x), wt, bt, 1, 1) * mul))
        close(ref_abs, nhwc(F.conv2d(nchw(x).abs(), wt.abs(), None if bt is None else bt.abs(), 1, 1)))
        assert (ref_abs * abs(mul) >= np.abs(ref) * (1 - 1e-12)).all()


@pytest.mark.parametrize("shape", UPFLOW_SHAPES)
@pytest.mark.parametrize("C", [2, 1, 8])
def test_upsample_flow_ref_is_conv_transpose2d_cropped_at_1(shape, C):
    (Hi, Wi), (Hc, Wc) = shape
    rs = np.random.RandomState(Hi * 10 + C)
    x, w, b = rs.randn(2, Hi, Wi, C), rs.randn(C, C, 4, 4), rs.randn(C)
    for bias in (b, None):
        ref, ref_abs = ref64.upsample_flow_ref(x, w, bias, Hc, Wc)
        bt = None if bias is None else torch.from_numpy(bias)
        full = F.conv_transpose2d(nchw(x), torch.from_numpy(w), bt, stride=2)
        assert full.shape[2:] == (2 * Hi + 2, 2 * Wi + 2)
        close(ref, nhwc(full[:, :, 1:1 + Hc, 1:1 + Wc]))
        full_abs = F.conv_transpose2d(nchw(x).abs(), torch.from_numpy(w).abs(), None if bt is None else bt.abs(), stride=2)
        close(ref_abs, nhwc(full_abs[:, :, 1:1 + Hc, 1:1 + Wc]))
    with pytest.raises(ValueError):
        ref64.upsample_flow_ref(x, w, None, 2 * Hi + 2, Wc)


@pytest.mark.parametrize("hw", AVG_SHAPES)
def test_avgpool2_full_ref_is_avg_pool2d_ceil_mode(hw):
    H, W = hw
    rs = np.random.RandomState(H + W)
    x = rs.randn(3, H, W, 8)
    avg, avg_abs = ref64.avgpool2_full_ref(x)
    want = F.avg_pool2d(nchw(x), 2, 2, ceil_mode=True, count_include_pad=False)
    close(avg, nhwc(want))
    close(avg_abs, nhwc(F.avg_pool2d(nchw(x).abs(), 2, 2, ceil_mode=True, count_include_pad=False)))
    # the float32 in-order form is a correctly rounded evaluation of the same thing: within gamma(4) * avg|x|
    x32 = x.astype(np.float32)
    avg32, abs32 = ref64.avgpool2_full_ref(x32)
    got = ref64.avgpool2_full_f32_in_order(x32)
    assert got.dtype == np.float32 and (np.abs(got - avg32) <= ref64.gamma(4) * abs32).all()


@pytest.mark.parametrize("hw", MAX_SHAPES)
def test_maxpool3x3s2_pad1_ref_is_max_pool2d(hw):
    H, W = hw
    rs = np.random.RandomState(H + W)
    for x in (rs.randn(2, H, W, 4), -1 - rs.rand(2, H, W, 4)):              # signed, and all negative: zero padding would win the second
        got = ref64.maxpool3x3s2_pad1_ref(x)
        want = nhwc(F.max_pool2d(nchw(x), 3, 2, 1))
        np.testing.assert_array_equal(got, want)
        x32 = x.astype(np.float32)
        got32 = ref64.maxpool3x3s2_pad1_ref(x32)
        assert got32.dtype == np.float32
        np.testing.assert_array_equal(got32, nhwc(F.max_pool2d(torch.from_numpy(x32).permute(0, 3, 1, 2), 3, 2, 1)))


@pytest.mark.parametrize("shape", NHWC_SHAPES)
def test_nchw_slice_to_nhwc_ref_is_permute(shape):
    N, Ctot, H, W, c0, C = shape
    if N * Ctot * H * W > 4000000:
        N = 2                                                                # the copy is per image; two keep the CPU test short
    x = np.random.RandomState(Ctot).randn(N, Ctot, H, W).astype(np.float32)
    x[0, c0, 0, 0] = -0.0
    got = ref64.nchw_slice_to_nhwc_ref(x, c0, C)
    want = torch.from_numpy(x)[:, c0:c0 + C].permute(0, 2, 3, 1).contiguous().numpy()
    assert got.dtype == np.float32 and got.flags['C_CONTIGUOUS']
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))


# --------------------------------------------------------------------------------------------------------------------------
FLOWNET_SHAPES = {
    'flow_conv1': (64, 6, 7, 7), 'conv2': (128, 64, 5, 5), 'conv3': (256, 128, 5, 5), 'conv3_1': (256, 256, 3, 3), 'conv4': (512, 256, 3, 3),
    'conv4_1': (512, 512, 3, 3), 'conv5': (512, 512, 3, 3), 'conv5_1': (512, 512, 3, 3), 'conv6': (1024, 512, 3, 3), 'conv6_1': (1024, 1024, 3, 3),
    'Convolution1': (2, 1024, 3, 3), 'Convolution2': (2, 1026, 3, 3), 'Convolution3': (2, 770, 3, 3), 'Convolution4': (2, 386, 3, 3),
    'Convolution5': (2, 194, 3, 3), 'Convolution5_scale': (1024, 194, 1, 1),
    'deconv5': (1024, 512, 4, 4), 'deconv4': (1026, 256, 4, 4), 'deconv3': (770, 128, 4, 4), 'deconv2': (386, 64, 4, 4),
    'upsample_flow6to5': (2, 2, 4, 4), 'upsample_flow5to4': (2, 2, 4, 4), 'upsample_flow4to3': (2, 2, 4, 4), 'upsample_flow3to2': (2, 2, 4, 4),
}


def flownet_params(seed):
    rs = np.random.RandomState(seed)
    arg = {}
    for name, shp in FLOWNET_SHAPES.items():
        fan_in = (shp[1] if 'deconv' not in name and 'upsample' not in name else shp[0]) * shp[2] * shp[3]
        arg[name + '_weight'] = (rs.randn(*shp) * (1.5 / np.sqrt(fan_in))).astype(np.float32)
        co = shp[0] if 'deconv' not in name and 'upsample' not in name else shp[1]
        arg[name + '_bias'] = (0.1 * rs.randn(co)).astype(np.float32)
    return arg


def test_refs_composed_like_get_flownet_reproduce_its_float64_flow():
    """oracle/graph_ref.get_flownet(dtype float64) on a 96 x 160 pair, against the same network whose five flow heads, four flow
    upsamplings and last pooling are tests/ref64.py (every other layer stays torch float64): flow equal to 1e-10."""
    arg = flownet_params(3)
    p = graph_ref.Params(arg, {}, dtype=torch.float64)
    rs = np.random.RandomState(4)
    cur = rs.uniform(0, 255, (1, 3, 96, 160)).astype(np.float32)
    prev = np.clip(np.roll(cur, 2, 3) + rs.randn(1, 3, 96, 160) * 4, 0, 255).astype(np.float32)
    want_flow, _ = graph_ref.get_flownet(p, cur, prev)
    assert want_flow.dtype == torch.float64 and want_flow.shape == (1, 2, 6, 10)

    def conv(x, name, stride=1, pad=1):
        return F.leaky_relu(F.conv2d(x, p.w(name + '_weight'), p.w(name + '_bias'), stride, pad), 0.1)

    def deconv_crop(x, name, like):
        y = F.conv_transpose2d(x, p.w(name + '_weight'), p.w(name + '_bias'), stride=2)
        return F.leaky_relu(y[:, :, 1:1 + like.shape[2], 1:1 + like.shape[3]], 0.1)

    def head(x, name, mul=1.0):
        w = arg[name + '_weight'].transpose(0, 2, 3, 1)                     # (Cout, 3, 3, Cin): the layout lsfa_head_conv3x3 reads
        return nchw(ref64.head_conv3x3_ref(nhwc(x), w, arg[name + '_bias'], mul)[0])

    def upflow(f, name, like):
        return nchw(ref64.upsample_flow_ref(nhwc(f), arg[name + '_weight'], arg[name + '_bias'], like.shape[2], like.shape[3])[0])

    data = torch.cat([p.T(cur) / 255.0, p.T(prev) / 255.0], 1)
    x = nchw(ref64.avgpool2_full_ref(nhwc(data))[0])
    r1 = conv(x, 'flow_conv1', 2, 3)
    r2 = conv(r1, 'conv2', 2, 2)
    r3 = conv(r2, 'conv3', 2, 2)
    r4 = conv(r3, 'conv3_1')
    r5 = conv(r4, 'conv4', 2)
    r6 = conv(r5, 'conv4_1')
    r7 = conv(r6, 'conv5', 2)
    r8 = conv(r7, 'conv5_1')
    r9 = conv(r8, 'conv6', 2)
    r10 = conv(r9, 'conv6_1')
    f6 = head(r10, 'Convolution1')
    c2 = torch.cat([r8, deconv_crop(r10, 'deconv5', r8), upflow(f6, 'upsample_flow6to5', r8)], 1)
    f5 = head(c2, 'Convolution2')
    c3 = torch.cat([r6, deconv_crop(c2, 'deconv4', r6), upflow(f5, 'upsample_flow5to4', r6)], 1)
    f4 = head(c3, 'Convolution3')
    c4 = torch.cat([r4, deconv_crop(c3, 'deconv3', r4), upflow(f4, 'upsample_flow4to3', r4)], 1)
    f3 = head(c4, 'Convolution4')
    c5 = torch.cat([r2, deconv_crop(c4, 'deconv2', r2), upflow(f3, 'upsample_flow3to2', r2)], 1)
    c5 = nchw(ref64.avgpool2_full_ref(nhwc(c5))[0])
    flow = head(c5, 'Convolution5', 2.5)
    assert [t.shape[1] for t in (c2, c3, c4, c5)] == [1026, 770, 386, 194]
    assert float(want_flow.abs().max()) > 1e-3                                # a flow that is all bias would compare nothing
    err = float((flow - want_flow).abs().max() / want_flow.abs().max())
    assert err <= 1e-10, err
