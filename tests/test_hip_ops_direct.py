"""FlowNet's small kernels, the layout copies and the batched / padded R-FCN head, each called on its own through the C ABI.

The whole-network tests reach these kernels only through one number at the end of FlowNet; here each is compared, per output element,
with a float64 statement of its operator (tests/ref64.py, pinned to torch on the CPU by tests/test_ref64_cpu.py) at FlowNet's own
shapes (1000 x 600 and the 720p demo size) and at small awkward ones.

Float sums (head_conv3x3, upsample_flow, avgpool2_nhwc) are held to the a-priori bound of a fixed-order fp32 sum,
    |got - ref64| <= gamma(n_ops) * ref_abs64,     gamma(n) = n u / (1 - n u),  u = 2^-24,
ref_abs64 the same operation on |x|, |w|, |bias| and n_ops the longest chain of roundings a term passes through in the order the
kernel's header comment states.  The bound is derived, not measured, and takes no margin; the largest observed err / bound is
written with parity_util.record('direct_<kernel>', ...).  Copies, maxima, the pooling's stated order and the R-FCN head are compared
bit for bit.
Every refusal tested here is a host-side check that returns before any launch.
"""
import numpy as np
import pytest
import torch

import oracle
import parity_util
import ref64
from test_hip_ops import rand_rois

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = np.float32(-7.0625e9)                       # what untouched output holds; compared as bits
SENT_BITS = int(np.array([SENT]).view(np.int32)[0])

_worst = {}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a).view(np.int32)


def sentinel_map(shape):
    return torch.full(shape, float(SENT), dtype=torch.float32, device=DEV)


def holds_sentinel(x):
    """every element of the (possibly strided) float32 view still has the sentinel's bits (checked on the device: the maps are large)"""
    return x.numel() == 0 or bool((x.contiguous().view(torch.int32) == SENT_BITS).all().item())


def slot_max(slots):
    return slots.view(torch.float32).max().item()


def check_bound(kernel, case, got, ref, ref_abs, n_ops, mul=1.0):
    """per element |got - ref| <= gamma(n_ops) * ref_abs * |mul|; keeps the largest err / bound of the kernel for the record"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (case, got.shape, ref.shape)
    assert np.isfinite(got).all(), case
    err, bound = np.abs(got - ref), ref64.gamma(n_ops) * ref_abs * abs(mul)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max())
    rec = _worst.setdefault(kernel, {'max_err_over_bound': 0.0, 'case': None, 'cases': 0})
    rec['cases'] += 1
    if worst >= rec['max_err_over_bound']:
        rec['max_err_over_bound'], rec['case'] = worst, repr(case)
    parity_util.record('direct_' + kernel, rec)
    assert worst <= 1.0, "%s %r: err / bound = %.3f at %s (err %.3e, bound %.3e)" % (
        kernel, case, worst, np.unravel_index(ratio.argmax(), ratio.shape), err.flat[ratio.argmax()], bound.flat[ratio.argmax()])


# ------------------------------------------------------------------ head_conv3x3 --------
HEAD_SHAPES = [(5, 8, 1024, 1.0), (10, 16, 1026, 1.0), (19, 32, 770, 1.0), (38, 63, 386, 1.0), (38, 63, 194, 2.5),
               (1, 1, 3, 1.0), (2, 7, 255, -0.75), (3, 3, 257, 1.0), (4, 5, 1, 3.0)]


def head_n_ops(cin):
    # per-thread fmaf chain (9 taps per channel, channels t, t + 256, ...), six shuffle steps, three wave adds, bias, mul
    return 9 * -(-cin // 256) + 6 + 3 + 2


def run_head_forms(hip, case, x, xbuf, w4, b4, mul):
    """x (N, H, W, Cin) numpy; xbuf the same values inside an (N, H, W, L > Cin) device map whose other channels hold 1e30.
    Every Cout, bias None / given, lda == Cin / > Cin, and the three output forms."""
    N, H, W, Cin = x.shape
    xd = t(x)
    refs = {None: ref64.head_conv3x3_ref(x, w4, None, mul), 'b': ref64.head_conv3x3_ref(x, w4, b4, mul)}
    for cout in (1, 2, 3, 4):
        wd = t(w4[:cout])
        for bkey in (None, 'b'):
            bd = None if bkey is None else t(b4[:cout])
            ref, ref_abs = refs[bkey][0][..., :cout], refs[bkey][1][..., :cout]
            for xin, lda in ((xd, 'lda=Cin'), (xbuf, 'lda>Cin')):
                tag = case + (cout, bkey, lda)
                got = hip.head_conv3x3(xin, wd, bd, cin=Cin, mul=mul)                        # a fresh (N, H, W, Cout) map
                assert got.shape == (N, H, W, cout)
                check_bound('head_conv3x3', tag + ('nhwc',), got.cpu().numpy(), ref, ref_abs, head_n_ops(Cin), mul)
                g2 = hip.head_conv3x3(xin, wd, bd, cin=Cin, mul=mul, nchw=True)
                assert g2.shape == (N, cout, H, W)
                # the output form changes where a value goes, not the value
                np.testing.assert_array_equal(bits(g2.permute(0, 2, 3, 1).contiguous()), bits(got), err_msg=repr(tag + ('nchw',)))
                for c0 in (0, 3, 5):
                    wide = sentinel_map((N, H, W, cout + 5))
                    hip.head_conv3x3(xin, wd, bd, cin=Cin, mul=mul, out=wide, c0=c0)
                    np.testing.assert_array_equal(bits(wide[..., c0:c0 + cout].contiguous()), bits(got), err_msg=repr(tag + ('c0', c0)))
                    assert holds_sentinel(wide[..., :c0]) and holds_sentinel(wide[..., c0 + cout:]), tag + ('c0', c0)


@pytest.mark.parametrize("N", [1, 2, 9])
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_head_conv3x3_vs_float64(hip, shape, N):
    H, W, Cin, mul = shape
    rs = np.random.RandomState(H * 1000 + Cin + N)
    x = f32(rs.randn(N, H, W, Cin))
    w4, b4 = f32(rs.randn(4, 3, 3, Cin) / np.sqrt(9 * Cin)), f32(rs.randn(4))
    xbuf = torch.full((N, H, W, Cin + 3), 1e30, dtype=torch.float32, device=DEV)           # a channel read past Cin shows as 1e30
    xbuf[..., :Cin] = t(x)
    run_head_forms(hip, (H, W, Cin, N, 'randn'), x, xbuf, w4, b4, mul)


@pytest.mark.parametrize("shape", [(5, 8, 1024, 1.0), (38, 63, 194, 2.5), (3, 3, 257, 1.0), (4, 5, 1, 3.0), (1, 1, 3, 1.0)])
@pytest.mark.parametrize("where", ["ring", "interior"])
def test_head_conv3x3_border_taps(hip, shape, where):
    """Only the border ring of x is non-zero / only the interior is: a tap taken from the clamped address instead of the padding's
    zero, or dropped, is then the whole output of a pixel and not a small term of it."""
    H, W, Cin, mul = shape
    N = 2
    rs = np.random.RandomState(H + Cin)
    x = f32(1.0 + rs.rand(N, H, W, Cin))                                                  # one sign: nothing cancels
    ring = np.ones((H, W), bool)
    ring[1:H - 1, 1:W - 1] = False
    x[:, ~ring if where == "ring" else ring] = 0
    w4, b4 = f32((1.0 + rs.rand(4, 3, 3, Cin)) / (9 * Cin)), f32(rs.randn(4))
    xbuf = torch.full((N, H, W, Cin + 1), 1e30, dtype=torch.float32, device=DEV)
    xbuf[..., :Cin] = t(x)
    run_head_forms(hip, (H, W, Cin, N, where), x, xbuf, w4, b4, mul)


def test_head_conv3x3_refusals(hip):
    x, w = torch.zeros(1, 3, 3, 8, device=DEV), torch.zeros(5, 3, 3, 8, device=DEV)
    with pytest.raises(hip.LsfaError):                                      # Cout 5
        hip.head_conv3x3(x, w, None)
    with pytest.raises(hip.LsfaError):                                      # more input channels than the map has
        hip.head_conv3x3(x, torch.zeros(2, 3, 3, 9, device=DEV), None)
    with pytest.raises(hip.LsfaError):                                      # channels [3, 5) of a 4-channel map
        hip.head_conv3x3(x, w[:2], None, out=torch.zeros(1, 3, 3, 4, device=DEV), c0=3)


# ------------------------------------------------------------------ upsample_flow -------
UPFLOW_SHAPES = [((5, 8), (10, 16)), ((10, 16), (19, 32)), ((19, 32), (38, 63)), ((38, 63), (75, 125)), ((6, 10), (12, 20)),
                 ((1, 1), (1, 1)), ((1, 1), (3, 3)), ((2, 3), (5, 7)), ((3, 2), (5, 3))]


def run_upflow(hip, case, x, w, b, Hc, Wc, L, c0, out=None):
    """one launch into channels [c0, c0 + C) of an L-channel sentinel map -> the slice (numpy), after the checks every case gets"""
    N, Hi, Wi, C = x.shape
    out = sentinel_map((N, Hc, Wc, L)) if out is None else out.fill_(float(SENT))
    slots = hip.amax_slots(1, DEV)[0]
    ret = hip.upsample_flow(t(x), t(w), None if b is None else t(b), out, c0, amax_out=slots)
    assert ret is out
    assert holds_sentinel(out[..., :c0]) and holds_sentinel(out[..., c0 + C:]), case
    got = out[..., c0:c0 + C].contiguous().cpu().numpy()
    ref, ref_abs = ref64.upsample_flow_ref(x, w, b, Hc, Wc)
    check_bound('upsample_flow', case, got, ref, ref_abs, 4 * C + 1)      # at most four taps per input channel reach one output, then the bias
    assert slot_max(slots) == float(np.abs(got).max()), case               # exactly max|out[..., c0:c0+C]| of the GPU's own output
    return got


@pytest.mark.parametrize("N", [1, 2, 12])
@pytest.mark.parametrize("C", [2, 1, 8])
@pytest.mark.parametrize("shape", UPFLOW_SHAPES)
def test_upsample_flow_vs_float64(hip, shape, C, N):
    (Hi, Wi), (Hc, Wc) = shape
    rs = np.random.RandomState(Hi * 100 + C * 10 + N)
    x, w, b = f32(rs.randn(N, Hi, Wi, C)), f32(rs.randn(C, C, 4, 4)), f32(rs.randn(C))
    L = 1024 + C + 2
    out = sentinel_map((N, Hc, Wc, L))
    for c0 in (0, 1024, L - C):
        for bias in (None, b):
            run_upflow(hip, (Hi, Wi, Hc, Wc, C, N, c0, bias is not None), x, w, bias, Hc, Wc, L, c0, out=out)


def test_upsample_flow_every_crop_up_to_the_limit(hip):
    """Hc = 2 * Hi - 1, 2 * Hi, 2 * Hi + 1 (and the same for Wc): the last rows / columns see one tap where the interior sees two."""
    rs = np.random.RandomState(9)
    for Hi, Wi in ((3, 4), (1, 1), (5, 2)):
        x, w, b = f32(rs.randn(2, Hi, Wi, 2)), f32(rs.randn(2, 2, 4, 4)), f32(rs.randn(2))
        for Hc in (2 * Hi - 1, 2 * Hi, 2 * Hi + 1):
            for Wc in (2 * Wi - 1, 2 * Wi, 2 * Wi + 1):
                run_upflow(hip, (Hi, Wi, Hc, Wc, 'crop'), x, w, b, Hc, Wc, 4, 1)


def test_upsample_flow_amax_of_a_negative_maximum_and_a_partial_wave(hip):
    rs = np.random.RandomState(10)
    # every output negative (x < 0, w > 0, no bias); 2 * 5 * 7 * 1 = 70 elements: one full wave and 6 lanes of the next
    x, w = f32(-1 - rs.rand(2, 2, 3, 1)), f32(1 + rs.rand(1, 1, 4, 4))
    got = run_upflow(hip, 'negative', x, w, None, 5, 7, 3, 2)
    assert got.size % 64 != 0 and (got < 0).all()
    # the largest magnitude is negative among positive values, and sits in the last, partial wave (the last element)
    x = f32(rs.rand(1, 3, 3, 1))
    x[0, 2, 2, 0] = -50.0
    w[0, 0, 3, 3] = 3.0                                                     # out[6, 6] = x[2, 2] * w[3, 3] alone
    got = run_upflow(hip, 'negative-last', x, w, None, 7, 7, 1, 0)
    assert got.size == 49 and np.abs(got).argmax() == 48 and got.flat[48] == -150.0
    # a slot row that other producers of the same map wrote before keeps their larger maximum (atomic max, not a store)
    slots = hip.amax_slots(1, DEV)[0]
    slots.view(torch.float32).fill_(1e6)
    hip.upsample_flow(t(x), t(w), None, sentinel_map((1, 7, 7, 1)), 0, amax_out=slots)
    assert slot_max(slots) == 1e6


def test_upsample_flow_refusals(hip):
    x, w = torch.zeros(1, 2, 3, 2, device=DEV), torch.zeros(2, 2, 4, 4, device=DEV)
    with pytest.raises(hip.LsfaError):                                      # a crop larger than the deconvolution leaves at offset 1
        hip.upsample_flow(x, w, None, torch.zeros(1, 6, 7, 2, device=DEV), 0)
    with pytest.raises(hip.LsfaError):                                      # channels [1, 3) of a 2-channel map
        hip.upsample_flow(x, w, None, torch.zeros(1, 5, 7, 2, device=DEV), 1)
    with pytest.raises(hip.LsfaError):                                      # out is a channel slice, not a contiguous map
        hip.upsample_flow(x, w, None, torch.zeros(1, 5, 7, 4, device=DEV)[..., :2], 0)
    with pytest.raises(hip.LsfaError):
        hip.upsample_flow(x, w, None, torch.zeros(1, 5, 7, 2, device=DEV, dtype=torch.float64), 0)
    with pytest.raises(hip.LsfaError):                                      # another batch size
        hip.upsample_flow(x, w, None, torch.zeros(2, 5, 7, 2, device=DEV), 0)
    with pytest.raises(hip.LsfaError):
        hip.upsample_flow(x, w, None, torch.zeros(1, 5, 7, 2), 0)


# ------------------------------------------------------------------ avgpool2_nhwc -------
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("C", [4, 64, 196])
@pytest.mark.parametrize("hw", [(75, 125), (150, 250), (1, 1), (1, 7), (7, 1), (2, 2), (3, 5)])
def test_avgpool2_nhwc_full_convention(hip, hw, C, N):
    H, W = hw
    rs = np.random.RandomState(H + W + C + N)
    x = f32(rs.randn(N, H, W, C) + 3.0)              # a non-zero mean: a window divided by 4 instead of its own size is far off
    got = hip.avgpool2_nhwc(t(x)).cpu().numpy()
    assert got.shape == (N, (H + 1) // 2, (W + 1) // 2, C)
    np.testing.assert_array_equal(bits(got), bits(ref64.avgpool2_full_f32_in_order(x)))
    ref, ref_abs = ref64.avgpool2_full_ref(x)
    check_bound('avgpool2_nhwc', (H, W, C, N), got, ref, ref_abs, 4)      # three additions at most (the first onto 0 is exact), one division


def test_avgpool2_nhwc_refusals(hip):
    with pytest.raises(hip.LsfaError):                                      # C % 4
        hip.avgpool2_nhwc(torch.zeros(1, 4, 4, 6, device=DEV))
    buf = torch.zeros(1 * 4 * 4 * 8 + 4, device=DEV)
    x = buf[1:1 + 128].view(1, 4, 4, 8)                                     # contiguous, 4 bytes past a 16-byte boundary
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    with pytest.raises(hip.LsfaError):
        hip.avgpool2_nhwc(x)


# ------------------------------------------------------------------ nchw_to_nhwc --------
@pytest.mark.parametrize("shape", [(1, 1024, 38, 63, 512, 512), (9, 1024, 38, 63, 0, 1024), (2, 70, 5, 13, 3, 65), (1, 1, 1, 1, 0, 1),
                                   (3, 130, 9, 7, 64, 66), (1, 64, 64, 1, 0, 64)])
def test_nchw_to_nhwc_bitwise_slices_and_amax(hip, shape):
    N, Ctot, H, W, c0, C = shape
    rs = np.random.RandomState(Ctot + H)
    x = f32(rs.randn(N, Ctot, H, W))
    x[0, c0, 0, 0] = -0.0
    x[:, :c0] += 1e6                                                        # channels outside the slice are larger: they are not part of amax
    x[:, c0 + C:] -= 1e6
    # the slice's largest magnitude: negative, in the last image's last pixel (a partial 64 x 64 tile unless HW and C are multiples
    # of 64), in a channel that is not the first of its group of four
    k = C - 1 if (C - 1) % 4 else max(C - 2, 0)
    x[N - 1, c0 + k, H - 1, W - 1] = -9.5
    want = ref64.nchw_slice_to_nhwc_ref(x, c0, C)
    xd = t(x)
    slots = hip.amax_slots(1, DEV)[0]
    got = hip.nchw_to_nhwc(xd, c0, C, amax_out=slots)
    assert got.shape == (N, H, W, C) and got.is_contiguous()
    np.testing.assert_array_equal(bits(got), bits(want))
    assert slot_max(slots) == 9.5 == float(np.abs(want).max())
    # into the leading N images of a buffer of N + 3 (the nine-frame pass fills 9 of the key pass's 12)
    buf = sentinel_map((N + 3, H, W, C))
    slots2 = hip.amax_slots(1, DEV)[0]
    ret = hip.nchw_to_nhwc(xd, c0, C, out=buf[:N], amax_out=slots2)
    assert ret.data_ptr() == buf.data_ptr()
    np.testing.assert_array_equal(bits(buf[:N]), bits(want))
    assert holds_sentinel(buf[N:])
    assert slot_max(slots2) == 9.5
    if c0 == 0 and C == Ctot:
        np.testing.assert_array_equal(bits(hip.nchw_to_nhwc(xd)), bits(want))      # the defaults: every channel
    if N * H * W > 1:
        with pytest.raises(hip.LsfaError):                                  # a channel slice is not a contiguous map
            hip.nchw_to_nhwc(xd, c0, C, out=sentinel_map((N, H, W, C + 1))[..., :C])
    if C > 1:
        with pytest.raises(hip.LsfaError):                                  # channels past the map
            hip.nchw_to_nhwc(xd, Ctot - C + 1, C)


# ------------------------------------------------------------------ maxpool3x3s2_nhwc ---
def maxpool_input(rs, kind, N, H, W, C):
    if kind == "randn":
        return f32(rs.randn(N, H, W, C))
    x = f32(-0.5 - rs.rand(N, H, W, C))                                     # all negative: a padding of 0 would win every edge window
    if kind == "corners":
        for yy, xx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            x[:, yy, xx] = 2.0 + rs.rand(N, C)
    return x


@pytest.mark.parametrize("C", [4, 64])
@pytest.mark.parametrize("kind", ["randn", "negative", "corners"])
@pytest.mark.parametrize("hw", [(300, 500), (37, 50), (1, 1), (2, 2), (9, 8), (71, 131)])
def test_maxpool3x3s2_nhwc_signed_inputs_and_amax(hip, hw, kind, C):
    H, W = hw
    N = 1 if H * W > 10000 else 2
    rs = np.random.RandomState(H + W + C)
    x = maxpool_input(rs, kind, N, H, W, C)
    want = ref64.maxpool3x3s2_pad1_ref(x)
    assert want.dtype == np.float32 and np.isfinite(want).all()
    xd = t(x)
    slots = hip.amax_slots(1, DEV)[0]
    got = hip.maxpool3x3s2_nhwc(xd, amax_out=slots)
    assert got.shape == (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C)
    np.testing.assert_array_equal(bits(got), bits(want))
    assert slot_max(slots) == float(np.abs(want).max())                      # one output: max|y| (of negative values too)
    np.testing.assert_array_equal(bits(hip.maxpool3x3s2_nhwc(xd)), bits(want))
    # with the first unit's bn1 + relu1 as a second output: relu(p * s + t) in float32, the product rounded before the sum
    s2, t2 = f32(rs.uniform(0.5, 1.5, C) * rs.choice([-1, 1], C)), f32(rs.randn(C))
    want2 = np.maximum(want * s2 + t2, np.float32(0))
    assert want2.dtype == np.float32
    slots2 = hip.amax_slots(1, DEV)[0]
    p1, p2 = hip.maxpool3x3s2_nhwc(xd, scale2=t(s2), shift2=t(t2), amax_out=slots2)
    np.testing.assert_array_equal(bits(p1), bits(want))
    np.testing.assert_array_equal(p2.cpu().numpy(), want2)
    assert slot_max(slots2) == float(want2.max())                            # two outputs: the maximum of the second
    if kind != "randn":
        assert float(want2.max()) != float(np.abs(want).max())


def test_maxpool3x3s2_nhwc_refusals(hip):
    with pytest.raises(hip.LsfaError):                                      # C % 4
        hip.maxpool3x3s2_nhwc(torch.zeros(1, 4, 4, 6, device=DEV))


# ------------------------------------------------------------------ R-FCN head, batched and padded ----
NCLS, NBOX, GG = 31, 8, 49


@pytest.mark.parametrize("N", [2, 9])
@pytest.mark.parametrize("hw", [(38, 63), (5, 9)])
def test_rfcn_head_batched_and_padded_bit_exact(hip, hw, N):
    """The three forms of the head (NCHW maps, position-sensitive cells, cells `cell_ld` floats apart with NaN in the padding) on N
    images with ROIs of every image but one, against the oracle's PSROI pooling (which takes the image from the ROI's first column)."""
    H, W = hw
    D = NCLS + NBOX
    rs = np.random.RandomState(N * 100 + H)
    cls_map = rs.standard_normal((N, NCLS * GG, H, W)).astype(np.float32)
    box_map = (0.1 * rs.standard_normal((N, NBOX * GG, H, W))).astype(np.float32)
    nchw = np.concatenate([cls_map.reshape(N, NCLS, GG, H * W), box_map.reshape(N, NBOX, GG, H * W)], 1)       # (N, D, 49, HW)
    ps = np.ascontiguousarray(nchw.transpose(0, 3, 2, 1)).reshape(N, H, W, GG, D)
    del nchw
    cls_d, box_d, ps_d = t(cls_map), t(box_map), t(ps)
    empty = 0 if N == 2 else 4                                             # the image that gets no ROI
    others = np.array([n for n in range(N) if n != empty])
    for R in (300, 1, 0):
        rois = rand_rois(rs, R, im_w=W * 16, im_h=H * 16)
        rois[:, 0] = others[rs.randint(0, len(others), R)] if R != 1 else N - 1
        if R == 300:                                                       # the integer / half-integer / multiple-of-16 edges land in several images
            rois[:len(others), 0] = others
            assert set(rois[:, 0].astype(int)) == set(others.tolist())
        want_prob, want_score, want_box = oracle.rfcn_head(cls_map, box_map, rois)
        assert want_prob.shape == (R, NCLS) and np.isfinite(want_prob).all() and np.isfinite(want_box).all()
        rd = t(rois)
        prob, score, box = hip.rfcn_head(cls_d, box_d, rd, want_score=True)
        np.testing.assert_array_equal(bits(score), bits(want_score))
        np.testing.assert_array_equal(bits(box), bits(want_box))
        np.testing.assert_array_equal(bits(prob), bits(want_prob))
        prob, score, box = hip.rfcn_head_ps(ps_d, rd, NCLS, NBOX, want_score=True)
        np.testing.assert_array_equal(bits(score), bits(want_score))
        np.testing.assert_array_equal(bits(box), bits(want_box))
        np.testing.assert_array_equal(bits(prob), bits(want_prob))
        for pad in (0, 1, 9, 137):
            ld = GG * D + pad
            padded = torch.full((N, H, W, ld), float('nan'), dtype=torch.float32, device=DEV)
            padded[..., :GG * D] = ps_d.view(N, H, W, GG * D)
            prob, box = hip.rfcn_head_ps_ld(padded, ld, rd, H, W, NCLS, NBOX)
            assert prob.shape == (R, NCLS) and box.shape == (R, NBOX)
            np.testing.assert_array_equal(bits(box), bits(want_box), err_msg="pad %d R %d" % (pad, R))
            np.testing.assert_array_equal(bits(prob), bits(want_prob), err_msg="pad %d R %d" % (pad, R))
            del padded
    if N == 2:
        # the same ROIs pointed at the other image give that image's pooling: the batch index is read, not assumed
        rois = rand_rois(rs, 40, im_w=W * 16, im_h=H * 16)
        rois[:, 0] = 1
        a = hip.rfcn_head_ps(ps_d, t(rois), NCLS, NBOX)[1].cpu().numpy()
        np.testing.assert_array_equal(a, oracle.rfcn_head(cls_map[1:], box_map[1:], np.concatenate([rois[:, :1] * 0, rois[:, 1:]], 1))[2])


def test_rfcn_head_ps_ld_refusals(hip):
    D = NCLS + NBOX
    rois = torch.zeros(2, 5, device=DEV)
    small = torch.zeros(1, 5, 9, GG * D - 1, device=DEV)
    with pytest.raises(hip.LsfaError):                                      # cells closer together than their 49 * 39 values
        hip.rfcn_head_ps_ld(small, GG * D - 1, rois, 5, 9, NCLS, NBOX)
    ok = torch.zeros(1, 5, 9, GG * D + 9, device=DEV)
    with pytest.raises(hip.LsfaError):                                      # cell_ld is not the map's last dimension
        hip.rfcn_head_ps_ld(ok, GG * D, rois, 5, 9, NCLS, NBOX)
    with pytest.raises(hip.LsfaError):                                      # nor is the map H x W
        hip.rfcn_head_ps_ld(ok, GG * D + 9, rois, 5, 10, NCLS, NBOX)
    prob, box = hip.rfcn_head_ps_ld(ok, GG * D + 9, rois, 5, 9, NCLS, NBOX)
    assert prob.shape == (2, NCLS) and box.shape == (2, NBOX)


# ------------------------------------------------------------------ the unpadded im2col entry point ----
def test_deform_im2col_cl_entry_without_offset_ld(hip):
    """lsfa_deform_im2col_cl (offsets exactly 2 * kh * kw * groups channels apart): hip.deform_im2col_cl goes through the _ld entry, so
    this one is called through ctypes - against the oracle's NCHW statement, col_cl[n, pixel, tap, c] == col[n, c * KK + tap, pixel]."""
    import ctypes
    rs = np.random.RandomState(12)
    N, C, H, W, k, dg = 2, 24, 9, 7, 3, 2
    data = f32(rs.randn(N, C, H, W))
    offset = f32(2.0 * rs.randn(N, 2 * k * k * dg, H, W))
    offset[:, :, 0, :] *= 8.0                                              # some taps leave the image
    want = oracle.deform_im2col(data, offset, k, k, 1, 1, 1, dg)
    want_cl = want.reshape(N, C, k * k, H * W).transpose(0, 3, 2, 1).reshape(N, H * W, k * k * C)
    d, o = t(data.transpose(0, 2, 3, 1)), t(offset.transpose(0, 2, 3, 1))
    col = sentinel_map((N, H * W, k * k * C))
    ci, vp = ctypes.c_int, ctypes.c_void_p
    rc = hip.lib().lsfa_deform_im2col_cl(vp(d.data_ptr()), vp(o.data_ptr()), ci(N), ci(C), ci(H), ci(W), ci(k), ci(k), ci(1), ci(1), ci(1),
                                         ci(dg), ci(H), ci(W), vp(col.data_ptr()), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    np.testing.assert_array_equal(col.cpu().numpy(), want_cl)
    np.testing.assert_array_equal(bits(hip.deform_im2col_cl(d, o, k, k, 1, 1, 1, dg)), bits(col))

