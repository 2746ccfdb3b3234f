"""The one-piece (bf16) form of lsfa_conv_fwd - every convolution of dtype=torch.bfloat16 - against its specification.

The specification (tests/ref_bf16.py, pinned on the CPU by tests/test_ref_bf16_cpu.py): both operands rounded to one bf16 value to
nearest even, exact products, fp32 accumulation.  The reference is a float64 convolution of the ROUNDED operands, so the operand
rounding is not inside the tolerance: every comparison asserts the derived per-element bound gamma(K + 3, 2^-23) * ref_abs AND the
project's fp32 criterion 2e-6 * sqrt(K) * max(max|ref|, 1) (ref_bf16.bound_ratios).  A kernel that cut by truncation, or that got one
tap of one pixel wrong, leaves both by factors of 6 to 100 (test_ref_bf16_cpu.py shows the former).  The worst err / bound per case is
written with parity_util.record('conv_bf16', ...).  Outputs a launch must not write hold a sentinel and are checked bit for bit.

CASES is the one table of shapes and forced plans; tests/test_ref_bf16_cpu.py asks lsfa_conv_plan_query which kernel instantiation every
entry runs and holds the set to the list of one-piece instantiations that have to be covered.  Inputs are made by inputs_of on the CPU
from a fixed seed, so that the CPU test can hold the reference itself to the bounds at the same shapes.
"""
import numpy as np
import pytest
import torch

import parity_util
import ref_bf16

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = np.float32(-7.0625e9)                       # what untouched output holds; compared as bits
SENT_BITS = int(np.array([SENT]).view(np.int32)[0])

# (kernel, nt, st, slices) of lsfa_conv_plan_override; zeros = the plan's own choice.  kernel 1: mixed-role waves, 2: loader / consumer
# waves, 4: 256-pixel tiles of eight mixed-role waves
OWN = (0, 0, 0, 0)
RING_PLANS = [OWN] + [(k, nt, st, sl) for k in (1, 2) for nt in (2, 4) for st in (2, 3, 4) for sl in (1, 2, 5, 7)] + \
             [(4, 4, st, sl) for st in (2, 3) for sl in (1, 2, 5, 7)]
CUT_PLANS = [OWN] + [(k, nt, st, sl) for k in (1, 2) for nt in (2, 4) for st in (2, 3, 4) for sl in (1, 3)]
WV8_PLANS = [(4, 4, st, sl) for st in (2, 3) for sl in (1, 3)]

# name -> the convolution (fields as lsfa_conv_desc names them; kw / pad_w follow kh / pad_h unless given) and the plans it runs under
CASES = {
    "one_product": dict(N=1, H=4, W=8, Cin=32, Cout=64, kh=1, plans=[OWN, (1, 2, 2, 1)]),
    "one_product_cut": dict(N=1, H=4, W=8, Cin=32, Cout=64, kh=1, in_scale=1, plans=[OWN, (1, 2, 2, 1)]),
    "ring": dict(N=1, H=23, W=31, Cin=256, Cout=128, kh=3, pad_h=2, dil=2, plans=RING_PLANS),      # 72 chunks of K; five full 128-pixel tiles and a partial one
    "cut_256_64": dict(N=2, H=13, W=23, Cin=256, Cout=64, kh=1, in_scale=1, plans=[p for p in CUT_PLANS if p[1] != 4]),      # 64 channels: no 128-wide tiles
    "cut_512_128_s2": dict(N=2, H=14, W=22, Cin=512, Cout=128, kh=1, stride=2, in_scale=1, plans=CUT_PLANS),
    "own_128x128": dict(N=2, H=50, W=64, Cin=256, Cout=1024, kh=1, plans=[OWN]),
    "own_128x128_cut": dict(N=2, H=50, W=64, Cin=256, Cout=1024, kh=1, in_scale=1, plans=[OWN]),
    "direct_3x3": dict(N=2, H=13, W=9, Cin=64, Cout=64, kh=3, pad_h=1, plans=[OWN]),
    "direct_kmajor": dict(N=2, H=7, W=9, Cin=512, Cout=64, kh=1, x_nchw=1, lda=640, plans=[OWN]),
    "view_5x5_s2": dict(N=1, H=19, W=32, Cin=128, Cout=256, kh=5, stride=2, pad_h=2, lda=160, plans=[OWN]),
    "nchw_out": dict(N=2, H=13, W=23, Cin=64, Cout=256, kh=3, pad_h=1, y_nchw=1, plans=[OWN] + [(1, nt, st, 1) for nt in (2, 4) for st in (2, 3)]),
    "wv8_cut": dict(N=2, H=14, W=22, Cin=512, Cout=128, kh=1, stride=2, in_scale=1, plans=WV8_PLANS),
}
# the transposed convolutions (Cin, Cout, channels of the output map, channel offset), each 10 x 16 -> 19 x 32; K = 4 * Cin (1056: sliced)
DECONVS = [(96, 128, 416, 256), (1056, 256, 800, 512)]

_worst = {}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def inputs_of(name):
    """the case's operands as float32 numpy arrays (the same on every machine): x channels-last (N, H, W, Cin), w (Cout, Cin, kh, kw), bias,
    residual (N, Ho, Wo, Cout), in_scale / in_shift (None unless the case has them), scale2 / shift2"""
    c = CASES[name]
    rs = np.random.RandomState(sum(ord(ch) for ch in name))
    N, H, W, Cin, Cout, k = c["N"], c["H"], c["W"], c["Cin"], c["Cout"], c["kh"]
    stride, pad, dil = c.get("stride", 1), c.get("pad_h", 0), c.get("dil", 1)
    Ho, Wo = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    d = dict(stride=stride, pad=pad, dil=dil, K=k * k * Cin, in_scale=None, in_shift=None)
    if c.get("in_scale"):
        d["x"] = f32(rs.randn(N, H, W, Cin) * 3.0)                       # a pre-activation map
        d["in_scale"], d["in_shift"] = f32(rs.uniform(0.5, 1.5, Cin)), f32(rs.randn(Cin))
    else:
        d["x"] = f32(np.maximum(rs.randn(N, H, W, Cin), 0) * 2.0)        # activations like the network's: non-negative, many exact zeros
    d["w"] = f32(rs.randn(Cout, Cin, k, k) / np.sqrt(Cin * k * k))
    d["bias"], d["residual"] = f32(rs.randn(Cout)), f32(rs.randn(N, Ho, Wo, Cout))
    d["scale2"], d["shift2"] = f32(rs.uniform(0.5, 1.5, Cout)), f32(rs.randn(Cout))
    return d


def deconv_inputs_of(cin, cout):
    rs = np.random.RandomState(cin + cout)
    return f32(rs.randn(1, 10, 16, cin)), f32(rs.randn(cin, cout, 4, 4) / np.sqrt(4 * cin)), f32(rs.randn(cout))


def check(case, tag, got, ref, ref_abs, K):
    """both bounds of ref_bf16 on one result; keeps the case's worst ratios for the record"""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    r_gamma, r_fp32 = ref_bf16.bound_ratios(got, ref, ref_abs, K)
    rec = _worst.setdefault(case, {"gamma_err_over_bound": 0.0, "fp32_err_over_bound": 0.0, "launches": 0, "worst_at": None})
    rec["launches"] += 1
    if r_gamma >= rec["gamma_err_over_bound"]:
        rec["gamma_err_over_bound"], rec["worst_at"] = r_gamma, repr(tag)
    rec["fp32_err_over_bound"] = max(rec["fp32_err_over_bound"], r_fp32)
    parity_util.record("conv_bf16", _worst)
    assert r_gamma <= 1.0, "%s %r: err / (gamma(K + 3, 2^-23) * ref_abs) = %.3f" % (case, tag, r_gamma)
    assert r_fp32 < 1.0, "%s %r: max err / (2e-6 * sqrt(K) * max(max|ref|, 1)) = %.3f" % (case, tag, r_fp32)


def guarded(shape, guard_rows=300):
    """a contiguous float32 map of `shape` with `guard_rows` rows (of the last dimension) of sentinel in front of it and behind it: what a launch
    writes past either end of its output (a partial last tile) shows in intact()"""
    n, row = int(np.prod(shape)), int(shape[-1])
    buf = torch.full((n + 2 * guard_rows * row,), float(SENT), dtype=torch.float32, device=DEV)
    out = buf[guard_rows * row:guard_rows * row + n].view(*shape)

    def intact():
        return bool((buf[:guard_rows * row].view(torch.int32) == SENT_BITS).all().item()) and \
            bool((buf[guard_rows * row + n:].view(torch.int32) == SENT_BITS).all().item())
    return out, intact


def holds_sentinel(x):
    return x.numel() == 0 or bool((x.contiguous().view(torch.int32) == SENT_BITS).all().item())


def kernel_names_of(hip, launch):
    """the kernel instantiations (lsfa_conv_plan_query, as the binding's counters name them) of the convolutions `launch` runs"""
    hip.conv_flops_reset(True)
    try:
        out = launch()
        return out, sorted(hip.conv_by_kernel())
    finally:
        hip.conv_flops_reset(False)


# ------------------------------------------------------------------ one product per output ----
ONE_PRODUCT_X = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,                         # ties: to the even neighbour below (1), above (1 + 2^-6)
                          1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23,   # one ulp beside a tie
                          1.9999999, 255.99998,                                     # a carry into the exponent
                          -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), -1.9999999, -3.1415927, 0.33333334, 123456.79, 1e-20, -7e19,
                          3 * 2.0 ** -9, 1 + 2.0 ** -7], np.float32)
ONE_PRODUCT_W = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1.9999999, -1.9999999, 1 + 2.0 ** -8 + 2.0 ** -23, 3 * 2.0 ** -9,
                          0.33333334], np.float32)


@pytest.mark.parametrize("cut", [None, (1.0, 0.0), (-1.0, 0.0), (0.7310586, 0.25)])
def test_one_product_per_output_is_the_product_of_the_rounded_operands(hip, cut):
    """One non-zero input channel: every output is ONE product, and got == float32(bf16_rne(x) * bf16_rne(w)) exactly (the product of two
    bf16 values has 16 significant bits; every other term of the sum is 0 * 0).  Rounding ties both ways, values one ulp beside a tie, a
    carry into the exponent, negatives, 1e-20, -7e19, in both operands; under the plan's own choice and under a forced ring kernel; and with
    the input's affine + ReLU at the cut (in_scale 1, -1 keep the positive / the negated negative values exactly; a third pair rounds twice).
    No bf16 subnormal and no product below 2^-126 is used: whether the matrix pipe flushes them is stated nowhere in the project."""
    c = CASES["one_product" if cut is None else "one_product_cut"]
    rs = np.random.RandomState(5)
    Cin, Cout, H, W = c["Cin"], c["Cout"], c["H"], c["W"]
    x = np.zeros((1, H, W, Cin), np.float32)
    x[0, :, :, 7] = np.resize(ONE_PRODUCT_X, H * W).reshape(H, W)
    w = np.zeros((Cout, Cin, 1, 1), np.float32)
    w[:, 7, 0, 0] = f32(rs.randn(Cout) * 1.7) + np.float32(2.0 ** -12)
    w[:ONE_PRODUCT_W.size, 7, 0, 0] = ONE_PRODUCT_W                              # hand values on the weight side too
    sc = sh = None
    if cut is not None:
        sc, sh = f32(rs.uniform(0.5, 1.5, Cin)), f32(-np.abs(rs.randn(Cin)))     # the empty channels: max(0 * s + t, 0) = 0
        sc[7], sh[7] = cut
    xr, wr = ref_bf16.bf16_rne(ref_bf16.input_at_the_cut(x, sc, sh))[0, :, :, 7], ref_bf16.bf16_rne(w)[:, 7, 0, 0]
    want64 = xr.astype(np.float64)[:, :, None] * wr.astype(np.float64)[None, None, :]
    want = want64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), want64)                       # exact in fp32
    nz = want[want != 0]
    assert np.abs(nz).min() >= 2.0 ** -126 and np.abs(xr[xr != 0]).min() >= 2.0 ** -126 and (wr != 0).all()
    assert (want != 0).sum() >= (8 if cut is not None else H * W) * Cout
    sw = hip.SplitWeight(t(w), pieces=1)
    try:
        for plan in c["plans"]:
            hip.conv_plan_override(*plan)
            got = hip.conv_split(t(x), sw, None, in_scale=None if sc is None else t(sc), in_shift=None if sh is None else t(sh))
            np.testing.assert_array_equal(got.cpu().numpy()[0], want, err_msg=repr((cut, plan)))
    finally:
        hip.conv_plan_override()


# ------------------------------------------------------------------ every ring plan ----
def test_every_ring_plan_against_the_reference(hip):
    """1 x 23 x 31, 256 -> 128, 3x3 with dilation 2 (72 chunks of K: two-level accumulation; under 128-pixel tiles five full tiles and a
    partial one, under 256-pixel tiles two and a partial one) with bias + residual + second output + amax_out, under the plan's own choice
    and every tile width x ring depth x wave roles x K cut (a slice count that leaves the last slice short; the reduce pass), incl. the
    256-pixel tiles of eight waves: each against the reference; out2 == relu(out * sc2 + sh2) bit for bit; the amax slots hold the exact
    maximum of out2; nothing is written in front of or behind either output; and within a (tile width, K cut) class the results are
    bit-identical - ring depth and wave roles only change who issues the copies and how far ahead they run."""
    name = "ring"
    d = inputs_of(name)
    ref, ref_abs = ref_bf16.conv_ref(d["x"], d["w"], d["bias"], 1, (d["pad"], d["pad"]), d["dil"], 0, residual=d["residual"])
    x, b, res, sc2, sh2 = t(d["x"]), t(d["bias"]), t(d["residual"]), t(d["scale2"]), t(d["shift2"])
    sw = hip.SplitWeight(t(d["w"]), pieces=1)
    by_cut = {}
    try:
        for plan in CASES[name]["plans"]:
            kern, nt, st, slices = plan
            hip.conv_plan_override(*plan)
            slots = hip.amax_slots(1, DEV)[0]
            (y, y_ok), (y2, y2_ok) = guarded(res.shape), guarded(res.shape)
            hip.conv_split(x, sw, b, 1, d["pad"], d["dil"], out=y, residual=res, out2=y2, scale2=sc2, shift2=sh2, amax_out=slots)
            check(name, plan, y, ref, ref_abs, d["K"])
            assert y_ok() and y2_ok(), plan
            assert torch.equal(y2, torch.relu(y * sc2 + sh2)), plan
            assert slots.view(torch.float32).max().item() == y2.max().item(), plan
            if kern:
                key = (nt, slices)
                if key in by_cut:
                    assert torch.equal(by_cut[key], y), plan
                by_cut[key] = y.clone()
    finally:
        hip.conv_plan_override()
    assert len(by_cut) == 8


# ------------------------------------------------------------------ the input's activation at the cut ----
def run_cut_case(hip, name, pieces_and_checks):
    """in_scale / in_shift under every plan of the case: pieces 1 against the reference, and (every pieces) bit-identical to the same
    convolution of the stored max(x * s + t, 0) under the same forced plan (the plan's own choice may send the stored map to the direct
    kernel, which sums in another order: there only the reference counts)"""
    d = inputs_of(name)
    ref, ref_abs = ref_bf16.conv_ref(d["x"], d["w"], d["bias"], d["stride"], (0, 0), 1, 1, in_scale=d["in_scale"], in_shift=d["in_shift"])
    x, b, sc, sh = t(d["x"]), t(d["bias"]), t(d["in_scale"]), t(d["in_shift"])
    stored = torch.relu(x * sc + sh)                     # two roundings, like the epilogue that used to store it
    assert np.array_equal(stored.cpu().numpy(), ref_bf16.input_at_the_cut(d["x"], d["in_scale"], d["in_shift"]))
    am = hip.amax_partial(stored)
    try:
        for pieces, against_ref in pieces_and_checks:
            sw = hip.SplitWeight(t(d["w"]), pieces=pieces)
            for plan in CASES[name]["plans"]:
                hip.conv_plan_override(*plan)
                s1, s2 = hip.amax_slots(2, DEV)
                got, got_ok = guarded(ref.shape)
                hip.conv_split(x, sw, b, d["stride"], 0, 1, relu=True, out=got, amax_in=am, amax_out=s2, in_scale=sc, in_shift=sh)
                assert got_ok(), (pieces, plan)
                if against_ref:
                    check(name, (pieces, plan), got, ref, ref_abs, d["K"])
                assert s2.view(torch.float32).max().item() == got.max().item(), (pieces, plan)
                want = hip.conv_split(stored, sw, b, d["stride"], 0, 1, relu=True, amax_in=am, amax_out=s1)
                if plan == OWN:
                    if against_ref:
                        check(name, (pieces, plan, "stored"), want, ref, ref_abs, d["K"])
                    continue
                assert torch.equal(got, want), (pieces, plan)
                assert torch.equal(s1.max(), s2.max()), (pieces, plan)
    finally:
        hip.conv_plan_override()


@pytest.mark.parametrize("name", ["cut_256_64", "cut_512_128_s2"])
def test_input_activation_at_the_cut_against_the_reference(hip, name):
    """bn1 + relu1 applied where conv1 cuts its operand (1x1; two images, a partial last tile; stride 2 reads every other pixel), one piece:
    max(x * s + t, 0) in fp32 with two roundings, THEN the bf16 rounding - against the reference of exactly that, under every plan of the
    ring kernel, and bit-identical to the stored-activation form."""
    run_cut_case(hip, name, [(1, True)])


# ------------------------------------------------------------------ the plan's own 128 x 128 one-piece choice ----
@pytest.mark.parametrize("name,kernel", [("own_128x128", "conv_ring_kernel<4, 1, 3, false, false, 4>"),
                                         ("own_128x128_cut", "conv_ring_kernel<4, 1, 2, false, true, 4>")])
def test_the_plans_own_128x128_choice(hip, name, kernel):
    """2 x 50 x 64, 256 -> 1024, 1x1: 400 tiles of 128 x 128, one slice, mixed roles - the one-piece form's three-stage ring, and with
    in_scale the two-stage one (the table in LDS would leave one workgroup per CU): what the bf16 mode's backbone runs, chosen by the plan
    itself, with residual + ReLU."""
    d = inputs_of(name)
    ref, ref_abs = ref_bf16.conv_ref(d["x"], d["w"], d["bias"], 1, (0, 0), 1, 1, residual=d["residual"], in_scale=d["in_scale"], in_shift=d["in_shift"])
    sw = hip.SplitWeight(t(d["w"]), pieces=1)
    cut = {} if d["in_scale"] is None else dict(in_scale=t(d["in_scale"]), in_shift=t(d["in_shift"]))
    got, got_ok = guarded(ref.shape, guard_rows=64)
    _, names = kernel_names_of(hip, lambda: hip.conv_split(t(d["x"]), sw, t(d["bias"]), relu=True, out=got, residual=t(d["residual"]), **cut))
    assert names == [kernel]
    assert got_ok()
    check(name, kernel, got, ref, ref_abs, d["K"])


# ------------------------------------------------------------------ the direct kernel ----
def test_direct_kernel_against_the_reference(hip):
    """conv_split_direct_kernel<1>: a 3x3 on a small map (2 x 13 x 9: a ragged last pixel tile, K dealt to three waves), and its K-major
    form on channels [0, 512) of a 640-channel NCHW map whose other channels hold NaN."""
    name = "direct_3x3"
    d = inputs_of(name)
    ref, ref_abs = ref_bf16.conv_ref(d["x"], d["w"], d["bias"], 1, (1, 1), 1, 1)
    got, got_ok = guarded(ref.shape)
    _, names = kernel_names_of(hip, lambda: hip.conv_split(t(d["x"]), hip.SplitWeight(t(d["w"]), pieces=1), t(d["bias"]), 1, 1, 1, relu=True, out=got))
    assert names == ["conv_split_direct_kernel<1>"] and got_ok()
    check(name, "nhwc", got, ref, ref_abs, d["K"])
    name = "direct_kmajor"
    d = inputs_of(name)
    ref, ref_abs = ref_bf16.conv_ref(d["x"], d["w"], d["bias"], 1, (0, 0), 1, 0)
    c = CASES[name]
    x_nchw = np.full((c["N"], c["lda"], c["H"], c["W"]), np.nan, np.float32)
    x_nchw[:, :c["Cin"]] = d["x"].transpose(0, 3, 1, 2)
    got, got_ok = guarded(ref.shape)
    _, names = kernel_names_of(hip, lambda: hip.conv_split(t(x_nchw), hip.SplitWeight(t(d["w"]), pieces=1), t(d["bias"]), out=got, x_nchw=True))
    assert names == ["conv_split_direct_kernel<1>"] and got_ok()
    check(name, "x_nchw", got, ref, ref_abs, d["K"])


# ------------------------------------------------------------------ views and the transposed convolution ----
def test_views_and_transposed_convolution_phases(hip):
    """One piece between VIEWS: a strided 5x5 reading 128 of a map's 160 channels (the others hold 1e30) into channels [64, 320) of a
    416-channel map, LeakyReLU; and Deconvolution(4x4, stride 2) + Crop(offset 1), 10 x 16 -> 19 x 32 into a channel offset, with
    deconv_phase_weights(pieces=1): as ONE four-phase launch and as four view launches (Cin 1056: K slices), both against the reference.
    The rest of every output map keeps its sentinel."""
    name = "view_5x5_s2"
    c, d = CASES[name], inputs_of(name)
    ref, ref_abs = ref_bf16.conv_ref(d["x"], d["w"], d["bias"], 2, (2, 2), 1, 2)
    L, Lout, c0, Cout = c["lda"], 416, 64, c["Cout"]
    xw = torch.full((c["N"], c["H"], c["W"], L), 1e30, dtype=torch.float32, device=DEV)
    xw[..., :c["Cin"]] = t(d["x"])
    out = torch.full(ref.shape[:3] + (Lout,), float(SENT), dtype=torch.float32, device=DEV)
    hip.conv_split_view(xw, hip.SplitWeight(t(d["w"]), pieces=1), t(d["bias"]), out, stride=2, pad=(2, 2), act=2, cin=c["Cin"], c0=c0)
    check(name, "view", out[..., c0:c0 + Cout], ref, ref_abs, d["K"])
    assert holds_sentinel(out[..., :c0]) and holds_sentinel(out[..., c0 + Cout:])
    Hc, Wc = 19, 32
    for cin, cout, Lout, c0 in DECONVS:
        name = "deconv_%d_%d" % (cin, cout)
        x, wt, b = deconv_inputs_of(cin, cout)
        ref, ref_abs = ref_bf16.deconv_crop_ref(x, wt, b, Hc, Wc, 2)
        sws = hip.deconv_phase_weights(t(wt), pieces=1)
        assert sws.pieces == 1
        one = torch.full((1, Hc, Wc, Lout), float(SENT), dtype=torch.float32, device=DEV)
        hip.deconv4x4s2_crop(t(x), sws, t(b), one, c0=c0, act=2)
        four = torch.full((1, Hc, Wc, Lout), float(SENT), dtype=torch.float32, device=DEV)
        for py in (0, 1):
            for px in (0, 1):
                hip.conv_split_view(t(x), sws[py * 2 + px], t(b), four, stride=1, pad=(1 - py, 1 - px), act=2, c0=c0,
                                    grid=((Hc - py + 1) // 2, (Wc - px + 1) // 2), place=(py, px, 2, 2))
        for tag, got in (("one launch", one), ("four launches", four)):
            check(name, tag, got[..., c0:c0 + cout], ref, ref_abs, 4 * cin)
            assert holds_sentinel(got[..., :c0]) and holds_sentinel(got[..., c0 + cout:]), (name, tag)


# ------------------------------------------------------------------ NCHW output ----
def test_nchw_output_against_the_reference(hip):
    """y_nchw with one piece, per tile width and ring depth (the three-stage rings turn the tiles in LDS, the two-stage 128 x 128 one is too
    small for that and stores fragment-shaped): 2 x 13 x 23, 64 -> 256, 3x3, whose 128-pixel tiles straddle the images and end in a partial
    one; bias + NCHW residual + LeakyReLU."""
    name = "nchw_out"
    d = inputs_of(name)
    ref, ref_abs = ref_bf16.conv_ref(d["x"], d["w"], d["bias"], 1, (1, 1), 1, 2, residual=d["residual"])
    ref, ref_abs = np.ascontiguousarray(ref.transpose(0, 3, 1, 2)), np.ascontiguousarray(ref_abs.transpose(0, 3, 1, 2))
    x, b, res_n = t(d["x"]), t(d["bias"]), t(np.ascontiguousarray(d["residual"].transpose(0, 3, 1, 2)))
    sw = hip.SplitWeight(t(d["w"]), pieces=1)
    try:
        for plan in CASES[name]["plans"]:
            hip.conv_plan_override(*plan)
            slots = hip.amax_slots(1, DEV)[0]
            got, got_ok = guarded(ref.shape)
            hip.conv_split(x, sw, b, 1, 1, 1, act=2, out=got, residual=res_n, nchw=True, amax_out=slots)
            assert got_ok(), plan
            check(name, plan, got, ref, ref_abs, d["K"])
            assert slots.view(torch.float32).max().item() == got.abs().max().item(), plan
    finally:
        hip.conv_plan_override()


# ------------------------------------------------------------------ eight waves with the activation at the cut (last: never launched before) ----
def test_eight_wave_tiles_with_the_activation_at_the_cut(hip):
    """conv_ring_kernel<4, PC, ST, false, true, 8>, PC 1 and 2, ST 2 and 3: 256-pixel tiles of eight mixed-role waves with in_scale /
    in_shift.  All 512 threads fill the affine table (stride 64 * WV) behind the prologue's copies, and the barrier in front of the first
    cut (preceded by an lgkmcnt(0)) makes it visible to every wave.  One piece: against the reference; one and two pieces: bit-identical to
    the stored-activation form under the same plan.  (2 x 7 x 11 output pixels of 512 -> 128, stride 2: one partial 256-pixel tile; K whole
    and cut in three.)"""
    run_cut_case(hip, "wv8_cut", [(1, True), (2, False)])
