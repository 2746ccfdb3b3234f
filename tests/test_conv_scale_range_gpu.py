"""The fp16 two-piece form's power-of-two scale rule over float32's exponent range (pieces = 2, per-channel weight scales).

THE RULE, stated once here and checked below on every kernel that has a copy of it:
  map      s_exp = min(13 - floor(log2(amax_in)), 100): the map's maximum goes to [2^13, 2^14) unless it is below 2^-87; then the scale stays
           2^100 and the scaled maximum is smaller (fp16's subnormals take over: the bound below).  A zero or subnormal maximum has
           s_exp = 13: every scaled value is below 2^-112, both fp16 pieces are zero, the output is the bias exactly.
  weights  hip._fp16_exponent, +-100 per output channel; a channel whose maximum is 2^114 or more (its scale would be clamped at 2^-100 and
           the scaled maximum would leave [2^13, 2^14) towards fp16's overflow) is REFUSED at bind time with LsfaError - the decision
           asked for: no status bit at run time.
  columns  the accumulator columns are multiplied back by ONE float, 2^-w_exp[co] * 2^-s_exp.  From s_exp + w_exp = 150 on that float is
           zero (2^-150 rounds to 0 in float32) and the channel's output is flushed to the bias, although the convolution's value
           (up to about 2^(28 - 150) K) may still be a normal float32 number; up to 149 it is an exact (subnormal) power of two.
  stem     scale_of (stem.hip) scales a patch whose maximum has a biased exponent in [32, 240]; a tinier patch keeps scale 1, its fp16
           pieces are zero and the output is the bias.  (A patch maximum of 2^114 or more also keeps scale 1 and overflows fp16: outside
           this file's sweep, which stops the stem at k = 100.)

BOUNDS.  K = Cin kh kw.  Where no clamp binds: the suite's criterion (test_conv_split_vs_float64_and_fp32_mfma), error <= 2e-6 sqrt(K) max|want|,
against a float64 convolution of the same float32 operands.  Where the map's clamp binds, derived from the formats alone:
  a = x 2^100 is exact, |a| < 2^13.  hi = fp16(a): |a - hi| <= max(2^-11 |a|, 2^-25)  (11 significant bits; spacing 2^-24 below 2^-14).
  r = a - hi is exact in float32.  lo = fp16(r): |r - lo| <= max(2^-11 |r|, 2^-25) <= max(2^-22 |a|, 2^-25).
  So hi + lo = a + d with |d| <= 2^-22 |a| + 2^-25.  The first term is the cut's ordinary relative error, part of the criterion above.  The
  second is new: 2^-25 under the scale = 2^-125 per activation in the map's units, times the weight it meets (hi' + lo' = w (1 + 2^-22) at
  most), summed over the K taps: at most 2^-125 (1 + 2^-20) max_co sum|w[co]|.  The stored float32 may be subnormal: + 2^-150 (half of 2^-149).
  bound = 2e-6 sqrt(K) max|want| + 2^-125 (1 + 2^-20) max_co sum|w[co]| + 2^-150.
The same with the roles exchanged where a weight channel's clamp binds (its scaled values sit below 2^13 under 2^100):
  bound = 2e-6 sqrt(K) max|want[co]| + 2^-125 (1 + 2^-20) max_pixel sum|x| + 2^-150.

A power-of-two scale commutes with every step: while map, weights and outputs stay normal numbers, the output for x 2^k is the output for x
times 2^k bit for bit.

The map sweep's k = -128 leaves a maximum of about 2^-124.5 (the map's own maximum is about 2^3.5), a normal number with many subnormal
values beneath it; the subnormal-MAXIMUM case is its own test (k = -132)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAP_KS = [-128, -126, -120, -115, -114, -113, -101, -100, -88, -87, -40, 0, 40, 100, 113]
WEIGHT_JS = [-120, -101, -100, -60, 60, 90]
JOINT_SUMS = [40, 126, 149, 150, 160]
F32_MIN_NORMAL = 2.0 ** -126
CLAMP = 100
ABS_TERM = 2.0 ** -125 * (1.0 + 2.0 ** -20)
PLANS = {"mixed 64x": (1, 2, 2, 1), "loader 64x": (2, 2, 3, 1), "mixed 128x": (1, 4, 2, 1), "eight waves": (4, 4, 2, 1), "sliced": (2, 2, 3, 2)}
ODD = 5                          # the output channel the weight sweeps single out
SMALL = ("direct 1x1", "x_nchw")     # the paths on 2 x 5 x 7 pixels, 64 -> 64


def weight_name(path):
    return "w64" if path in SMALL else "w3x3" if path == "3x3 sliced" else "w128"


def scaled(t, k):
    """t * 2^k as float32: exact while no value leaves the normal range, rounded once to nearest where one does"""
    return (t.double() * 2.0 ** k).float()


def conv64(x_nhwc, w, pad=0):
    return F.conv2d(x_nhwc.permute(0, 3, 1, 2).double(), w.double(), padding=pad).permute(0, 2, 3, 1).contiguous()


def floor_log2(v):
    return math.frexp(v)[1] - 1


def map_regime(amax):
    """-> 'bias' (zero or subnormal maximum), 'scaled' (the maximum reaches [2^13, 2^14)) or 'clamped'"""
    if amax < F32_MIN_NORMAL:
        return "bias"
    return "scaled" if 13 - floor_log2(amax) <= CLAMP else "clamped"


@pytest.fixture(scope="module")
def B(hip):
    """the operands of every path at k = 0 (CPU float32, never written to) and their weights, bound once"""
    g = torch.Generator().manual_seed(62)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    b = {}
    b["x_small"], b["x"] = torch.relu(rn(2, 5, 7, 64)) * 3, torch.relu(rn(2, 13, 23, 64)) * 3
    b["x_small"][0, 0, 0, :] = 0.0
    b["x"][1, 2, 3, :] = 0.0
    b["w64"], b["w128"], b["w3x3"] = rn(64, 64, 1, 1) / 8, rn(128, 64, 1, 1) / 8, rn(128, 64, 3, 3) / 24
    b["raw"], b["in_scale"], b["in_shift"] = rn(2, 13, 23, 64) * 3, 0.5 + torch.rand(64, generator=g), rn(64)
    b["x_deconv"], b["wt"] = torch.relu(rn(1, 5, 8, 32)) * 3, rn(32, 64, 4, 4) / math.sqrt(128)
    b["x_pair"], b["w3"], b["w1"] = torch.relu(rn(1, 5, 5, 64)) * 3, rn(256, 64, 1, 1) / 8, rn(64, 256, 1, 1) / 16
    b["s2"], b["res"], b["h2"], b["b1"] = 0.5 + torch.rand(256, generator=g), rn(1, 5, 5, 256), 0.1 * rn(256), rn(64)
    b["img"], b["w_stem"] = torch.relu(rn(1, 3, 9, 8)) * 3, rn(64, 3, 7, 7) * 0.05
    b["bias64"], b["bias128"] = rn(64), rn(128)
    for name in ("w64", "w128", "w3x3", "w3", "w1"):
        b["sw_" + name] = hip.SplitWeight(b[name].to(DEV), pieces=2)
        assert b["sw_" + name].w_scale is not None
    b["sw_deconv"] = hip.deconv_phase_weights(b["wt"].to(DEV), pieces=2)
    b["stem_frag"] = hip.stem_weight_layout(b["w_stem"].to(DEV))
    b["cache"] = {}
    return b


def split_launch(hip, plan, x, sw, am, bias=None, pad=0, **kw):
    """conv_split under a forced plan (None: the plan's own choice) -> (y, max of the amax_out slots, status word)"""
    slots, status = hip.amax_slots(1, DEV)[0], hip.new_status(DEV)
    try:
        if plan:
            hip.conv_plan_override(kernel=plan[0], nt=plan[1], st=plan[2], slices=plan[3])
        y = hip.conv_split(x, sw, bias, 1, pad, 1, amax_in=am, amax_out=slots, status=status, **kw)
    finally:
        hip.conv_plan_override()
    return y, slots.view(torch.float32).max().item(), status


def run_path(hip, B, path, k, with_bias=False, w=None, sw=None, zero=False):
    """One launch of `path` on its k = 0 map times 2^k (zero: the all-zero map) -> dict(y, want (float64, CPU), K, sum_w = max_co sum|w[co]|,
    amax = the map's maximum, amax_out, status, extra).  w / sw: another weight of the path's shape (the weight sweeps)."""
    pick = lambda name: (torch.zeros_like(B[name]) if zero else scaled(B[name], k))
    dev = lambda t: t.to(DEV)
    r = dict(extra={})
    if path == "direct 1x1" or path in PLANS or path == "3x3 sliced" or path == "x_nchw":
        # (x_nchw is the direct kernel's: the small map)
        xname, wname, pad = ("x_small", "w64", 0) if path in SMALL else ("x", "w3x3", 1) if path == "3x3 sliced" else ("x", "w128", 0)
        x = pick(xname)
        w = B[wname] if w is None else w
        sw = B["sw_" + wname] if sw is None else sw
        bias = B["bias%d" % w.shape[0]] if with_bias else None
        want = conv64(x, w, pad) + (bias.double() if with_bias else 0.0)
        plan = PLANS.get(path, PLANS["sliced"] if path == "3x3 sliced" else None)
        xd = dev(x)
        am = hip.amax_partial(xd)
        if path == "x_nchw":
            xd = xd.permute(0, 3, 1, 2).contiguous()
        y, amax_out, status = split_launch(hip, plan, xd, sw, am, dev(bias) if with_bias else None, pad, x_nchw=(path == "x_nchw"))
        r.update(y=y, want=want, K=w[0].numel(), sum_w=w.abs().double().reshape(w.shape[0], -1).sum(1).max().item(), amax=x.abs().max().item(),
                 amax_out=amax_out, status=status, sum_x=F.conv2d(x.permute(0, 3, 1, 2).double(), torch.ones(1, 64, w.shape[2], w.shape[3],
                                                                                                             dtype=torch.float64), padding=pad).max().item())
    elif path == "at the cut":
        raw, shift = pick("raw"), pick("in_shift")
        w = B["w128"] if w is None else w
        sw = B["sw_w128"] if sw is None else sw
        bias = B["bias128"] if with_bias else None
        act = torch.relu(raw * B["in_scale"] + shift)                  # two roundings, as the kernel applies it where it cuts
        want = conv64(act, w) + (bias.double() if with_bias else 0.0)
        am = hip.amax_partial(dev(act))
        y, amax_out, status = split_launch(hip, None, dev(raw), sw, am, dev(bias) if with_bias else None, in_scale=dev(B["in_scale"]), in_shift=dev(shift))
        r.update(y=y, want=want, K=64, sum_w=w.abs().double().reshape(w.shape[0], -1).sum(1).max().item(), amax=act.abs().max().item(),
                 amax_out=amax_out, status=status, sum_x=act.double().sum(3).max().item())
    elif path == "deconv":
        x, wt = pick("x_deconv"), B["wt"]
        bias = B["bias64"] if with_bias else None
        full = F.conv_transpose2d(x.permute(0, 3, 1, 2).double(), wt.double(), bias.double() if with_bias else None, stride=2)
        want = full[:, :, 1:10, 1:16].permute(0, 2, 3, 1).contiguous()
        slots, status = hip.amax_slots(1, DEV)[0], hip.new_status(DEV)
        xd = dev(x)
        y = hip.deconv4x4s2_crop(xd, B["sw_deconv"], dev(bias) if with_bias else None, torch.empty((1, 9, 15, 64), device=DEV), act=0,
                                 amax_in=hip.amax_partial(xd), amax_out=slots, status=status)
        # an output pixel meets 2 x 2 of the 4 x 4 taps: the largest sum over any phase bounds it
        sum_w = max(wt[:, :, ky, :][:, :, :, kx].abs().double().sum(dim=(0, 2, 3)).max().item() for ky in ((3, 1), (2, 0)) for kx in ((3, 1), (2, 0)))
        r.update(y=y, want=want, K=128, sum_w=sum_w, amax=x.abs().max().item(), amax_out=slots.view(torch.float32).max().item(), status=status)
    elif path == "conv_pair":
        x = pick("x_pair")
        res = B["res"] if with_bias else torch.zeros_like(B["res"])                       # the residual is conv3's "bias"
        h2, b1 = (B["h2"], B["b1"]) if with_bias else (torch.zeros(256), None)
        want = conv64(x, B["w3"]) + res.double()
        xd, resd, s2d, h2d = dev(x), dev(res), dev(B["s2"]), dev(h2)
        am = hip.amax_partial(xd)
        slots, status = hip.amax_slots(2, DEV), hip.new_status(DEV)
        y, z = hip.conv_pair(xd, B["sw_w3"], resd, s2d, h2d, B["sw_w1"], None if b1 is None else dev(b1), amax_in=am, amax_out_sum=slots[0],
                             amax_out_z=slots[1], status=status)
        y_split, amax_split, status_split = split_launch(hip, PLANS["mixed 128x"], xd, B["sw_w3"], am, residual=resd, scale2=s2d, shift2=h2d)
        a = torch.relu(y * s2d + h2d)
        want_z = torch.relu(a.double().cpu().reshape(-1, 256) @ B["w1"].double().reshape(64, 256).t() + (0.0 if b1 is None else b1.double()))
        r.update(y=y, want=want, K=64, sum_w=B["w3"].abs().double().reshape(256, -1).sum(1).max().item(), amax=x.abs().max().item(),
                 amax_out=slots[0].view(torch.float32).max().item(), status=status,
                 extra=dict(z=z, want_z=want_z.reshape(1, 5, 5, 64), a_max=a.max().item(), z_amax=slots[1].view(torch.float32).max().item(),
                            y_split=y_split, amax_split=amax_split, status_split=status_split))
    else:
        raise KeyError(path)
    return r


def clear(status):
    return int(status[0].item()) == 0                 # word 0 is the one lsfa_status_check reads


def error(y, want):
    return (y.double().cpu() - want).abs().max().item()


MAP_PATHS = ["direct 1x1"] + list(PLANS) + ["3x3 sliced", "at the cut", "x_nchw", "deconv", "conv_pair"]


def at_k0(hip, B, path):
    if path not in B["cache"]:
        B["cache"][path] = run_path(hip, B, path, 0)
    return B["cache"][path]


@pytest.mark.parametrize("k", MAP_KS)
@pytest.mark.parametrize("path", MAP_PATHS)
def test_map_sweep(hip, B, path, k):
    """(a) and (d): the map times 2^k, zero bias, weights of order 1 / sqrt(K), amax_in the exact maximum.  Where the scale reaches [2^13, 2^14):
    the criterion, a clear status word, amax_out = max|y| exactly, and the k = 0 output times 2^k bit for bit on every value that stays a
    normal number.  Where the clamp binds: finite, status clear, the derived bound (module docstring).  conv_pair's y equals conv_split's
    under the unsliced 128-wide plan bit for bit at every k."""
    r = run_path(hip, B, path, k)
    y, want = r["y"], r["want"]
    regime = map_regime(r["amax"])
    err, top = error(y, want), want.abs().max().item()
    criterion = 2e-6 * math.sqrt(r["K"]) * top
    bound = criterion + ABS_TERM * r["sum_w"] + 2.0 ** -150
    print("%s k=%d: %s, amax %.3e, max|want| %.3e, err %.3e, criterion %.3e, clamped bound %.3e, status %s, finite %s" %
          (path, k, regime, r["amax"], top, err, criterion, bound, r["status"].tolist(), bool(torch.isfinite(y).all())))
    assert regime != "bias", "none of the sweep's maps has a subnormal maximum"
    assert bool(torch.isfinite(y).all()), "non-finite output, status %s" % r["status"].tolist()
    assert clear(r["status"]), r["status"].tolist()
    if path == "conv_pair":
        e = r["extra"]
        assert torch.equal(y, e["y_split"]) and clear(e["status_split"])
        assert bool(torch.isfinite(e["z"]).all())
        assert r["amax_out"] == e["a_max"] == e["amax_split"] and e["z_amax"] == e["z"].abs().max().item()
    else:
        assert r["amax_out"] == y.abs().max().item()
    if regime == "clamped":
        assert err <= bound, (err, bound)
        return
    assert err <= criterion, (err, criterion)
    if path == "conv_pair":      # conv1 on the GPU's own sum, under the block scales
        ez = r["extra"]
        assert error(ez["z"], ez["want_z"]) <= 2e-6 * math.sqrt(256) * ez["want_z"].abs().max().item()
    y0 = at_k0(hip, B, path)["y"].double().cpu() * 2.0 ** k
    normal = (y0.abs() >= F32_MIN_NORMAL) | (y0 == 0)
    assert bool(normal.any()) and torch.equal(y.double().cpu()[normal], y0[normal])


@pytest.mark.parametrize("case", ["zeros", "subnormal maximum"])
@pytest.mark.parametrize("path", MAP_PATHS)
def test_zero_and_subnormal_maximum_give_the_bias(hip, B, path, case):
    """an all-zero map and a map whose maximum is a subnormal number (k = -132) give the bias exactly (conv_pair: y = the residual, z =
    conv1 of the activated residual as for any other y), status clear"""
    r = run_path(hip, B, path, -132, with_bias=True, zero=(case == "zeros"))
    if case == "zeros":
        assert r["amax"] == 0.0
    else:
        assert 0.0 < r["amax"] < F32_MIN_NORMAL
    assert clear(r["status"]), r["status"].tolist()
    if path == "conv_pair":
        assert torch.equal(r["y"].cpu(), B["res"])
        ez = r["extra"]
        assert torch.equal(r["y"], ez["y_split"])
        assert error(ez["z"], ez["want_z"]) <= 2e-6 * math.sqrt(256) * ez["want_z"].abs().max().item()
        return
    bias = B["bias%d" % r["y"].shape[3]]
    assert torch.equal(r["y"].cpu(), bias.expand_as(r["y"]))
    assert r["amax_out"] == bias.abs().max().item()


WEIGHT_PATHS = ["direct 1x1"] + list(PLANS) + ["3x3 sliced", "at the cut", "x_nchw"]


def odd_weight(B, path, j):
    w = B[weight_name(path)].clone()
    w[ODD] = scaled(w[ODD], j)
    return w


@pytest.mark.parametrize("j", WEIGHT_JS)
@pytest.mark.parametrize("path", WEIGHT_PATHS)
def test_weight_sweep(hip, B, path, j):
    """(b): one output channel's weights times 2^j.  The other channels come out bit-identical to the run without the odd channel; the odd
    channel meets the criterion on its own scale while its exponent is unclamped and the derived bound (roles exchanged) beyond."""
    w = odd_weight(B, path, j)
    r = run_path(hip, B, path, 0, w=w, sw=hip.SplitWeight(w.to(DEV), pieces=2))
    base = at_k0(hip, B, path)
    y, want = r["y"], r["want"]
    others = [c for c in range(y.shape[3]) if c != ODD]
    assert bool(torch.isfinite(y).all()) and clear(r["status"])
    assert torch.equal(y[..., others], base["y"][..., others])
    raw = 13 - floor_log2(w[ODD].abs().max().item())
    err, top = error(y[..., ODD], want[..., ODD]), want[..., ODD].abs().max().item()
    criterion = 2e-6 * math.sqrt(r["K"]) * top
    bound = criterion + ABS_TERM * r["sum_x"] + 2.0 ** -150
    print("%s j=%d: w_exp %d before the clamp, max|want| %.3e, err %.3e, criterion %.3e, clamped bound %.3e" % (path, j, raw, top, err, criterion, bound))
    if abs(raw) <= CLAMP:
        assert err <= criterion, (err, criterion)
    else:
        assert raw > CLAMP and err <= bound, (raw, err, bound)
    assert r["amax_out"] == y.abs().max().item()


def test_a_weight_channel_past_the_upper_clamp_is_refused_at_bind_time(hip, B):
    """a channel (or a tensor) whose maximum is 2^114 or more would be scaled by the clamped 2^-100 and leave [2^13, 2^14) towards fp16's
    overflow: SplitWeight and deconv_phase_weights refuse it; the largest maximum below 2^114 is taken and meets the criterion"""
    w = B["w128"].clone()
    w[ODD] = scaled(w[ODD], floor_log2(2.0 ** 113) - floor_log2(w[ODD].abs().max().item()))          # the channel's maximum into [2^113, 2^114)
    assert 2.0 ** 113 <= w[ODD].abs().max().item() < 2.0 ** 114
    r = run_path(hip, B, "mixed 64x", 0, w=w, sw=hip.SplitWeight(w.to(DEV), pieces=2))
    assert bool(torch.isfinite(r["y"]).all()) and clear(r["status"])
    assert error(r["y"][..., ODD], r["want"][..., ODD]) <= 2e-6 * 8 * r["want"][..., ODD].abs().max().item()
    w[ODD] *= 2.0
    with pytest.raises(hip.LsfaError, match="2\\^114"):
        hip.SplitWeight(w.to(DEV), pieces=2)
    with pytest.raises(hip.LsfaError, match="2\\^114"):
        hip.SplitWeight(w.to(DEV), pieces=2, per_channel_scale=False)
    wt = B["wt"].clone()
    wt[3, 7, 1, 2] = 2.0 ** 114
    with pytest.raises(hip.LsfaError, match="2\\^114"):
        hip.deconv_phase_weights(wt.to(DEV), pieces=2)
    hip.SplitWeight(w.to(DEV), pieces=3)                                                               # the three-piece form has no scale


@pytest.mark.parametrize("total", JOINT_SUMS)
@pytest.mark.parametrize("path", ["direct 1x1", "mixed 64x", "eight waves", "sliced", "3x3 sliced"])
def test_joint_sweep(hip, B, path, total):
    """(c): a map exponent s_exp and the odd channel's exponent w_exp with s_exp + w_exp = total, neither clamped.  Up to 149 the column factor
    2^-total is a power of two float32 holds exactly: the criterion on the channel's own scale (+ 2^-150, half the spacing of the subnormal
    float32 some outputs are stored as).  From 150 on the factor is zero: the odd channel is flushed to (zero) bias - pinned as it is,
    although at 150 the float64 convolution still holds normal float32 numbers (asserted, so that the flush is known to be premature).  The
    other channels (w_exp about 15) meet the criterion throughout."""
    base = at_k0(hip, B, path)
    wname = weight_name(path)
    s_exp = total // 2
    k = 13 - floor_log2(base["amax"]) - s_exp
    j = 13 - floor_log2(B[wname][ODD].abs().max().item()) - (total - s_exp)
    w = odd_weight(B, path, j)
    assert 13 - floor_log2(w[ODD].abs().max().item()) == total - s_exp
    r = run_path(hip, B, path, k, w=w, sw=hip.SplitWeight(w.to(DEV), pieces=2))
    assert 13 - floor_log2(r["amax"]) == s_exp
    y, want = r["y"], r["want"]
    others = [c for c in range(y.shape[3]) if c != ODD]
    assert bool(torch.isfinite(y).all()) and clear(r["status"])
    rootK = math.sqrt(r["K"])
    assert error(y[..., others], want[..., others]) <= 2e-6 * rootK * want[..., others].abs().max().item()
    err, top = error(y[..., ODD], want[..., ODD]), want[..., ODD].abs().max().item()
    print("%s s_exp %d + w_exp %d: max|want| %.3e (2^%d), err %.3e, max|y| %.3e" % (path, s_exp, total - s_exp, top, floor_log2(top), err,
                                                                                   y[..., ODD].abs().max().item()))
    if total <= 149:
        assert err <= 2e-6 * rootK * top + 2.0 ** -150, (err, top)
    else:
        if total == 150:
            assert top >= F32_MIN_NORMAL
        assert bool((y[..., ODD] == 0).all())


@pytest.mark.parametrize("k", [k for k in MAP_KS if k <= 100])
def test_stem_follows_its_own_rule(hip, B, k):
    """(d): stem_conv on a 1 x 9 x 8 image times 2^k.  scale_of scales a patch whose maximum has a biased exponent in [32, 240] (2^-95 up to
    2^114): the criterion with K = 147.  Below, the documented 'scale 1 for tiny': fp16(x) = 0 for |x| < 2^-25, so the output is the bias
    exactly.  (The image is one patch: one maximum decides.)"""
    img = scaled(B["img"], k)
    bias = B["bias64"]
    slots = hip.amax_slots(1, DEV)[0]
    y = hip.stem_conv(img.to(DEV), B["stem_frag"], bias.to(DEV), act=0, amax_out=slots)
    assert y.shape == (1, 5, 4, 64) and bool(torch.isfinite(y).all())
    assert slots.view(torch.float32).max().item() == y.abs().max().item()
    amax = img.abs().max().item()
    if amax < 2.0 ** -95:
        assert torch.equal(y.cpu(), bias.expand_as(y))
        return
    # without the bias in the way of the scale: the criterion is on the convolution's own magnitude
    y = hip.stem_conv(img.to(DEV), B["stem_frag"], None, act=0)
    want = F.conv2d(img.double(), B["w_stem"].double(), stride=2, padding=3).permute(0, 2, 3, 1)
    assert error(y, want) <= 2e-6 * math.sqrt(147) * want.abs().max().item()


def test_conv_pair_tiny_block_next_to_normal_blocks(hip):
    """(d): one 128-channel block of the activated sum 2^-110 below its neighbours (through scale2 / shift2, after
    test_conv_pair_gpu.make_case(block_scales=True)): its block scale is clamped at 2^100, everything stays finite, and next to blocks of
    ordinary size its contribution to z is below half a unit in the last place of every partial sum - z equals, bit for bit, the z of the
    same launch with that block switched off behind the ReLU, and y is the same map."""
    from test_conv_pair_gpu import make_case
    out = {}
    for tag in ("tiny", "off"):
        c = make_case((2, 14, 22, 128, 512, 128))
        if tag == "tiny":
            c["s2"][384:512] *= 2.0 ** -110
            c["h2"][384:512] *= 2.0 ** -110
        else:
            c["s2"][384:512] = 0.0
            c["h2"][384:512] = -1.0
        sw3, sw1 = hip.SplitWeight(c["w3"], pieces=2), hip.SplitWeight(c["w1"], pieces=2)
        slots, status = hip.amax_slots(2, DEV), hip.new_status(DEV)
        y, z = hip.conv_pair(c["x"], sw3, c["res"], c["s2"], c["h2"], sw1, c["b1"], amax_in=hip.amax_partial(c["x"]), amax_out_sum=slots[0],
                             amax_out_z=slots[1], status=status)
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(z).all()) and clear(status)
        a = torch.relu(y * c["s2"] + c["h2"])
        out[tag] = (y, z, a)
    a = out["tiny"][2]
    assert 0 < a[..., 384:512].max().item() < 2.0 ** -100 and a[..., :384].max().item() > 1.0
    assert bool((out["off"][2][..., 384:512] == 0).all())
    assert torch.equal(out["tiny"][0], out["off"][0])
    assert torch.equal(out["tiny"][1], out["off"][1])
