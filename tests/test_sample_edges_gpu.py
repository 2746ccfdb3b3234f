"""Every warp and deformable-sampling kernel on the coordinates where a bilinear sampler's index decision is made.

The fields are those of tests/ref_sample.py (test_sample_edges_cpu.py shows that they hold every edge class on both axes and every pair of
border classes): whole-pixel flows, 0, one step either side of 0, -1, L - 1, L, the bands between, coordinates beyond 2^31, inf and NaN.
One statement of each sampler's edge behaviour, run over every kernel that holds a copy of the sampling statement:

  warp        gather (float4 / float2 / scalar by the plane's size, and the scalar form misaligned maps fall back to), LDS-staged, channels-last,
              and the bn form of the gather and channels-last kernels
  deformable  NCHW, channels-last general, channels-last power-of-two, through lsfa_deform_im2col_cl_ld with a padded offset row too

Policy.  Every comparison is assert_array_equal against BOTH the numpy statement (ref_sample.*_f32) and the C oracle.
  warp: on every cell neither of whose coordinates is inf or NaN - cells at or beyond 2^31 included, where the sample is exactly zero.  A cell
        with a non-finite coordinate has NaN weights: each of its outputs must be NaN or what the epilogue makes of a zero sample, nothing else,
        and it must leave every other cell of the map bit-equal.
  deformable: on every cell.  Its guard runs before any conversion, so NaN, +-inf and +-3e38 give exactly 0.0."""
import ctypes

import numpy as np
import pytest
import torch

import guarded_arena as ga
import oracle
import ref_sample as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HW_IDS = lambda hw: "%dx%d" % hw
CFG_IDS = lambda c: "pad%d-s%d-d%d-dg%d" % c
SUBSETS = ("plain", "add", "res", "res+add")              # the cur path's operands
_want = {}


def t(a):
    return torch.from_numpy(np.array(a, np.float32, order="C")).to(DEV)              # (a copy: the cases' arrays are read-only)


def nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def warp_want(hw, C, field, subset, feat_n):
    """(the numpy statement, the oracle, what the epilogue makes of a zero sample) for all K maps of a field, map n sampling feature
    n mod feat_n; computed once, never written to"""
    key = (hw, C, field, subset, feat_n)
    if key not in _want:
        case = R.warp_case(hw, C)
        flow = case[field]
        K = flow.shape[0]
        kw = R.warp_operands(case, subset, slice(0, K))
        ref = R.warp_ref_f32(case["feat"][:feat_n], flow, **kw)
        # the oracle has no bn argument and takes one feature or one per map: bn is asserted against the numpy statement alone, and a second
        # feature goes through it two maps at a time
        orc = None
        if "bn" not in subset:
            def okw(sl):
                o = dict((k, kw[k][sl]) for k in ("mul", "add") if k in kw)
                if "res" in kw:
                    o.update(res=kw["res"][0][sl], res_w=kw["res"][1], res_b=kw["res"][2])
                return o
            orc = np.concatenate([oracle.warp_bilinear(case["feat"][:feat_n], flow[i:i + 2], **okw(slice(i, i + 2))) for i in range(0, K, 2)])
        zero = R.warp_zero_sample(ref.shape, **kw)
        for a in (ref, orc, zero):
            if a is not None:
                a.setflags(write=False)
        _want[key] = (ref, orc, zero)
    return _want[key]


def check_warp(got, hw, C, field, subset, feat_n, i):
    """maps [i, i + 2) of a field: got (2, C, H, W) numpy"""
    case = R.warp_case(hw, C)
    ref, orc, zero = warp_want(hw, C, field, subset, feat_n)
    _, _, nonfinite, zero_sample = R.warp_classes(case[field][i:i + 2])
    m = np.broadcast_to(~nonfinite[:, None], got.shape)
    np.testing.assert_array_equal(got[m], ref[i:i + 2][m])
    if orc is not None:
        np.testing.assert_array_equal(got[m], orc[i:i + 2][m])
    z = np.broadcast_to(zero_sample[:, None], got.shape)
    np.testing.assert_array_equal(got[z], zero[i:i + 2][z])
    assert (np.isnan(got) | (got == zero[i:i + 2]))[~m].all(), "a non-finite coordinate gave something other than NaN or a zero sample"
    assert np.isfinite(got[m]).all()


def dev_operands(case, subset, sl, cl=False):
    """the wrapper's keyword operands on the device for maps `sl`"""
    kw = {}
    for name, v in R.warp_operands(case, subset, sl).items():
        if name == "res":
            kw.update(res=t(v[0]), res_w=t(v[1]), res_b=t(v[2]))
        elif name == "bn":
            kw["bn"] = (t(v[0]), t(v[1]))
        elif name == "add" and cl:
            kw["add_cl"] = t(nhwc(v))
        else:
            kw[name] = t(v)
    return kw


@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("hw", R.SHAPES, ids=HW_IDS)
def test_warp_nchw_kernels_on_the_edge_field(hip, hw, C):
    """'gather', 'staged' and 'auto' on every operand subset (and the scale map), one feature for both maps of a call and one each.  A plane of
    an odd number of pixels is refused by 'staged' (an LsfaError, as ever); every even one here - 9 x 16 with 16 channels among them - must be
    taken.  Then the bn form (the gather kernel), and the scalar form that maps starting 4 bytes off a 16-byte boundary fall back to."""
    H, W = hw
    case = R.warp_case(hw, C)
    flow = case["flow"]
    try:
        for variant in ("gather", "staged", "auto"):
            hip.warp_set_variant(variant)
            for i in range(0, flow.shape[0], 2):
                sl = slice(i, i + 2)
                for feat_n in (1, 2):
                    for subset in SUBSETS + ("mul",):
                        call = lambda: hip.warp_bilinear(t(case["feat"][:feat_n]), t(flow[sl]), **dev_operands(case, subset, sl))
                        if variant == "staged" and (H * W) % 2:
                            with pytest.raises(hip.LsfaError):
                                call()
                        else:
                            check_warp(call().cpu().numpy(), hw, C, "flow", subset, feat_n, i)
        hip.warp_set_variant("auto")
        for i in range(0, flow.shape[0], 2):
            sl = slice(i, i + 2)
            for subset in SUBSETS:
                sub = "bn" if subset == "plain" else subset + "+bn"
                got = hip.warp_bilinear(t(case["feat"][:1]), t(flow[sl]), **dev_operands(case, sub, sl))
                check_warp(got.cpu().numpy(), hw, C, "flow", sub, 1, i)
            # misaligned `add` and `out`: the scalar gather kernel whatever the plane's size asks for
            hip.warp_set_variant("gather")
            n = 2 * C * H * W
            off4 = lambda: torch.empty(n + 1, device=DEV)[1:].view(2, C, H, W)
            kw = dev_operands(case, "res+add", sl)
            add, out = off4(), off4()
            assert add.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
            add.copy_(kw["add"])
            got = hip.warp_bilinear(t(case["feat"][:1]), t(flow[sl]), **dict(kw, add=add, out=out))
            assert got.data_ptr() == out.data_ptr()
            check_warp(got.cpu().numpy(), hw, C, "flow", "res+add", 1, i)
    finally:
        hip.warp_set_variant("auto")


@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("hw", R.SHAPES, ids=HW_IDS)
def test_warp_channels_last_kernels_on_the_edge_field(hip, hw, C):
    """lsfa_warp_bilinear_cl and its bn form on every operand subset.  Then the field whose non-finite cells are wild ones instead: every
    output is finite, and amax_out holds exactly max|out|."""
    case = R.warp_case(hw, C)
    for field in ("flow", "flow_wild"):
        flow = case[field]
        for i in range(0, flow.shape[0], 2):
            sl = slice(i, i + 2)
            for feat_n in (1, 2):
                for subset in SUBSETS + tuple("bn" if s == "plain" else s + "+bn" for s in SUBSETS):
                    if feat_n == 2 and "bn" in subset:
                        continue
                    slots = hip.amax_slots(1, DEV)[0] if field == "flow_wild" else None
                    got = hip.warp_bilinear_cl(t(nhwc(case["feat"][:feat_n])), t(flow[sl]), amax_out=slots, **dev_operands(case, subset, sl, cl=True))
                    got = got.permute(0, 3, 1, 2).cpu().numpy()
                    check_warp(got, hw, C, field, subset, feat_n, i)
                    if slots is not None:
                        assert np.isfinite(got).all()
                        assert slots.view(torch.float32).max().item() == float(np.abs(warp_want(hw, C, field, subset, feat_n)[0][sl]).max())


# ---- the deformable sampler --------------------------------------------------------------------------------------------------------------------------
def deform_want(hw, C, cfg):
    key = ("deform", hw, C, cfg)
    if key not in _want:
        pad, stride, dil, dg = cfg
        case = R.deform_case(hw, C, cfg)
        ref = R.deform_ref_f32(case["data"], case["offset"], 3, pad, stride, dil, dg)
        orc = oracle.deform_im2col(case["data"], case["offset"], 3, 3, pad, stride, dil, dg)
        assert np.isfinite(ref).all()
        ref.setflags(write=False)
        orc.setflags(write=False)
        _want[key] = (ref, orc)
    return _want[key]


def to_cl(col, N, C):
    """col (N, C * 9, Ho * Wo) -> the channels-last kernel's (N, Ho * Wo, 9 * C): col_cl[n, pixel, tap, c] == col[n, c * 9 + tap, pixel]"""
    return col.reshape(N, C, 9, -1).transpose(0, 3, 2, 1).reshape(N, -1, 9 * C)


def cl_channels(dg):
    """16: the power-of-two kernel; 12 (48 where four groups need a multiple of 16): the general one"""
    return (16, 12) if dg == 1 else (16, 48)


def deform_cl_ld(hip, data_cl, offset_cl, ld, shape, cfg, col):
    N, C, H, W, Ho, Wo = shape
    pad, stride, dil, dg = cfg
    ci, vp = ctypes.c_int, ctypes.c_void_p
    rc = hip.lib().lsfa_deform_im2col_cl_ld(vp(data_cl.data_ptr()), vp(offset_cl.data_ptr()), ci(ld), ci(N), ci(C), ci(H), ci(W), ci(3), ci(3), ci(pad),
                                            ci(stride), ci(dil), ci(dg), ci(Ho), ci(Wo), vp(col.data_ptr()), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    return col


def padded_rows(offset_cl, pad_value=np.nan):
    """(N, Ho, Wo, L) -> (N, Ho, Wo, L + 6) with NaN in the six channels no tap owns"""
    N, Ho, Wo, L = offset_cl.shape
    wide = np.full((N, Ho, Wo, L + 6), pad_value, np.float32)
    wide[..., :L] = offset_cl
    return wide


@pytest.mark.parametrize("cfg", R.DEFORM_CFGS, ids=CFG_IDS)
@pytest.mark.parametrize("hw", R.SHAPES, ids=HW_IDS)
def test_deform_kernels_on_the_edge_field(hip, hw, cfg):
    """every cell - wild and non-finite offsets included, which give exactly 0.0 - equals the numpy statement and the oracle bit for bit"""
    H, W = hw
    pad, stride, dil, dg = cfg
    for C in R.CHANNELS:
        case = R.deform_case(hw, C, cfg)
        ref, orc = deform_want(hw, C, cfg)
        got = hip.deform_im2col(t(case["data"]), t(case["offset"]), 3, 3, pad, stride, dil, dg).cpu().numpy()
        np.testing.assert_array_equal(got, ref)
        np.testing.assert_array_equal(got, orc)
    for C in cl_channels(dg):
        case = R.deform_case(hw, C, cfg)
        ref, orc = deform_want(hw, C, cfg)
        N, _, Ho, Wo = case["offset"].shape
        data_cl, offset_cl = t(nhwc(case["data"])), nhwc(case["offset"])
        got = hip.deform_im2col_cl(data_cl, t(offset_cl), 3, 3, pad, stride, dil, dg).cpu().numpy()
        np.testing.assert_array_equal(got, to_cl(ref, N, C))
        np.testing.assert_array_equal(got, to_cl(orc, N, C))
        wide = padded_rows(offset_cl)
        col = torch.full((N, Ho * Wo, 9 * C), float("nan"), device=DEV)
        got = deform_cl_ld(hip, data_cl, t(wide), wide.shape[3], (N, C, H, W, Ho, Wo), cfg, col).cpu().numpy()
        np.testing.assert_array_equal(got, to_cl(ref, N, C))


# ---- memory: no output depends on what lies around a map ------------------------------------------------------------------------------------------
# Every operand and output stands alone between two bands of a byte pattern (tests/guarded_arena.py): 0xFF reads as NaN, 0x7F as 3.39e38.
# A tap that reads past a map - row H of the last plane with weight 0, which is what `h_low > H - 1` in place of `>=` does for a
# coordinate of exactly H - 1 - multiplies a NaN by its weight and shows in the output; a store past a map shows in a band.
@pytest.mark.parametrize("pattern", ga.PATTERNS, ids=lambda p: "0x%02X" % p)
@pytest.mark.parametrize("hw", R.SHAPES, ids=HW_IDS)
def test_warp_on_the_edge_field_reads_and_writes_its_own_maps_only(hip, hw, pattern):
    """one call per layout (NCHW through 'auto', channels-last) for each pair of maps of the field, operands res + add"""
    C = 16
    case = R.warp_case(hw, C)
    flow = case["flow"]
    f32 = torch.float32
    for i in range(0, flow.shape[0], 2):
        sl = slice(i, i + 2)
        for cl in (False, True):
            arena = ga.Arena(pattern, device=DEV)
            put = lambda a, role: arena.place(a.shape, f32, role, values=torch.from_numpy(np.array(a, np.float32, order="C")))
            lay = nhwc if cl else (lambda a: a)
            kw = dict(res=put(case["res"][sl], "res"), res_w=put(case["res_w"], "res_w"), res_b=put(case["res_b"], "res_b"))
            kw["add_cl" if cl else "add"] = put(lay(case["add"][sl]), "add")
            feat, fl = put(lay(case["feat"][:1]), "feat"), put(flow[sl], "flow")
            with pytest.MonkeyPatch.context() as mp, ga.guarded_allocations(mp, arena):
                got = (hip.warp_bilinear_cl if cl else hip.warp_bilinear)(feat, fl, **kw)
            assert arena.record(got) is not None, "the output was not placed by the arena"
            arena.check()
            got = got.permute(0, 3, 1, 2) if cl else got
            check_warp(got.cpu().numpy(), hw, C, "flow", "res+add", 1, i)


@pytest.mark.parametrize("pattern", ga.PATTERNS, ids=lambda p: "0x%02X" % p)
@pytest.mark.parametrize("cfg", R.DEFORM_CFGS, ids=CFG_IDS)
@pytest.mark.parametrize("hw", R.SHAPES, ids=HW_IDS)
def test_deform_on_the_edge_field_reads_and_writes_its_own_maps_only(hip, hw, cfg, pattern):
    """one call per kernel: NCHW, channels-last power-of-two and general, and the padded-row entry (the padding holds the pattern too)"""
    H, W = hw
    pad, stride, dil, dg = cfg
    f32 = torch.float32
    for kernel, C in [("nchw", 16)] + [("cl", c) for c in cl_channels(dg)] + [("cl_ld", 16)]:
        case = R.deform_case(hw, C, cfg)
        ref, _ = deform_want(hw, C, cfg)
        N, _, Ho, Wo = case["offset"].shape
        arena = ga.Arena(pattern, device=DEV)
        put = lambda a, role: arena.place(a.shape, f32, role, values=torch.from_numpy(np.array(a, np.float32, order="C")))
        if kernel == "nchw":
            data, offset = put(case["data"], "data"), put(case["offset"], "offset")
            with pytest.MonkeyPatch.context() as mp, ga.guarded_allocations(mp, arena):
                got = hip.deform_im2col(data, offset, 3, 3, pad, stride, dil, dg)
            want = ref
        else:
            data = put(nhwc(case["data"]), "data")
            want = to_cl(ref, N, C)
            if kernel == "cl":
                offset = put(nhwc(case["offset"]), "offset")
                with pytest.MonkeyPatch.context() as mp, ga.guarded_allocations(mp, arena):
                    got = hip.deform_im2col_cl(data, offset, 3, 3, pad, stride, dil, dg)
            else:
                wide = padded_rows(nhwc(case["offset"]), np.frombuffer(bytes([pattern] * 4), np.float32)[0])
                offset = put(wide, "offset")
                got = deform_cl_ld(hip, data, offset, wide.shape[3], (N, C, H, W, Ho, Wo), cfg, arena.place((N, Ho * Wo, 9 * C), f32, "col"))
        assert arena.record(got) is not None, "the output was not placed by the arena"
        arena.check()
        np.testing.assert_array_equal(got.cpu().numpy(), want)
