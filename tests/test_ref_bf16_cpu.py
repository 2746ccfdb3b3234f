"""tests/ref_bf16.py - the specification tests/test_conv_bf16_gpu.py holds the one-piece convolution kernels to - pinned without a GPU:
bf16_rne to torch's cast bit for bit, conv_ref to a six-loop numpy statement, deconv_crop_ref to conv_transpose2d + slicing; an fp32
evaluation of the same products stays far inside both bounds at every shape the GPU tests use, a cut by truncation (or one dropped tap
of one pixel) leaves both; and the table of cases and forced plans reaches every one-piece kernel instantiation (lsfa_conv_plan_query:
host arithmetic, as in tests/test_conv_plan_cpu.py)."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_bf16
from test_conv_bf16_gpu import CASES, DECONVS, OWN, deconv_inputs_of, inputs_of

HERE = os.path.dirname(os.path.abspath(__file__))


def torch_bf16(a):
    """the rounding by torch's own cast: what bf16_rne must NOT be written with, and what it is compared with here"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_bf16_rne_is_torchs_cast_bit_for_bit():
    rs = np.random.RandomState(1)
    u = rs.randint(0, 2 ** 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    u = u[(u & 0x7F800000) != 0x7F800000]                    # finite patterns: every exponent, subnormals, both zeros
    assert u.size > 10 ** 6
    x = u.view(np.float32)
    np.testing.assert_array_equal(bits(ref_bf16.bf16_rne(x)), bits(torch_bf16(x)))
    # every pattern whose dropped half is exactly a tie, or one beside it
    hi = (rs.randint(0, 0x7F80, size=4096).astype(np.uint32) << 16) | (rs.randint(0, 2, size=4096).astype(np.uint32) << 31)
    for low in (0x7FFF, 0x8000, 0x8001):
        x = (hi | np.uint32(low)).view(np.float32)
        np.testing.assert_array_equal(bits(ref_bf16.bf16_rne(x)), bits(torch_bf16(x)))


def test_bf16_rne_hand_cases():
    one = lambda v: float(ref_bf16.bf16_rne(np.array([v], np.float32))[0])
    for s in (1.0, -1.0):
        assert one(s * (1 + 2.0 ** -8)) == s * 1.0                      # a tie: down to the even neighbour
        assert one(s * (1 + 3 * 2.0 ** -8)) == s * (1 + 2.0 ** -6)      # a tie: up to the even neighbour
        assert one(s * 1.9999999) == s * 2.0                            # a carry into the exponent
    assert one(2.0 ** -126) == 2.0 ** -126
    largest_finite = np.array([0x7F7F7FFF], np.uint32).view(np.float32)[0]      # just below the tie between the largest bf16 and 2^128
    first_to_inf = np.array([0x7F7F8000], np.uint32).view(np.float32)[0]
    assert one(largest_finite) == float(np.array([0x7F7F0000], np.uint32).view(np.float32)[0])
    assert one(first_to_inf) == np.inf and one(-first_to_inf) == -np.inf
    assert np.isnan(one(np.nan)) and one(np.inf) == np.inf and bits(ref_bf16.bf16_rne(np.float32(-0.0)))[()] == 0x80000000


@pytest.mark.parametrize("cut", [False, True])
def test_conv_ref_is_the_six_loop_statement(cut):
    """stride 2, dilation 2, padding (2, 1), bias + residual + LeakyReLU; the operands rounded by torch's cast"""
    rs = np.random.RandomState(3)
    N, H, W, Cin, Cout, kh, kw, stride, dil, pad = 1, 7, 8, 3, 2, 3, 2, 2, 2, (2, 1)
    x, w, b = rs.randn(N, H, W, Cin).astype(np.float32), rs.randn(Cout, Cin, kh, kw).astype(np.float32), rs.randn(Cout).astype(np.float32)
    sc, sh = (rs.uniform(0.5, 1.5, Cin).astype(np.float32), rs.randn(Cin).astype(np.float32)) if cut else (None, None)
    Ho, Wo = (H + 2 * pad[0] - dil * (kh - 1) - 1) // stride + 1, (W + 2 * pad[1] - dil * (kw - 1) - 1) // stride + 1
    res = rs.randn(N, Ho, Wo, Cout).astype(np.float32)
    xa = np.maximum(x * sc + sh, np.float32(0)) if cut else x
    assert xa.dtype == np.float32
    xr, wr = torch_bf16(xa).astype(np.float64), torch_bf16(w).astype(np.float64)
    want, want_abs = np.zeros((N, Ho, Wo, Cout)), np.zeros((N, Ho, Wo, Cout))
    for oy in range(Ho):
        for ox in range(Wo):
            for o in range(Cout):
                s, sa = float(b[o]) + float(res[0, oy, ox, o]), abs(float(b[o])) + abs(float(res[0, oy, ox, o]))
                for ky in range(kh):
                    for kx in range(kw):
                        for c in range(Cin):
                            iy, ix = oy * stride - pad[0] + ky * dil, ox * stride - pad[1] + kx * dil
                            if 0 <= iy < H and 0 <= ix < W:
                                s += xr[0, iy, ix, c] * wr[o, c, ky, kx]
                                sa += abs(xr[0, iy, ix, c] * wr[o, c, ky, kx])
                want[0, oy, ox, o], want_abs[0, oy, ox, o] = (s if s > 0 else 0.1 * s), sa
    ref, ref_abs = ref_bf16.conv_ref(x, w, b, stride, pad, dil, 2, residual=res, in_scale=sc, in_shift=sh)
    assert ref.shape == want.shape and ref.dtype == np.float64 and (want < 0).any() and (want > 0).any()
    np.testing.assert_allclose(ref, want, rtol=0, atol=1e-13)
    np.testing.assert_allclose(ref_abs, want_abs, rtol=0, atol=1e-13)
    assert np.array_equal(ref_bf16.conv_ref(x, w, None, stride, pad, dil, 1, in_scale=sc, in_shift=sh)[0],
                          np.maximum(ref_bf16.conv_ref(x, w, None, stride, pad, dil, 0, in_scale=sc, in_shift=sh)[0], 0))


def test_deconv_crop_ref_is_conv_transpose2d_plus_slicing():
    rs = np.random.RandomState(4)
    x, wt, b = rs.randn(2, 5, 6, 7).astype(np.float32), rs.randn(7, 3, 4, 4).astype(np.float32), rs.randn(3).astype(np.float32)
    xr, wr = torch.from_numpy(torch_bf16(x)).double(), torch.from_numpy(torch_bf16(wt)).double()
    for Hc, Wc in ((9, 11), (10, 12), (11, 13)):
        full = F.conv_transpose2d(xr.permute(0, 3, 1, 2), wr, torch.from_numpy(b).double(), stride=2)
        want = F.leaky_relu(full, 0.1)[:, :, 1:1 + Hc, 1:1 + Wc].permute(0, 2, 3, 1).numpy()
        want_abs = F.conv_transpose2d(xr.abs().permute(0, 3, 1, 2), wr.abs(), torch.from_numpy(b).double().abs(), stride=2)[:, :, 1:1 + Hc, 1:1 + Wc]
        ref, ref_abs = ref_bf16.deconv_crop_ref(x, wt, b, Hc, Wc, 2)
        np.testing.assert_allclose(ref, want, rtol=0, atol=1e-13)
        np.testing.assert_allclose(ref_abs, want_abs.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-13)


def _conv_with(cut_fn, d, dtype):
    """conv(cut_fn(x'), cut_fn(w)) + bias + residual, evaluated by F.conv2d in `dtype`, channels-last"""
    xa = torch.from_numpy(cut_fn(ref_bf16.input_at_the_cut(d["x"], d["in_scale"], d["in_shift"]))).to(dtype)
    y = F.conv2d(xa.permute(0, 3, 1, 2), torch.from_numpy(cut_fn(d["w"])).to(dtype), torch.from_numpy(d["bias"]).to(dtype), d["stride"], d["pad"], d["dil"])
    return (y.permute(0, 2, 3, 1) + torch.from_numpy(d["residual"]).to(dtype)).numpy()


@pytest.fixture(scope="module")
def refs():
    """(inputs, ref, ref_abs) of every case, computed once: bias + residual, no activation"""
    out = {}
    for name in CASES:
        d = inputs_of(name)
        out[name] = (d,) + ref_bf16.conv_ref(d["x"], d["w"], d["bias"], d["stride"], (d["pad"], d["pad"]), d["dil"], 0, residual=d["residual"],
                                             in_scale=d["in_scale"], in_shift=d["in_shift"])
    return out


def test_an_fp32_evaluation_of_the_reference_is_inside_both_bounds(refs):
    """F.conv2d in float32 on the rounded operands - exact products, fp32 sums in the library's order - at every shape of the GPU tests:
    inside the gamma bound (far inside: it is an a-priori bound, and roundings largely cancel; the ratios are printed) and the fp32 criterion"""
    worst = {}
    for name, (d, ref, ref_abs) in refs.items():
        worst[name] = ref_bf16.bound_ratios(_conv_with(ref_bf16.bf16_rne, d, torch.float32), ref, ref_abs, d["K"])
    for cin, cout, _, _ in DECONVS:
        x, wt, b = deconv_inputs_of(cin, cout)
        ref, ref_abs = ref_bf16.deconv_crop_ref(x, wt, b, 19, 32, 0)
        got = F.conv_transpose2d(torch.from_numpy(ref_bf16.bf16_rne(x)).permute(0, 3, 1, 2), torch.from_numpy(ref_bf16.bf16_rne(wt)), torch.from_numpy(b), stride=2)
        worst["deconv_%d_%d" % (cin, cout)] = ref_bf16.bound_ratios(got[:, :, 1:20, 1:33].permute(0, 2, 3, 1).numpy(), ref, ref_abs, 4 * cin)
    print(worst)
    assert all(g <= 1.0 and f < 1.0 for g, f in worst.values()), worst


@pytest.mark.parametrize("name", ["ring", "cut_256_64", "direct_3x3", "view_5x5_s2"])
def test_a_truncating_cut_and_a_dropped_tap_leave_both_bounds(refs, name):
    """what the comparison is for: operands cut by truncation instead of round-to-nearest-even (evaluated in float64: nothing but the cut
    differs) are outside the per-element bound (on 17 % to 97 % of the outputs of these shapes) and outside the fp32 criterion; and so is a
    result in which ONE input pixel's taps are missing (about 1 / (kh kw) of a few outputs' sums).  The ratios are printed."""
    d, ref, ref_abs = refs[name]
    trunc = lambda a: (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    got = _conv_with(trunc, d, torch.float64)
    err, bound = np.abs(got - ref), ref_bf16.ref64.gamma(d["K"] + 3, ref_bf16.U_FAITHFUL) * ref_abs
    r_gamma, r_fp32 = ref_bf16.bound_ratios(got, ref, ref_abs, d["K"])
    print(name, "truncation: outside the gamma bound on %.0f %% of the outputs, worst ratios %.1f / %.1f" % (100 * (err > bound).mean(), r_gamma, r_fp32))
    assert r_gamma > 1.0 and r_fp32 > 1.0             # (the longer K, the wider the a-priori bound: 3.6 x at K = 3200, 120 x at K = 256)
    dropped = dict(d, x=d["x"].copy())
    n, y, x = 0, d["x"].shape[1] // 2, d["x"].shape[2] // 2
    dropped["x"][n, y, x, :] = 0
    if d["in_scale"] is not None:                          # the cut-time activation of a zero is max(shift, 0): drop the pixel behind it instead
        dropped["in_scale"] = dropped["in_shift"] = None
        dropped["x"] = ref_bf16.input_at_the_cut(d["x"], d["in_scale"], d["in_shift"])
        dropped["x"][n, y, x, :] = 0
    got = _conv_with(ref_bf16.bf16_rne, dropped, torch.float64)
    r_gamma, r_fp32 = ref_bf16.bound_ratios(got, ref, ref_abs, d["K"])
    assert (got != ref).any()
    print(name, "one pixel's taps dropped: worst ratios %.1f / %.1f" % (r_gamma, r_fp32))
    assert r_gamma > 1.0 and r_fp32 > 1.0


def test_the_table_reaches_every_one_piece_kernel():
    """lsfa_conv_plan_query on every (case, forced plan) of the table, in a fresh process without lab switches: the instantiations named
    are all 24 four-wave one-piece ring kernels, the four eight-wave ones, the direct kernel, and - chosen by the plan itself - the
    three-stage 128 x 128 ring and, with in_scale, the two-stage one (the stage fix of plan_of)."""
    spec = importlib.util.spec_from_file_location("make_conv_plans", os.path.join(HERE, "golden", "make_conv_plans.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    fields = ["N", "H", "W", "Cin", "Cout", "kh", "stride", "pad_h", "dil", "in_scale", "x_nchw", "y_nchw", "lda", "pieces"]
    groups = [{"factors": [[fields, [tuple(c.get(f, rec.DEFAULTS[f]) if f != "pieces" else 1 for f in fields)]], [rec.FORCE[:4], [list(p) for p in c["plans"]]]]}
              for c in CASES.values()]
    b = lambda v: "true" if v else "false"
    names, own = set(), {}
    for (case, c), answers in zip(CASES.items(), rec.eval_in_child(groups, {})):
        assert len(answers) == len(c["plans"])
        for plan, (rc, kind, nt, st, sp, wv, slices, af, pieces, _) in zip(c["plans"], answers):
            assert rc == 0 and pieces == 1, (case, plan)
            name = "conv_split_direct_kernel<1>" if kind == 2 else "conv_ring_kernel<%d, 1, %d, %s, %s, %d>" % (nt, st, b(sp), b(af), wv)
            names.add(name)
            if tuple(plan) == OWN:
                own[case] = name
            elif plan[0] != 4:
                assert (nt, st, slices) == tuple(plan[1:]) and sp == (plan[0] == 2) and wv == 4, (case, plan, name)      # the forced plan is what runs
            else:
                assert (nt, st, slices, wv) == (4, plan[2], plan[3], 8), (case, plan, name)
    need = {"conv_ring_kernel<%d, 1, %d, %s, %s, 4>" % (nt, st, b(sp), b(af)) for nt in (2, 4) for st in (2, 3, 4) for sp in (0, 1) for af in (0, 1)}
    need |= {"conv_ring_kernel<4, 1, %d, false, %s, 8>" % (st, b(af)) for st in (2, 3) for af in (0, 1)}
    need |= {"conv_split_direct_kernel<1>"}
    assert len(need) == 29 and not (need - names), sorted(need - names)
    assert own["own_128x128"] == "conv_ring_kernel<4, 1, 3, false, false, 4>" and own["own_128x128_cut"] == "conv_ring_kernel<4, 1, 2, false, true, 4>"
    assert own["direct_3x3"] == own["direct_kmajor"] == "conv_split_direct_kernel<1>"
