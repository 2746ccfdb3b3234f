"""The asymmetric ring of conv_ring_kernel<4, 2, 2, false, false, 4> (conv_ring_kernel.h, ring_step_deep_a): two stages of B, three of A.

The kernel is forced with lsfa_conv_plan_override (kernel 1 = mixed roles, nt 4, st 2) onto small maps.  Every case is held to
  * bit-identity with the same convolution on two other plans - loader / consumer waves on a three-stage ring, and 128 x 64 tiles:
    the ring only changes where a chunk waits and how far ahead it was fetched, never a product or the order of a sum;
  * the float64 criterion of the family: |y - ref| <= 2e-6 sqrt(K) max(max|ref|, 1) against a float64 torch convolution.
The K walks (1, 2, 3, 4, 5, 12, 13, 25 chunks of 32) cover prologues shorter than the ring (A(1), A(2) past the slice's end), the turn of
the six (B stage, A stage) pairs, the kFlush boundary and one chunk past it.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KERNEL = "conv_ring_kernel<4, 2, 2, false, false, 4>"
UNDER_TEST = dict(kernel=1, nt=4, st=2)
OTHER_PLANS = (dict(kernel=2, nt=4, st=3), dict(kernel=1, nt=2, st=3))      # loader / consumer waves, three stages; 128 x 64 tiles

# (id, H, W, Cin, Cout, k, stride, pad, dil, slices, extras)
K_WALKS = [("k%02d_chunks" % c, 10, 13, 32 * c, 128, 1, 1, 0, 1, 1, False) for c in (1, 2, 3, 4, 5, 12, 13, 25)]
OTHERS = [
    ("3x3_pad1_cout256", 19, 32, 64, 256, 3, 1, 1, 1, 1, False),
    ("3x3_pad6_dil6", 19, 32, 32, 128, 3, 1, 6, 6, 1, False),
    ("3x3_stride2", 19, 32, 96, 128, 3, 2, 1, 1, 1, False),
    ("1x1_stride2_cout256", 19, 32, 160, 256, 1, 2, 0, 1, 1, False),
    ("3x3_two_slices", 10, 13, 128, 128, 3, 1, 1, 1, 2, False),
    ("1x1_residual_out2", 19, 32, 416, 256, 1, 1, 0, 1, 1, True),
    ("3x3_residual_out2_two_slices", 10, 13, 96, 128, 3, 1, 1, 1, 2, True),
]
CASES = K_WALKS + OTHERS


def _run(hip, plan, slices, x, sw, bias, stride, pad, dil, am, extras):
    hip.conv_plan_override(slices=slices, **plan)
    status = hip.new_status(DEV)
    if extras is None:
        out = (hip.conv_split(x, sw, bias, stride, pad, dil, amax_in=am, status=status),)
    else:
        res, sc2, sh2 = extras
        slots = hip.amax_slots(1, DEV)[0]
        y, y2 = hip.conv_split(x, sw, bias, stride, pad, dil, residual=res, out2=torch.empty_like(res), scale2=sc2, shift2=sh2,
                               amax_in=am, amax_out=slots, status=status)
        out = (y, y2, slots)
    hip.check_status(status)
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_deep_a_ring_matches_the_other_plans_and_float64(hip, case):
    _, H, W, ci, co, k, stride, pad, dil, slices, with_extras = case
    g = torch.Generator(device=DEV).manual_seed(1400 + H * W + ci + co + k + stride + dil)
    x = torch.relu(torch.randn((1, H, W, ci), device=DEV, generator=g)) * 2.0
    w = torch.randn((co, ci, k, k), device=DEV, generator=g) * (1.0 / (ci * k * k) ** 0.5)
    b = torch.randn(co, device=DEV, generator=g)
    ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double().cpu(), w.double().cpu(), b.double().cpu(), stride=stride, padding=pad, dilation=dil)
    extras = None
    if with_extras:
        res = torch.randn((1, ref.shape[2], ref.shape[3], co), device=DEV, generator=g)
        extras = (res, torch.rand(co, device=DEV, generator=g) + 0.5, torch.randn(co, device=DEV, generator=g))
        ref = ref + res.permute(0, 3, 1, 2).double().cpu()
    ref = ref.permute(0, 2, 3, 1)
    P = ref.shape[1] * ref.shape[2]
    assert P % 128 != 0 and P > 128, "a last pixel tile that is not full, and more than one workgroup"
    sw = hip.SplitWeight(w, pieces=2)
    am = hip.amax_partial(x)
    K = ci * k * k
    tol = 2e-6 * K ** 0.5 * max(float(ref.abs().max()), 1.0)
    try:
        hip.conv_flops_reset(True)
        got = _run(hip, UNDER_TEST, slices, x, sw, b, stride, pad, dil, am, extras)
        names = list(hip.conv_by_kernel())
        hip.conv_flops_reset(False)
        assert names == [KERNEL + (" +split_reduce" if slices > 1 else "")], names      # the launch under test IS the asymmetric ring's kernel
        y = got[0]
        assert tuple(y.shape) == tuple(ref.shape)
        err = float((y.double().cpu() - ref).abs().max())
        print("%s: K %d, max|y - ref| %.3e, bound %.3e" % (case[0], K, err, tol))
        assert err <= tol, (case[0], err, tol)
        if with_extras:
            assert torch.equal(got[1], torch.relu(y * extras[1] + extras[2]))
            assert got[2].view(torch.float32).max().item() == got[1].max().item()
        for plan in OTHER_PLANS:
            other = _run(hip, plan, slices, x, sw, b, stride, pad, dil, am, extras)
            for t_new, t_other in zip(got[:2], other[:2]):      # the output and the second output
                assert torch.equal(t_new, t_other), (case[0], plan)
            if with_extras:      # (which workgroup publishes into which amax slot follows the tile grid: the slots' maximum is the plan-independent figure)
                assert got[2].view(torch.float32).max().item() == other[2].view(torch.float32).max().item(), (case[0], plan)
    finally:
        hip.conv_flops_reset(False)
        hip.conv_plan_override()
