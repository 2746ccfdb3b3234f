"""lsfa_conv_pair_fwd (hip.conv_pair): a ResNet unit's conv3 + shortcut add and the next unit's conv1 in one launch.

conv3's part is the ring kernel's arithmetic (same products, same order per accumulator): bit-identical to hip.conv_split under the unsliced
128 x 128 ring plan.  conv1's part cuts its operand with one scale per 32-pixel x 128-channel block instead of one per map and is held to
test_conv_split_vs_float64_and_fp32_mfma's criterion, teacher-forced on the GPU's own sum."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (N, H, W, Cm, C, Cn)
SHAPES = [
    (2, 13, 23, 64, 256, 64),       # two images, ragged last tile, P % 32 != 0
    (1, 19, 31, 64, 256, 128),      # the stage 1 -> stage 2 transition's widths
    (2, 14, 22, 128, 512, 128),     # stage 2
    (1, 5, 5, 64, 256, 64),         # fewer pixels than one tile
]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_case(shape, block_scales=False):
    N, H, W, Cm, C, Cn = shape
    g = torch.Generator().manual_seed(1000 * Cm + 10 * H + Cn)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    c = dict(shape=shape)
    # c2 like the network's: non-negative with a per-channel gain, a few exact zeros and tiny values
    x = torch.relu(rn(N, H, W, Cm)) * (0.1 + 2.9 * torch.rand(Cm, generator=g))
    x[0, 0, 0, :] = 1e-30
    res = rn(N, H, W, C)
    s2 = 0.5 + torch.rand(C, generator=g)
    h2 = 0.1 * rn(C)
    if block_scales:
        # the 128-channel blocks of the activated sum 2^20 apart, one block exactly zero behind the ReLU, one pixel row 2^12 above its block
        assert C == 512
        s2[128:256] *= 2.0 ** 20
        h2[128:256] *= 2.0 ** 20
        s2[256:384] = 0.0
        h2[256:384] = -1.0
        s2[384:512] *= 2.0 ** -20
        h2[384:512] *= 2.0 ** -20
        res[0, 3, 5, 0:128] *= 2.0 ** 12
    c['x'], c['res'], c['s2'], c['h2'] = x.to(DEV), res.to(DEV), s2.to(DEV), h2.to(DEV)
    c['w3'] = (rn(C, Cm, 1, 1) / np.sqrt(Cm)).to(DEV)
    c['w1'] = (rn(Cn, C, 1, 1) / np.sqrt(C)).to(DEV)
    c['b1'] = rn(Cn).to(DEV)
    return c


@pytest.fixture(scope="module")
def cases(hip):
    """per shape: the inputs, both weights, and ONE reference of conv3 under the forced ring plan (shared, never written to)"""
    out = {}
    for shape in SHAPES:
        c = make_case(shape)
        c['sw3'], c['sw1'] = hip.SplitWeight(c['w3'], pieces=2), hip.SplitWeight(c['w1'], pieces=2)
        c['am_in'] = hip.amax_partial(c['x'])
        slots = hip.amax_slots(1, DEV)[0]
        hip.conv_plan_override(kernel=1, nt=4, st=2, slices=1)
        try:
            c['y_ref'] = hip.conv_split(c['x'], c['sw3'], None, residual=c['res'], scale2=c['s2'], shift2=c['h2'], amax_in=c['am_in'], amax_out=slots)
        finally:
            hip.conv_plan_override()
        c['amax_ref'] = slots.view(torch.float32).max().item()
        out[shape] = c
    return out


def run_pair(hip, c, in_place):
    N, H, W, Cm, C, Cn = c['shape']
    res = c['res'].clone()
    slots, status = hip.amax_slots(2, DEV), hip.new_status(DEV)
    y, z = hip.conv_pair(c['x'], c['sw3'], res, c['s2'], c['h2'], c['sw1'], c['b1'], out=res if in_place else None, amax_in=c['am_in'],
                         amax_out_sum=slots[0], amax_out_z=slots[1], status=status)
    assert y.shape == (N, H, W, C) and z.shape == (N, H, W, Cn)
    assert (y.data_ptr() == res.data_ptr()) == in_place
    return y, z, slots, status


def conv1_errors(hip, c, y, z):
    """-> (error of z, error of the fp32-MFMA kernel, error of the unfused two-piece launch, the output scale), all against a float64
    convolution of max(y * s + t, 0) (fp32, two roundings) - the operand both launches see"""
    N, H, W, Cm, C, Cn = c['shape']
    a = torch.relu(y * c['s2'] + c['h2'])
    want = torch.relu(a.double().reshape(-1, C) @ c['w1'].double().reshape(Cn, C).t() + c['b1'].double()).reshape(N, H, W, Cn)
    scale = max(want.abs().max().item(), 1.0)
    ref32 = hip.conv_nhwc(a, hip.conv_weight_kc(c['w1']), c['b1'], 1, 1, 1, 0, 1, relu=True)
    two = hip.conv_split(a, c['sw1'], c['b1'], relu=True)
    err = lambda v: (v.double() - want).abs().max().item()
    return err(z), err(ref32), err(two), scale


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "separate"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv_pair(hip, cases, shape, in_place):
    c = cases[shape]
    C = shape[4]
    y, z, slots, status = run_pair(hip, c, in_place)
    # conv3: the same products in the same order per accumulator as the ring kernel
    assert torch.equal(y, c['y_ref'])
    assert slots[0].view(torch.float32).max().item() == c['amax_ref']
    # conv1, teacher-forced on the GPU's own y
    err, err_mfma, err_two, scale = conv1_errors(hip, c, y, z)
    print("conv_pair %s: err %.3e, fp32 mfma %.3e, two-launch %.3e, bound %.3e" % (shape, err, err_mfma, err_two, 2e-6 * np.sqrt(C) * scale))
    assert err < 2e-6 * np.sqrt(C) * scale
    assert err <= 1.5 * err_mfma + 1e-7 * scale, (err, err_mfma)
    assert err_two < 2e-6 * np.sqrt(C) * scale and err_two <= 1.5 * err_mfma + 1e-7 * scale, (err_two, err_mfma)
    # amax, status, repeatability
    assert slots[1].view(torch.float32).max().item() == z.abs().max().item()
    hip.check_status(status)
    y2, z2, slots2, _ = run_pair(hip, c, in_place)
    assert torch.equal(y2, y) and torch.equal(z2, z) and torch.equal(slots2, slots)


def test_conv_pair_block_scales(hip):
    """the blocks of the activated sum 2^20 apart, one exactly zero, one pixel row 2^12 above its block: every block is cut under its own scale"""
    c = make_case((2, 14, 22, 128, 512, 128), block_scales=True)
    c['sw3'], c['sw1'] = hip.SplitWeight(c['w3'], pieces=2), hip.SplitWeight(c['w1'], pieces=2)
    c['am_in'] = hip.amax_partial(c['x'])
    y, z, slots, status = run_pair(hip, c, False)
    a = torch.relu(y * c['s2'] + c['h2'])
    assert (a[..., 256:384] == 0).all() and a[..., 128:256].max().item() > 2.0 ** 30 * a[..., 384:512].max().item() > 0
    assert a[0, 3, 5, 0:128].max().item() > 2.0 ** 9 * a[0, 3, 6, 0:128].max().item()
    assert torch.isfinite(y).all() and torch.isfinite(z).all()
    hip.check_status(status)
    err, err_mfma, err_two, scale = conv1_errors(hip, c, y, z)
    print("conv_pair block scales: err %.3e, fp32 mfma %.3e, two-launch %.3e, bound %.3e" % (err, err_mfma, err_two, 2e-6 * np.sqrt(512) * scale))
    assert err < 2e-6 * np.sqrt(512) * scale
    assert slots[1].view(torch.float32).max().item() == z.abs().max().item()


def test_conv_pair_refusals(hip):
    """everything the entry point does not take raises LsfaError: piece counts other than two, C != 4 Cm, Cm or Cn outside {64, 128},
    views, NCHW, a stride"""
    def weights(Cm, C, Cn, pieces=2):
        g = torch.Generator().manual_seed(Cm + C + Cn)
        return (hip.SplitWeight(torch.randn(C, Cm, 1, 1, generator=g).to(DEV), pieces=pieces),
                hip.SplitWeight(torch.randn(Cn, C, 1, 1, generator=g).to(DEV), pieces=pieces))

    def call(Cm, C, Cn, sw3, sw1, x=None, out=None, out_z=None, **kw):
        x = torch.rand(1, 6, 7, Cm, device=DEV) if x is None else x
        res = torch.rand(1, 6, 7, C, device=DEV)
        return hip.conv_pair(x, sw3, res, torch.ones(C, device=DEV), torch.zeros(C, device=DEV), sw1, None, out=out, out_z=out_z, **kw)

    good = weights(64, 256, 64)
    call(64, 256, 64, *good)                                            # the plain call is taken
    for pieces in (3, 1):
        with pytest.raises(hip.LsfaError):
            call(64, 256, 64, *weights(64, 256, 64, pieces))
    with pytest.raises(hip.LsfaError):                                  # one of the two in another form
        call(64, 256, 64, good[0], weights(64, 256, 64, 3)[1])
    with pytest.raises(hip.LsfaError):                                  # C != 4 Cm
        call(64, 192, 64, *weights(64, 192, 64))
    with pytest.raises(hip.LsfaError):                                  # Cm outside {64, 128}
        call(32, 128, 64, *weights(32, 128, 64))
    with pytest.raises(hip.LsfaError):
        call(256, 1024, 128, *weights(256, 1024, 128))
    with pytest.raises(hip.LsfaError):                                  # Cn outside {64, 128}
        call(64, 256, 256, *weights(64, 256, 256))
    with pytest.raises(hip.LsfaError):                                  # x a channel slice of a wider map
        call(64, 256, 64, *good, x=torch.rand(1, 6, 7, 128, device=DEV)[..., :64])
    with pytest.raises(hip.LsfaError):                                  # y a channel slice of a wider map
        call(64, 256, 64, *good, out=torch.empty(1, 6, 7, 512, device=DEV)[..., :256])
    with pytest.raises(hip.LsfaError):                                  # z a channel slice of a wider map
        call(64, 256, 64, *good, out_z=torch.empty(1, 6, 7, 128, device=DEV)[..., :64])
    with pytest.raises(hip.LsfaError):
        call(64, 256, 64, *good, nchw=True)
    with pytest.raises(hip.LsfaError):
        call(64, 256, 64, *good, stride=2)
