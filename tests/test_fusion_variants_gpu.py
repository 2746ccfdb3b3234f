"""The small net's fuse variants on the GPU (small_net_fuse_type add / addv2 / concat / concatv1 / concatv2, stride 4 / 8, cur_scale,
bn_before_fuse): the new kernels against numpy restatements of their documented order, the non-key graph of every variant against a
CPU statement composed here from oracle.graph_ref's pieces (float32 and float64), the exact-fp32 and bf16 modes, hipGraph replay, the
batched pipeline, the no-library-kernel guard and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from oracle import e2e, graph_ref
from parity_util import np_, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
TOL_DENSE = 2e-5          # as tests/test_parity_fullres_gpu.py
TOL_SCORE = 1e-4
TOL_BOX_PX_BACKSTOP = 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- weights ---------------------------------------------------------------------------------------------------------------------------
def variant_cfg(fuse, stride=4, scale=False, bn=False, interval=10):
    from lsfa_amd.config.config import lsfa_test_config
    cfg = lsfa_test_config(interval)
    n = cfg.network
    n.small_net_fuse_type, n.small_net_stride, n.small_net_scale_before_fuse, n.small_net_bn_before_fuse = fuse, stride, scale, bn
    return cfg


def variant_params(base_arg, base_aux, cfg, seed=11):
    """The base (key-frame) weights + every layer of the variant's non-key symbol, the fuse layers re-drawn so that they do real work:
    convolutions at unit gain, BatchNorm statistics away from identity, gate pre-activations spread so that s covers ~(0.05, 0.95)."""
    from lsfa_amd.symbols import params as P
    arg, aux = dict(base_arg), dict(base_aux)
    carg, caux = P.init_params(cfg, seed=0)
    sarg, saux = P.cur_symbol_spec(cfg)
    rs = np.random.RandomState(seed)
    for k in sarg:
        if k not in arg:
            arg[k] = carg[k].copy()
    for k in saux:
        if k not in aux:
            aux[k] = caux[k].copy()
    for k, shp in sarg.items():
        if not k.startswith(('cur_scale', 'fuse_reduce', 's_feat_', 'cur_feat_bn', 'warp_conv_feat_bn')):
            continue
        if k.endswith('_weight'):
            fan = float(np.prod(shp[1:]))
            g = 0.5 if k.startswith('s_feat_conv2') else 1.0
            arg[k] = (rs.randn(*shp) * g / np.sqrt(fan)).astype(np.float32)
        elif k.endswith('_gamma'):
            arg[k] = rs.uniform(0.5, 1.5, shp).astype(np.float32)
        elif k.endswith('_beta'):
            arg[k] = (rs.randn(*shp) * 0.2).astype(np.float32)
        elif k.startswith('s_feat_conv2') and k.endswith('_bias'):
            arg[k] = rs.uniform(-2.5, 2.5, shp).astype(np.float32)
        elif k.endswith('_bias'):
            arg[k] = (rs.randn(*shp) * 0.05).astype(np.float32)
    for k, shp in saux.items():
        if k.startswith(('cur_feat_bn', 'warp_conv_feat_bn')):
            aux[k] = (rs.randn(*shp) * 0.2).astype(np.float32) if k.endswith('_mean') else rs.uniform(0.5, 2.0, shp).astype(np.float32)
    return arg, aux


# ---- the CPU statement of the non-key frame ----------------------------------------------------------------------------------------------
def ref_fuse(cfg, arg, aux, data, feat_key, mv, res, im_info, dtype=torch.float32):
    """get_cur_test_symbol (:553-659) with fuse_small_net (:209-274), composed from graph_ref's pieces + torch.nn.functional."""
    net = cfg.network
    p = graph_ref.Params(arg, aux, dtype)
    with torch.no_grad():
        x = p.T(data)
        if net.small_net_stride == 4:
            cur = graph_ref.resnet_backbone(p, F.avg_pool2d(x, 4, 4, ceil_mode=True), 'small_net_', True, False, 1)[0]
        else:
            cur = graph_ref.resnet_backbone(p, F.avg_pool2d(x, 2, 2, ceil_mode=True), 'small_net_', True, False, 2)[1]
        if net.small_net_scale_before_fuse:
            cur = p.conv(cur, 'cur_scale', 1)
        warp = p.T(oracle.warp_bilinear(np.asarray(feat_key, np.float32), mv, res=res, res_w=arg['rnet_conv0_weight'], res_b=arg['rnet_conv0_bias']))
        fuse, bn = net.small_net_fuse_type, net.small_net_bn_before_fuse

        def gate(v):
            m = v.mean((2, 3), keepdim=True)
            return torch.sigmoid(p.conv(F.relu(p.conv(m, 's_feat_conv1', 1)), 's_feat_conv2', 1))
        if fuse in ('add', 'addv2'):
            if fuse == 'add':
                cur = p.conv(cur, 'fuse_reduce_add', 3)
            else:
                cur = p.conv(F.relu(p.conv(cur, 'fuse_reduce_add_conv1', 3)), 'fuse_reduce_add_conv2', 1)
            if bn:
                cur, warp = p.bn(cur, 'cur_feat_bn'), p.bn(warp, 'warp_conv_feat_bn')
            out = cur + warp
        elif fuse in ('concat', 'concatv1'):
            c1, c2 = p.conv(cur, 'fuse_reduce_c1', 3), p.conv(warp, 'fuse_reduce_c2', 3)
            out = p.conv(torch.cat([c2, c1], 1), 'fuse_reduce', 3)
            if fuse == 'concatv1':
                out = F.relu(out)
                out = out * gate(out) + out
        else:
            c1 = p.conv(cur, 'fuse_reduce_c1', 3)
            out = c1 * gate(torch.cat([warp, c1], 1)) + warp
        r = dict(conv_feat=out.numpy())
        prob, bbox, cls_map, box_map = graph_ref.head_maps(p, out, cfg)
        r.update(rpn_cls_prob=prob.numpy(), rpn_bbox_pred=bbox.numpy(), cls_map=cls_map.numpy(), box_map=box_map.numpy())
        rois, cls_prob, bbox_pred = graph_ref.detect_from_maps(prob, bbox, cls_map, box_map,
                                                               im_info, cfg, r)
        r.update(rois_output=rois, cls_prob_reshape_output=cls_prob[None], bbox_pred_reshape_output=bbox_pred[None])
        return r


def _bind(cfg, arg, aux, dtype=torch.float32, pieces=None):
    from lsfa_amd.symbols.resnet_v1_101_flownet_rfcn import resnet_v1_101_flownet_rfcn
    return resnet_v1_101_flownet_rfcn(cfg).get_cur_test_symbol(cfg).bind(arg, aux, DEV, dtype, pieces)


def _key_world(H, W, clip_seed=0):
    """the key frame 0 once (GPU, fp32 and float64 statements): only the non-key path differs between variants"""
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.symbols import params as P
    from lsfa_amd.symbols.resnet_v1_101_flownet_rfcn import resnet_v1_101_flownet_rfcn
    from lsfa_amd.utils.synthetic import SyntheticClip
    cfg = lsfa_test_config(10)
    arg, aux = P.init_params(cfg, seed=0)
    key = resnet_v1_101_flownet_rfcn(cfg).get_key_test_symbol(cfg).bind(arg, aux, DEV)
    clip = SyntheticClip(clip_seed, 12, H, W)
    im_info = clip.im_info()
    f0 = clip.frame(0)
    out0 = key.forward(data=f0.to(DEV), im_info=torch.from_numpy(im_info).to(DEV), data_key_old=f0.to(DEV),
                       feat_key_old=torch.zeros(1, 1024, 1, 1, device=DEV))
    z = np.zeros((1, 1024, 1, 1), np.float32)
    ref0 = graph_ref.key_forward(cfg, arg, aux, f0.numpy(), f0.numpy(), z, im_info)
    d0 = graph_ref.key_forward(cfg, arg, aux, f0.numpy(), f0.numpy(), z, im_info, dtype=F64)
    return dict(cfg=cfg, arg=arg, aux=aux, key=key, clip=clip, im_info=im_info, feat0=out0['choose_feat_output'].clone(),
                ref_feat0=ref0['choose_feat_output'], d_feat0=d0['choose_feat_output'], H=H, W=W)


@pytest.fixture(scope="module")
def small_world():
    return _key_world(192, 320)


@pytest.fixture(scope="module")
def full_world():
    return _key_world(600, 1000)


def _frame_check(w, cfg, f=3):
    """non-key frame f of the world's clip: GPU vs the fp32 statement (conv_feat) and the float64-anchored end-to-end criterion"""
    arg, aux = variant_params(w['arg'], w['aux'], cfg)
    cur = _bind(cfg, arg, aux)
    clip, im_info = w['clip'], w['im_info']
    data, mv, res = clip.frame(f), clip.motion_vector(f, 0), clip.res_diff(f)
    cur.taps = {}
    out = cur.forward(data=data.to(DEV), im_info=torch.from_numpy(im_info).to(DEV), feat_key=w['feat0'], motion_vector=mv.to(DEV),
                      res_diff=res.to(DEV))
    torch.cuda.synchronize()
    cur.check_status()
    taps = dict(cur.taps)
    ref = ref_fuse(cfg, arg, aux, data.numpy(), w['ref_feat0'], mv.numpy(), res.numpy(), im_info)
    d64 = ref_fuse(cfg, arg, aux, data.numpy(), w['d_feat0'], mv.numpy(), res.numpy(), im_info, dtype=F64)
    gap = e2e.frame_gap(cfg, e2e.gpu_side(cfg, taps, out, im_info), ref, d64, im_info, w['H'], w['W'])
    return dict(cur=cur, arg=arg, aux=aux, out=out, taps=taps, ref=ref, d64=d64, gap=gap,
                dense=rel_err(np_(out['conv_feat']), ref['conv_feat']))


# ---- 1. kernels ---------------------------------------------------------------------------------------------------------------------------
def np_channel_mean(x, chunk=16):
    """lsfa_channel_mean's order (include/lsfa_hip.h): sequential fp32 sums over runs of 16 pixels, the runs added in order, / HW"""
    N, H, W, C = x.shape
    x = x.reshape(N, H * W, C).astype(np.float32)
    parts = []
    for p0 in range(0, H * W, chunk):
        acc = np.zeros((N, C), np.float32)
        for p in range(p0, min(p0 + chunk, H * W)):
            acc = (acc + x[:, p]).astype(np.float32)
        parts.append(acc)
    s = parts[0]
    for q in parts[1:]:
        s = (s + q).astype(np.float32)
    return (s / np.float32(H * W)).astype(np.float32)


def test_channel_mean_bit_exact_single_and_concatenated():
    from lsfa_amd import hip
    g = torch.Generator().manual_seed(1)
    for (N, H, W, C1, C2) in ((1, 7, 9, 64, 0), (3, 13, 11, 1024, 1024), (2, 38, 63, 512, 512)):
        x1 = torch.randn(N, H, W, C1, generator=g) * 3 + 1
        x2 = torch.randn(N, H, W, C2, generator=g) - 2 if C2 else None
        m = hip.channel_mean(x1.to(DEV), None if x2 is None else x2.to(DEV))
        want = np_channel_mean(x1.numpy() if x2 is None else np.concatenate([x1.numpy(), x2.numpy()], 3))
        np.testing.assert_array_equal(np_(m), want)
        # the same bits image by image (batch independence) and on a second run
        for n in range(N):
            mn = hip.channel_mean(x1[n:n + 1].to(DEV), None if x2 is None else x2[n:n + 1].to(DEV))
            assert torch.equal(mn[0], m[n])
        assert torch.equal(hip.channel_mean(x1.to(DEV), None if x2 is None else x2.to(DEV)), m)


def test_gate_apply_bit_exact_with_amax():
    from lsfa_amd import hip
    g = torch.Generator().manual_seed(2)
    N, H, W, C = 3, 9, 13, 1024
    x, y = torch.randn(N, H, W, C, generator=g) * 4, torch.randn(N, H, W, C, generator=g)
    s = torch.rand(N, C, generator=g)
    slots = hip.amax_slots(1, DEV)
    out = hip.gate_apply(x.to(DEV), s.to(DEV), y.to(DEV), amax_out=slots[0], amax_c0=512)
    prod = (x.numpy() * s.numpy()[:, None, None, :]).astype(np.float32)
    want = (prod + y.numpy()).astype(np.float32)
    np.testing.assert_array_equal(np_(out), want)
    amax = float(slots[0].view(torch.float32).max())
    assert amax == float(np.abs(want[..., 512:]).max())
    same = hip.gate_apply(x.to(DEV), s.to(DEV), x.to(DEV))        # concatv1's x = y
    np.testing.assert_array_equal(np_(same), ((x.numpy() * s.numpy()[:, None, None, :]).astype(np.float32) + x.numpy()).astype(np.float32))


def test_gate_within_a_few_ulps_of_float64_and_batch_invariant():
    from lsfa_amd import hip
    g = torch.Generator().manual_seed(3)
    for K in (1024, 2048):
        N = 11
        m = torch.randn(N, K, generator=g)
        w1, b1 = torch.randn(1024, K, generator=g) / K ** 0.5, torch.randn(1024, generator=g) * 0.1
        w2, b2 = torch.randn(1024, 1024, generator=g) * 0.5 / 32, torch.rand(1024, generator=g) * 5 - 2.5
        s = hip.channel_gate(m.to(DEV), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV))
        h = torch.relu(m.double() @ w1.double().T + b1.double())
        want = torch.sigmoid(h @ w2.double().T + b2.double())
        ulp = np.spacing(np.float32(want.numpy()).astype(np.float32))
        err = np.abs(np_(s).astype(np.float64) - want.numpy()) / ulp
        assert err.max() <= 16, err.max()
        assert float(want.min()) < 0.2 and float(want.max()) > 0.8
        for n in (0, 5, 10):
            sn = hip.channel_gate(m[n:n + 1].to(DEV), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV))
            assert torch.equal(sn[0], s[n])
        assert torch.equal(hip.channel_gate(m.to(DEV), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV)), s)


def test_warp_with_batchnorm_bit_exact_in_both_layouts():
    from lsfa_amd import hip
    g = torch.Generator().manual_seed(4)
    N, C, H, W = 3, 1024, 19, 31
    feat = torch.randn(1, C, H, W, generator=g)
    flow = torch.randn(N, 2, H, W, generator=g) * 3
    flow[:, :, :2] += 40.0                                           # taps outside the map (the shift must not leak into them)
    res = torch.randn(N, 3, H, W, generator=g)
    rw, rb = torch.randn(C, 3, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    add = torch.randn(N, C, H, W, generator=g)
    sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    w = oracle.warp_bilinear(feat.numpy(), flow.numpy(), add=None, res=res.numpy(), res_w=rw.numpy(), res_b=rb.numpy())
    want = ((w * sc.numpy()[None, :, None, None]).astype(np.float32) + sh.numpy()[None, :, None, None]).astype(np.float32)
    want = (want + add.numpy()).astype(np.float32)
    t = lambda a: a.to(DEV)
    got = hip.warp_bilinear(t(feat), t(flow), add=t(add), res=t(res), res_w=t(rw), res_b=t(rb), bn=(t(sc), t(sh)))
    np.testing.assert_array_equal(np_(got), want)
    slots = hip.amax_slots(1, DEV)
    got_cl = hip.warp_bilinear_cl(t(feat.permute(0, 2, 3, 1).contiguous()), t(flow), add_cl=t(add.permute(0, 2, 3, 1).contiguous()),
                                  res=t(res), res_w=t(rw), res_b=t(rb), amax_out=slots[0], amax_c0=512, bn=(t(sc), t(sh)))
    np.testing.assert_array_equal(np_(got_cl).transpose(0, 3, 1, 2), want)
    assert float(slots[0].view(torch.float32).max()) == float(np.abs(want[:, 512:]).max())


# ---- 2. graph parity at 192x320 ------------------------------------------------------------------------------------------------------------
SMALL_VARIANTS = [('add', 4, False, False), ('addv2', 4, False, False), ('concat', 4, False, False), ('concatv1', 4, False, False),
                  ('concatv2', 4, False, False), ('add', 8, False, False), ('concatv2', 8, False, False), ('add', 4, True, True),
                  ('addv2', 4, True, True)]


@pytest.mark.parametrize("fuse,stride,scale,bn", SMALL_VARIANTS)
def test_variant_graph_parity_at_192x320(small_world, fuse, stride, scale, bn):
    cfg = variant_cfg(fuse, stride, scale, bn)
    r = _frame_check(small_world, cfg)
    assert r['out']['conv_feat'].shape == (1, 1024, 12, 20)
    assert r['dense'] < TOL_DENSE, r['dense']
    assert not r['gap']['failures'], r['gap']
    assert r['gap']['max_abs_dscore'] <= TOL_SCORE, r['gap']
    if fuse in ('concatv1', 'concatv2'):
        s = np_(r['taps']['gate'])
        assert s.min() < 0.1 and s.max() > 0.9, (s.min(), s.max())     # the gate does real work


# ---- 3. graph parity at 1000x600 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse,stride,scale,bn", [('concatv2', 4, False, False), ('addv2', 4, True, True)])
def test_variant_graph_parity_at_1000x600(full_world, fuse, stride, scale, bn):
    cfg = variant_cfg(fuse, stride, scale, bn)
    r = _frame_check(full_world, cfg)
    assert r['dense'] < TOL_DENSE, r['dense']
    e = r['gap']
    assert not e['failures'], e
    assert e['max_abs_dscore'] <= TOL_SCORE, e
    assert e['rois_compared'] >= 250, e
    assert e['max_abs_dbox'] <= TOL_BOX_PX_BACKSTOP, e


# ---- 4. modes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse,scale,bn", [('concatv2', False, False), ('addv2', True, True)])
def test_exact_fp32_and_bf16_modes_at_1000x600(full_world, fuse, scale, bn):
    w = full_world
    cfg = variant_cfg(fuse, 4, scale, bn)
    arg, aux = variant_params(w['arg'], w['aux'], cfg)
    clip, im_info = w['clip'], w['im_info']
    data, mv, res = clip.frame(3), clip.motion_vector(3, 0), clip.res_diff(3)
    inp = dict(data=data.to(DEV), im_info=torch.from_numpy(im_info).to(DEV), feat_key=w['feat0'], motion_vector=mv.to(DEV), res_diff=res.to(DEV))
    exact = _bind(cfg, arg, aux, pieces=0)
    exact.taps = {}
    out = exact.forward(**inp)
    ref = ref_fuse(cfg, arg, aux, data.numpy(), w['ref_feat0'], mv.numpy(), res.numpy(), im_info)
    d64 = ref_fuse(cfg, arg, aux, data.numpy(), w['d_feat0'], mv.numpy(), res.numpy(), im_info, dtype=F64)
    e = e2e.frame_gap(cfg, e2e.gpu_side(cfg, exact.taps, out, im_info), ref, d64, im_info, w['H'], w['W'])
    assert not e['failures'], e
    two = _bind(cfg, arg, aux)
    a, b = np_(out['conv_feat']), np_(two.forward(**inp)['conv_feat'])
    assert rel_err(b, a) < TOL_DENSE
    bf = _bind(cfg, arg, aux, dtype=torch.bfloat16)
    ob = bf.forward(**inp)
    torch.cuda.synchronize()
    bf.check_status()
    for k in ('conv_feat', 'cls_prob_reshape_output', 'bbox_pred_reshape_output'):
        assert bool(torch.isfinite(ob[k]).all()), k
    assert rel_err(np_(ob['conv_feat']), ref['conv_feat']) < 0.08


# ---- 5. pipeline ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse,scale,bn", [('concatv2', False, False), ('addv2', True, True), ('concat', False, False)])
def test_graph_replay_equals_eager(small_world, fuse, scale, bn):
    from lsfa_amd.core.graphs import FrameGraphs
    w = small_world
    cfg = variant_cfg(fuse, 4, scale, bn, interval=4)
    arg, aux = variant_params(w['arg'], w['aux'], cfg)
    cur = _bind(cfg, arg, aux)
    from lsfa_amd.symbols.resnet_v1_101_flownet_rfcn import resnet_v1_101_flownet_rfcn
    key = resnet_v1_101_flownet_rfcn(cfg).get_key_test_symbol(cfg).bind(arg, aux, DEV)
    clip = w['clip']
    runs = []
    for graphs in (False, True):
        fg = FrameGraphs(key, cur, cfg, w['H'], w['W'], DEV, use_graphs=graphs, taps=True)
        assert fg.small_cur.shape[1] == cur.small_net_channels
        fg.first_frame(clip.frame(0, DEV), next_data=clip.frame(1, DEV))
        fg.capture()
        got = []
        for f in (1, 2, 3):
            fg.cur_frame(clip.frame(f, DEV), clip.motion_vector(f, 0, DEV), clip.res_diff(f, DEV), next_data=clip.frame(f + 1, DEV))
            got.append((fg.cur_out['conv_feat'].clone(), fg.post_bufs[0].clone(), fg.post_bufs[1].clone()))
        torch.cuda.synchronize()
        fg.close()
        runs.append(got)
        cur.check_status()
    for a, b in zip(*runs):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
        for j, c in enumerate(a[2].flatten().tolist()):            # detection rows up to each class's count (the rest is never written)
            assert torch.equal(a[1].reshape(-1, *a[1].shape[2:])[j, :c], b[1].reshape(-1, *b[1].shape[2:])[j, :c])
    # eager, frame 3 without the prefetch: the same bits as the graphs' frame 3
    cur.taps = None
    o = cur.forward(data=clip.frame(3, DEV), im_info=torch.tensor([[w['H'], w['W'], 1.0]], device=DEV), feat_key=_feat_of(key, clip, w),
                    motion_vector=clip.motion_vector(3, 0, DEV), res_diff=clip.res_diff(3, DEV))
    assert torch.equal(o['conv_feat'].contiguous(), runs[1][2][0].contiguous())


def _feat_of(key, clip, w):
    f0 = clip.frame(0, DEV)
    return key.forward(data=f0, im_info=torch.tensor([[w['H'], w['W'], 1.0]], device=DEV), data_key_old=f0,
                       feat_key_old=torch.zeros(1, 1024, 1, 1, device=DEV))['choose_feat_output']


@pytest.mark.parametrize("fuse,scale,bn", [('concatv2', False, False), ('addv2', False, True)])
def test_batched_pipeline_equals_hand_issued_passes(small_world, fuse, scale, bn):
    """FramePipeline(segment=9, key_group=2, lanes=2) with two clips in lock-step: every non-key frame as delivered equals the same segment pass
    issued by hand (bit for bit), and each image's conv_feat equals the frame run alone through the non-key graph (the gate is per image)."""
    from parity_util import clone_dict
    from lsfa_amd.core.graphs import FramePipeline
    from lsfa_amd.symbols.resnet_v1_101_flownet_rfcn import resnet_v1_101_flownet_rfcn
    from lsfa_amd.utils.synthetic import SyntheticClip
    w = small_world
    H, W = w['H'], w['W']
    cfg = variant_cfg(fuse, 4, scale, bn, interval=10)
    arg, aux = variant_params(w['arg'], w['aux'], cfg)
    key = resnet_v1_101_flownet_rfcn(cfg).get_key_test_symbol(cfg).bind(arg, aux, DEV)
    cur = _bind(cfg, arg, aux)
    B, K, Fs = 2, 10, 9
    clips = [SyntheticClip(5 + b, 21, H, W, K) for b in range(B)]
    cat = lambda fn: torch.cat([fn(c) for c in clips], 0)
    sched = [(f, 1 + K * ((f - 1) // K)) for f in range(1, 21)]      # keys 1, 11; segments 2-10, 12-20
    keys = [1, 11]
    frames = {f: cat(lambda c: c.frame(f, DEV)) for f in range(21)}
    mvs = {f: cat(lambda c: c.motion_vector(f, kf, DEV)) for f, kf in sched if f != kf}
    ress = {f: cat(lambda c: c.res_diff(f, DEV)) for f, kf in sched if f != kf}
    fp = FramePipeline(key, cur, cfg, H, W, DEV, lanes=2, taps=True, batch=B, segment=Fs, key_group=2)
    outs = {}

    def keep(f, is_key):
        def deliver(bufs):
            lane = fp.delivering
            if is_key:
                outs[f] = dict(feat=lane.feat.clone(), dets=bufs[0].clone(), counts=bufs[1].clone())
            else:
                _, i, n = bufs[0].lsfa_segment
                outs[f] = dict(out=clone_dict(lane.cur_out), index=i, dets=bufs[0].clone(), counts=bufs[1].clone())
        return deliver
    fp.first_frame(frames[0])
    fp.capture()
    for f, kf in sched:
        if f == kf:
            fp.key_frame(frames[f], deliver=keep(f, True), upcoming=[frames[k] for k in keys if k > f])
        else:
            fp.cur_frame(frames[f], mvs[f], ress[f], deliver=keep(f, False))
    fp.join()
    torch.cuda.synchronize()
    fp.close()
    cur.check_status()
    im_t = torch.tensor([[H, W, 1.0]] * (B * Fs), device=DEV)
    for k in keys:
        seg = list(range(k + 1, k + 1 + Fs))
        out = cur.forward(data=torch.cat([frames[f] for f in seg], 0), im_info=im_t, feat_key=outs[k]['feat'],
                          motion_vector=torch.cat([mvs[f] for f in seg], 0), res_diff=torch.cat([ress[f] for f in seg], 0))
        for i, f in enumerate(seg):
            assert outs[f]['index'] == i
            assert torch.equal(outs[f]['out']['conv_feat'], out['conv_feat']), f
    # per image: the mean and the gate do not look across the batch
    seg = list(range(2, 2 + Fs))
    for b in range(B):
        f = seg[4]
        one = cur.forward(data=frames[f][b:b + 1], im_info=im_t[:1], feat_key=outs[1]['feat'][b:b + 1], motion_vector=mvs[f][b:b + 1],
                          res_diff=ress[f][b:b + 1])
        full = outs[f]['out']['conv_feat'][4 * B + b:4 * B + b + 1]
        assert rel_err(np_(one['conv_feat']), np_(full)) < TOL_DENSE


# ---- 6. no library kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", ["concatv1", "concatv2"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fuse_variants_run_without_a_library_kernel(small_world, monkeypatch, fuse, dtype):
    w = small_world
    cfg = variant_cfg(fuse)
    arg, aux = variant_params(w['arg'], w['aux'], cfg)
    cur = _bind(cfg, arg, aux, torch.float32 if dtype == "f32" else torch.bfloat16)
    clip = w['clip']
    inp = dict(data=clip.frame(3, DEV), im_info=torch.from_numpy(w['im_info']).to(DEV), feat_key=w['feat0'],
               motion_vector=clip.motion_vector(3, 0, DEV), res_diff=clip.res_diff(3, DEV))

    def forbidden(*a, **k):
        raise AssertionError("a library kernel was called")
    for name in ("conv2d", "conv_transpose2d", "conv1d", "conv3d", "max_pool2d", "avg_pool2d", "adaptive_avg_pool2d", "unfold", "linear",
                 "softmax", "sigmoid"):
        monkeypatch.setattr(F, name, forbidden)
    for name in ("mm", "addmm", "matmul", "bmm", "baddbmm", "einsum", "softmax", "sigmoid", "mean", "cat"):
        monkeypatch.setattr(torch, name, forbidden)
    out = cur.forward(**inp)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert bool(torch.isfinite(out['conv_feat']).all())
    cur.check_status()


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------------------
def test_command_line_with_a_concatv2_yaml(tmp_path):
    src = os.path.join(ROOT, 'lsfa_amd', 'config', 'resnet_v1_101_flownet_imagenet_vid_rfcn_end2end_ohem.yaml')
    y = tmp_path / 'concatv2.yaml'
    y.write_text(open(src).read().replace("small_net_fuse_type: 'add'", "small_net_fuse_type: 'concatv2'"))
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable, '-m', 'lsfa_amd.test', '--cfg', str(y), '--clips', '2', '--frames', '24'], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    text = r.stdout + r.stderr
    assert 'detections' in text.lower() or 'mAP' in text or 'frames' in text.lower(), text[-2000:]
