"""Executor._resnet with a unit's conv3 and the next unit's conv1 as one launch (LSFA_PAIR_1X1 / Executor.pair_1x1) against the two-launch
form: the sums are the same arithmetic, conv1's operand scale is per block instead of per map - the stage outputs and the features agree
within the dense stages' bound (2e-5 of each map's maximum), and a captured graph replays the eager launches bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, W = 96, 160


@pytest.fixture(scope="module")
def world(hip):
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.symbols import params as P
    from lsfa_amd.symbols.resnet_v1_101_flownet_rfcn import resnet_v1_101_flownet_rfcn
    cfg = lsfa_test_config(key_frame_interval=10)
    arg, aux = P.init_params(cfg, seed=5)
    net = resnet_v1_101_flownet_rfcn(cfg)
    key = net.get_key_test_symbol(cfg).bind(arg, aux, DEV)
    cur = net.get_cur_test_symbol(cfg).bind(arg, aux, DEV)
    g = torch.Generator().manual_seed(11)
    data = (255.0 * torch.rand(2, 3, H, W, generator=g)).to(DEV)
    return dict(key=key, cur=cur, data=data)


def backbone(key, data, pair):
    key.pair_1x1, key.stage_taps = pair, {}
    feat = key._backbone(data).clone()
    taps, key.stage_taps = {k: v.clone() for k, v in key.stage_taps.items()}, None
    return feat, taps


def close(a, b, what):
    bound = 2e-5 * b.abs().max().item()
    err = (a - b).abs().max().item()
    print("%s: max |difference| %.3e, bound %.3e" % (what, err, bound))
    assert err <= bound, (what, err, bound)


def test_backbone_pair_vs_two_launches(world):
    key, data = world['key'], world['data']
    assert key.pieces == 2
    f0, t0 = backbone(key, data, 0)
    f2, t2 = backbone(key, data, 2)
    f1, t1 = backbone(key, data, 1)
    assert 'backbone_stage1' in t0 and 'backbone_stage2' in t0
    for f, taps, tag in ((f2, t2, "stages 1-2"), (f1, t1, "stage 1")):
        close(taps['backbone_stage1'], t0['backbone_stage1'], tag + ": stage 1 output")
        close(taps['backbone_stage2'], t0['backbone_stage2'], tag + ": stage 2 output")
        close(f, f0, tag + ": backbone feature")
    assert not torch.equal(f2, f0)                 # the fused launches really ran (conv1's scale is per block)
    key.check_status()


def test_small_net_pair_vs_two_launches(world):
    cur, data = world['cur'], world['data']
    if not cur.cfg.network.add_small_net:
        pytest.skip("the configuration has no small net")
    out = {}
    for pair in (0, 2):
        cur.pair_1x1 = pair
        out[pair] = cur._resnet(data, cur.small, cur.small_stages, 'small')[0].clone()
    close(out[2], out[0], "small-net feature")
    assert not torch.equal(out[2], out[0])
    cur.check_status()


def test_pair_graph_replay_equals_eager(world):
    key, data = world['key'], world['data']
    eager, _ = backbone(key, data, 2)
    key.pair_1x1 = 2
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = key._backbone(data)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    key.check_status()
