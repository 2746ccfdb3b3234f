"""Recorder of the executor's convolution launches: what the roofline counters (hip.conv_flops_read, the two piece shares,
hip.conv_bytes_read, hip.conv_by_kernel) report for whole passes of the bound test symbols at 192x320.

    python tests/golden/make_executor_launches.py            # writes tests/golden/executor_launches.json (needs the GPU)

executor_launches.json was recorded on an MI355X on the commit BEFORE the convolution binding (lsfa_amd/hip.py) and the executor
(lsfa_amd/symbols/resnet_v1_101_flownet_rfcn.py) were refactored, and is not regenerated when they change:
tests/test_executor_launches_gpu.py holds every later build to it.  The kernel names in it are the launch plan's
choices on that device.

A group is one set of bound executors; a pass is one forward() of one of them.  The shipped config (lsfa_test_config + P.init_params;
the counters depend on shapes, not on values) in f32 and bf16: a first key frame, a second key frame (FlowNet, warp, Nq), a non-key
frame, the batch symbol with two other frames.  In f32 also: the non-key frame of every small-net fuse variant, and the first key
frame + the non-key frame with pair_1x1 = 0 / 2 and with input_activation_min_bytes = 0 (set on the bound executors)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "executor_launches.json")
DEV = "cuda:0"
H, W = 192, 320
# (fuse type, stride, scale_before_fuse, bn_before_fuse): what tests/test_fusion_variants_gpu.py binds at this size
VARIANTS = [('add', 4, False, False), ('addv2', 4, False, False), ('concat', 4, False, False), ('concatv1', 4, False, False),
            ('concatv2', 4, False, False), ('add', 8, False, False), ('concatv2', 8, False, False), ('add', 4, True, True),
            ('addv2', 4, True, True)]
SETTINGS = [("pair_1x1", 0), ("pair_1x1", 2), ("input_activation_min_bytes", 0)]
GROUPS = ["f32", "bf16"] + ["cur %s stride %d scale %d bn %d" % v for v in VARIANTS] + ["%s = %d" % s for s in SETTINGS]


class World(object):
    """the inputs and the bound executors, made once and shared by every group that needs them"""

    def __init__(self):
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        import numpy as np
        import torch
        from lsfa_amd.config.config import lsfa_test_config
        from lsfa_amd.symbols import params as P
        from lsfa_amd.utils.synthetic import SyntheticClip
        self.torch, self.P, self.cfg = torch, P, lsfa_test_config(10)
        self.arg, self.aux = P.init_params(self.cfg, seed=0)
        clip = SyntheticClip(0, 4, H, W)
        self.frames = [clip.frame(i, DEV) for i in range(3)]
        self.mv, self.res = clip.motion_vector(2, 0, DEV), clip.res_diff(2, DEV)
        self.im_info = torch.from_numpy(clip.im_info()).to(DEV)
        self.im_info3 = torch.from_numpy(np.tile(clip.im_info(), (3, 1)).astype(np.float32)).to(DEV)
        g = torch.Generator(device=DEV).manual_seed(0)
        self.feat = torch.relu(torch.randn((1, 1024, H // 16, W // 16), device=DEV, generator=g))      # a key feature: only its shape matters
        self._bound = {}

    def bound(self, kind, dtype="f32", cfg=None):
        from lsfa_amd.symbols.resnet_v1_101_flownet_rfcn import resnet_v1_101_flownet_rfcn
        if cfg is not None:      # a fuse variant: its own weights, bound once, not kept
            arg, aux = self.P.init_params(cfg, seed=0)
            return resnet_v1_101_flownet_rfcn(cfg).get_cur_test_symbol(cfg).bind(arg, aux, DEV)
        if (kind, dtype) not in self._bound:
            sym = getattr(resnet_v1_101_flownet_rfcn(self.cfg), "get_%s_test_symbol" % kind)(self.cfg)
            self._bound[kind, dtype] = sym.bind(self.arg, self.aux, DEV, self.torch.float32 if dtype == "f32" else self.torch.bfloat16)
        return self._bound[kind, dtype]

    def counted(self, forward):
        from lsfa_amd import hip
        hip.conv_flops_reset(True)
        try:
            forward()
            self.torch.cuda.synchronize()
            flops, launches = hip.conv_flops_read()
            return {"flops": flops, "launches": launches, "flops_three_products": hip.conv_flops_three_products(),
                    "flops_one_product": hip.conv_flops_one_product(), "bytes": hip.conv_bytes_read(), "by_kernel": hip.conv_by_kernel()}
        finally:
            hip.conv_flops_reset(False)

    def key_first(self, key):
        f0 = self.frames[0]
        return lambda: key.forward(data=f0, im_info=self.im_info, data_key_old=f0, feat_key_old=self.torch.zeros(1, 1024, 1, 1, device=DEV))

    def key_second(self, key):
        return lambda: key.forward(data=self.frames[1], im_info=self.im_info, data_key_old=self.frames[0], feat_key_old=self.feat)

    def non_key(self, cur):
        return lambda: cur.forward(data=self.frames[2], im_info=self.im_info, feat_key=self.feat, motion_vector=self.mv, res_diff=self.res)

    def batch(self, sym):
        other = self.torch.cat(self.frames[1:3], 0)
        return lambda: sym.forward(data_key=self.frames[0], data_other=other, im_info=self.im_info3)

    def run(self, group):
        """-> {pass name: its counters}"""
        if group in ("f32", "bf16"):
            key, cur, bat = (self.bound(k, group) for k in ("key", "cur", "batch"))
            return {"first key frame": self.counted(self.key_first(key)), "second key frame": self.counted(self.key_second(key)),
                    "non-key frame": self.counted(self.non_key(cur)), "batch of 1 + 2": self.counted(self.batch(bat))}
        if group.startswith("cur "):
            from lsfa_amd.config.config import lsfa_test_config
            fuse, stride, scale, bn = VARIANTS[GROUPS.index(group) - 2]
            cfg = lsfa_test_config(10)
            n = cfg.network
            n.small_net_fuse_type, n.small_net_stride, n.small_net_scale_before_fuse, n.small_net_bn_before_fuse = fuse, stride, scale, bn
            return {"non-key frame": self.counted(self.non_key(self.bound("cur", cfg=cfg)))}
        name, value = SETTINGS[GROUPS.index(group) - 2 - len(VARIANTS)]
        key, cur = self.bound("key"), self.bound("cur")
        was = [getattr(e, name) for e in (key, cur)]
        try:
            for e in (key, cur):
                setattr(e, name, value)
            return {"first key frame": self.counted(self.key_first(key)), "non-key frame": self.counted(self.non_key(cur))}
        finally:
            for e, v in zip((key, cur), was):
                setattr(e, name, v)


def main():
    w = World()
    rec = {"height": H, "width": W, "groups": {g: w.run(g) for g in GROUPS}}
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d groups, %d passes" % (len(rec["groups"]), sum(len(v) for v in rec["groups"].values())))


if __name__ == "__main__":
    main()
