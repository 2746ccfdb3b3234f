#!/usr/bin/env python
"""Cost of every small-net fuse variant at 1000x600 (GPU tool).

    python tools/fusion_variants.py [--variants add,addv2,...] [--reps 20] [--fps-frames 0]

For each variant (small_net_fuse_type, stride, scale_before_fuse, bn_before_fuse) it prints one JSON line:
  * `nonkey_ms`: one non-key frame (Executor.forward, batch 1), median of --reps, HIP events around the call;
  * `fps`: frames/s of FramePipeline(segment=9, key_group=12, lanes=2) - bench.py's pipelined settings - over --fps-frames frames of a
    synthetic clip (0 skips it).
The new kernels' own time comes from a separate run under the kernel tracer:
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/fusion_variants.py --variants concatv2 --fps-frames 0
(channel_mean_*, gate_fc_kernel, gate_apply_kernel, warp_cl_kernel<.., true> in the stats); their bytes over time against 8 TB/s is
what --bytes prints for the 1000x600 shapes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = {'add': ('add', 4, False, False), 'addv2': ('addv2', 4, False, False), 'concat': ('concat', 4, False, False),
            'concatv1': ('concatv1', 4, False, False), 'concatv2': ('concatv2', 4, False, False), 'add_s8': ('add', 8, False, False),
            'concatv2_s8': ('concatv2', 8, False, False), 'add_bn': ('add', 4, True, True), 'addv2_bn': ('addv2', 4, True, True)}


def bytes_of_new_kernels(h=38, w=63):
    """HBM bytes of the gate kernels at one 1000x600 image (fp32): mean reads, gate weights, apply reads 2 maps + writes 1"""
    hw, f = h * w, 4
    return dict(mean_concatv2=2048 * hw * f, mean_concatv1=1024 * hw * f, gate_concatv2=(1024 * 2048 + 1024 * 1024) * f,
                gate_concatv1=2 * 1024 * 1024 * f, apply=3 * 1024 * hw * f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variants', default=','.join(VARIANTS))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--fps-frames', type=int, default=120)
    ap.add_argument('--bytes', action='store_true')
    a = ap.parse_args()
    if a.bytes:
        print(json.dumps(bytes_of_new_kernels()))
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.core.graphs import FramePipeline
    from lsfa_amd.symbols import params as P
    from lsfa_amd.symbols.resnet_v1_101_flownet_rfcn import resnet_v1_101_flownet_rfcn
    from lsfa_amd.utils.synthetic import SyntheticClip
    dev, H, W = 'cuda:0', 600, 1000
    for name in a.variants.split(','):
        fuse, stride, scale, bn = VARIANTS[name]
        cfg = lsfa_test_config(10)
        n = cfg.network
        n.small_net_fuse_type, n.small_net_stride, n.small_net_scale_before_fuse, n.small_net_bn_before_fuse = fuse, stride, scale, bn
        arg, aux = P.init_params(cfg, seed=0)
        net = resnet_v1_101_flownet_rfcn(cfg)
        key = net.get_key_test_symbol(cfg).bind(arg, aux, dev)
        cur = net.get_cur_test_symbol(cfg).bind(arg, aux, dev)
        clip = SyntheticClip(0, 12, H, W)
        im = torch.from_numpy(clip.im_info()).to(dev)
        f0 = clip.frame(0, dev)
        feat = key.forward(data=f0, im_info=im, data_key_old=f0, feat_key_old=torch.zeros(1, 1024, 1, 1, device=dev))['choose_feat_output']
        inp = dict(data=clip.frame(3, dev), im_info=im, feat_key=feat, motion_vector=clip.motion_vector(3, 0, dev), res_diff=clip.res_diff(3, dev))
        for _ in range(3):
            cur.forward(**inp)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cur.forward(**inp)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        cur.check_status()
        row = dict(variant=name, fuse=fuse, stride=stride, scale=scale, bn=bn, nonkey_ms=float(np.median(ts)))
        if a.fps_frames:
            fp = FramePipeline(key, cur, cfg, H, W, dev, lanes=2, segment=9, key_group=12)
            frames = [clip.frame(i % 12, dev) for i in range(a.fps_frames + 1)]
            fp.first_frame(frames[0])
            fp.capture()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(1, a.fps_frames + 1):
                kf = 1 + 10 * ((i - 1) // 10)
                if i == kf:
                    fp.key_frame(frames[i], upcoming=[frames[k] for k in range(i + 10, min(a.fps_frames + 1, i + 10 * 12), 10)])
                else:
                    fp.cur_frame(frames[i], clip.motion_vector(i % 12, kf % 12, dev), clip.res_diff(i % 12, dev))
            fp.join()
            torch.cuda.synchronize()
            row['fps'] = a.fps_frames / (time.perf_counter() - t0)
            fp.close()
        print(json.dumps(row), flush=True)
        del key, cur
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
