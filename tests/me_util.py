"""What the motion-estimation GPU tests share (tests/test_me_gpu.py, test_me_segment_gpu.py, test_me_pyramid_gpu.py): host arrays onto the
device, the translated clip of tests/ref_me.py and stacks of luma planes as the chain exports take them."""
import numpy as np
import torch

import ref_me

DEV = "cuda:0"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def clip(n, width, height, seed, m=(3, -2), sigma=3.0):
    return ref_me.translated_clip(n, width, height, m, seed=seed, sigma=sigma)


def plane_stack(planes, chains, stride=None):
    """chains: a list of lists of indices into `planes` -> a (C, F + 1, H, W) uint8 view on the device whose planes lie `stride` bytes apart
    (default: the plane's size rounded up to a multiple of 4, which the search requires), the bytes between them 0xA5"""
    H, W = planes[0].shape
    stride = stride or -(-H * W // 4) * 4
    C, F1 = len(chains), len(chains[0])
    buf = torch.full((C * F1 * stride,), 0xA5, dtype=torch.uint8, device=DEV)
    view = buf.as_strided((C, F1, H, W), (F1 * stride, stride, W, 1))
    for c, chain in enumerate(chains):
        for f, i in enumerate(chain):
            view[c, f].copy_(t(planes[i]))
    return view
