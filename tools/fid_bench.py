#!/usr/bin/env python3
"""ttv_inception_features on 64 images per launch with seeded Inception-v3 weights: ms per image (HIP events around a window of calls,
after a warm-up) and the network's FLOPs over that time as a fraction of the fp32 MFMA peak; the same for the preprocessing of 64
frames of 3 x 128 x 128 bf16 plus the network (InceptionV3.features).  GPU box only."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.model.metrics import metrics as M  # noqa: E402
from titok_video_amd.synthetic import seeded_inception_state  # noqa: E402

DEV = "cuda:0"
F32_PEAK = 157.3e12
IMAGES, WARMUP, ITERS = 64, 3, 10


def network_flops() -> float:
    """2 x MACs of the 94 convolutions and the fc at the fixed input 299 x 299, per image."""
    sizes = M.spatial_sizes()
    total, n = 2.0 * M.FEATURES * M.CLASSES, M.INPUT_SIZE
    for name, cin, cout, k, s, p in M.UNIT_SPECS:
        block = name.split(".")[0]
        if "." in name:      # every unit of a block works at the block's input size (its stride-2 units are the last of their branch)
            idx = list(sizes).index(block)
            n = sizes[list(sizes)[idx - 1]]
        ho, wo = M.conv_out(n, k[0], s[0], p[0]), M.conv_out(n, k[1], s[1], p[1])
        total += 2.0 * ho * wo * cin * cout * k[0] * k[1]
        if "." not in name:
            n = sizes["maxpool1"] if name == "Conv2d_2b_3x3" else sizes["maxpool2"] if name == "Conv2d_4a_3x3" else ho
    return total


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


def main():
    net = M.InceptionV3(seeded_inception_state(0)).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    frames = [(torch.rand((3, 128, 128), generator=g, device=DEV) * 2 - 1).to(torch.bfloat16) for _ in range(IMAGES)]
    flop = IMAGES * network_flops()
    ms_all = timed(lambda: net.features([(frames, True)]))
    x, ws = net._buffers(IMAGES)
    acts = torch.empty(IMAGES, M.FEATURES, device=DEV)
    probs = torch.empty(IMAGES, M.CLASSES, device=DEV)
    stream = _lib.stream_ptr(torch.device(DEV))

    def call():
        _lib.check(_lib.lib().ttv_inception_features(C.byref(net.table), x.data_ptr(), IMAGES, acts.data_ptr(), probs.data_ptr(),
                                                     ws.data_ptr(), ws.numel(), stream), "ttv_inception_features")
    ms = timed(call)
    print(f"network FLOPs per image: {network_flops() / 1e9:.3f} G", flush=True)
    print(f"ttv_inception_features  {IMAGES} images: {ms:8.3f} ms = {ms / IMAGES:.4f} ms per image  {flop / ms / 1e9:6.2f} TF/s = "
          f"{flop / ms / 1e9 / (F32_PEAK / 1e12):.3f} of the fp32 MFMA peak", flush=True)
    print(f"InceptionV3.features (preprocess 3 x 128 x 128 bf16 + network)  {IMAGES} images: {ms_all:8.3f} ms = "
          f"{ms_all / IMAGES:.4f} ms per image", flush=True)


if __name__ == "__main__":
    main()
