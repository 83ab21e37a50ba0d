#!/usr/bin/env python3
"""EvalMetrics(['fvd']).update on 32 clip pairs of 3 x 16 x 128 x 128, bf16 (the benchmark batch), with seeded I3D weights: µs per
update (HIP events around a window of updates, after a warm-up) and the network's FLOPs over that time as a fraction of the fp32
MFMA peak; the same network restated with torch's fp32 conv3d / max_pool3d (explicit TF-SAME F.pad, same folded weights) on the same
preprocessed inputs, timed in the same process.  Prints the max |difference| of the two feature sets.  GPU box only."""
import os
import sys
from types import SimpleNamespace

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from titok_video_amd.model.metrics import fvd  # noqa: E402
from titok_video_amd.model.metrics.eval_metrics import EvalMetrics  # noqa: E402
from titok_video_amd.synthetic import seeded_i3d_state  # noqa: E402

DEV = "cuda:0"
F32_PEAK = 157.3e12
SHAPE, PAIRS, WARMUP, ITERS = (3, 16, 128, 128), 32, 2, 5


def network_flops() -> float:
    """2 x MACs of the 58 convolutions at the fixed input 10 x 224 x 224, per clip."""
    sizes = {"Conv3d_1a_7x7": 5 * 112 * 112, "Conv3d_2b_1x1": 5 * 56 * 56, "Conv3d_2c_3x3": 5 * 56 * 56, "logits": 1}
    total = 0.0
    for unit, cin, cout, k in fvd.CONV_SPECS:
        block = unit.split(".")[0]
        pos = sizes.get(block) or (5 * 28 * 28 if block.startswith("Mixed_3") else 3 * 14 * 14 if block.startswith("Mixed_4") else 2 * 7 * 7)
        total += 2.0 * pos * cin * cout * k ** 3
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
    return e0.elapsed_time(e1) * 1e3 / ITERS


def torch_network(sd):
    """fp32 torch restatement with the folded weights: NCDHW conv3d + scale / shift + ReLU, max_pool3d on -inf padding."""
    units = {u: [t.to(DEV) for t in fvd.fold_unit(sd, u)] for u, *_ in fvd.CONV_SPECS}
    w5 = {u: sd[f"{u}.conv3d.weight"].float().to(DEV) for u, *_ in fvd.CONV_SPECS}

    def pad(x, k, s, value=0.0):
        p = []
        for n, kk, ss in reversed(list(zip(x.shape[2:], k, s))):
            _, f, b = fvd.same_pad(n, kk, ss)
            p += [f, b]
        return F.pad(x, p, value=value)

    def unit(x, u, s=1, relu=True):
        k = w5[u].shape[2]
        y = F.conv3d(pad(x, (k,) * 3, (s,) * 3), w5[u], stride=s)
        y = y * units[u][1].view(1, -1, 1, 1, 1) + units[u][2].view(1, -1, 1, 1, 1)
        return y.clamp_min(0) if relu else y

    def pool(x, k, s):
        return F.max_pool3d(pad(x, k, s, -float("inf")), k, s)

    def run(x):
        x = unit(x, "Conv3d_1a_7x7", 2)
        x = pool(x, (1, 3, 3), (1, 2, 2))
        x = unit(unit(x, "Conv3d_2b_1x1"), "Conv3d_2c_3x3")
        x = pool(x, (1, 3, 3), (1, 2, 2))
        for name in fvd.INCEPTION:
            if name == "Mixed_4b":
                x = pool(x, (3, 3, 3), (2, 2, 2))
            elif name == "Mixed_5b":
                x = pool(x, (2, 2, 2), (2, 2, 2))
            x = torch.cat([unit(x, f"{name}.b0"), unit(unit(x, f"{name}.b1a"), f"{name}.b1b"),
                           unit(unit(x, f"{name}.b2a"), f"{name}.b2b"), unit(pool(x, (3, 3, 3), (1, 1, 1)), f"{name}.b3b")], dim=1)
        x = F.avg_pool3d(x, (2, 7, 7), 1)
        y = F.conv3d(x, w5["logits"]) + units["logits"][2].view(1, -1, 1, 1, 1)
        return y.mean(dim=2).flatten(1)
    return run


def main():
    torch.backends.cudnn.allow_tf32 = False
    sd = seeded_i3d_state(0)
    det = fvd.I3D(sd)
    g = torch.Generator(device=DEV).manual_seed(0)
    target = [(torch.rand(SHAPE, generator=g, device=DEV) * 2 - 1).to(torch.bfloat16) for _ in range(PAIRS)]
    recon = [(t.float() + 0.1 * torch.randn(SHAPE, generator=g, device=DEV)).to(torch.bfloat16) for t in target]
    m = EvalMetrics(SimpleNamespace(training=SimpleNamespace(eval=SimpleNamespace(log_metrics=["fvd"]))), fvd_detector=det)

    def upd():
        m.update(recon, target)
        m._fvd.reset()          # keep the feature list from growing over the timing window
    us = timed(upd)
    flop = 2 * PAIRS * network_flops()
    print(f"fvd update()  {PAIRS} pairs x {SHAPE} bf16: {us:9.1f} us  {flop / 1e12:.3f} TFLOP  {flop / us / 1e6:6.2f} TF/s = "
          f"{flop / us / 1e6 / (F32_PEAK / 1e12):.3f} of the fp32 MFMA peak", flush=True)

    # torch fp32 restatement on the same preprocessed inputs (NCDHW)
    x = det._x[:2 * PAIRS * 10 * 224 * 224 * 3].view(2 * PAIRS, 10, 224, 224, 3)
    m.update(recon, target)
    ours = torch.cat(m._fvd.features())
    xt = x.permute(0, 4, 1, 2, 3).contiguous()
    net = torch_network(sd)
    with torch.no_grad():
        us_t = timed(lambda: [net(xt[i:i + 16]) for i in range(0, 2 * PAIRS, 16)])
        ref = torch.cat([net(xt[i:i + 16]) for i in range(0, 2 * PAIRS, 16)])
    print(f"torch fp32 conv3d restatement, same inputs (16 clips per call): {us_t:9.1f} us  {flop / us_t / 1e6:6.2f} TF/s = "
          f"{flop / us_t / 1e6 / (F32_PEAK / 1e12):.3f} of peak;  HIP / torch time {us / us_t:.3f};  "
          f"max |features HIP - torch| {float((ours - ref).abs().max()):.3e} (max |f| {float(ref.abs().max()):.3e})", flush=True)


if __name__ == "__main__":
    main()
