#!/usr/bin/env python3
"""The perceptual term at the training shape: LPIPS forward on 25 reconstruction + 25 target crops of 128 x 128 plus the
input-gradient backward for the 25 reconstruction crops, bf16.  Alternating in the same process, torch's own bf16 VGG (conv2d =
MIOpen) on the same crops computing the same forward + input gradient.  Reports ms (median of the repeats), the algorithmic GFLOP
(from shapes) and the fraction of the nominal 2.5 PFLOP/s bf16 peak.  GPU box only."""
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from titok_video_amd.model.metrics.lpips_gram import LPIPS, CONV_INDICES, VGG_FEATURES  # noqa: E402
from titok_video_amd.synthetic import seeded_lpips_state  # noqa: E402

N, S = int(os.environ.get("N", "25")), int(os.environ.get("S", "128"))
REPS, ITERS = int(os.environ.get("REPS", "5")), int(os.environ.get("ITERS", "10"))
PEAK = 2.5e15


def gflop_per_image(s):
    """3x3 conv MACs x 2 of the forward (one image) and of the input-gradient backward (conv1_1's dgrad included)."""
    dims = {f[0]: (f[2], f[3]) for f in VGG_FEATURES if f[1] == "conv"}
    stage = {0: 0, 2: 0, 5: 1, 7: 1, 10: 2, 12: 2, 14: 2, 17: 3, 19: 3, 21: 3, 24: 4, 26: 4, 28: 4}
    fwd = sum(2 * 9 * dims[i][0] * dims[i][1] * (s >> stage[i]) ** 2 for i in CONV_INDICES)
    return fwd / 1e9, fwd / 1e9


def torch_vgg(sd):
    convs = [(sd[k + ".weight"].to("cuda", torch.bfloat16), sd[k + ".bias"].to("cuda", torch.bfloat16))
             for k in (f"net.slice{s}.{i}" for s, i in [(1, 0), (1, 2), (2, 5), (2, 7), (3, 10), (3, 12), (3, 14), (4, 17), (4, 19),
                                                       (4, 21), (5, 24), (5, 26), (5, 28)])]
    lins = [sd[f"lin{k}.model.1.weight"].to("cuda", torch.bfloat16) for k in range(5)]
    shift = torch.tensor([-0.030, -0.088, -0.188], device="cuda").view(1, 3, 1, 1)
    scale = torch.tensor([0.458, 0.448, 0.450], device="cuda").view(1, 3, 1, 1)

    def taps(x):
        h = ((x.float() - shift) / scale).to(torch.bfloat16)
        out = []
        for l, (w, b) in enumerate(convs):
            h = F.relu(F.conv2d(h, w, b, padding=1))
            if l in (1, 3, 6, 9, 12):
                out.append(h)
            if l in (1, 3, 6, 9):
                h = F.max_pool2d(h, 2, 2)
        return out

    def lpips(x, y):
        feats = taps(torch.cat([x, y]))
        lp = 0
        for f, lin in zip(feats, lins):
            f = f.float()
            n = f / (torch.sqrt((f * f).sum(1, keepdim=True) + 1e-10) + 1e-10)
            d = (n[:x.shape[0]] - n[x.shape[0]:]) ** 2
            lp = lp + (d * lin.float().view(1, -1, 1, 1)).sum(1).mean((1, 2))
        return lp

    return lpips


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(ITERS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / ITERS


def main():
    sd = seeded_lpips_state(0)
    m = LPIPS()
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    g = torch.Generator(device="cuda").manual_seed(0)
    y = (torch.rand((N, 3, S, S), device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
    x = (0.8 * y.float() + 0.1 * torch.randn((N, 3, S, S), device="cuda", generator=g)).to(torch.bfloat16)
    tv = torch_vgg(sd)

    def hip_step():
        xg = x.detach().requires_grad_(True)
        lp, _ = m(xg, y, compute_gram=False)
        lp.mean().backward()

    def torch_step():
        xg = x.detach().requires_grad_(True)
        tv(xg, y).mean().backward()

    for _ in range(3):
        hip_step()
        torch_step()
    hip, ref = [], []
    for _ in range(REPS):                       # alternating
        hip.append(timed(hip_step))
        ref.append(timed(torch_step))
    hip.sort()
    ref.sort()
    f, b = gflop_per_image(S)
    gflop = 2 * N * f + N * b
    hm, rm = hip[len(hip) // 2], ref[len(ref) // 2]
    print(json.dumps({"crops": N, "size": S, "gflop": round(gflop, 1), "hip_ms": round(hm, 3), "hip_peak_frac": round(gflop * 1e9 / (hm * 1e-3) / PEAK, 4),
                      "torch_miopen_ms": round(rm, 3), "torch_peak_frac": round(gflop * 1e9 / (rm * 1e-3) / PEAK, 4),
                      "hip_ms_all": [round(v, 3) for v in hip], "torch_ms_all": [round(v, 3) for v in ref]}))


if __name__ == "__main__":
    main()
