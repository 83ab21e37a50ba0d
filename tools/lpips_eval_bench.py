#!/usr/bin/env python3
"""The evaluation LPIPS at the benchmark clip: `LPIPS.frame_distances` on one bf16 clip pair of 16 x 128 x 128 and of 16 x 136 x 168
(one pass each, the reconstruction's clamp and the frame gather inside the first convolution), and the loss path's `LPIPS.forward`
under no_grad on the same 16 frame pairs of 128 x 128 already gathered into [16, 3, 128, 128] (tape and all, no Gram term).  The
three alternate in one process; ms per call = median over the repeats of a window of ITERS calls ended by a device synchronise.
Also checks that the first and the third give the same values.  GPU box only."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from titok_video_amd.model.metrics.lpips_gram import LPIPS  # noqa: E402
from titok_video_amd.synthetic import seeded_lpips_state  # noqa: E402

REPS, ITERS = int(os.environ.get("REPS", "7")), int(os.environ.get("ITERS", "200"))


def clip_pair(T, H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    y = (torch.rand((3, T, H, W), device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
    x = (1.1 * y.float() + 0.2 * torch.randn(y.shape, device="cuda", generator=g)).to(torch.bfloat16)
    return x, y


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(ITERS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / ITERS


def main():
    m = LPIPS()
    m.load_state_dict(seeded_lpips_state(0))
    m = m.to("cuda").eval()
    xa, ya = clip_pair(16, 128, 128, 0)
    xb, yb = clip_pair(16, 136, 168, 1)
    xf, yf = xa.clamp(-1, 1).permute(1, 0, 2, 3).contiguous(), ya.permute(1, 0, 2, 3).contiguous()

    def loss_path():
        with torch.no_grad():
            return m(xf, yf, compute_gram=False)[0]

    steps = {"eval_16x128x128_ms": lambda: m.frame_distances([xa], [ya]), "eval_16x136x168_ms": lambda: m.frame_distances([xb], [yb]),
             "forward_nograd_16x128x128_ms": loss_path}
    same = bool(torch.equal(steps["eval_16x128x128_ms"](), loss_path()))
    for _ in range(3):
        for fn in steps.values():
            fn()
    runs = {k: [] for k in steps}
    for _ in range(REPS):                       # alternating
        for k, fn in steps.items():
            runs[k].append(timed(fn))
    out = {"dtype": "bf16", "iters": ITERS, "reps": REPS, "eval_equals_forward_bits": same}
    for k, v in runs.items():
        v.sort()
        out[k] = round(v[len(v) // 2], 4)
        out[k + "_min_max"] = [round(v[0], 4), round(v[-1], 4)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
