"""Float64 restatement of the evaluation LPIPS (EvalMetrics 'lpips', LPIPS.frame_distances), for the tests.

Per clip pair [3, T, H, W]: the reconstruction clamped to [-1, 1], the target not; every frame pair a batch entry of its own of the
network restated in tests/lpips_ref.py (whose max-pools already floor: F.max_pool2d(h, 2, 2)), LPIPS only, no Gram term.
`frame_values_bf16` is the same network with every activation rounded to bf16 the way the bf16 kernels store them (weights rounded
to bf16, the scaled input of the first convolution rounded, every ReLU output rounded; sums in float64, the head in float64): the
yardstick for what bf16 storage alone costs at shapes where one stage-4 pixel carries a whole tap.
Also: the shapes and the seeded input recipe of tests/golden/lpips_eval_kat.npz.
"""
from __future__ import annotations

import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_ref as R  # noqa: E402

WEIGHT_SEED = 11
CLIP_SEED = 40
# (T, H, W): smallest legal frame; odd at stages 0, 1, 2; multiples of 8 but not 16 (both ways round); the reference's ragged size;
# one-row images at stage 4 beside a wide row; the benchmark clip
SHAPES = [(5, 16, 16), (2, 17, 23), (3, 24, 40), (2, 40, 24), (2, 136, 168), (1, 16, 520), (16, 128, 128)]


def clip_pair(shape, seed):
    """(recon, target) [3, T, H, W] fp32 CPU, every value bf16-representable (one float64 result is the reference for both dtypes);
    the target lies in [-1, 1], about a tenth of the reconstruction outside."""
    T, H, W = shape
    g = torch.Generator().manual_seed(int(seed))
    target = (torch.rand((3, T, H, W), generator=g) * 2 - 1).to(torch.bfloat16).float()
    recon = (1.1 * target + 0.2 * torch.randn(target.shape, generator=g)).to(torch.bfloat16).float()
    return recon, target


def fixture_pairs():
    return [clip_pair(s, CLIP_SEED + i) for i, s in enumerate(SHAPES)]


def fingerprint(recon, target):
    return [float(recon.double().abs().sum()), float(target.double().abs().sum())]


def lpips_only(t0, t1, lins):
    lp = 0
    for f0, f1, lin in zip(t0, t1, lins):
        d = (R.normalise(f0) - R.normalise(f1)) ** 2
        lp = lp + (d * lin.view(1, -1, 1, 1)).sum(1).mean((1, 2))
    return lp


def frame_values(sd, recon, target, clamp=True, dtype=torch.float64):
    """Per-frame LPIPS [T] of one clip pair, in `dtype` on the CPU."""
    x = recon.to(dtype).permute(1, 0, 2, 3)
    y = target.to(dtype).permute(1, 0, 2, 3)
    if clamp:
        x = x.clamp(-1, 1)
    return lpips_only(R.taps(sd, x), R.taps(sd, y), R.lin_weights(sd, dtype))


def _bf16(t):
    return t.to(torch.bfloat16).double()


def taps_bf16(sd, x):
    shift = torch.tensor(R.SHIFT, dtype=torch.float64).view(1, 3, 1, 1)
    scale = torch.tensor(R.SCALE, dtype=torch.float64).view(1, 3, 1, 1)
    # the kernel scales in fp32 and rounds once to bf16
    h = _bf16(((x.float() - shift.float()) / scale.float()))
    out = []
    for l, (w, b) in enumerate(R.conv_weights(sd, torch.float64)):
        h = _bf16(torch.relu(F.conv2d(h, _bf16(w), b, padding=1)))
        if l in R.TAP_AFTER:
            out.append(h)
        if l in R.POOL_AFTER:
            h = F.max_pool2d(h, 2, 2)
    return out


def frame_values_bf16(sd, recon, target, clamp=True):
    """Per-frame LPIPS [T] (float64) with bf16 storage of the inputs, weights and activations."""
    x = _bf16(recon).permute(1, 0, 2, 3)
    y = _bf16(target).permute(1, 0, 2, 3)
    if clamp:
        x = x.clamp(-1, 1)
    return lpips_only(taps_bf16(sd, x), taps_bf16(sd, y), R.lin_weights(sd, torch.float64))
