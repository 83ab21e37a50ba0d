"""Float64 restatement of the LPIPS / Gram perceptual terms and of the generator-step perceptual loss, for the tests.

Written from the definitions (reference model/metrics/lpips_gram.py semantics, restated here):
  scaled = (x - shift) / scale;  VGG16 features[0:30] (3x3 conv + bias, zero padding 1, ReLU; 2x2/2 max-pool after conv 2, 4, 7, 10);
  taps = the ReLU outputs of conv 2, 4, 7, 10, 13;  normalise(f) = f / (sqrt(sum_c f^2 + 1e-10) + 1e-10);
  lpips[b] = sum_k mean_{h,w} sum_c lin_k[c] (normalise(f0) - normalise(f1))^2;
  gram[b] = mean_k mean_{i,j} (G0 - G1)^2,  G = F F^T / (h w) on the un-normalised taps.
`flip` and `halo_shift` are deliberately wrong variants (kernels flipped, or every convolution's window moved one pixel right), used
to show that the tests' bounds tell them apart from the right answer.  Also: the seeded input recipes of tests/golden/lpips_kat.npz.
"""
from __future__ import annotations

import random

import numpy as np
import torch
import torch.nn.functional as F

CONV_KEYS = [(1, 0), (1, 2), (2, 5), (2, 7), (3, 10), (3, 12), (3, 14), (4, 17), (4, 19), (4, 21), (5, 24), (5, 26), (5, 28)]
POOL_AFTER = {1, 3, 6, 9}
TAP_AFTER = [1, 3, 6, 9, 12]
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)


def conv_weights(sd, dtype=torch.float64):
    return [(sd[f"net.slice{s}.{i}.weight"].to(dtype), sd[f"net.slice{s}.{i}.bias"].to(dtype)) for s, i in CONV_KEYS]


def lin_weights(sd, dtype=torch.float64):
    return [sd[f"lin{k}.model.1.weight"].to(dtype).reshape(-1) for k in range(5)]


def conv3x3(h, w, b, flip=False, halo_shift=False):
    if flip:
        w = w.flip(2, 3)
    if halo_shift:
        return F.conv2d(F.pad(h, (0, 2, 1, 1)), w, b)
    return F.conv2d(h, w, b, padding=1)


def taps(sd, x, flip=False, halo_shift=False):
    shift = torch.tensor(SHIFT, dtype=x.dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=x.dtype).view(1, 3, 1, 1)
    h = (x - shift) / scale
    out = []
    for l, (w, b) in enumerate(conv_weights(sd, x.dtype)):
        h = torch.relu(conv3x3(h, w, b, flip, halo_shift))
        if l in TAP_AFTER:
            out.append(h)
        if l in POOL_AFTER:
            h = F.max_pool2d(h, 2, 2)
    return out


def normalise(f):
    return f / (torch.sqrt((f * f).sum(1, keepdim=True) + 1e-10) + 1e-10)


def lpips_gram(sd, x, y, flip=False, halo_shift=False):
    """(lpips[B], gram[B]) in x's dtype (float64 for the tests)."""
    t0, t1 = taps(sd, x, flip, halo_shift), taps(sd, y, flip, halo_shift)
    lins = lin_weights(sd, x.dtype)
    lp = 0
    grams = []
    for f0, f1, lin in zip(t0, t1, lins):
        d = (normalise(f0) - normalise(f1)) ** 2
        lp = lp + (d * lin.view(1, -1, 1, 1)).sum(1).mean((1, 2))
        B, C, H, W = f0.shape
        g0 = f0.reshape(B, C, H * W) @ f0.reshape(B, C, H * W).transpose(1, 2) / (H * W)
        g1 = f1.reshape(B, C, H * W) @ f1.reshape(B, C, H * W).transpose(1, 2) / (H * W)
        grams.append(((g0 - g1) ** 2).reshape(B, -1).mean(1))
    return lp, torch.stack(grams, -1).mean(-1)


# ---- seeded inputs of the fixture (tests/golden/make_golden_lpips.py) ------------------------------------------------------
def pair_inputs(d):
    """[(input [1,3,H,W], target [1,3,H,W])] fp32 CPU, drawn in the fixture's order."""
    g = torch.Generator().manual_seed(int(d["input_seed"]))
    out = []
    for H, W in d["pair_shapes"].tolist():
        y = torch.rand((1, 3, H, W), generator=g) * 2 - 1
        x = 0.7 * y + 0.3 * (torch.rand((1, 3, H, W), generator=g) * 2 - 1)
        out.append((x, y))
    return out


def clip_inputs(d):
    """(target clips, recon clips) [C,T,H,W] fp32 CPU."""
    g = torch.Generator().manual_seed(int(d["clip_seed"]))
    shapes = [tuple(s) for s in d["clip_shapes"].tolist()]
    target = [torch.rand(s, generator=g) * 2 - 1 for s in shapes]
    recon = [1.1 * t + 0.2 * torch.randn(t.shape, generator=g) for t in target]
    return target, recon


def projections(shape, seed, k):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((k,) + tuple(shape), generator=g, dtype=torch.float64)


def project(grad, seed, k):
    v = projections(grad.shape, seed, k)
    return (v * grad.double().cpu()[None]).flatten(1).sum(1).numpy()


class RandomLog:
    """Records every random.random / random.randrange call made inside the `with` block as (a, b, value) rows ((0, 0, v) for
    random())."""

    def __enter__(self):
        self.rows = []
        self._r, self._rr = random.random, random.randrange

        def rec_random():
            v = self._r()
            self.rows.append((0.0, 0.0, v))
            return v

        def rec_randrange(a, b):
            v = self._rr(a, b)
            self.rows.append((float(a), float(b), float(v)))
            return v

        random.random, random.randrange = rec_random, rec_randrange
        return self

    def __exit__(self, *exc):
        random.random, random.randrange = self._r, self._rr
        return False

    def array(self):
        return np.array(self.rows, dtype=np.float64)


def rel_err(a, b):
    """max |a - b| / max |b| (a scalar; both tensors or arrays)."""
    a = torch.as_tensor(np.asarray(a), dtype=torch.float64) if not torch.is_tensor(a) else a.double().cpu()
    b = torch.as_tensor(np.asarray(b), dtype=torch.float64) if not torch.is_tensor(b) else b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
