"""Float64 restatement of the FVD preprocessing and of the I3D detector, for the tests.

Written from the definitions (reference model/metrics/fvd.py semantics and the published I3D architecture, restated here):
  preprocess: trilinear resample (torch align_corners=False: src = max((dst + 0.5) in / out - 0.5, 0), upper neighbour clamped; the
  source index and the weights in fp32 arithmetic as torch computes them for the reference's fp32 input, the blend in float64) of
  [3, T, H, W] to 3 x 224 x 224 (the reference's size (C, 224, 224): the time axis goes to C = 3 frames), then the last frame
  repeated to 10 frames;
  unit = conv (no bias, TF-SAME padding: out = ceil(n / s), pad = max((out - 1) s + k - n, 0), front pad // 2) -> eval BatchNorm
  (eps 1e-3, no scale when the state has no bn.weight) -> ReLU; max-pools with the same padding rule (padded cells never win);
  Inception = concat(b0, b1b(b1a), b2b(b2a), b3b(maxpool 3^3 / 1)); AvgPool 2x7x7 VALID; logits 1^3 conv with bias; mean over time.
Convolutions are im2col products (tensor.unfold + tensordot) on zero-padded inputs, so this file shares no code path with
torch's conv3d / max_pool3d, which the CPU tests use to check it.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from titok_video_amd.model.metrics.fvd import BN_EPS, INCEPTION, same_pad


def _resample_matrix(n_in: int, n_out: int) -> torch.Tensor:
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    # the source index as torch computes it for fp32 inputs: fp32 scale, scale * (dst + 0.5) - 0.5 with one rounding (a fused
    # multiply-add), fp32 weights
    scale = np.float32(n_in) / np.float32(n_out)
    for d in range(n_out):
        src = max(np.float32(np.float64(scale) * (d + 0.5) - 0.5), np.float32(0.0))
        i0 = int(src)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        l1 = np.float32(src - np.float32(i0))
        m[d, i0] += float(np.float32(1.0) - l1)
        m[d, i1] += float(l1)
    return m


def preprocess(clip: torch.Tensor, clamp: bool = False) -> torch.Tensor:
    """[3, T, H, W] -> [3, 10, 224, 224] float64."""
    x = clip.double()
    if clamp:
        x = x.clamp(-1, 1)
    C, T, H, W = x.shape
    x = torch.einsum("ut,cthw->cuhw", _resample_matrix(T, C), x)     # the time axis to C frames (the reference's size argument)
    x = torch.einsum("vh,cthw->ctvw", _resample_matrix(H, 224), x)
    x = torch.einsum("xw,cthw->cthx", _resample_matrix(W, 224), x)
    return torch.cat([x, x[:, -1:].expand(-1, 10 - x.shape[1], -1, -1)], dim=1) if x.shape[1] < 10 else x


def _pad_same(x: torch.Tensor, k, s, value=0.0) -> torch.Tensor:
    pads = []
    for dim, kk, ss in reversed(list(zip(x.shape[2:], k, s))):
        _, f, b = same_pad(dim, kk, ss)
        pads += [f, b]
    return F.pad(x, pads, value=value)


def _windows(x: torch.Tensor, k, s) -> torch.Tensor:
    """[B, C, T, H, W] (padded) -> [B, C, To, Ho, Wo, kt, kh, kw]."""
    return x.unfold(2, k[0], s[0]).unfold(3, k[1], s[1]).unfold(4, k[2], s[2])


def conv3d(x: torch.Tensor, w: torch.Tensor, stride: int = 1) -> torch.Tensor:
    """TF-SAME 3-D convolution of [B, Cin, T, H, W] with [Cout, Cin, k, k, k], float64, no bias."""
    k = tuple(w.shape[2:])
    s = (stride,) * 3
    win = _windows(_pad_same(x, k, s), k, s)
    y = torch.tensordot(win, w.double(), dims=([1, 5, 6, 7], [1, 2, 3, 4]))   # [B, To, Ho, Wo, Cout]
    return y.permute(0, 4, 1, 2, 3).contiguous()


def maxpool3d(x: torch.Tensor, k, s) -> torch.Tensor:
    return _windows(_pad_same(x, k, s, value=-float("inf")), k, s).amax(dim=(5, 6, 7))


def bn_fold(sd, unit):
    cout = sd[f"{unit}.conv3d.weight"].shape[0]
    gamma = sd[f"{unit}.bn.weight"].double() if f"{unit}.bn.weight" in sd else torch.ones(cout, dtype=torch.float64)
    scale = gamma / torch.sqrt(sd[f"{unit}.bn.running_var"].double() + BN_EPS)
    return scale, sd[f"{unit}.bn.bias"].double() - sd[f"{unit}.bn.running_mean"].double() * scale


def unit(x, sd, name, stride=1, relu=True):
    y = conv3d(x, sd[f"{name}.conv3d.weight"], stride)
    scale, shift = bn_fold(sd, name)
    y = y * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)
    return y.clamp_min(0) if relu else y


def features(x: torch.Tensor, sd) -> torch.Tensor:
    """[B, 3, 10, 224, 224] -> [B, 400] float64: the logits before the softmax, averaged over time."""
    x = x.double()
    x = unit(x, sd, "Conv3d_1a_7x7", 2)
    x = maxpool3d(x, (1, 3, 3), (1, 2, 2))
    x = unit(x, sd, "Conv3d_2b_1x1")
    x = unit(x, sd, "Conv3d_2c_3x3")
    x = maxpool3d(x, (1, 3, 3), (1, 2, 2))
    for name in INCEPTION:
        if name == "Mixed_4b":
            x = maxpool3d(x, (3, 3, 3), (2, 2, 2))
        elif name == "Mixed_5b":
            x = maxpool3d(x, (2, 2, 2), (2, 2, 2))
        b0 = unit(x, sd, f"{name}.b0")
        b1 = unit(unit(x, sd, f"{name}.b1a"), sd, f"{name}.b1b")
        b2 = unit(unit(x, sd, f"{name}.b2a"), sd, f"{name}.b2b")
        b3 = unit(maxpool3d(x, (3, 3, 3), (1, 1, 1)), sd, f"{name}.b3b")
        x = torch.cat([b0, b1, b2, b3], dim=1)
    x = _windows(x, (2, 7, 7), (1, 1, 1)).mean(dim=(5, 6, 7))                     # AvgPool 2x7x7 VALID -> [B, 1024, T', 1, 1]
    y = torch.tensordot(x, sd["logits.conv3d.weight"].double()[:, :, 0, 0, 0], dims=([1], [1]))   # [B, T', 1, 1, 400]
    y = y + sd["logits.conv3d.bias"].double()
    return y.mean(dim=1).reshape(x.shape[0], -1)


# ---- numpy loops on tiny tensors (the second cross-check) -------------------------------------------------------------------
def conv3d_loop(x: np.ndarray, w: np.ndarray, stride: int) -> np.ndarray:
    B, C, T, H, W = x.shape
    O, _, k, _, _ = w.shape
    (To, pt, _), (Ho, ph, _), (Wo, pw, _) = same_pad(T, k, stride), same_pad(H, k, stride), same_pad(W, k, stride)
    y = np.zeros((B, O, To, Ho, Wo))
    for b in range(B):
        for o in range(O):
            for t in range(To):
                for h in range(Ho):
                    for v in range(Wo):
                        s = 0.0
                        for c in range(C):
                            for dt in range(k):
                                for dh in range(k):
                                    for dw in range(k):
                                        ti, hi, wi = t * stride - pt + dt, h * stride - ph + dh, v * stride - pw + dw
                                        if 0 <= ti < T and 0 <= hi < H and 0 <= wi < W:
                                            s += x[b, c, ti, hi, wi] * w[o, c, dt, dh, dw]
                        y[b, o, t, h, v] = s
    return y


def maxpool3d_loop(x: np.ndarray, k, s) -> np.ndarray:
    B, C, T, H, W = x.shape
    (To, pt, _), (Ho, ph, _), (Wo, pw, _) = same_pad(T, k[0], s[0]), same_pad(H, k[1], s[1]), same_pad(W, k[2], s[2])
    y = np.full((B, C, To, Ho, Wo), -np.inf)
    for t in range(To):
        for h in range(Ho):
            for v in range(Wo):
                for dt in range(k[0]):
                    for dh in range(k[1]):
                        for dw in range(k[2]):
                            ti, hi, wi = t * s[0] - pt + dt, h * s[1] - ph + dh, v * s[2] - pw + dw
                            if 0 <= ti < T and 0 <= hi < H and 0 <= wi < W:
                                y[:, :, t, h, v] = np.maximum(y[:, :, t, h, v], x[:, :, ti, hi, wi])
    return y
