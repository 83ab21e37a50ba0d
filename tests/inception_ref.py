"""Float64 restatement of the frame preprocessing and of Inception-v3 as the FID / IS / MMD extractor runs it, for the tests.

Written from the definitions (reference model/metrics/metrics.py semantics and the published architecture, restated here):
  preprocess: bilinear resize of [3, H, W] to 299 x 299 with torch's align_corners=True rule (scale = (in - 1) / (out - 1), src = scale
  * dst, upper neighbour clamped; the source index and the weights in fp32 arithmetic as torch computes them for the reference's fp32
  input, the blend in the working dtype); no clamp unless asked, no normalisation;
  unit = conv (no bias, zero padding) -> eval BatchNorm (eps 1e-3) -> ReLU; max-pool 3 x 3 stride 2 VALID; avg-pool 3 x 3 stride 1
  padding 1 with the padded cells counted (always / 9); the blocks A .. E with their concatenation orders; mean over 8 x 8 -> acts;
  fc -> softmax -> probs.
Convolutions are im2col products (tensor.unfold + tensordot) on zero-padded inputs, so this file shares no code path with torch's
conv2d / pooling.  `features(x, state, dtype)` runs the same arithmetic in another dtype: torch.float32 is the yardstick the GPU test
measures the HIP path against.  The kernel sizes, strides and paddings come from metrics.UNIT_SPECS; the wiring is written out here.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from titok_video_amd.model.metrics.metrics import BN_EPS, INPUT_SIZE, UNIT_SPECS

GEOMETRY = {name: (k, s, p) for name, _cin, _cout, k, s, p in UNIT_SPECS}


def _resize_matrix(n_in: int, n_out: int) -> torch.Tensor:
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)
    for d in range(n_out):
        src = np.float32(scale * np.float32(d))
        i0 = min(int(src), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        l1 = np.float32(src - np.float32(i0))
        m[d, i0] += float(np.float32(1.0) - l1)
        m[d, i1] += float(l1)
    return m


def preprocess(img: torch.Tensor, clamp: bool = False, dtype=torch.float64) -> torch.Tensor:
    """[3, H, W] -> [3, 299, 299]."""
    x = img.to(dtype)
    if clamp:
        x = x.clamp(-1, 1)
    _, H, W = x.shape
    x = torch.einsum("vh,chw->cvw", _resize_matrix(H, INPUT_SIZE).to(dtype), x)
    return torch.einsum("xw,chw->chx", _resize_matrix(W, INPUT_SIZE).to(dtype), x)


def _windows(x: torch.Tensor, k, s) -> torch.Tensor:
    """[B, C, H, W] (padded) -> [B, C, Ho, Wo, kh, kw]."""
    return x.unfold(2, k[0], s[0]).unfold(3, k[1], s[1])


def conv2d(x: torch.Tensor, w: torch.Tensor, stride=(1, 1), pad=(0, 0)) -> torch.Tensor:
    """Zero-padded 2-D convolution of [B, Cin, H, W] with [Cout, Cin, kh, kw] in x's dtype, no bias."""
    win = _windows(F.pad(x, (pad[1], pad[1], pad[0], pad[0])), tuple(w.shape[2:]), stride)
    y = torch.tensordot(win, w.to(x.dtype), dims=([1, 4, 5], [1, 2, 3]))     # [B, Ho, Wo, Cout]
    return y.permute(0, 3, 1, 2).contiguous()


def maxpool3s2(x: torch.Tensor) -> torch.Tensor:
    return _windows(x, (3, 3), (2, 2)).amax(dim=(4, 5))


def avgpool3(x: torch.Tensor) -> torch.Tensor:
    """3 x 3, stride 1, padding 1, count_include_pad: the zero-padded window sum over 9."""
    return _windows(F.pad(x, (1, 1, 1, 1)), (3, 3), (1, 1)).sum(dim=(4, 5)) / 9


def bn_fold(sd, name):
    scale = sd[f"{name}.bn.weight"].double() / torch.sqrt(sd[f"{name}.bn.running_var"].double() + BN_EPS)
    return scale, sd[f"{name}.bn.bias"].double() - sd[f"{name}.bn.running_mean"].double() * scale


def unit(x, sd, name):
    k, s, p = GEOMETRY[name]
    w = sd[f"{name}.conv.weight"]
    assert tuple(w.shape[2:]) == k, name
    y = conv2d(x, w, s, p)
    scale, shift = bn_fold(sd, name)
    return (y * scale.to(x.dtype).view(1, -1, 1, 1) + shift.to(x.dtype).view(1, -1, 1, 1)).clamp_min(0)


def block_a(x, sd, n):
    u = lambda t, s: unit(t, sd, f"{n}.{s}")
    b1 = u(x, "branch1x1")
    b5 = u(u(x, "branch5x5_1"), "branch5x5_2")
    b3 = u(u(u(x, "branch3x3dbl_1"), "branch3x3dbl_2"), "branch3x3dbl_3")
    bp = u(avgpool3(x), "branch_pool")
    return torch.cat([b1, b5, b3, bp], 1)


def block_b(x, sd, n):
    u = lambda t, s: unit(t, sd, f"{n}.{s}")
    b3 = u(x, "branch3x3")
    bd = u(u(u(x, "branch3x3dbl_1"), "branch3x3dbl_2"), "branch3x3dbl_3")
    return torch.cat([b3, bd, maxpool3s2(x)], 1)


def block_c(x, sd, n):
    u = lambda t, s: unit(t, sd, f"{n}.{s}")
    b1 = u(x, "branch1x1")
    b7 = u(u(u(x, "branch7x7_1"), "branch7x7_2"), "branch7x7_3")
    bd = x
    for i in range(1, 6):
        bd = u(bd, f"branch7x7dbl_{i}")
    bp = u(avgpool3(x), "branch_pool")
    return torch.cat([b1, b7, bd, bp], 1)


def block_d(x, sd, n):
    u = lambda t, s: unit(t, sd, f"{n}.{s}")
    b3 = u(u(x, "branch3x3_1"), "branch3x3_2")
    b7 = x
    for i in range(1, 5):
        b7 = u(b7, f"branch7x7x3_{i}")
    return torch.cat([b3, b7, maxpool3s2(x)], 1)


def block_e(x, sd, n):
    u = lambda t, s: unit(t, sd, f"{n}.{s}")
    b1 = u(x, "branch1x1")
    b3 = u(x, "branch3x3_1")
    b3 = torch.cat([u(b3, "branch3x3_2a"), u(b3, "branch3x3_2b")], 1)
    bd = u(u(x, "branch3x3dbl_1"), "branch3x3dbl_2")
    bd = torch.cat([u(bd, "branch3x3dbl_3a"), u(bd, "branch3x3dbl_3b")], 1)
    bp = u(avgpool3(x), "branch_pool")
    return torch.cat([b1, b3, bd, bp], 1)


BLOCKS = [("Mixed_5b", block_a), ("Mixed_5c", block_a), ("Mixed_5d", block_a), ("Mixed_6a", block_b), ("Mixed_6b", block_c),
          ("Mixed_6c", block_c), ("Mixed_6d", block_c), ("Mixed_6e", block_c), ("Mixed_7a", block_d), ("Mixed_7b", block_e),
          ("Mixed_7c", block_e)]


def trunk(x: torch.Tensor, sd) -> torch.Tensor:
    """[B, 3, 299, 299] -> [B, 2048, 8, 8]."""
    x = unit(x, sd, "Conv2d_1a_3x3")
    x = unit(x, sd, "Conv2d_2a_3x3")
    x = unit(x, sd, "Conv2d_2b_3x3")
    x = maxpool3s2(x)
    x = unit(x, sd, "Conv2d_3b_1x1")
    x = unit(x, sd, "Conv2d_4a_3x3")
    x = maxpool3s2(x)
    for name, fn in BLOCKS:
        x = fn(x, sd, name)
    return x


def tail(x: torch.Tensor, sd):
    """[B, 2048, 8, 8] -> (acts [B, 2048], probs [B, 1000])."""
    acts = x.mean(dim=(2, 3))
    logits = acts @ sd["fc.weight"].to(x.dtype).t() + sd["fc.bias"].to(x.dtype)
    z = logits - logits.amax(dim=1, keepdim=True)
    e = z.exp()
    return acts, e / e.sum(dim=1, keepdim=True)


def features(x: torch.Tensor, sd, dtype=torch.float64):
    """[B, 3, 299, 299] (preprocess) -> (acts, probs) in `dtype`."""
    return tail(trunk(x.to(dtype), sd), sd)


# ---- the frames of the whole-network tests (tests/test_fid_cpu.py asserts that they give non-degenerate features) -------------
NETWORK_FRAME_SHAPES = [(128, 128), (96, 160), (168, 136)]
NETWORK_FRAME_SEED, NETWORK_STATE_SEED = 21, 3


def seeded_frames(shapes, seed, dtype=torch.float32, spread=1.2):
    """[3, H, W] frames, U(-spread, spread), drawn in order from one CPU generator."""
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand((3,) + tuple(s), generator=g) * 2 - 1) * spread).to(dtype) for s in shapes]


# ---- explicit loops on tiny tensors (the second cross-check) ----------------------------------------------------------------
def conv2d_loop(x: np.ndarray, w: np.ndarray, stride, pad) -> np.ndarray:
    B, C, H, W = x.shape
    O, _, kh, kw = w.shape
    Ho, Wo = (H + 2 * pad[0] - kh) // stride[0] + 1, (W + 2 * pad[1] - kw) // stride[1] + 1
    y = np.zeros((B, O, Ho, Wo))
    for b in range(B):
        for o in range(O):
            for h in range(Ho):
                for v in range(Wo):
                    s = 0.0
                    for c in range(C):
                        for dh in range(kh):
                            for dw in range(kw):
                                hi, wi = h * stride[0] - pad[0] + dh, v * stride[1] - pad[1] + dw
                                if 0 <= hi < H and 0 <= wi < W:
                                    s += x[b, c, hi, wi] * w[o, c, dh, dw]
                    y[b, o, h, v] = s
    return y


def avgpool3_loop(x: np.ndarray) -> np.ndarray:
    B, C, H, W = x.shape
    y = np.zeros_like(x)
    for h in range(H):
        for v in range(W):
            for dh in (-1, 0, 1):
                for dw in (-1, 0, 1):
                    if 0 <= h + dh < H and 0 <= v + dw < W:
                        y[:, :, h, v] += x[:, :, h + dh, v + dw]
    return y / 9


def maxpool3s2_loop(x: np.ndarray) -> np.ndarray:
    B, C, H, W = x.shape
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    y = np.full((B, C, Ho, Wo), -np.inf)
    for h in range(Ho):
        for v in range(Wo):
            for dh in range(3):
                for dw in range(3):
                    y[:, :, h, v] = np.maximum(y[:, :, h, v], x[:, :, 2 * h + dh, 2 * v + dw])
    return y
