"""A plain torch restatement of JEDi's feature extractor (reference model/metrics/jedi.py get_feats): preprocessing, upstream
V-JEPA's VisionTransformer (patch_embed Conv3d, pos_embed, pre-norm blocks with MHA and a GELU MLP, final norm) and the SSv2
probe's AttentivePooler (one query, one CrossAttentionBlock).  Any width / head count (the CPU tests run it small), any dtype
(float64 for the yardstick).

`bf16=True` rounds to bf16 where the reference's bf16-autocast validation step does: the conv's input, every Linear / Conv3d
output, the operands of every Linear (LayerNorm outputs, the attention output, the GELU output) and the attention's q / k / v.
LayerNorm statistics, softmax and the residual stream stay in the working dtype."""
from __future__ import annotations

import math
from typing import Mapping

import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _r(x: torch.Tensor, on: bool) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype) if on else x


def preprocess(clip: torch.Tensor, size: int = 224, frames: int = 16) -> torch.Tensor:
    """[3, T, S, S] -> [3, 16, size, size] in fp32: clamp, (v + 1) / 2, bicubic (align_corners=False, no antialias), ImageNet
    normalisation, last frame repeated (get_feats + pad_frames)."""
    v = (clip.float().clamp(-1, 1) + 1) / 2
    v = v.permute(1, 0, 2, 3)                                     # T C H W
    if v.shape[-1] != size:
        v = F.interpolate(v, size=(size, size), mode="bicubic", align_corners=False, antialias=False)
    mean = torch.tensor(MEAN, device=v.device)[None, :, None, None]
    std = torch.tensor(STD, device=v.device)[None, :, None, None]
    v = ((v - mean) / std).permute(1, 0, 2, 3)                   # C T H W
    if v.shape[1] < frames:
        v = torch.cat([v, v[:, -1:].expand(-1, frames - v.shape[1], -1, -1)], 1)
    return v


def patch_rows(v: torch.Tensor, patch: int = 16, tubelet: int = 2) -> torch.Tensor:
    """[C, T, H, W] -> [(T/2)(H/16)(W/16), C * 2 * 16 * 16] in (t, h, w) token order, (c, kt, kh, kw) column order."""
    Cc, T, H, W = v.shape
    x = v.reshape(Cc, T // tubelet, tubelet, H // patch, patch, W // patch, patch)
    return x.permute(1, 3, 5, 0, 2, 4, 6).reshape((T // tubelet) * (H // patch) * (W // patch), -1)


def layer_norm(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = (x - mu).square().mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def linear(x, w, b, bf16):
    return _r(_r(x, bf16) @ _r(w, bf16).T + _r(b, bf16), bf16)


def mha(q, k, v, heads):
    """softmax(q k^T / sqrt(hd)) v per head; q [n, d], k / v [N, d]."""
    n, d = q.shape
    hd = d // heads
    qh = q.reshape(n, heads, hd).transpose(0, 1)
    kh = k.reshape(-1, heads, hd).transpose(0, 1)
    vh = v.reshape(-1, heads, hd).transpose(0, 1)
    p = torch.softmax(qh @ kh.transpose(1, 2) / math.sqrt(hd), -1)
    return (p @ vh).transpose(0, 1).reshape(n, d)


def encoder(rows: torch.Tensor, sd: Mapping[str, torch.Tensor], heads: int = 16, bf16: bool = True, depth: int | None = None) -> torch.Tensor:
    """rows [N, Kin] (patch_rows of one clip) -> the final norm's output [N, d] in rows.dtype."""
    dt = rows.dtype
    g = lambda k: sd[k].to(device=rows.device, dtype=dt)
    d = sd["norm.weight"].shape[0]
    if depth is None:
        depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    x = linear(rows, g("patch_embed.proj.weight").reshape(d, -1), g("patch_embed.proj.bias"), bf16) + g("pos_embed")[0, :rows.shape[0]]
    for i in range(depth):
        p = f"blocks.{i}."
        h = layer_norm(x, g(p + "norm1.weight"), g(p + "norm1.bias"), 1e-6)
        qkv = linear(h, g(p + "attn.qkv.weight"), g(p + "attn.qkv.bias"), bf16)
        q, k, v = qkv.split(d, -1)
        a = _r(mha(q, k, v, heads), bf16)
        x = x + linear(a, g(p + "attn.proj.weight"), g(p + "attn.proj.bias"), bf16)
        h = layer_norm(x, g(p + "norm2.weight"), g(p + "norm2.bias"), 1e-6)
        f = _r(F.gelu(linear(h, g(p + "mlp.fc1.weight"), g(p + "mlp.fc1.bias"), bf16)), bf16)
        x = x + linear(f, g(p + "mlp.fc2.weight"), g(p + "mlp.fc2.bias"), bf16)
    return layer_norm(x, g("norm.weight"), g("norm.bias"), 1e-6)


def pooler(y: torch.Tensor, sd: Mapping[str, torch.Tensor], heads: int = 16, bf16: bool = True) -> torch.Tensor:
    """AttentivePooler(num_queries=1, depth=1) of the encoder output y [N, d] -> [d]."""
    dt = y.dtype
    g = lambda k: sd[k].to(device=y.device, dtype=dt)
    p = "pooler.cross_attention_block."
    qt = g("pooler.query_tokens").reshape(1, -1)
    h = layer_norm(y, g(p + "norm1.weight"), g(p + "norm1.bias"), 1e-5)
    q = linear(qt, g(p + "xattn.q.weight"), g(p + "xattn.q.bias"), bf16)
    k, v = linear(h, g(p + "xattn.kv.weight"), g(p + "xattn.kv.bias"), bf16).chunk(2, -1)
    a = _r(mha(q, k, v, heads), bf16)
    z = qt + linear(a, g(p + "xattn.proj.weight"), g(p + "xattn.proj.bias"), bf16)
    h = layer_norm(z, g(p + "norm2.weight"), g(p + "norm2.bias"), 1e-5)
    f = _r(F.gelu(linear(h, g(p + "mlp.fc1.weight"), g(p + "mlp.fc1.bias"), bf16)), bf16)
    z = z + linear(f, g(p + "mlp.fc2.weight"), g(p + "mlp.fc2.bias"), bf16)
    return z[0]


def features(clip: torch.Tensor, enc: Mapping[str, torch.Tensor], probe: Mapping[str, torch.Tensor] | None, finetuned: bool = True,
             dtype=torch.float64, bf16: bool = True, depth: int | None = None) -> torch.Tensor:
    """get_feats of one clip [3, T, S, S] -> [d]."""
    rows = _r(patch_rows(preprocess(clip)), bf16).to(dtype)
    y = encoder(rows, enc, bf16=bf16, depth=depth)
    return pooler(y, probe, bf16=bf16) if finetuned else y.mean(0)
