"""Seeded synthetic inputs for measurement and parity runs.

There is no network for checkpoints or datasets, so benchmarks and parity tests use
* clips  : `[3,T,H,W]`, values U(-1,1) (the loader's range, reference dataset/video_dataset.py:118-119)
* weights: a deterministic recipe keyed by the reference's state-dict names.  The reference's own
  init (trunc_normal std 0.02, model/base/utils.py:54-58) maps every latent token to a single FSQ
  index, so the recipe scales the linear weights up and perturbs the norm gains to
  get non-degenerate token indices.

The recipe only depends on torch's CPU generator, so it reproduces bit-identically on any box with
this image; golden fixtures therefore store inputs/outputs only, never weights.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, List, Sequence, Tuple

import torch

from .model.base.utils import geglu_inner_dim, get_model_dims


def tower_param_shapes(kind: str, model_size: str, patch_size: Sequence[int], in_channels: int,
                       out_channels: int) -> "OrderedDict[str, Tuple[int, ...]]":
    """State-dict keys and shapes of one tower (reference model/base/blocks.py:31-69,108-146)."""
    width, layers, heads, _ = get_model_dims(model_size)
    hq, hkv = heads
    g = (width // hq) * hkv
    inner = geglu_inner_dim(width)
    pd = math.prod(patch_size)
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    if kind == "encoder":
        s["proj_in.weight"] = (width, in_channels * pd)
        s["proj_in.bias"] = (width,)
    else:
        s["proj_in.weight"] = (width, in_channels)
        s["proj_in.bias"] = (width,)
    s["mask_token"] = (1, 1)
    s["ln_pre_t.weight"] = (width,)
    s["ln_pre_p.weight"] = (width,)
    for i in range(layers):
        s[f"model_layers.attn_layer.{i}.pre_ln.weight"] = (width,)
        s[f"model_layers.attn_layer.{i}.to_qkv.weight"] = (2 * width + 2 * g, width)
        s[f"model_layers.attn_layer.{i}.out_proj.weight"] = (width, width)
    for i in range(layers):
        s[f"model_layers.ffd_layer.{i}.norm.weight"] = (width,)
        s[f"model_layers.ffd_layer.{i}.w12.weight"] = (2 * inner, width)
        s[f"model_layers.ffd_layer.{i}.w3.weight"] = (width, inner)
    for i in range(layers - 1):
        s[f"model_layers.attn_post_ln.{i}.weight"] = (width,)
    for i in range(layers - 1):
        s[f"model_layers.ffd_post_ln.{i}.weight"] = (width,)
    s["ln_post.weight"] = (width,)
    if kind == "encoder":
        s["proj_out.weight"] = (out_channels, width)
        s["proj_out.bias"] = (out_channels,)
    else:
        s["proj_out.weight"] = (out_channels * pd, width)
        s["proj_out.bias"] = (out_channels * pd,)
    return s


def seeded_tower_state(kind: str, model_size: str, patch_size: Sequence[int], in_channels: int,
                       out_channels: int, seed: int, gain: float = 6.0) -> Dict[str, torch.Tensor]:
    """fp32 CPU state dict for one tower from `seed` (keys in `tower_param_shapes` order)."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    out: Dict[str, torch.Tensor] = OrderedDict()
    for key, shape in tower_param_shapes(kind, model_size, patch_size, in_channels, out_channels).items():
        r = torch.randn(shape, generator=gen, dtype=torch.float32)
        if key == "mask_token":
            t = 0.5 * r
        elif key.endswith("bias"):
            t = 0.02 * r
        elif len(shape) == 1:          # RMSNorm gains
            t = 1.0 + 0.1 * r
        else:                          # Linear weights
            t = (0.02 * gain) * r.clamp(-2.0, 2.0)
        out[key] = t.contiguous()
    return out


def seeded_titok_state(seed: int = 0, encoder_size: str = "tiny", decoder_size: str = "tiny",
                       patch_size: Sequence[int] = (4, 8, 8), token_size: int = 5,
                       gain: float = 6.0) -> Dict[str, torch.Tensor]:
    """State dict of a whole `TiTok` (`encoder.*`, `decoder.*`; FSQ has no persistent keys)."""
    sd: Dict[str, torch.Tensor] = OrderedDict()
    enc = seeded_tower_state("encoder", encoder_size, patch_size, 3, token_size, 1000 + seed, gain)
    dec = seeded_tower_state("decoder", decoder_size, patch_size, token_size, 3, 2000 + seed, gain)
    for k, v in enc.items():
        sd["encoder." + k] = v
    for k, v in dec.items():
        sd["decoder." + k] = v
    return sd


def seeded_lpips_state(seed: int = 0) -> Dict[str, torch.Tensor]:
    """fp32 CPU state dict with the reference LPIPS keys (model/metrics/lpips_gram.py) from `seed`: He-normal 3x3 convolutions
    (std sqrt(2 / (9 Cin))), biases N(0, 0.05^2), lin weights |N(0, 1)| / C (trained LPIPS lin weights are non-negative).
    Drawn in key order from one CPU generator."""
    from .model.metrics.lpips_gram import CHNS, CONV_INDICES, VGG_FEATURES, _slice_of
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    out: Dict[str, torch.Tensor] = OrderedDict()
    out["scaling_layer.shift"] = torch.tensor([-0.030, -0.088, -0.188])[None, :, None, None]
    out["scaling_layer.scale"] = torch.tensor([0.458, 0.448, 0.450])[None, :, None, None]
    dims = {f[0]: (f[2], f[3]) for f in VGG_FEATURES if f[1] == "conv"}
    for i in CONV_INDICES:
        cin, cout = dims[i]
        out[f"net.slice{_slice_of(i)}.{i}.weight"] = torch.randn((cout, cin, 3, 3), generator=gen) * math.sqrt(2.0 / (9 * cin))
        out[f"net.slice{_slice_of(i)}.{i}.bias"] = 0.05 * torch.randn((cout,), generator=gen)
    for k, c in enumerate(CHNS):
        out[f"lin{k}.model.1.weight"] = torch.randn((1, c, 1, 1), generator=gen).abs() / c
    return out


def seeded_i3d_state(seed: int = 0) -> Dict[str, torch.Tensor]:
    """Canonical I3D state dict (model/metrics/fvd.py canonical_shapes) of seeded values: He-normal convolutions, BatchNorm with no
    scale (as TF's I3D), small means and shifts, running_var in [0.5, 1.5]; logits He-normal with a small bias."""
    from .model.metrics.fvd import canonical_shapes

    g = torch.Generator().manual_seed(seed)
    out = OrderedDict()
    for key, shape in canonical_shapes().items():
        if key.endswith(".bn.weight"):
            continue
        if len(shape) == 5:
            fan_in = shape[1] * shape[2] * shape[3] * shape[4]
            out[key] = torch.randn(shape, generator=g) * math.sqrt(2.0 / fan_in)
        elif key.endswith("running_var"):
            out[key] = 0.5 + torch.rand(shape, generator=g)
        else:   # bn.bias, bn.running_mean, logits.conv3d.bias
            out[key] = 0.1 * torch.randn(shape, generator=g)
    return out


def seeded_inception_state(seed: int = 0) -> Dict[str, torch.Tensor]:
    """torchvision-keyed Inception-v3 state dict (model/metrics/metrics.py canonical_shapes) of seeded values: He-normal
    convolutions and BatchNorm statistics near identity (weight 1 +- 0.05, running_var in [0.9, 1.1], bias and running_mean
    N(0, 0.05^2)), so that activations neither die nor blow up through the 47 convolutions of the deepest path; fc N(0, 0.02^2)
    with a small bias, which keeps the softmax away from one-hot."""
    from .model.metrics.metrics import canonical_shapes

    g = torch.Generator().manual_seed(seed)
    out = OrderedDict()
    for key, shape in canonical_shapes().items():
        if len(shape) == 4:
            out[key] = torch.randn(shape, generator=g) * math.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        elif key == "fc.weight":
            out[key] = 0.02 * torch.randn(shape, generator=g)
        elif key.endswith("bn.weight"):
            out[key] = 1.0 + 0.05 * torch.randn(shape, generator=g)
        elif key.endswith("running_var"):
            out[key] = 0.9 + 0.2 * torch.rand(shape, generator=g)
        else:   # bn.bias, bn.running_mean, fc.bias
            out[key] = 0.05 * torch.randn(shape, generator=g)
    return out


def _vjepa_values(shapes, g: torch.Generator) -> Dict[str, torch.Tensor]:
    out = OrderedDict()
    for key, shape in shapes.items():
        if key == "pos_embed":      # a sincos table of token index, |values| <= 1, like upstream's uniform-power table
            pos = torch.arange(shape[1], dtype=torch.float64)[:, None]
            freq = 1.0 / 10000.0 ** (torch.arange(shape[2] // 2, dtype=torch.float64) / (shape[2] // 2))
            out[key] = torch.cat([torch.sin(pos * freq), torch.cos(pos * freq)], 1).float()[None]
        elif "norm" in key and key.endswith(".weight"):
            out[key] = 1.0 + 0.05 * torch.randn(shape, generator=g)
        elif key.endswith(".bias"):
            out[key] = 0.02 * torch.randn(shape, generator=g)
        else:                       # linears, the patch Conv3d, query_tokens: trunc-normal std 0.02 (upstream's init)
            out[key] = torch.nn.init.trunc_normal_(torch.empty(shape), std=0.02, a=-0.04, b=0.04, generator=g)
    return out


def seeded_vjepa_state(depth: int = 24, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Canonical V-JEPA ViT-L/16 encoder state dict (model/metrics/jedi.py encoder_shapes) of `depth` blocks with seeded values:
    trunc-normal std 0.02 linears, LayerNorm weights 1 + N(0, 0.05^2), biases N(0, 0.02^2), a sincos pos_embed."""
    from .model.metrics.jedi import encoder_shapes

    return _vjepa_values(encoder_shapes(depth), torch.Generator().manual_seed(seed))


def seeded_probe_state(seed: int = 0) -> Dict[str, torch.Tensor]:
    """Canonical pooler state dict of the SSv2 probe (model/metrics/jedi.py probe_shapes), seeded as seeded_vjepa_state."""
    from .model.metrics.jedi import probe_shapes

    return _vjepa_values(probe_shapes(), torch.Generator().manual_seed(seed))


def synthetic_clips(shapes: Sequence[Sequence[int]], seed: int = 1234,
                    dtype: torch.dtype = torch.float32, device="cpu") -> List[torch.Tensor]:
    """List of `[3,T,H,W]` clips, U(-1,1), generated on CPU from `seed` then moved/cast."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    clips = []
    for (t, h, w) in shapes:
        c = torch.rand((3, int(t), int(h), int(w)), generator=gen, dtype=torch.float32) * 2.0 - 1.0
        clips.append(c.to(device=device, dtype=dtype))
    return clips


def synthetic_token_counts(n: int, lo: int, hi: int, seed: int = 1234) -> List[int]:
    """K ~ U[lo, hi] per clip (reference configs/tiny.yaml:57 token_range)."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed) + 7)
    return torch.randint(lo, hi + 1, (n,), generator=gen).tolist()
